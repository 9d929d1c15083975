// pose_graph_kernels.hpp -- loop closure's back half (OptimizationProblem::solve, src/OptimizationProblem.cpp:26-44): Open3D v0.15.1
// GlobalOptimization with GlobalOptimizationLevenbergMarquardt (GlobalOptimization.cpp, restated; Open3D is not part of this project).
// All arithmetic is f64.  The LM control flow stays on the host (o3ds_global_optimization); these kernels produce every number it reads,
// each in a fixed order, so a run is bit-reproducible across handles, launches and storage precisions.
//   * pg_edge_kernel      one thread per edge: X^-1, Ts, Tt^-1, e = lin(X^-1 Tt^-1 Ts), Js from the six generators (Jt = -Js exactly),
//                         the residual term with the confidence it was given, the line-process confidence update of an uncertain edge,
//                         and with the NEW confidence P = conf Js^T Info Js and q = conf Js^T Info e.
//   * pg_assemble_h_kernel one workgroup per structural non-zero 6x6 block of H: +-P of its edges in edge order (a per-block list built
//                         on the host once per pass), as Open3D's serial loop adds them.  No atomics.
//   * pg_assemble_b_kernel one thread per node: b_i = -(sum over its edge ends, in edge order, of +-q).
//   * pg_small_solve_kernel m = 6N <= 128: (H + lambda I) delta = b in one workgroup, the matrix in LDS (128 KiB): Cholesky, forward
//                         and back substitution.
//   * pg_panel_kernel / pg_trsm_kernel / pg_syrk_kernel   the blocked right-looking Cholesky of the padded M x M matrix (64-wide
//                         blocks): the diagonal block in LDS, the panel below it, and the trailing update L_ij -= L_ik L_jk^T on
//                         v_mfma_f64_16x16x4_f64 (C/D: col = lane & 15, row = (lane >> 4) + 4 reg).
//   * pg_fwd_kernel / pg_bwd_kernel  blocked forward / back substitution, one launch per block column.
//   * pg_update_kernel    one thread per node: the trial pose V6toM4(delta_i) T_i, and the node's share of |delta|^2, |x|^2 and
//                         delta . (lambda delta + b).
//   * pg_reduce_kernel    one workgroup: the sums and maxima of one LM step in a fixed order (a strided pass per thread, then a fixed
//                         tree), into the record the host reads.
#pragma once
#include "common.hpp"

namespace o3ds {

#pragma clang fp contract(off)  // the per-edge and per-node arithmetic rounds product by product, as Eigen's (no FMA) does

constexpr int kPgEdgeOut = 52;   // doubles per edge: e[6] P[36] q[6] rterm conf_new valid rsq
constexpr int kPgNB = 64;        // block size of the blocked factorisation; M is 6N rounded up to it
constexpr int kPgSmallMax = 128; // 6N up to this: the one-workgroup factor-and-solve in LDS
constexpr int kPgLds = kPgNB + 1;

struct PgEdgeIn {
  double X[16];     // column-major, as the ABI's
  double info[36];  // row-major
  int src, tgt, uncertain, pad;
};

struct PgRecord {   // what the host reads once per LM step
  double residual, dn2, xn2, ddb, maxb, maxdiag;
  int valid, err;   // err: 1 + the row of the first non-positive pivot (0: none)
  int pad[2];
};

__device__ inline void pg_load_rowmajor(const double* __restrict__ cm, double m[16]) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) m[r * 4 + c] = cm[c * 4 + r];
}

// 4x4 inverse by cofactors (Eigen's method for fixed 4x4), row-major in and out
__device__ inline void pg_inv4(const double* __restrict__ m, double* __restrict__ o) {
  double inv[16];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  const double rdet = 1.0 / det;
  for (int k = 0; k < 16; ++k) o[k] = inv[k] * rdet;
}

__device__ inline void pg_mul4(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = a[r * 4] * b[c];
      for (int k = 1; k < 4; ++k) s += a[r * 4 + k] * b[k * 4 + c];
      o[r * 4 + c] = s;
    }
}

// lin6(A G_i Ts) for generator i: G_i Ts has two non-zero rows (rotations) or one (translations, the last row of Ts)
__device__ inline void pg_jac_col(const double* __restrict__ A, const double* __restrict__ Ts, int i, double out[6]) {
  double GT[16];
  for (int k = 0; k < 16; ++k) GT[k] = 0.0;
  switch (i) {
    case 0: for (int c = 0; c < 4; ++c) GT[4 + c] = -Ts[8 + c], GT[8 + c] = Ts[4 + c]; break;   // (1,2) = -1, (2,1) = 1
    case 1: for (int c = 0; c < 4; ++c) GT[0 + c] = Ts[8 + c], GT[8 + c] = -Ts[0 + c]; break;   // (0,2) = 1, (2,0) = -1
    case 2: for (int c = 0; c < 4; ++c) GT[0 + c] = -Ts[4 + c], GT[4 + c] = Ts[0 + c]; break;   // (0,1) = -1, (1,0) = 1
    default: for (int c = 0; c < 4; ++c) GT[(i - 3) * 4 + c] = Ts[12 + c]; break;               // (i-3, 3) = 1
  }
  double M[16];
  pg_mul4(A, GT, M);
  out[0] = (-M[1 * 4 + 2] + M[2 * 4 + 1]) / 2.0;
  out[1] = (-M[2 * 4 + 0] + M[0 * 4 + 2]) / 2.0;
  out[2] = (-M[0 * 4 + 1] + M[1 * 4 + 0]) / 2.0;
  out[3] = M[0 * 4 + 3];
  out[4] = M[1 * 4 + 3];
  out[5] = M[2 * 4 + 3];
}

__global__ __launch_bounds__(64) void pg_edge_kernel(const double* __restrict__ poses, const PgEdgeIn* __restrict__ edges, int n_edges,
                                                     const double* __restrict__ conf_in, double* __restrict__ conf_out,
                                                     double* __restrict__ out, double lpw, double prune) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_edges) return;
  const PgEdgeIn& E = edges[k];
  double A[16], Ts[16];
  {
    double X[16], Xi[16], Tt[16], Tti[16];
    pg_load_rowmajor(E.X, X);
    pg_inv4(X, Xi);
    pg_load_rowmajor(poses + (size_t)E.tgt * 16, Tt);
    pg_inv4(Tt, Tti);
    pg_mul4(Xi, Tti, A);  // (X^-1 Tt^-1) Ts, Eigen's left-to-right order
  }
  pg_load_rowmajor(poses + (size_t)E.src * 16, Ts);
  double e[6];
  {
    double M[16];
    pg_mul4(A, Ts, M);
    e[0] = (-M[1 * 4 + 2] + M[2 * 4 + 1]) / 2.0;
    e[1] = (-M[2 * 4 + 0] + M[0 * 4 + 2]) / 2.0;
    e[2] = (-M[0 * 4 + 1] + M[1 * 4 + 0]) / 2.0;
    e[3] = M[3], e[4] = M[7], e[5] = M[11];
  }
  double Js[36];  // row-major 6x6, column i = lin(A G_i Ts)
  for (int i = 0; i < 6; ++i) {
    double col[6];
    pg_jac_col(A, Ts, i, col);
    for (int r = 0; r < 6; ++r) Js[r * 6 + i] = col[r];
  }
  double rsq = 0.0;  // e^T Info e
  for (int r = 0; r < 6; ++r) {
    double s = e[0] * E.info[r * 6 + 0];  // (e^T Info)_r
    for (int c = 1; c < 6; ++c) s += e[c] * E.info[c * 6 + r];
    rsq += s * e[r];
  }
  const double c0 = conf_in[k];
  const double sq = sqrt(c0) - 1.0;
  const double rterm = c0 * rsq + lpw * (sq * sq);
  double c1 = c0;
  if (E.uncertain) {
    const double t = lpw / (lpw + rsq);
    c1 = t * t;
  }
  conf_out[k] = c1;
  double* o = out + (size_t)k * kPgEdgeOut;
  for (int r = 0; r < 6; ++r) o[r] = e[r];
  for (int r = 0; r < 6; ++r) {
    double W[6];  // row r of (Js^T Info) conf
    for (int c = 0; c < 6; ++c) {
      double s = Js[0 * 6 + r] * E.info[0 * 6 + c];
      for (int l = 1; l < 6; ++l) s += Js[l * 6 + r] * E.info[l * 6 + c];
      W[c] = s * c1;
    }
    for (int c = 0; c < 6; ++c) {
      double s = W[0] * Js[0 * 6 + c];
      for (int l = 1; l < 6; ++l) s += W[l] * Js[l * 6 + c];
      o[6 + r * 6 + c] = s;
    }
    double s = W[0] * e[0];
    for (int l = 1; l < 6; ++l) s += W[l] * e[l];
    o[42 + r] = s;
  }
  o[48] = rterm;
  o[49] = c1;
  o[50] = (E.uncertain && c1 > prune) ? 1.0 : 0.0;
  o[51] = rsq;
}

// H block (bi, bj) = sum over its list, in order, of +-P; list entry = edge * 2 + negate
__global__ __launch_bounds__(64) void pg_assemble_h_kernel(const int4* __restrict__ blocks /* bi, bj, first, count */,
                                                           const int* __restrict__ list, const double* __restrict__ eout,
                                                           double* __restrict__ H, size_t ld) {
  const int4 B = blocks[blockIdx.x];
  const int t = threadIdx.x;
  if (t >= 36) return;
  const int r = t / 6, c = t % 6;
  double s = 0.0;
  for (int k = 0; k < B.w; ++k) {
    const int v = list[B.z + k];
    const double p = eout[(size_t)(v >> 1) * kPgEdgeOut + 6 + r * 6 + c];
    s += (v & 1) ? -p : p;
  }
  H[(size_t)(6 * B.x + r) * ld + 6 * B.y + c] = s;
}

// b_i = 0 - sum of its entries in order (entry = edge * 2 + is_target: the target end subtracts -q)
__global__ __launch_bounds__(64) void pg_assemble_b_kernel(const int2* __restrict__ nodes /* first, count */, const int* __restrict__ list,
                                                           const double* __restrict__ eout, int n_nodes, double* __restrict__ b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * n_nodes) return;
  const int i = t / 6, r = t % 6;
  const int2 N = nodes[i];
  double s = 0.0;
  for (int k = 0; k < N.y; ++k) {
    const int v = list[N.x + k];
    const double q = eout[(size_t)(v >> 1) * kPgEdgeOut + 42 + r];
    s -= (v & 1) ? -q : q;
  }
  b[t] = s;
}

// H's non-structural entries: zero, the padding diagonal 1 (once per pass)
__global__ __launch_bounds__(256) void pg_init_h_kernel(double* __restrict__ H, size_t M, size_t m) {
  const size_t n = M * M;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    const size_t r = k / M, c = k % M;
    H[k] = (r == c && r >= m) ? 1.0 : 0.0;
  }
}

// L = lower(H) + lambda I over the lower-triangle tiles (the factorisation reads nothing else)
__global__ __launch_bounds__(256) void pg_shift_copy_kernel(const double* __restrict__ H, double* __restrict__ L, size_t M, double lambda) {
  const size_t n = M * M;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    const size_t r = k / M, c = k % M;
    if (c / kPgNB > r / kPgNB) continue;
    const double v = H[k];
    L[k] = r == c ? v + lambda : v;
  }
}

// ---- m <= 128: everything in one workgroup ----------------------------------------------------------------------------------------
constexpr int kPgSmallThreads = 1024;
__global__ __launch_bounds__(kPgSmallThreads) void pg_small_solve_kernel(const double* __restrict__ H, size_t ld, int m, double lambda,
                                                                          const double* __restrict__ b, double* __restrict__ x,
                                                                          PgRecord* __restrict__ rec) {
  __shared__ double A[kPgSmallMax * kPgSmallMax];
  __shared__ double v[kPgSmallMax];
  __shared__ int bad;
  const int t = threadIdx.x;
  for (int k = t; k < m * m; k += kPgSmallThreads) {
    const int r = k / m, c = k % m;
    A[r * kPgSmallMax + c] = H[(size_t)r * ld + c] + (r == c ? lambda : 0.0);
  }
  for (int k = t; k < m; k += kPgSmallThreads) v[k] = b[k];
  if (t == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < m; ++j) {
    if (t == 0) {
      double d = A[j * kPgSmallMax + j];
      if (!(d > 0.0) || !isfinite(d)) {
        if (!bad) bad = j + 1;
        d = 1.0;
      }
      A[j * kPgSmallMax + j] = sqrt(d);
    }
    __syncthreads();
    const double ljj = A[j * kPgSmallMax + j];
    for (int i = j + 1 + t; i < m; i += kPgSmallThreads) A[i * kPgSmallMax + j] = A[i * kPgSmallMax + j] / ljj;
    __syncthreads();
    const int w = m - j - 1;
    for (int k = t; k < w * w; k += kPgSmallThreads) {
      const int i = j + 1 + k / w, c = j + 1 + k % w;
      if (c <= i) A[i * kPgSmallMax + c] -= A[i * kPgSmallMax + j] * A[c * kPgSmallMax + j];
    }
    __syncthreads();
  }
  for (int j = 0; j < m; ++j) {  // L y = b
    if (t == 0) v[j] = v[j] / A[j * kPgSmallMax + j];
    __syncthreads();
    for (int i = j + 1 + t; i < m; i += kPgSmallThreads) v[i] -= A[i * kPgSmallMax + j] * v[j];
    __syncthreads();
  }
  for (int j = m - 1; j >= 0; --j) {  // L^T x = y
    if (t == 0) v[j] = v[j] / A[j * kPgSmallMax + j];
    __syncthreads();
    for (int i = t; i < j; i += kPgSmallThreads) v[i] -= A[j * kPgSmallMax + i] * v[j];
    __syncthreads();
  }
  for (int k = t; k < m; k += kPgSmallThreads) x[k] = v[k];
  if (t == 0 && bad) rec->err = bad;
}

// ---- blocked Cholesky -------------------------------------------------------------------------------------------------------------
// factor the diagonal block k (already updated by every earlier column block) in LDS
__global__ __launch_bounds__(256) void pg_panel_kernel(double* __restrict__ L, size_t M, int k, PgRecord* __restrict__ rec) {
  __shared__ double A[kPgNB * kPgLds];
  __shared__ int bad;
  const int t = threadIdx.x;
  double* base = L + (size_t)k * kPgNB * M + (size_t)k * kPgNB;
  for (int e = t; e < kPgNB * kPgNB; e += 256) A[(e / kPgNB) * kPgLds + e % kPgNB] = base[(size_t)(e / kPgNB) * M + e % kPgNB];
  if (t == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < kPgNB; ++j) {
    if (t == 0) {
      double d = A[j * kPgLds + j];
      if (!(d > 0.0) || !isfinite(d)) {
        if (!bad) bad = k * kPgNB + j + 1;
        d = 1.0;
      }
      A[j * kPgLds + j] = sqrt(d);
    }
    __syncthreads();
    const double ljj = A[j * kPgLds + j];
    if (t > j && t < kPgNB) A[t * kPgLds + j] = A[t * kPgLds + j] / ljj;
    __syncthreads();
    const int w = kPgNB - j - 1;
    for (int e = t; e < w * w; e += 256) {
      const int i = j + 1 + e / w, c = j + 1 + e % w;
      if (c <= i) A[i * kPgLds + c] -= A[i * kPgLds + j] * A[c * kPgLds + j];
    }
    __syncthreads();
  }
  for (int e = t; e < kPgNB * kPgNB; e += 256) {
    const int r = e / kPgNB, c = e % kPgNB;
    if (c <= r) base[(size_t)r * M + c] = A[r * kPgLds + c];
  }
  if (t == 0 && bad && !rec->err) rec->err = bad;  // the first one: once a pivot has been replaced, later blocks fail in its wake
}

// L_ik = A_ik L_kk^-T for the row blocks i > k: one workgroup per row block, one thread per row
__global__ __launch_bounds__(kPgNB) void pg_trsm_kernel(double* __restrict__ L, size_t M, int k) {
  __shared__ double D[kPgNB * kPgLds];
  __shared__ double X[kPgNB * kPgLds];
  const int t = threadIdx.x;
  const int i = k + 1 + blockIdx.x;
  const double* dk = L + (size_t)k * kPgNB * M + (size_t)k * kPgNB;
  double* ak = L + (size_t)i * kPgNB * M + (size_t)k * kPgNB;
  for (int r = 0; r < kPgNB; ++r) {
    D[r * kPgLds + t] = t <= r ? dk[(size_t)r * M + t] : 0.0;
    X[r * kPgLds + t] = ak[(size_t)r * M + t];
  }
  __syncthreads();
  double* x = X + t * kPgLds;  // row t: x L_kk^T = a, column by column
  for (int j = 0; j < kPgNB; ++j) {
    double s = x[j];
    for (int l = 0; l < j; ++l) s -= x[l] * D[j * kPgLds + l];
    x[j] = s / D[j * kPgLds + j];
  }
  __syncthreads();
  for (int r = 0; r < kPgNB; ++r) ak[(size_t)r * M + t] = X[r * kPgLds + t];
}

typedef double pg_d4 __attribute__((ext_vector_type(4)));

// trailing update of column block k: L_ij -= L_ik L_jk^T for k < j <= i; four waves, wave w owns rows 16w..16w+15 of the tile
__global__ __launch_bounds__(256) void pg_syrk_kernel(double* __restrict__ L, size_t M, int k) {
  const int i = k + 1 + blockIdx.y, j = k + 1 + blockIdx.x;
  if (j > i) return;
  __shared__ double Ai[kPgNB * kPgLds];
  __shared__ double Aj[kPgNB * kPgLds];
  const int t = threadIdx.x;
  const double* pi = L + (size_t)i * kPgNB * M + (size_t)k * kPgNB;
  const double* pj = L + (size_t)j * kPgNB * M + (size_t)k * kPgNB;
  for (int e = t; e < kPgNB * kPgNB; e += 256) {
    const int r = e / kPgNB, c = e % kPgNB;
    Ai[r * kPgLds + c] = pi[(size_t)r * M + c];
    Aj[r * kPgLds + c] = pj[(size_t)r * M + c];
  }
  __syncthreads();
  const int w = t >> 6, lane = t & 63;
  const int lr = lane & 15, lk = lane >> 4;
  pg_d4 acc[4];
  for (int s = 0; s < 4; ++s) acc[s] = pg_d4{0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < kPgNB; kk += 4) {
    const double a = Ai[(16 * w + lr) * kPgLds + kk + lk];  // A[row = lane & 15][k = lane >> 4]
    for (int s = 0; s < 4; ++s) {
      const double bb = Aj[(16 * s + lr) * kPgLds + kk + lk];  // B[k = lane >> 4][col = lane & 15] = L_jk[col][k]
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[s], 0, 0, 0);
    }
  }
  double* out = L + (size_t)i * kPgNB * M + (size_t)j * kPgNB;
  for (int s = 0; s < 4; ++s)
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + lk + 4 * r, col = 16 * s + lr;
      out[(size_t)row * M + col] -= acc[s][r];
    }
}

// forward substitution, column block k: every workgroup solves y_k = L_kk^-1 b_k (the same arithmetic in each); workgroup 0 writes
// it, workgroup g > 0 then updates b_{k+g} -= L_{k+g,k} y_k
__global__ __launch_bounds__(kPgNB) void pg_fwd_kernel(const double* __restrict__ L, size_t M, int k, double* __restrict__ b,
                                                       double* __restrict__ y) {
  __shared__ double T[kPgNB * kPgLds];
  __shared__ double v[kPgNB];
  const int t = threadIdx.x;
  const double* dk = L + (size_t)k * kPgNB * M + (size_t)k * kPgNB;
  for (int r = 0; r < kPgNB; ++r) T[r * kPgLds + t] = dk[(size_t)r * M + t];
  v[t] = b[(size_t)k * kPgNB + t];
  __syncthreads();
  for (int j = 0; j < kPgNB; ++j) {
    if (t == j) v[j] = v[j] / T[j * kPgLds + j];
    __syncthreads();
    if (t > j) v[t] -= T[t * kPgLds + j] * v[j];
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    y[(size_t)k * kPgNB + t] = v[t];
    return;
  }
  const int i = k + blockIdx.x;
  const double* li = L + (size_t)i * kPgNB * M + (size_t)k * kPgNB;
  for (int r = 0; r < kPgNB; ++r) T[r * kPgLds + t] = li[(size_t)r * M + t];
  __syncthreads();
  double s = 0.0;
  for (int c = 0; c < kPgNB; ++c) s += T[t * kPgLds + c] * v[c];
  b[(size_t)i * kPgNB + t] -= s;
}

// back substitution, column block k (descending): x_k = L_kk^-T y_k; workgroup g > 0 updates y_{k-g} -= L_{k,k-g}^T x_k
__global__ __launch_bounds__(kPgNB) void pg_bwd_kernel(const double* __restrict__ L, size_t M, int k, double* __restrict__ y,
                                                       double* __restrict__ x) {
  __shared__ double T[kPgNB * kPgLds];
  __shared__ double v[kPgNB];
  const int t = threadIdx.x;
  const double* dk = L + (size_t)k * kPgNB * M + (size_t)k * kPgNB;
  for (int r = 0; r < kPgNB; ++r) T[r * kPgLds + t] = dk[(size_t)r * M + t];
  v[t] = y[(size_t)k * kPgNB + t];
  __syncthreads();
  for (int j = kPgNB - 1; j >= 0; --j) {
    if (t == j) v[j] = v[j] / T[j * kPgLds + j];
    __syncthreads();
    if (t < j) v[t] -= T[j * kPgLds + t] * v[j];
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    x[(size_t)k * kPgNB + t] = v[t];
    return;
  }
  const int i = k - blockIdx.x;
  const double* lk = L + (size_t)k * kPgNB * M + (size_t)i * kPgNB;
  for (int r = 0; r < kPgNB; ++r) T[r * kPgLds + t] = lk[(size_t)r * M + t];
  __syncthreads();
  double s = 0.0;
  for (int r = 0; r < kPgNB; ++r) s += T[r * kPgLds + t] * v[r];
  y[(size_t)i * kPgNB + t] -= s;
}

// ---- the step's update and its sums -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pg_update_kernel(const double* __restrict__ poses, const double* __restrict__ delta,
                                                       const double* __restrict__ b, double lambda, int n_nodes,
                                                       double* __restrict__ poses_new, double* __restrict__ part /* n x 3 */) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const double* d = delta + (size_t)6 * i;
  double T[16];
  pg_load_rowmajor(poses + (size_t)i * 16, T);
  // |x_i|^2, x = TransformMatrix4dToVector6d(T_i)
  double xv[6];
  const double sy = sqrt(T[0] * T[0] + T[4] * T[4]);
  if (!(sy < 1e-6)) {
    xv[0] = atan2(T[9], T[10]);
    xv[1] = atan2(-T[8], sy);
    xv[2] = atan2(T[4], T[0]);
  } else {
    xv[0] = atan2(-T[6], T[5]);
    xv[1] = atan2(-T[8], sy);
    xv[2] = 0.0;
  }
  xv[3] = T[3], xv[4] = T[7], xv[5] = T[11];
  double xn = 0.0, dn = 0.0, db = 0.0;
  for (int r = 0; r < 6; ++r) {
    xn += xv[r] * xv[r];
    dn += d[r] * d[r];
    db += d[r] * (lambda * d[r] + b[(size_t)6 * i + r]);
  }
  part[(size_t)i * 3 + 0] = dn;
  part[(size_t)i * 3 + 1] = xn;
  part[(size_t)i * 3 + 2] = db;
  // D = [Rz(g) Ry(b) Rx(a) | t], new = D T
  const double ca = cos(d[0]), sa = sin(d[0]), cb = cos(d[1]), sb = sin(d[1]), cg = cos(d[2]), sg = sin(d[2]);
  const double Rzy[9] = {cg * cb, -sg, cg * sb, sg * cb, cg, sg * sb, -sb, 0.0, cb};  // Rz Ry
  const double Rx[9] = {1.0, 0.0, 0.0, 0.0, ca, -sa, 0.0, sa, ca};
  double D[16];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) D[r * 4 + c] = Rzy[r * 3 + 0] * Rx[0 * 3 + c] + Rzy[r * 3 + 1] * Rx[1 * 3 + c] + Rzy[r * 3 + 2] * Rx[2 * 3 + c];
  D[3] = d[3], D[7] = d[4], D[11] = d[5];
  D[12] = D[13] = D[14] = 0.0, D[15] = 1.0;
  double N[16];
  pg_mul4(D, T, N);
  double* o = poses_new + (size_t)i * 16;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) o[c * 4 + r] = N[r * 4 + c];
}

constexpr int kPgRed = 1024;
// one workgroup: residual = sum of rterm, valid = count, sums of the node parts (part may be null), max(b[0, m)), max diag(H[0, m))
__global__ __launch_bounds__(kPgRed) void pg_reduce_kernel(const double* __restrict__ eout, int n_edges, const double* __restrict__ part,
                                                           int n_nodes, const double* __restrict__ b, const double* __restrict__ H,
                                                           size_t ld, int m, PgRecord* __restrict__ rec) {
  __shared__ double s0[kPgRed], s1[kPgRed], s2[kPgRed], s3[kPgRed], s4[kPgRed], s5[kPgRed], s6[kPgRed];
  const int t = threadIdx.x;
  double res = 0.0, val = 0.0, dn = 0.0, xn = 0.0, db = 0.0, mb = -INFINITY, md = -INFINITY;
  for (int k = t; k < n_edges; k += kPgRed) {
    res += eout[(size_t)k * kPgEdgeOut + 48];
    val += eout[(size_t)k * kPgEdgeOut + 50];
  }
  if (part)
    for (int k = t; k < n_nodes; k += kPgRed) {
      dn += part[(size_t)k * 3 + 0];
      xn += part[(size_t)k * 3 + 1];
      db += part[(size_t)k * 3 + 2];
    }
  for (int k = t; k < m; k += kPgRed) {
    mb = fmax(mb, b[k]);
    if (H) md = fmax(md, H[(size_t)k * ld + k]);
  }
  s0[t] = res, s1[t] = val, s2[t] = dn, s3[t] = xn, s4[t] = db, s5[t] = mb, s6[t] = md;
  __syncthreads();
  for (int w = kPgRed / 2; w > 0; w >>= 1) {
    if (t < w) {
      s0[t] += s0[t + w], s1[t] += s1[t + w], s2[t] += s2[t + w], s3[t] += s3[t + w], s4[t] += s4[t + w];
      s5[t] = fmax(s5[t], s5[t + w]), s6[t] = fmax(s6[t], s6[t + w]);
    }
    __syncthreads();
  }
  if (t == 0) {
    rec->residual = s0[0];
    rec->valid = (int)s1[0];
    rec->dn2 = s2[0];
    rec->xn2 = s3[0];
    rec->ddb = s4[0];
    rec->maxb = s5[0];
    rec->maxdiag = s6[0];
  }
}

#pragma clang fp contract(on)

}  // namespace o3ds
