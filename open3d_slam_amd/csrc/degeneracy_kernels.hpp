// degeneracy_kernels.hpp -- degeneracy-aware ICP on the step-loop family (Zhang, Kaess, Singh, "On degeneracy of optimization-based
// state estimation", ICRA 2016: solution remapping; Tuna et al., X-ICP, 2022: rotation and translation analysed apart): which directions
// the normal equations of one pass leave unconstrained, and the update solved in the others only.
//
// The result is DEFINED in include/o3ds_backend.h (the degeneracy section) without reference to this kernel; tests/degeneracy_restatement.py
// is the same text in numpy.  All arithmetic is f64, every operation rounded on its own (contraction off); every 6x6 product is the dense
// one, sum_k P[i][k] Q[k][j] from k = 0 upwards starting with the first product, zeros included.
//
//   icp_degeneracy_update_kernel   one workgroup of 128, in the place of icp_update_kernel: the analysis of the pass's record under the
//                                  pose it ran under, published into DegeneracyDev; then the tail every step loop runs (icp_step_block:
//                                  convergence test, solve6_wave, T <- U T) -- on the ORIGINAL record when no direction is degenerate
//                                  (the bits of icp_update_kernel), otherwise on the unit system whose solution is the constrained x.
// The 6x6 matrices live in LDS, one entry per lane of the first 36; the two 3x3 eigen-decompositions run side by side in lanes 0 and 1
// on statically indexed registers (no scratch).
#pragma once
#include "icp_kernels.hpp"

namespace o3ds {

struct DegeneracyDev {
  double centre[3];         // c = T c0 of the last pass
  double eigenvalues[6];    // normalised, of the last pass
  double eigenvectors[36];  // V, row-major
  double x[6];              // the update the last pass solved
  int degenerate[6];
  int n_degenerate;
  int ever_degenerate[6];  // OR over the passes whose update was applied
  int n_passes_constrained;
};

constexpr int kDegSweeps = 8;  // cyclic Jacobi sweeps over (0,1), (0,2), (1,2): a 3x3 is at rounding level after five

// one Jacobi rotation on the pair (p, q); r is the third index.  app, aqq, apq: the pair's entries; arp, arq: the third row's; v*: the
// two columns of the vector matrix
__device__ __forceinline__ void deg_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                           double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  double p = arp, q = arq;
  arp = c * p - s * q;
  arq = s * p + c * q;
  p = v0p, q = v0q;
  v0p = c * p - s * q;
  v0q = s * p + c * q;
  p = v1p, q = v1q;
  v1p = c * p - s * q;
  v1q = s * p + c * q;
  p = v2p, q = v2q;
  v2p = c * p - s * q;
  v2q = s * p + c * q;
}

// exchange of two eigenpairs when the first value is the larger (strictly)
__device__ __forceinline__ void deg_order(double& la, double& lb, double& a0, double& a1, double& a2, double& b0, double& b1, double& b2) {
  if (la > lb) {
    double t = la;
    la = lb, lb = t;
    t = a0, a0 = b0, b0 = t;
    t = a1, a1 = b1, b1 = t;
    t = a2, a2 = b2, b2 = t;
  }
}

// the sign of a vector: its component of largest magnitude (the first of equals) is not negative
__device__ __forceinline__ void deg_sign(double& v0, double& v1, double& v2) {
  double big = v0;
  if (fabs(v1) > fabs(big)) big = v1;
  if (fabs(v2) > fabs(big)) big = v2;
  if (big < 0.0) v0 = -v0, v1 = -v1, v2 = -v2;
}

// eigenvalues ascending and eigenvectors (columns) of the symmetric 3x3 whose upper triangle sits at S[o..o+2][o..o+2] of a 6x6 in LDS;
// the vectors go to the same block of V, the raw values to lam[o..o+2]
__device__ __forceinline__ void deg_eigen3(const double* S, int o, double* V, double* lam) {
#pragma clang fp contract(off)
  double a00 = S[o * 6 + o], a01 = S[o * 6 + o + 1], a02 = S[o * 6 + o + 2];
  double a11 = S[(o + 1) * 6 + o + 1], a12 = S[(o + 1) * 6 + o + 2], a22 = S[(o + 2) * 6 + o + 2];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < kDegSweeps; ++sweep) {
    deg_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    deg_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    deg_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  deg_order(a00, a11, v00, v10, v20, v01, v11, v21);
  deg_order(a11, a22, v01, v11, v21, v02, v12, v22);
  deg_order(a00, a11, v00, v10, v20, v01, v11, v21);
  deg_sign(v00, v10, v20);
  deg_sign(v01, v11, v21);
  deg_sign(v02, v12, v22);
  lam[o] = a00, lam[o + 1] = a11, lam[o + 2] = a22;
  V[o * 6 + o] = v00, V[o * 6 + o + 1] = v01, V[o * 6 + o + 2] = v02;
  V[(o + 1) * 6 + o] = v10, V[(o + 1) * 6 + o + 1] = v11, V[(o + 1) * 6 + o + 2] = v12;
  V[(o + 2) * 6 + o] = v20, V[(o + 2) * 6 + o + 1] = v21, V[(o + 2) * 6 + o + 2] = v22;
}

// entry (r, c), r <= c, of the packed upper triangle of a record
__device__ __forceinline__ int deg_packed(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }

// c0: the centre of the source as stored (center_finish_kernel's three doubles).  `dg` is next to the state; its ever_degenerate and
// n_passes_constrained accumulate over a loop, everything else is of this pass.
__global__ __launch_bounds__(128) void icp_degeneracy_update_kernel(const double* __restrict__ record, IcpStateDev* state, DegeneracyDev* dg,
                                                                    const double* __restrict__ c0, double min_rot, double min_trans,
                                                                    unsigned long long n_src_total, int max_iter, double rel_fitness, double rel_rmse) {
#pragma clang fp contract(off)
  if (state->done) return;
  __shared__ double s_out[kRec], s_rec[kRec];
  __shared__ double s_x[8], s_sc[8], s_U[16];
  __shared__ int s_go;
  __shared__ double s_H[36], s_M[36], s_W[36], s_Hc[36], s_V[36], s_A[36];
  __shared__ double s_g[6], s_gc[6], s_b[6], s_y[8], s_xc[6], s_lam[6], s_c[3];
  __shared__ int s_deg[6];
  const int t = threadIdx.x;
  const int i = t / 6, j = t - 6 * i;  // t < 36: the entry this lane owns
  if (t < kRec) s_out[t] = record[t];
  if (t < 3) {
    const double* T = state->T;  // column-major; the pose the pass ran under
    s_c[t] = ((T[t] * c0[0] + T[4 + t] * c0[1]) + T[8 + t] * c0[2]) + T[12 + t];
  }
  __syncthreads();
  if (t < 36) {
    s_H[t] = s_out[deg_packed(min(i, j), max(i, j))];
    double m = i == j ? 1.0 : 0.0;  // M = [[I, 0], [[c]x, I]]
    if (i >= 3 && j < 3 && i - 3 != j) {
      const int a = i - 3;
      const int k = 3 - a - j;  // the third axis
      m = (j == (a + 1) % 3) ? -s_c[k] : s_c[k];
    }
    s_M[t] = m;
    s_V[t] = 0.0;
  }
  if (t < 6) s_g[t] = -s_out[21 + t];
  __syncthreads();
  if (t < 36) {  // W = H M
    double s = s_H[i * 6] * s_M[j];
    for (int k = 1; k < 6; ++k) s = s + s_H[i * 6 + k] * s_M[k * 6 + j];
    s_W[t] = s;
  }
  if (t < 6) {  // g_c = M^T g
    double s = s_M[t] * s_g[0];
    for (int k = 1; k < 6; ++k) s = s + s_M[k * 6 + t] * s_g[k];
    s_gc[t] = s;
  }
  __syncthreads();
  if (t < 36) {  // H_c = M^T W; what follows reads its upper triangle
    double s = s_M[i] * s_W[j];
    for (int k = 1; k < 6; ++k) s = s + s_M[k * 6 + i] * s_W[k * 6 + j];
    s_Hc[t] = s;
  }
  __syncthreads();
  if (t < 2) deg_eigen3(s_Hc, 3 * t, s_V, s_lam);
  __syncthreads();
  const double n_corr = s_out[kRecCount];
  if (t < 6) {
    const double lh = n_corr > 0.0 ? s_lam[t] / n_corr : 0.0;
    s_deg[t] = n_corr > 0.0 ? (lh < (t < 3 ? min_rot : min_trans) ? 1 : 0) : 1;
    dg->eigenvalues[t] = lh;
    dg->degenerate[t] = s_deg[t];
  }
  if (t < 36) dg->eigenvectors[t] = s_V[t];
  if (t < 3) dg->centre[t] = s_c[t];
  __syncthreads();
  const int n_deg = s_deg[0] + s_deg[1] + s_deg[2] + s_deg[3] + s_deg[4] + s_deg[5];  // uniform
  if (t == 0) dg->n_degenerate = n_deg;
  const double* rec = s_out;
  if (n_deg > 0) {
    if (t < 36) {  // W = H_c V, H_c symmetric from its upper triangle
      double s = s_Hc[i] * s_V[j];
      for (int k = 1; k < 6; ++k) s = s + s_Hc[min(i, k) * 6 + max(i, k)] * s_V[k * 6 + j];
      s_W[t] = s;
    }
    if (t < 6) {  // b = V^T g_c
      double s = s_V[t] * s_gc[0];
      for (int k = 1; k < 6; ++k) s = s + s_V[k * 6 + t] * s_gc[k];
      s_b[t] = s;
    }
    __syncthreads();
    if (t < 36) {  // A = V^T W
      double s = s_V[i] * s_W[j];
      for (int k = 1; k < 6; ++k) s = s + s_V[k * 6 + i] * s_W[k * 6 + j];
      s_A[t] = s;
    }
    if (t < kRec) s_rec[t] = 0.0;
    __syncthreads();
    // the system with the degenerate rows and columns replaced by those of the unit matrix, in the record's form (its [21..26] is -b)
    if (t < 36 && i <= j) s_rec[deg_packed(i, j)] = (s_deg[i] || s_deg[j]) ? (i == j ? 1.0 : 0.0) : s_A[t];
    if (t >= 64 && t < 70) s_rec[21 + t - 64] = s_deg[t - 64] ? -0.0 : -s_b[t - 64];
    __syncthreads();
    if (t < 64) solve6_wave(s_rec, s_y, t);
    __syncthreads();
    if (t < 6) {  // x_c = V y
      double s = s_V[t * 6] * s_y[0];
      for (int k = 1; k < 6; ++k) s = s + s_V[t * 6 + k] * s_y[k];
      s_xc[t] = s;
    }
    __syncthreads();
    // x = M x_c, and the unit system whose solution it is: what the shared tail composes is exactly x (products with 0 and 1 are exact;
    // + 0.0 makes a zero positive, which the unit solve would do anyway)
    if (t < kRec) s_rec[t] = (t == 0 || t == 6 || t == 11 || t == 15 || t == 18 || t == 20) ? 1.0 : 0.0;
    __syncthreads();
    if (t < 6) {
      double s = s_M[t * 6] * s_xc[0];
      for (int k = 1; k < 6; ++k) s = s + s_M[t * 6 + k] * s_xc[k];
      s_rec[21 + t] = -(s + 0.0);
    }
    if (t == kRecCount || t == kRecD2) s_rec[t] = s_out[t];
    __syncthreads();
    rec = s_rec;
  }
  icp_step_block(rec, state, n_src_total, max_iter, rel_fitness, rel_rmse, s_x, s_sc, s_U, &s_go, nullptr, O3DS_ICP_POINT_TO_PLANE, nullptr, false,
                 nullptr, 0);
  // (s_x and s_go were written in front of the tail's barrier)
  if (t < 6) {
    dg->x[t] = s_x[t];
    if (s_go && s_deg[t]) dg->ever_degenerate[t] = 1;
  }
  if (t == 0 && s_go && n_deg > 0) dg->n_passes_constrained += 1;
}

}  // namespace o3ds
