// ndt_kernels.hpp -- search-free registration against voxel Gaussians: the normal-distributions transform (Biber and Strasser 2003;
// Magnusson 2009) in the voxelised form of Koide et al. (VGICP, 2021).  The target is summarised ONCE as one Gaussian per voxel of a
// world-anchored grid; a pass then costs, per source point, a voxel key, a lookup and one or seven 3x3 quadratic forms -- no neighbour
// search.  The pass leaves the 32-double record of the step-loop family, so the solve / update tail (icp_update_kernel) is unchanged.
//
// Both results are DEFINED in include/o3ds_backend.h (the voxel-Gaussian section) without reference to these kernels;
// tests/ndt_restatement.py is the same text in numpy.  All arithmetic is f64 on stored values widened, every operation rounded on its
// own (contraction off), every sum in the one order the header states.
//
//   ndt_key_kernel      the voxel key of every point (key_world's rounding), kNdtNoVoxel for a point that belongs to none; the stable
//                       sort of (key, index) then yields every voxel's members in ascending original index
//   ndt_inside_kernel   where the points without a voxel begin in the sorted list (one thread, a binary search)
//   ndt_stats_kernel    one thread per voxel: mean, covariance, the 3x3 Jacobi of degeneracy_kernels.hpp on registers, the clamped
//                       inverse; the arrays a download returns and the 80-byte record the step reads
//   ndt_step_kernel     one lane per query, 256 per block: the lookup is a binary search over the sorted keys (no result depends on
//                       it), a found voxel is five 16-byte loads; the block tree and the fold are the robust step's
#pragma once
#include "degeneracy_kernels.hpp"
#include "robust_icp_kernels.hpp"

namespace o3ds {

constexpr unsigned long long kNdtNoVoxel = ~0ull;  // above every packed key (63 bits): such points sort behind every voxel
constexpr double kNdtKeyLimit = 1048576.0;         // 2^20: pack_key holds |k| < 2^20 per axis

// what a pass reads of a voxel: one aligned record, five 16-byte loads
struct alignas(16) NdtVoxel {
  double mu[3];
  double B[6];  // upper triangle, row-major: 00 01 02 11 12 22
  double valid; // 1.0 or 0.0
};
static_assert(sizeof(NdtVoxel) == 80, "five double2 loads");

// k = floor(x inv) of one axis; false: the coordinate belongs to no voxel (not finite, or |k| >= 2^20)
__device__ __forceinline__ bool ndt_coord(double x, double inv, long long& k) {
#pragma clang fp contract(off)
  const double f = floor(x * inv);
  if (!(fabs(f) < kNdtKeyLimit)) return false;  // (a NaN compares false)
  k = (long long)f;
  return true;
}

template <typename P4>
__global__ __launch_bounds__(kBlock) void ndt_key_kernel(const P4* __restrict__ pts, size_t n, double voxel, unsigned long long* __restrict__ keys,
                                                         uint32_t* __restrict__ vals) {
#pragma clang fp contract(off)
  const double inv = 1.0 / voxel;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const P4 p = pts[i];
    long long kx = 0, ky = 0, kz = 0;
    const bool ok = ndt_coord((double)p.x, inv, kx) & ndt_coord((double)p.y, inv, ky) & ndt_coord((double)p.z, inv, kz);
    keys[i] = ok ? pack_key(kx, ky, kz) : kNdtNoVoxel;
    vals[i] = (uint32_t)i;
  }
}

// the number of sorted keys that are a voxel's
__global__ void ndt_inside_kernel(const unsigned long long* __restrict__ keys, size_t n, unsigned long long* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (keys[mid] == kNdtNoVoxel)
      hi = mid;
    else
      lo = mid + 1;
  }
  *out = lo;
}

// eigenvalues ascending and eigenvectors (columns) of the symmetric 3x3 (a00 .. a22, upper triangle): deg_eigen3's sweeps, order and sign
// rule on values that never leave registers
__device__ __forceinline__ void ndt_eigen3(double a00, double a01, double a02, double a11, double a12, double a22, double (&lam)[3], double (&V)[3][3]) {
#pragma clang fp contract(off)
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
  lam[0] = a00, lam[1] = a11, lam[2] = a22;
  V[0][0] = v00, V[0][1] = v01, V[0][2] = v02;
  V[1][0] = v10, V[1][1] = v11, V[1][2] = v12;
  V[2][0] = v20, V[2][1] = v21, V[2][2] = v22;
}

// skeys / svals: the sorted (key, original index) pairs; seg_start[v]: where voxel v begins in them; the last voxel ends at n_inside.
// counters: [0] valid voxels, [1] voxels with enough members whose largest eigenvalue is not finite or not > 0
template <typename P4>
__global__ __launch_bounds__(kBlock) void ndt_stats_kernel(const P4* __restrict__ pts, const unsigned long long* __restrict__ skeys,
                                                           const uint32_t* __restrict__ svals, const int* __restrict__ seg_start, size_t n_vox,
                                                           size_t n_inside, int min_points, double ratio, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ counts, double* __restrict__ mean, double* __restrict__ cov,
                                                           double* __restrict__ info, uint8_t* __restrict__ valid, NdtVoxel* __restrict__ rec,
                                                           unsigned int* __restrict__ counters) {
#pragma clang fp contract(off)
  const size_t v = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vox) return;
  const size_t lo = (size_t)seg_start[v], hi = v + 1 < n_vox ? (size_t)seg_start[v + 1] : n_inside;
  const size_t nv = hi - lo;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (size_t j = lo; j < hi; ++j) {
    const P4 p = pts[svals[j]];
    sx = sx + (double)p.x;
    sy = sy + (double)p.y;
    sz = sz + (double)p.z;
  }
  const double dn = (double)nv;
  const double mx = sx / dn, my = sy / dn, mz = sz / dn;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t j = lo; j < hi; ++j) {
    const P4 p = pts[svals[j]];
    const double rx = (double)p.x - mx, ry = (double)p.y - my, rz = (double)p.z - mz;
    c[0] = c[0] + rx * rx;
    c[1] = c[1] + rx * ry;
    c[2] = c[2] + rx * rz;
    c[3] = c[3] + ry * ry;
    c[4] = c[4] + ry * rz;
    c[5] = c[5] + rz * rz;
  }
  if (nv > 1) {  // (one member: the sums are +0.0 and stay)
    const double d = (double)(nv - 1);
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = c[k] / d;
  }
  double B[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = false;
  if (nv >= (size_t)min_points) {
    double lam[3], V[3][3];
    ndt_eigen3(c[0], c[1], c[2], c[3], c[4], c[5], lam, V);
    ok = isfinite(lam[2]) && lam[2] > 0.0;
    if (ok) {
      const double f = ratio * lam[2];
      const double l0 = lam[0] < f ? f : lam[0], l1 = lam[1] < f ? f : lam[1], l2 = lam[2] < f ? f : lam[2];
      int k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) B[k++] = ((V[a][0] * V[b][0]) / l0 + (V[a][1] * V[b][1]) / l1) + (V[a][2] * V[b][2]) / l2;
      atomicAdd(counters, 1u);
    } else {
      atomicAdd(counters + 1, 1u);
    }
  }
  keys[v] = skeys[lo];
  counts[v] = (uint32_t)nv;
  mean[3 * v] = mx, mean[3 * v + 1] = my, mean[3 * v + 2] = mz;
  NdtVoxel r;
  r.mu[0] = mx, r.mu[1] = my, r.mu[2] = mz;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    cov[6 * v + k] = c[k];
    info[6 * v + k] = B[k];
    r.B[k] = B[k];
  }
  valid[v] = ok ? 1 : 0;
  r.valid = ok ? 1.0 : 0.0;
  rec[v] = r;
}

// the position of `key` among the n_vox ascending keys, or n_vox
__device__ __forceinline__ size_t ndt_find(const unsigned long long* __restrict__ keys, size_t n_vox, unsigned long long key) {
  size_t lo = 0, hi = n_vox;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < n_vox && keys[lo] == key) ? lo : n_vox;
}

// n_off: 1 or 7 offsets of the neighbourhood, in the header's order.  partial: [gridDim.x][kRec]
template <typename P4>
__global__ __launch_bounds__(kColStepBlock) void ndt_step_kernel(const P4* __restrict__ spts, size_t ns, Mat34 M, double voxel,
                                                                 const unsigned long long* __restrict__ keys, const NdtVoxel* __restrict__ vox,
                                                                 size_t n_vox, int n_off, RobustLossDev loss, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_v[kColTerms][kColStepBlock / 2];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kColStepBlock + (size_t)t;
  double v[kColTerms];
#pragma unroll
  for (int k = 0; k < kColTerms; ++k) v[k] = 0.0;
  if (i < ns) {
    const double inv = 1.0 / voxel;
    const P4 s = spts[i];
    const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
    // the query in f64, not rounded to storage: no search has to agree with it
    const double px = ((M.m[0] * x + M.m[1] * y) + M.m[2] * z) + M.m[3];
    const double py = ((M.m[4] * x + M.m[5] * y) + M.m[6] * z) + M.m[7];
    const double pz = ((M.m[8] * x + M.m[9] * y) + M.m[10] * z) + M.m[11];
    long long kx = 0, ky = 0, kz = 0;
    if (ndt_coord(px, inv, kx) & ndt_coord(py, inv, ky) & ndt_coord(pz, inv, kz)) {
      // J = d(U p) / d(omega, t) of an update applied on the left: columns e_c x p, then the unit vectors; zeros take part in the products
      const double J[3][6] = {{0.0, pz, -py, 1.0, 0.0, 0.0}, {-pz, 0.0, px, 0.0, 1.0, 0.0}, {py, -px, 0.0, 0.0, 0.0, 1.0}};
      bool found = false;
      double best = 0.0;
#pragma unroll 1
      for (int o = 0; o < n_off; ++o) {
        const long long d = (o & 1) ? 1 : -1;  // offsets 1, 3, 5 step up, 2, 4, 6 down
        const int axis = (o + 1) >> 1;         // 0: the query's own voxel; 1, 2, 3: x, y, z
        const long long nx = kx + (axis == 1 ? d : 0), ny = ky + (axis == 2 ? d : 0), nz = kz + (axis == 3 ? d : 0);
        const long long lim = (1ll << 20);
        if (nx <= -lim || nx >= lim || ny <= -lim || ny >= lim || nz <= -lim || nz >= lim) continue;  // no point has such a voxel
        const size_t at = ndt_find(keys, n_vox, pack_key(nx, ny, nz));
        if (at >= n_vox) continue;
        const double2* r = reinterpret_cast<const double2*>(vox + at);
        const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
        if (r4.y == 0.0) continue;  // not valid
        const double B[3][3] = {{r1.y, r2.x, r2.y}, {r2.x, r3.x, r3.y}, {r2.y, r3.y, r4.x}};
        const double e0 = px - r0.x, e1 = py - r0.y, e2 = pz - r1.x;
        double u[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = (B[a][0] * e0 + B[a][1] * e1) + B[a][2] * e2;
        const double m = col_dot(e0, e1, e2, u[0], u[1], u[2]);
        const double res = m > 0.0 ? sqrt(m) : 0.0;
        const double w = robust_weight(loss, res);
        double G[3][6];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 6; ++c) G[a][c] = (B[a][0] * J[0][c] + B[a][1] * J[1][c]) + B[a][2] * J[2][c];
        int k = 0;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr)
#pragma unroll
          for (int c = rr; c < 6; ++c) {
            v[k] = v[k] + w * ((J[0][rr] * G[0][c] + J[1][rr] * G[1][c]) + J[2][rr] * G[2][c]);
            ++k;
          }
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) v[21 + rr] = v[21 + rr] + w * ((J[0][rr] * u[0] + J[1][rr] * u[1]) + J[2][rr] * u[2]);
        v[kRecR2] = v[kRecR2] + m;
        const double ee = col_dot(e0, e1, e2, e0, e1, e2);
        if (!found || ee < best) best = ee;  // the first of equals stays
        found = true;
      }
      if (found) {
        v[kRecCount] = 1.0;
        v[kRecD2] = best;
      }
    }
  }
  robust_block_tree(v, s_v, t, partial + (size_t)blockIdx.x * kRec);
}

}  // namespace o3ds
