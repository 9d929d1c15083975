// colored_icp_kernels.hpp -- [O3D] coloured ICP (Park, Zhou, Koltun 2017; pipelines::registration::RegistrationColoredICP of Open3D
// v0.15.1) on device clouds: the colour gradients of a target (InitializePointCloudForColoredICP) and the joint geometric + photometric
// normal equations of one correspondence pass (TransformationEstimationForColoredICP::ComputeTransformation up to its solve).
//
// Both results are DEFINED in include/o3ds_backend.h (o3ds_compute_color_gradients, o3ds_colored_icp_step) without reference to these
// kernels; tests/colored_icp_restatement.py is the same text in numpy.  All arithmetic is f64 on stored values widened, every
// operation rounded on its own (contraction off), every sum in the one order the header states.  The neighbour lists and the
// correspondences are the neighbour search's (neighbor_kernels.hpp): no second definition of a nearest neighbour lives here.
//
//   color_gradient_kernel   one thread per point reads its Hybrid list from the arrays the search left on the device
//   colored_step_kernel     one workgroup per block of 256 queries, one query per thread: its 30 terms stay in registers, the
//                           halving tree of a block crosses wavefronts through LDS (s = 128, 64) and lanes by shuffles (s = 32 .. 1)
//   colored_finish_kernel   the block sums added in ascending block order; one thread per record term
#pragma once
#include "cloud_kernels.hpp"
#include "common.hpp"

namespace o3ds {

constexpr int kColTerms = 30;       // record terms that are summed: [0..20] JtJ, [21..26] Jtr, [27] r^2, [28] #corr, [29] d2
constexpr int kColStepBlock = 256;  // queries per block of the sum order (o3ds_backend.h): NOT a tuning knob

__device__ __forceinline__ double col_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}
template <typename P4>
__device__ __forceinline__ double col_intensity(const P4& c) {
#pragma clang fp contract(off)
  return (((double)c.x + (double)c.y) + (double)c.z) / 3.0;
}

// ---------------------------------------------------------------------------------------------- gradients
// idx / cnt: the Hybrid lists of every point in its own cloud, max_nn entries per row (neighbor_kernel); grad: n x 3
template <typename P4>
__global__ __launch_bounds__(kBlock) void color_gradient_kernel(const P4* __restrict__ pts, const P4* __restrict__ nrm, const P4* __restrict__ col, size_t n,
                                                                const uint32_t* __restrict__ idx, const uint32_t* __restrict__ cnt, int max_nn,
                                                                double* __restrict__ grad) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  const uint32_t c = min(cnt[i], (uint32_t)max_nn);
  if (c >= 4u) {
    const P4 pp = pts[i], nn = nrm[i];
    const double px = (double)pp.x, py = (double)pp.y, pz = (double)pp.z;
    const double nx = (double)nn.x, ny = (double)nn.y, nz = (double)nn.z;
    const double I = col_intensity(col[i]);
    double m00 = 0.0, m10 = 0.0, m11 = 0.0, m20 = 0.0, m21 = 0.0, m22 = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
    const uint32_t* row = idx + i * (size_t)max_nn;
    for (uint32_t k = 1; k < c; ++k) {  // the first entry is skipped, whichever point it is
      size_t j = (size_t)row[k];
      if (j >= n) j = i;  // (never: the list holds indices of the cloud)
      const P4 q = pts[j];
      const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
      const double d = col_dot(qx - px, qy - py, qz - pz, nx, ny, nz);
      const double ax = (qx - d * nx) - px, ay = (qy - d * ny) - py, az = (qz - d * nz) - pz;
      const double b = col_intensity(col[j]) - I;
      m00 = m00 + ax * ax;
      m10 = m10 + ay * ax;
      m11 = m11 + ay * ay;
      m20 = m20 + az * ax;
      m21 = m21 + az * ay;
      m22 = m22 + az * az;
      v0 = v0 + ax * b;
      v1 = v1 + ay * b;
      v2 = v2 + az * b;
    }
    {  // the last row: a = (|L| - 1) n, b = 0
      const double w = (double)(c - 1u);
      const double ax = w * nx, ay = w * ny, az = w * nz;
      m00 = m00 + ax * ax;
      m10 = m10 + ay * ax;
      m11 = m11 + ay * ay;
      m20 = m20 + az * ax;
      m21 = m21 + az * ay;
      m22 = m22 + az * az;
      v0 = v0 + ax * 0.0;
      v1 = v1 + ay * 0.0;
      v2 = v2 + az * 0.0;
    }
    // unpivoted LDL^T, the operation order of the header
    const double d0 = m00;
    if (d0 > 0.0 && isfinite(d0)) {
      const double l10 = m10 / d0, l20 = m20 / d0;
      const double d1 = m11 - l10 * m10;
      if (d1 > 0.0 && isfinite(d1)) {
        const double w21 = m21 - l20 * m10;
        const double l21 = w21 / d1;
        const double d2 = (m22 - l20 * m20) - l21 * w21;
        if (d2 > 0.0 && isfinite(d2)) {
          const double y0 = v0;
          const double y1 = v1 - l10 * y0;
          const double y2 = (v2 - l20 * y0) - l21 * y1;
          gz = y2 / d2;
          gy = y1 / d1 - l21 * gz;
          gx = (y0 / d0 - l10 * gy) - l20 * gz;
        }
      }
    }
  }
  grad[3 * i] = gx;
  grad[3 * i + 1] = gy;
  grad[3 * i + 2] = gz;
}

// ---------------------------------------------------------------------------------------------- the joint step
// nn_idx / nn_cnt / nn_d2: the search's Hybrid lists with max_nn = 1 of the queries storage(T s) in the target (original target indices)
template <typename P4>
__global__ __launch_bounds__(kColStepBlock) void colored_step_kernel(const P4* __restrict__ spts, const P4* __restrict__ scol, size_t ns, Mat34 M,
                                                                     const P4* __restrict__ tpts, const P4* __restrict__ tnrm, const P4* __restrict__ tcol,
                                                                     const double* __restrict__ tgrad, size_t nt, const uint32_t* __restrict__ nn_idx,
                                                                     const uint32_t* __restrict__ nn_cnt, const double* __restrict__ nn_d2, double sg, double sp,
                                                                     double* __restrict__ partial /* [gridDim.x][kRec] */) {
#pragma clang fp contract(off)
  using R = typename Scalar<P4>::type;
  __shared__ double s_v[kColTerms][kColStepBlock / 2];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kColStepBlock + (size_t)t;
  double v[kColTerms];
#pragma unroll
  for (int k = 0; k < kColTerms; ++k) v[k] = 0.0;
  size_t j = 0;
  bool have = false;
  if (i < ns && nn_cnt[i] > 0u) {
    j = (size_t)nn_idx[i];
    have = j < nt;  // (always: the list holds indices of the target)
  }
  if (have) {
    const P4 s = spts[i];
    const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
    // the query as the search formed it: storage(T s), widened
    const double px = (double)(R)((M.m[0] * x + M.m[1] * y) + M.m[2] * z + M.m[3]);
    const double py = (double)(R)((M.m[4] * x + M.m[5] * y) + M.m[6] * z + M.m[7]);
    const double pz = (double)(R)((M.m[8] * x + M.m[9] * y) + M.m[10] * z + M.m[11]);
    const P4 q = tpts[j], nn = tnrm[j];
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const double nx = (double)nn.x, ny = (double)nn.y, nz = (double)nn.z;
    const double gx = tgrad[3 * j], gy = tgrad[3 * j + 1], gz = tgrad[3 * j + 2];
    const double Is = col_intensity(scol[i]), It = col_intensity(tcol[j]);
    // geometric row
    const double dn = col_dot(px - qx, py - qy, pz - qz, nx, ny, nz);
    double jg[6], ji[6];
    jg[0] = sg * (py * nz - pz * ny);
    jg[1] = sg * (pz * nx - px * nz);
    jg[2] = sg * (px * ny - py * nx);
    jg[3] = sg * nx;
    jg[4] = sg * ny;
    jg[5] = sg * nz;
    const double rg = sg * dn;
    // photometric row
    const double ux = px - dn * nx, uy = py - dn * ny, uz = pz - dn * nz;  // p'
    const double I0 = col_dot(gx, gy, gz, ux - qx, uy - qy, uz - qz) + It;
    const double gn = col_dot(gx, gy, gz, nx, ny, nz);
    const double mx = gn * nx - gx, my = gn * ny - gy, mz = gn * nz - gz;  // g_M
    ji[0] = sp * (py * mz - pz * my);
    ji[1] = sp * (pz * mx - px * mz);
    ji[2] = sp * (px * my - py * mx);
    ji[3] = sp * mx;
    ji[4] = sp * my;
    ji[5] = sp * mz;
    const double ri = sp * (Is - I0);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) v[k++] = jg[r] * jg[c] + ji[r] * ji[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = jg[r] * rg + ji[r] * ri;
    v[kRecR2] = rg * rg + ri * ri;
    v[kRecCount] = 1.0;
    v[kRecD2] = nn_d2[i];
  }
  // the halving tree over the block's 256 queries: v[t] = v[t] + v[t + s], s = 128 .. 1
  if (t >= 128) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) s_v[k][t - 128] = v[k];
  }
  __syncthreads();
  if (t < 128) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) v[k] = v[k] + s_v[k][t];
  }
  __syncthreads();
  if (t >= 64 && t < 128) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) s_v[k][t - 64] = v[k];
  }
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) v[k] = v[k] + s_v[k][t];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < kColTerms; ++k) v[k] = v[k] + __shfl_down(v[k], s, 64);  // (lanes >= s hold values nobody reads again)
    }
    if (t == 0) {
      double* out = partial + (size_t)blockIdx.x * kRec;
#pragma unroll
      for (int k = 0; k < kColTerms; ++k) out[k] = v[k];
      out[30] = 0.0;
      out[31] = 0.0;
    }
  }
}

// record[k] = the block sums of term k added in ascending block order onto +0.0
__global__ __launch_bounds__(64) void colored_finish_kernel(const double* __restrict__ partial, size_t nblocks, double* __restrict__ record) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  if (k >= kRec) return;
  double sum = 0.0;
  for (size_t b0 = 0; b0 < nblocks; b0 += 16) {  // (the rows come from memory: sixteen loads in flight before the first add)
    double x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = b0 + u < nblocks ? partial[(b0 + u) * kRec + k] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (b0 + u < nblocks) sum = sum + x[u];
  }
  record[k] = k < kColTerms ? sum : 0.0;
}

}  // namespace o3ds
