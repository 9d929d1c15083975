// robust_icp_kernels.hpp -- [O3D] robust loss kernels (pipelines::registration::RobustKernel of Open3D v0.15.1: L2, L1, Huber, Cauchy,
// GM, Tukey) on the point-to-plane and the coloured estimator of the coloured-ICP family: the WEIGHTED normal equations of one
// correspondence pass (TransformationEstimationPointToPlane / ForColoredICP ::ComputeTransformation with a kernel, up to the solve).
//
// The result is DEFINED in include/o3ds_backend.h (o3ds_robust_icp_step) without reference to this kernel; tests/robust_icp_restatement.py
// is the same text in numpy.  Arithmetic, correspondences and sum order are the coloured step's (colored_icp_kernels.hpp): f64 on stored
// values widened, every operation rounded on its own, blocks of 256 queries, the halving tree inside a block, the block sums folded by
// colored_finish_kernel.  What is new is per pair: a residual's weight multiplies its row's products before the two rows meet.
//
//   robust_step_kernel   one workgroup per block of 256 queries, one query per thread.  The estimator is a template parameter (the
//                        point-to-plane form loads neither colours nor gradients), the loss a uniform argument: one branch per
//                        weight that every lane of the launch takes alike.
#pragma once
#include "colored_icp_kernels.hpp"

namespace o3ds {

struct RobustLossDev {
  int kind;  // o3ds_loss_kind, validated by the host
  double k;
};

// [O3D] RobustKernel.cpp, <Loss>::Weight(residual); the comparisons as written there, so a NaN residual takes what they give
__device__ __forceinline__ double robust_weight(RobustLossDev loss, double r) {
#pragma clang fp contract(off)
  const double e = fabs(r), k = loss.k;
  switch (loss.kind) {
    case O3DS_LOSS_L1:
      return r == 0.0 ? 1.0 : 1.0 / e;  // (DEPARTURE, o3ds_backend.h: Open3D divides by zero)
    case O3DS_LOSS_HUBER:
      return e > k ? k / e : 1.0;
    case O3DS_LOSS_CAUCHY: {
      const double u = r / k;
      return 1.0 / (1.0 + u * u);
    }
    case O3DS_LOSS_GM: {
      const double d = k + r * r;
      return k / (d * d);
    }
    case O3DS_LOSS_TUKEY: {
      const double q = e / k;
      const double u = q < 1.0 ? q : 1.0;
      const double v = 1.0 - u * u;
      return v * v;
    }
    default:
      return 1.0;  // O3DS_LOSS_L2
  }
}

// the halving tree of the sum order over a block's 256 queries, v[t] = v[t] + v[t + s] for s = 128 .. 1: the two upper levels cross
// wavefronts through LDS, the lower six lanes by shuffles; thread 0 writes the block's row
__device__ __forceinline__ void robust_block_tree(double (&v)[kColTerms], double (*s_v)[kColStepBlock / 2], int t, double* __restrict__ out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = kColStepBlock / 2; s >= 64; s >>= 1) {
    if (t >= s && t < 2 * s) {
#pragma unroll
      for (int k = 0; k < kColTerms; ++k) s_v[k][t - s] = v[k];
    }
    __syncthreads();
    if (t < s) {
#pragma unroll
      for (int k = 0; k < kColTerms; ++k) v[k] = v[k] + s_v[k][t];
    }
    if (s > 64) __syncthreads();  // (the next level writes rows this level still reads)
  }
  if (t >= 64) return;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) v[k] = v[k] + __shfl_down(v[k], s, 64);  // (lanes >= s hold values nobody reads again)
  }
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < kColTerms; ++k) out[k] = v[k];
    out[30] = 0.0;
    out[31] = 0.0;
  }
}

// nn_idx / nn_cnt / nn_d2: the search's Hybrid lists with max_nn = 1 of the queries storage(T s) in the target.  Colored = false:
// scol, tcol and tgrad are not read (and may be null), sg and sp are ignored.
template <typename P4, bool Colored>
__global__ __launch_bounds__(kColStepBlock) void robust_step_kernel(const P4* __restrict__ spts, const P4* __restrict__ scol, size_t ns, Mat34 M,
                                                                    const P4* __restrict__ tpts, const P4* __restrict__ tnrm, const P4* __restrict__ tcol,
                                                                    const double* __restrict__ tgrad, size_t nt, const uint32_t* __restrict__ nn_idx,
                                                                    const uint32_t* __restrict__ nn_cnt, const double* __restrict__ nn_d2, double sg, double sp,
                                                                    RobustLossDev loss, double* __restrict__ partial /* [gridDim.x][kRec] */) {
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
    const double dn = col_dot(px - qx, py - qy, pz - qz, nx, ny, nz);
    double jg[6];
    jg[0] = py * nz - pz * ny;
    jg[1] = pz * nx - px * nz;
    jg[2] = px * ny - py * nx;
    jg[3] = nx;
    jg[4] = ny;
    jg[5] = nz;
    if constexpr (Colored) {
      const double gx = tgrad[3 * j], gy = tgrad[3 * j + 1], gz = tgrad[3 * j + 2];
      const double Is = col_intensity(scol[i]), It = col_intensity(tcol[j]);
#pragma unroll
      for (int r = 0; r < 6; ++r) jg[r] = sg * jg[r];
      const double rg = sg * dn;
      const double ux = px - dn * nx, uy = py - dn * ny, uz = pz - dn * nz;  // p'
      const double I0 = col_dot(gx, gy, gz, ux - qx, uy - qy, uz - qz) + It;
      const double gn = col_dot(gx, gy, gz, nx, ny, nz);
      const double mx = gn * nx - gx, my = gn * ny - gy, mz = gn * nz - gz;  // g_M
      double ji[6];
      ji[0] = sp * (py * mz - pz * my);
      ji[1] = sp * (pz * mx - px * mz);
      ji[2] = sp * (px * my - py * mx);
      ji[3] = sp * mx;
      ji[4] = sp * my;
      ji[5] = sp * mz;
      const double ri = sp * (Is - I0);
      const double wg = robust_weight(loss, rg), wi = robust_weight(loss, ri);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[k++] = wg * (jg[r] * jg[c]) + wi * (ji[r] * ji[c]);
#pragma unroll
      for (int r = 0; r < 6; ++r) v[21 + r] = wg * (jg[r] * rg) + wi * (ji[r] * ri);
      v[kRecR2] = rg * rg + ri * ri;  // unweighted, as [O3D] ComputeJTJandJTr's r2 sum
    } else {
      const double w = robust_weight(loss, dn);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[k++] = w * (jg[r] * jg[c]);
#pragma unroll
      for (int r = 0; r < 6; ++r) v[21 + r] = w * (jg[r] * dn);
      v[kRecR2] = dn * dn;
    }
    v[kRecCount] = 1.0;
    v[kRecD2] = nn_d2[i];
  }
  robust_block_tree(v, s_v, t, partial + (size_t)blockIdx.x * kRec);
}

}  // namespace o3ds
