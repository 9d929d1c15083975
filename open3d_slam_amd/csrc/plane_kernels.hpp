// plane_kernels.hpp -- [O3D] PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations) on a device cloud and the split of the
// cloud by the plane found (o3ds_segment_plane).
//
// The result is defined in include/o3ds_backend.h without reference to this file (tests/plane_restatement.py is the same text in numpy):
// the seeded draw of o3ds_ransac_feature_matching, Open3D's triangle plane and GetPlaneFromPoints, its evaluation by the SUM of the
// inliers' distances, the serial winner rule, the refit on the winner's inliers.  All of it is f64 with contraction off, and every sum
// over points is taken in ONE order that depends on the number of terms m alone (plane_chunk_len): kPlaneChunks contiguous chunks of
// len = max(1, ceil(m / kPlaneChunks)) terms, each added up one term after the other from +0.0, then a halving tree over the chunk sums.
//
// Why this order: the work is dense -- every hypothesis against every point, 6.6e7 tests for a 65 536-point scan and 1 000 planes -- and
// the sequential chunk is what lets the hot kernel run with no reduction across lanes at all.  plane_eval_kernel gives each LANE of a
// wavefront one hypothesis: its four coefficients, its count and its error stay in registers; the wavefront walks one chunk of points,
// every lane reading the SAME point, so the address is uniform, the compiler fetches the points through the scalar cache (eight points'
// loads issued together, one wait) and the loop is 11.5 VALU instructions per point for 64 tests in f64 storage, 14.5 in f32 storage (the
// three conversions).  The grid is (groups of 64 hypotheses) x (kPlaneChunks chunks); the partials [chunk][hypothesis] go through the
// halving tree in plane_finish_kernel, one workgroup per eight hypotheses.
//
// A batch of at most kPlaneBatch hypotheses is four launches: plane_hypothesis_kernel (one thread per hypothesis: draw and fit),
// plane_eval_kernel, plane_finish_kernel (count, error -> fitness, inlier_rmse) and plane_fold_kernel, one workgroup that reduces the
// batch under the serial rule -- "better" is the strict order (fitness greater, or equal and inlier_rmse smaller), ties to the lower
// index, which is what reading the hypotheses one by one keeps -- and then holds the batch's best against the best so far, strictly, so
// the winner is the serial rule's whatever the batch size.  Nothing returns to the host between batches.
//
// Afterwards: plane_mask_kernel (the inlier flags and their complement), plane_sums_kernel twice (centroid, then the six moments about
// it; one wavefront per chunk, uniform and sequential, so the order is the documented one) each followed by plane_sums_finish_kernel
// (the tree; the second one fits the plane), and the filters' scan and compaction on the flags and on their complement.
#pragma once
#include "feature_kernels.hpp"

namespace o3ds {

// (Every kernel here is a template, the small ones of a parameter nobody sets, and backend.hip uses them last: see cluster_kernels.hpp.)
constexpr int kPlaneChunks = 256;  // chunks of the sum order (part of the definition: the header states it)
constexpr int kPlaneBatch = 1024;  // hypotheses per batch (no result depends on it)
constexpr int kPlaneFinishHyps = 8;  // hypotheses per workgroup of plane_finish_kernel
constexpr int kPlaneEvalUnroll = 8;  // points whose scalar loads plane_eval_kernel issues together
static_assert(kPlaneChunks == kBlock, "the finish kernels give one chunk to each thread");
static_assert(kPlaneBatch % 64 == 0 && kPlaneBatch % kPlaneFinishHyps == 0, "whole wavefronts and whole finish groups");

struct PlaneState {
  double best_plane[4], plane[4];
  double fitness, rmse;
  double centroid[3];
  unsigned long long n_inliers;
  long long best_t, n_degenerate;
};

__host__ __device__ __forceinline__ size_t plane_chunk_len(size_t m) {
  const size_t len = (m + kPlaneChunks - 1) / kPlaneChunks;
  return len ? len : 1;
}

#pragma clang fp contract(off)  // every product and sum rounds on its own, as the definition says

// [O3D] GetPlaneFromPoints from the centroid and the six moments about it
__device__ __forceinline__ void plane_from_moments(double cx, double cy, double cz, double xx, double xy, double xz, double yy, double yz, double zz,
                                                   double out[4]) {
  const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
  double a, b, c;
  if (det_x >= det_y && det_x >= det_z) {
    a = det_x, b = xz * yz - xy * zz, c = xy * yz - xz * yy;
  } else if (det_y >= det_z) {
    a = xz * yz - xy * zz, b = det_y, c = xy * xz - yz * xx;
  } else {
    a = xy * yz - xz * yy, b = xy * xz - yz * xx, c = det_z;
  }
  const double norm = sqrt((a * a + b * b) + c * c);
  if (norm == 0.0) {
    out[0] = out[1] = out[2] = out[3] = 0.0;
    return;
  }
  a /= norm, b /= norm, c /= norm;
  out[0] = a, out[1] = b, out[2] = c;
  out[3] = -((a * cx + b * cy) + c * cz);
}

// the documented order for m <= 8 terms: chunks of one term (0.0 + v), the levels above eight add +0.0 to a value that is not -0.0
__device__ __forceinline__ double plane_sum8(const double v[kRansacMaxN], int m) {
  double w[kRansacMaxN];
#pragma unroll
  for (int j = 0; j < kRansacMaxN; ++j) w[j] = j < m ? 0.0 + v[j] : 0.0;
  return ((w[0] + w[4]) + (w[2] + w[6])) + ((w[1] + w[5]) + (w[3] + w[7]));
}

__device__ __forceinline__ double plane_dist(double a, double b, double c, double d, double x, double y, double z) {
  return fabs(((a * x + b * y) + c * z) + d);
}

// ---- (a) one thread per hypothesis of the batch: the draw and the plane.  planes: [4][kPlaneBatch]; the slots from `count` up to the
// next multiple of 64 (the evaluation runs whole wavefronts) get the zero plane, which the fold never reads.
template <typename P4>
__global__ __launch_bounds__(64) void plane_hypothesis_kernel(const P4* __restrict__ pts, size_t n, int ransac_n, uint64_t seed, uint64_t t0, int count,
                                                              double* __restrict__ planes) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  double pl[4] = {0.0, 0.0, 0.0, 0.0};
  if (slot < count) {
    const uint64_t t = t0 + (uint64_t)slot;
    double px[kRansacMaxN], py[kRansacMaxN], pz[kRansacMaxN];
#pragma unroll
    for (int j = 0; j < kRansacMaxN; ++j) {
      px[j] = py[j] = pz[j] = 0.0;
      if (j < ransac_n) {
        const P4 p = pts[ransac_draw(seed, ransac_n, t, j, (uint64_t)n)];
        px[j] = (double)p.x, py[j] = (double)p.y, pz[j] = (double)p.z;
      }
    }
    if (ransac_n == 3) {  // [O3D] ComputeTrianglePlane
      const double ux = px[1] - px[0], uy = py[1] - py[0], uz = pz[1] - pz[0];
      const double vx = px[2] - px[0], vy = py[2] - py[0], vz = pz[2] - pz[0];
      double a = uy * vz - uz * vy, b = uz * vx - ux * vz, c = ux * vy - uy * vx;
      const double norm = sqrt((a * a + b * b) + c * c);
      if (norm != 0.0) {
        a /= norm, b /= norm, c /= norm;
        pl[0] = a, pl[1] = b, pl[2] = c;
        pl[3] = -((a * px[0] + b * py[0]) + c * pz[0]);
      }
    } else {  // [O3D] GetPlaneFromPoints over the sample
      const double k = (double)ransac_n;
      const double cx = plane_sum8(px, ransac_n) / k, cy = plane_sum8(py, ransac_n) / k, cz = plane_sum8(pz, ransac_n) / k;
      double m[6][kRansacMaxN];
#pragma unroll
      for (int j = 0; j < kRansacMaxN; ++j) {
        const double rx = px[j] - cx, ry = py[j] - cy, rz = pz[j] - cz;
        m[0][j] = rx * rx, m[1][j] = rx * ry, m[2][j] = rx * rz, m[3][j] = ry * ry, m[4][j] = ry * rz, m[5][j] = rz * rz;
      }
      plane_from_moments(cx, cy, cz, plane_sum8(m[0], ransac_n), plane_sum8(m[1], ransac_n), plane_sum8(m[2], ransac_n), plane_sum8(m[3], ransac_n),
                         plane_sum8(m[4], ransac_n), plane_sum8(m[5], ransac_n), pl);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[(size_t)k * kPlaneBatch + slot] = pl[k];
}

// ---- (b) the hot kernel: lane = hypothesis, workgroup = one wavefront, blockIdx.y = chunk of points.  Every lane reads the same point.
template <typename P4>
__global__ __launch_bounds__(64) void plane_eval_kernel(const P4* __restrict__ pts, size_t n, const double* __restrict__ planes, double thr,
                                                        double* __restrict__ perr, uint32_t* __restrict__ pcnt) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  const double a = planes[slot], b = planes[kPlaneBatch + slot], c = planes[2 * kPlaneBatch + slot], d = planes[3 * kPlaneBatch + slot];
  const size_t len = plane_chunk_len(n);
  const size_t lo = (size_t)blockIdx.y * len;
  const size_t hi = lo + len < n ? lo + len : n;
  double err = 0.0;
  uint32_t cnt = 0;
  const P4* __restrict__ q = pts + lo;
  const uint32_t m = hi > lo ? (uint32_t)(hi - lo) : 0u;  // (below 2^31 / kPlaneChunks)
  auto test = [&](const P4& p) {
    const double dist = plane_dist(a, b, c, d, (double)p.x, (double)p.y, (double)p.z);
    const bool in = dist < thr;
    err += in ? dist : 0.0;
    cnt += in ? 1u : 0u;
  };
  uint32_t k = 0;
  for (; k + kPlaneEvalUnroll <= m; k += kPlaneEvalUnroll) {  // the loads of a group first: one wait per group, the sums still in point order
    P4 p[kPlaneEvalUnroll];
#pragma unroll
    for (int u = 0; u < kPlaneEvalUnroll; ++u) p[u] = q[k + u];
#pragma unroll
    for (int u = 0; u < kPlaneEvalUnroll; ++u) test(p[u]);
  }
  for (; k < m; ++k) test(q[k]);
  perr[(size_t)blockIdx.y * kPlaneBatch + slot] = err;
  pcnt[(size_t)blockIdx.y * kPlaneBatch + slot] = cnt;
}

// the halving tree over the kPlaneChunks values each thread holds in LDS rows of kBlock; K rows
template <int K>
__device__ __forceinline__ void plane_tree(double (*s)[kBlock], int t) {
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    __syncthreads();
    if (t < w) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k][t] += s[k][t + w];
    }
  }
  __syncthreads();
}

// ---- the chunk partials of kPlaneFinishHyps hypotheses -> count, fitness, inlier_rmse.  Thread t holds chunk t.
template <int = 0>
__global__ __launch_bounds__(kBlock) void plane_finish_kernel(const double* __restrict__ perr, const uint32_t* __restrict__ pcnt, size_t n,
                                                              double* __restrict__ fit, double* __restrict__ rmse) {
  __shared__ double se[kPlaneFinishHyps][kBlock];
  __shared__ double sc[kPlaneFinishHyps][kBlock];  // counts: integers below 2^53, exact in any order
  const int t = threadIdx.x, h0 = blockIdx.x * kPlaneFinishHyps;
#pragma unroll
  for (int g = 0; g < kPlaneFinishHyps; ++g) {
    se[g][t] = perr[(size_t)t * kPlaneBatch + h0 + g];
    sc[g][t] = (double)pcnt[(size_t)t * kPlaneBatch + h0 + g];
  }
  plane_tree<kPlaneFinishHyps>(se, t);
  plane_tree<kPlaneFinishHyps>(sc, t);
  if (t < kPlaneFinishHyps) {
    const double count = sc[t][0], error = se[t][0];
    fit[h0 + t] = count / (double)n;
    rmse[h0 + t] = count > 0.0 ? error / sqrt(count) : 0.0;
  }
}

// (fitness, rmse, slot) a is better than b: the serial rule's strict order, ties to the lower index
__device__ __forceinline__ bool plane_better(double af, double ar, int ai, double bf, double br, int bi) {
  return af > bf || (af == bf && (ar < br || (ar == br && ai < bi)));
}

// ---- (c) the fold of one batch into the state, one workgroup.  A hypothesis takes part iff its plane is not the zero plane and it would
// replace the start (fitness 0, inlier_rmse 0); the best of those under plane_better is the one the serial reading of the batch ends with.
template <int = 0>
__global__ __launch_bounds__(kBlock) void plane_fold_kernel(const double* __restrict__ planes, const double* __restrict__ fit, const double* __restrict__ rmse,
                                                            int count, long long t0, PlaneState* __restrict__ st) {
  __shared__ double sf[kBlock], sr[kBlock];
  __shared__ int si[kBlock], sd[kBlock];
  const int t = threadIdx.x;
  double bf = 0.0, br = 0.0;
  int bi = -1, ndeg = 0;
  for (int h = t; h < count; h += kBlock) {
    if (planes[h] == 0.0 && planes[kPlaneBatch + h] == 0.0 && planes[2 * kPlaneBatch + h] == 0.0 && planes[3 * kPlaneBatch + h] == 0.0) {
      ++ndeg;
      continue;
    }
    const double f = fit[h], r = rmse[h];
    if (!(f > 0.0 || (f == 0.0 && r < 0.0))) continue;
    if (bi < 0 || plane_better(f, r, h, bf, br, bi)) bf = f, br = r, bi = h;
  }
  sf[t] = bf, sr[t] = br, si[t] = bi, sd[t] = ndeg;
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    __syncthreads();
    if (t < w) {
      sd[t] += sd[t + w];
      if (si[t + w] >= 0 && (si[t] < 0 || plane_better(sf[t + w], sr[t + w], si[t + w], sf[t], sr[t], si[t])))
        sf[t] = sf[t + w], sr[t] = sr[t + w], si[t] = si[t + w];
    }
  }
  __syncthreads();
  if (t == 0) {
    st->n_degenerate += sd[0];
    const int h = si[0];
    if (h >= 0 && (sf[0] > st->fitness || (sf[0] == st->fitness && sr[0] < st->rmse))) {
      st->fitness = sf[0];
      st->rmse = sr[0];
      st->best_t = t0 + h;
#pragma unroll
      for (int k = 0; k < 4; ++k) st->best_plane[k] = planes[(size_t)k * kPlaneBatch + h];
    }
  }
}

template <int = 0>
__global__ void plane_init_kernel(PlaneState* __restrict__ st) {
  PlaneState z{};
  z.best_t = -1;
  *st = z;
}

// ---- (d) the inliers of the winner: flags and their complement (both with the scan's sentinel); no winner: nothing is an inlier
template <typename P4>
__global__ __launch_bounds__(kBlock) void plane_mask_kernel(const P4* __restrict__ pts, size_t n, const PlaneState* __restrict__ st, double thr,
                                                            int* __restrict__ flags, int* __restrict__ nflags) {
  const bool won = st->best_t >= 0;
  const double a = st->best_plane[0], b = st->best_plane[1], c = st->best_plane[2], d = st->best_plane[3];
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const P4 p = pts[i];
    const int in = won && plane_dist(a, b, c, d, (double)p.x, (double)p.y, (double)p.z) < thr ? 1 : 0;
    flags[i] = in;
    nflags[i] = 1 - in;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = nflags[n] = 0;
}

// The chunk sums of the refit, one wavefront per chunk, every lane the same sequential sum (lane 0 stores).  MODE 0: x, y, z and the
// number of inliers -> partial [chunk][4]; MODE 1: the six moments about the state's centroid -> partial [chunk][6].
template <typename P4, int MODE>
__global__ __launch_bounds__(64) void plane_sums_kernel(const P4* __restrict__ pts, size_t n, const int* __restrict__ flags,
                                                        const PlaneState* __restrict__ st, double* __restrict__ partial) {
  constexpr int K = MODE == 0 ? 4 : 6;
  const size_t len = plane_chunk_len(n);
  const size_t lo = (size_t)blockIdx.x * len;
  const size_t hi = lo + len < n ? lo + len : n;
  const double cx = st->centroid[0], cy = st->centroid[1], cz = st->centroid[2];
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  const P4* __restrict__ q = pts + lo;
  const int* __restrict__ fl = flags + lo;
  const uint32_t m = hi > lo ? (uint32_t)(hi - lo) : 0u;
  auto add = [&](const P4& p, int flag) {
    const bool in = flag != 0;
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    if (MODE == 0) {
      s[0] += in ? x : 0.0;
      s[1] += in ? y : 0.0;
      s[2] += in ? z : 0.0;
      s[3] += in ? 1.0 : 0.0;
    } else {
      const double rx = x - cx, ry = y - cy, rz = z - cz;
      s[0] += in ? rx * rx : 0.0;
      s[1] += in ? rx * ry : 0.0;
      s[2] += in ? rx * rz : 0.0;
      s[3] += in ? ry * ry : 0.0;
      s[4] += in ? ry * rz : 0.0;
      s[5] += in ? rz * rz : 0.0;
    }
  };
  uint32_t k = 0;
  for (; k + kPlaneEvalUnroll <= m; k += kPlaneEvalUnroll) {  // as plane_eval_kernel: the loads of a group first
    P4 p[kPlaneEvalUnroll];
    int f[kPlaneEvalUnroll];
#pragma unroll
    for (int u = 0; u < kPlaneEvalUnroll; ++u) p[u] = q[k + u], f[u] = fl[k + u];
#pragma unroll
    for (int u = 0; u < kPlaneEvalUnroll; ++u) add(p[u], f[u]);
  }
  for (; k < m; ++k) add(q[k], fl[k]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) partial[(size_t)blockIdx.x * K + k] = s[k];
  }
}

// one workgroup: the tree over the chunks; MODE 0 leaves the centroid and the number of inliers in the state, MODE 1 the fitted plane
template <int MODE>
__global__ __launch_bounds__(kBlock) void plane_sums_finish_kernel(const double* __restrict__ partial, PlaneState* __restrict__ st) {
  constexpr int K = MODE == 0 ? 4 : 6;
  __shared__ double s[K][kBlock];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) s[k][t] = partial[(size_t)t * K + k];
  plane_tree<K>(s, t);
  if (t == 0 && st->best_t >= 0) {
    if (MODE == 0) {
      const double k = s[3][0];
      st->n_inliers = (unsigned long long)k;
      st->centroid[0] = s[0][0] / k;
      st->centroid[1] = s[1][0] / k;
      st->centroid[2] = s[2][0] / k;
    } else {
      double pl[4];
      plane_from_moments(st->centroid[0], st->centroid[1], st->centroid[2], s[0][0], s[1][0], s[2][0], s[3][0], s[4][0], s[5][0], pl);
#pragma unroll
      for (int k = 0; k < 4; ++k) st->plane[k] = pl[k];
    }
  }
}

#pragma clang fp contract(fast)

}  // namespace o3ds
