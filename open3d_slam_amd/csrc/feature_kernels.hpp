// feature_kernels.hpp -- place recognition's front half (PlaceRecognition::buildLoopClosureConstraints, PlaceRecognition.cpp:71-90;
// Submap::computeFeatures, Submap.cpp:228-248): [O3D] ComputeFPFHFeature, the feature correspondences of
// RegistrationRANSACBasedOnFeatureMatching and the hypothesis search of RegistrationRANSACBasedOnCorrespondence (Open3D v0.15.1
// Feature.cpp, Registration.cpp, CorrespondenceChecker.cpp, restated; Open3D is not part of this project).
//
// Arithmetic is f64 whatever the storage precision; only coordinates and normals are read at storage precision.
//   * fpfh_neighbours_kernel  one wavefront per point: the max_nn smallest (d2, index) among the points with d2 < r^2 (the set
//                             normals_kernel.hpp keeps), by ranking each chunk of 64 candidates against the sorted kept list in LDS.
//                             The list does not depend on the order the candidates arrive in.
//   * spfh_kernel / fpfh_kernel one thread per point, the bins in LDS (a register array indexed by bin would go to scratch).
//   * feature_nn_kernel       brute-force 1-NN in 33 dimensions, one thread per query, the other side tiled through LDS; the
//                             distance is the direct f64 sum over b = 0..32 in order, ties to the lower index.
//   * ransac_hypothesis_kernel one thread per hypothesis: draw, Umeyama from sums (umeyama_from_record), the two checkers.
//   * ransac_validate_kernel  one workgroup per hypothesis that passed: exact 1-NN within max_corr on the target's grid for every
//                             placed source point.  Each lane sums its own points in point order, then a fixed 256 -> 1 tree: the
//                             sum depends on neither the batch size nor the number of workgroups.
#pragma once
#include "common.hpp"
#include "icp_kernels.hpp"

namespace o3ds {

constexpr int kFeatDim = 33;
constexpr int kFpfhMaxNN = 128;
constexpr int kRansacMaxN = 8;
constexpr int kValBlock = 256;
constexpr int kFnnBlock = 256, kFnnTile = 32;

#pragma clang fp contract(off)  // products and sums round one by one, as Open3D's (Eigen, no FMA) do

// the splitmix64 finaliser, as o3ds_random_down_sample's keys (cloud_kernels.hpp)
__host__ __device__ __forceinline__ uint64_t feat_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// correspondence index j of hypothesis t
__host__ __device__ __forceinline__ uint32_t ransac_draw(uint64_t seed, int n, uint64_t t, int j, uint64_t m) {
  return (uint32_t)(feat_mix(seed + ((uint64_t)n * t + (uint64_t)j + 1ull) * 0x9E3779B97F4A7C15ull) % m);
}

__device__ __forceinline__ bool key_less(double ad, int ai, double bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

// ---- a. neighbour lists ---------------------------------------------------------------------------------------------------------
// Grid: the cloud's index (cell >= r / K).  Per point: the rows (2K+1)^2 around its cell, x in [ix - K, ix + K].
template <typename P4>
__global__ __launch_bounds__(64) void fpfh_neighbours_kernel(GridDev g, const P4* __restrict__ spts, const P4* __restrict__ pts, int n,
                                                             double r2, int max_nn, int K, int* __restrict__ nb_idx,
                                                             double* __restrict__ nb_d2, int* __restrict__ nb_cnt) {
  __shared__ double ld2[2][kFpfhMaxNN];
  __shared__ int lix[2][kFpfhMaxNN];
  __shared__ double cd2[64];
  __shared__ int cix[64];
  const int lane = threadIdx.x;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const P4 q = pts[i];
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const QueryCell c = locate(g, qx, qy, qz);
    int L = 0, buf = 0;
    for (int dz = -K; dz <= K; ++dz) {
      const int z = c.iz + dz;
      if ((unsigned)z >= (unsigned)g.nz) continue;
      for (int dy = -K; dy <= K; ++dy) {
        const int y = c.iy + dy;
        if ((unsigned)y >= (unsigned)g.ny) continue;
        const int xa = max(c.ix - K, 0), xb = min(c.ix + K, g.nx - 1);
        if (xa > xb) continue;
        const int row = (z * g.ny + y) * g.sx;
        const int s = g.cell_start[row + xa], e = g.cell_start[row + xb + 1];
        for (int base = s; base < e; base += 64) {
          const int p = base + lane;
          bool valid = p < e;
          double d2 = 0.0;
          int idx = 0x7fffffff;
          if (valid) {
            const P4 t = spts[p];
            const double dx = (double)t.x - qx, dy2 = (double)t.y - qy, dz2 = (double)t.z - qz;
            d2 = dx * dx + dy2 * dy2 + dz2 * dz2;
            idx = (int)t.i;
            valid = d2 < r2;
            if (valid && L == max_nn) valid = key_less(d2, idx, ld2[buf][L - 1], lix[buf][L - 1]);
          }
          const unsigned long long vm = __ballot(valid);
          if (vm == 0ull) continue;  // wave-uniform
          const int nv = __popcll(vm);
          cd2[lane] = valid ? d2 : INFINITY;
          cix[lane] = valid ? idx : 0x7fffffff;
          lds_wave_sync();
          const int nb = buf ^ 1;
          if (valid) {
            int rc = 0;
            for (int j = 0; j < 64; ++j) rc += key_less(cd2[j], cix[j], d2, idx) ? 1 : 0;
            int lo = 0, hi = L;  // kept entries smaller than this candidate
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (key_less(ld2[buf][mid], lix[buf][mid], d2, idx))
                lo = mid + 1;
              else
                hi = mid;
            }
            const int pos = lo + rc;
            if (pos < max_nn) {
              ld2[nb][pos] = d2;
              lix[nb][pos] = idx;
            }
          }
          for (int k = lane; k < L; k += 64) {
            const double kd = ld2[buf][k];
            const int ki = lix[buf][k];
            int cnt = 0;
            for (int j = 0; j < 64; ++j) cnt += key_less(cd2[j], cix[j], kd, ki) ? 1 : 0;
            const int pos = k + cnt;
            if (pos < max_nn) {
              ld2[nb][pos] = kd;
              lix[nb][pos] = ki;
            }
          }
          L = min(max_nn, L + nv);
          buf = nb;
          lds_wave_sync();
        }
      }
    }
    for (int k = lane; k < L; k += 64) {
      nb_idx[(size_t)i * max_nn + k] = lix[buf][k];
      nb_d2[(size_t)i * max_nn + k] = ld2[buf][k];
    }
    if (lane == 0) nb_cnt[i] = L;
    lds_wave_sync();
  }
}

// ---- pair feature (Feature.cpp ComputePairFeatures): {f0, f1, f2}; zero for |d| = 0 or |d x n1| = 0 ----------------------------
__device__ __forceinline__ void pair_feature(double p1x, double p1y, double p1z, double n1x, double n1y, double n1z, double p2x, double p2y,
                                             double p2z, double n2x, double n2y, double n2z, double* f0, double* f1, double* f2) {
  double dx = p2x - p1x, dy = p2y - p1y, dz = p2z - p1z;
  const double dn = sqrt(dx * dx + dy * dy + dz * dz);
  *f0 = *f1 = *f2 = 0.0;
  if (dn == 0.0) return;
  const double a1 = (n1x * dx + n1y * dy + n1z * dz) / dn, a2 = (n2x * dx + n2y * dy + n2z * dz) / dn;
  double ax = n1x, ay = n1y, az = n1z, bx = n2x, by = n2y, bz = n2z, f2v;
  if (acos(fabs(a1)) > acos(fabs(a2))) {
    ax = n2x, ay = n2y, az = n2z, bx = n1x, by = n1y, bz = n1z;
    dx = -dx, dy = -dy, dz = -dz;
    f2v = -a2;
  } else {
    f2v = a1;
  }
  double vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;  // d x n1
  const double vn = sqrt(vx * vx + vy * vy + vz * vz);
  if (vn == 0.0) return;
  vx /= vn, vy /= vn, vz /= vn;
  const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;  // n1 x v
  *f2 = f2v;
  *f1 = vx * bx + vy * by + vz * bz;
  *f0 = atan2(wx * bx + wy * by + wz * bz, ax * bx + ay * by + az * bz);
}

__device__ __forceinline__ int clamp_bin(double v) {
  int b = (int)floor(v);
  return b < 0 ? 0 : (b >= 11 ? 10 : b);
}

// ---- SPFH (Feature.cpp ComputeSPFHFeature): one thread per point, bins in LDS (column per thread) ------------------------------
template <typename P4>
__global__ __launch_bounds__(64) void spfh_kernel(const P4* __restrict__ pts, const P4* __restrict__ nrm, int n, const int* __restrict__ nb_idx,
                                                  const int* __restrict__ nb_cnt, int max_nn, double* __restrict__ spfh) {
  __shared__ double h[kFeatDim][64];
  const int i = blockIdx.x * 64 + threadIdx.x;
  for (int j = 0; j < kFeatDim; ++j) h[j][threadIdx.x] = 0.0;
  if (i < n) {
    const int L = nb_cnt[i];
    if (L > 1) {
      const double incr = 100.0 / (double)(L - 1);
      const P4 p = pts[i], pn = nrm[i];
      const double px = p.x, py = p.y, pz = p.z, nx = pn.x, ny = pn.y, nz = pn.z;
      for (int k = 1; k < L; ++k) {
        const int j = nb_idx[(size_t)i * max_nn + k];
        const P4 q = pts[j], qn = nrm[j];
        double f0, f1, f2;
        pair_feature(px, py, pz, nx, ny, nz, (double)q.x, (double)q.y, (double)q.z, (double)qn.x, (double)qn.y, (double)qn.z, &f0, &f1, &f2);
        h[clamp_bin(11.0 * (f0 + M_PI) / (2.0 * M_PI))][threadIdx.x] += incr;
        h[11 + clamp_bin(11.0 * (f1 + 1.0) * 0.5)][threadIdx.x] += incr;
        h[22 + clamp_bin(11.0 * (f2 + 1.0) * 0.5)][threadIdx.x] += incr;
      }
    }
    for (int j = 0; j < kFeatDim; ++j) spfh[(size_t)i * kFeatDim + j] = h[j][threadIdx.x];
  }
}

// ---- FPFH (Feature.cpp ComputeFPFHFeature): one thread per point, the 33 sums in registers (fully unrolled) ---------------------
__global__ __launch_bounds__(64) void fpfh_kernel(const double* __restrict__ spfh, int n, const int* __restrict__ nb_idx,
                                                  const double* __restrict__ nb_d2, const int* __restrict__ nb_cnt, int max_nn,
                                                  double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double F[kFeatDim];
#pragma unroll
  for (int j = 0; j < kFeatDim; ++j) F[j] = 0.0;
  const int L = nb_cnt[i];
  if (L > 1) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 1; k < L; ++k) {
      const double d2 = nb_d2[(size_t)i * max_nn + k];
      if (d2 == 0.0) continue;
      const double* sp = spfh + (size_t)nb_idx[(size_t)i * max_nn + k] * kFeatDim;
#pragma unroll
      for (int j = 0; j < kFeatDim; ++j) {
        const double v = sp[j] / d2;
        if (j < 11)
          s0 += v;
        else if (j < 22)
          s1 += v;
        else
          s2 += v;
        F[j] += v;
      }
    }
    if (s0 != 0.0) s0 = 100.0 / s0;
    if (s1 != 0.0) s1 = 100.0 / s1;
    if (s2 != 0.0) s2 = 100.0 / s2;
    const double* own = spfh + (size_t)i * kFeatDim;
#pragma unroll
    for (int j = 0; j < kFeatDim; ++j) F[j] = F[j] * (j < 11 ? s0 : (j < 22 ? s1 : s2)) + own[j];
  }
#pragma unroll
  for (int j = 0; j < kFeatDim; ++j) out[(size_t)i * kFeatDim + j] = F[j];
}

// ---- b. nearest feature: out[i] = argmin_j sum_b (a_i,b - b_j,b)^2, ties to the lower j; -1 when nb == 0 -----------------------
__global__ __launch_bounds__(kFnnBlock) void feature_nn_kernel(const double* __restrict__ A, int na, const double* __restrict__ B, int nb,
                                                               int* __restrict__ out) {
  __shared__ double tile[kFnnTile][kFeatDim + 1];
  const int i = blockIdx.x * kFnnBlock + threadIdx.x;
  double a[kFeatDim];
#pragma unroll
  for (int b = 0; b < kFeatDim; ++b) a[b] = i < na ? A[(size_t)i * kFeatDim + b] : 0.0;
  double best = INFINITY;
  int arg = -1;
  for (int j0 = 0; j0 < nb; j0 += kFnnTile) {
    const int rows = min(kFnnTile, nb - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * kFeatDim; e += kFnnBlock) tile[e / kFeatDim][e % kFeatDim] = B[(size_t)j0 * kFeatDim + e];
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      double d = 0.0;
#pragma unroll
      for (int b = 0; b < kFeatDim; ++b) {
        const double t = a[b] - tile[r][b];
        d += t * t;
      }
      if (d < best || arg < 0) {
        best = d;
        arg = j0 + r;
      }
    }
  }
  if (i < na) out[i] = arg;
}

// ---- c. RANSAC hypotheses ------------------------------------------------------------------------------------------------------
struct RansacArgs {
  const uint32_t* corr;  // [m][2]: (source index, target index)
  unsigned long long m;
  unsigned long long seed;
  int n;              // ransac_n
  long long t0;       // first hypothesis of the batch
  int count;          // hypotheses in the batch
  double edge;        // similarity (<= 0: off)
  double dist;        // threshold (<= 0: off)
  double* T;          // [count][16] column-major
  int* checks;        // [count]: bit 0 edge length passed (or off), bit 1 distance passed (or off)
  uint32_t* samples;  // [count][kRansacMaxN] or null
  int* list;          // [count]: batch slots that passed both, in any order
  int* list_count;    // [1], zero on entry
};

template <typename P4>
__device__ __forceinline__ void load_xyz(const P4* __restrict__ p, uint32_t k, double* x, double* y, double* z) {
  const P4 v = p[k];
  *x = (double)v.x, *y = (double)v.y, *z = (double)v.z;
}

template <typename P4>
__global__ __launch_bounds__(256) void ransac_hypothesis_kernel(const P4* __restrict__ src, const P4* __restrict__ tgt, RansacArgs a) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.count) return;
  const uint64_t t = (uint64_t)(a.t0 + slot);
  double rec[kRec];
#pragma unroll
  for (int k = 0; k < kRec; ++k) rec[k] = 0.0;
  // the sums are of coordinates relative to the multiples of 1024 m nearest to the first drawn pair (pivot_round; source and target each
  // about its own: Sigma does not depend on either shift, and formed from far absolute coordinates its subtraction cancels;
  // umeyama_from_record puts the two pivots back into t).  Clouds within 512 m of the origin: both zero, the sums of the coordinates.
  double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < a.n; ++j) {
    const uint32_t c = ransac_draw(a.seed, a.n, t, j, a.m);
    if (a.samples) a.samples[(size_t)slot * kRansacMaxN + j] = c;
    double px, py, pz, qx, qy, qz;
    load_xyz(src, a.corr[2 * (size_t)c], &px, &py, &pz);
    load_xyz(tgt, a.corr[2 * (size_t)c + 1], &qx, &qy, &qz);
    if (j == 0) {
      cp[0] = pivot_round(px), cp[1] = pivot_round(py), cp[2] = pivot_round(pz);
      cq[0] = pivot_round(qx), cq[1] = pivot_round(qy), cq[2] = pivot_round(qz);
    }
    px -= cp[0], py -= cp[1], pz -= cp[2], qx -= cq[0], qy -= cq[1], qz -= cq[2];
    rec[0] += qx * px, rec[1] += qx * py, rec[2] += qx * pz;
    rec[3] += qy * px, rec[4] += qy * py, rec[5] += qy * pz;
    rec[6] += qz * px, rec[7] += qz * py, rec[8] += qz * pz;
    rec[9] += px, rec[10] += py, rec[11] += pz;
    rec[12] += qx, rec[13] += qy, rec[14] += qz;
    rec[kRecCount] += 1.0;
  }
  double U[16];
  umeyama_from_record(rec, U, cp, cq);
  bool edge_ok = true, dist_ok = true;
  if (a.edge > 0.0) {  // CorrespondenceCheckerBasedOnEdgeLength::Check
    for (int i = 0; i < a.n && edge_ok; ++i) {
      const uint32_t ci = ransac_draw(a.seed, a.n, t, i, a.m);
      double sx, sy, sz, tx, ty, tz;
      load_xyz(src, a.corr[2 * (size_t)ci], &sx, &sy, &sz);
      load_xyz(tgt, a.corr[2 * (size_t)ci + 1], &tx, &ty, &tz);
      for (int j = i + 1; j < a.n; ++j) {
        const uint32_t cj = ransac_draw(a.seed, a.n, t, j, a.m);
        double sx2, sy2, sz2, tx2, ty2, tz2;
        load_xyz(src, a.corr[2 * (size_t)cj], &sx2, &sy2, &sz2);
        load_xyz(tgt, a.corr[2 * (size_t)cj + 1], &tx2, &ty2, &tz2);
        const double ex = sx - sx2, ey = sy - sy2, ez = sz - sz2, fx = tx - tx2, fy = ty - ty2, fz = tz - tz2;
        const double ds = sqrt(ex * ex + ey * ey + ez * ez), dt = sqrt(fx * fx + fy * fy + fz * fz);
        if (ds < dt * a.edge || dt < ds * a.edge) {
          edge_ok = false;
          break;
        }
      }
    }
  }
  if (a.dist > 0.0) {  // CorrespondenceCheckerBasedOnDistance::Check
    for (int j = 0; j < a.n; ++j) {
      const uint32_t c = ransac_draw(a.seed, a.n, t, j, a.m);
      double px, py, pz, qx, qy, qz;
      load_xyz(src, a.corr[2 * (size_t)c], &px, &py, &pz);
      load_xyz(tgt, a.corr[2 * (size_t)c + 1], &qx, &qy, &qz);
      const double x = U[0] * px + U[4] * py + U[8] * pz + U[12], y = U[1] * px + U[5] * py + U[9] * pz + U[13],
                   z = U[2] * px + U[6] * py + U[10] * pz + U[14];
      const double ex = qx - x, ey = qy - y, ez = qz - z;
      if (sqrt(ex * ex + ey * ey + ez * ez) > a.dist) {
        dist_ok = false;
        break;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) a.T[(size_t)slot * 16 + k] = U[k];
  a.checks[slot] = (edge_ok ? 1 : 0) | (dist_ok ? 2 : 0);
  if (edge_ok && dist_ok) a.list[atomicAdd(a.list_count, 1)] = slot;
}

// ---- validation ([O3D] GetRegistrationResultAndCorrespondences): one workgroup per listed hypothesis --------------------------
// out[k] = {slot, pairs, sum d^2} for list entry k.  The target's grid has cell >= r / K; a match is the nearest target point with
// d2 < r^2, ties to the lower index (KDTreeFlann::SearchHybrid(q, r, 1)).
template <typename P4>
__global__ __launch_bounds__(kValBlock) void ransac_validate_kernel(const P4* __restrict__ src, int n_src, GridDev g, const P4* __restrict__ tp,
                                                                    double r2, int K, const double* __restrict__ T, const int* __restrict__ list,
                                                                    const int* __restrict__ list_count, double* __restrict__ out) {
  __shared__ double s_e[kValBlock];
  __shared__ int s_c[kValBlock];
  const int nl = *list_count;
  for (int k = blockIdx.x; k < nl; k += gridDim.x) {
    const int slot = list[k];
    const double* U = T + (size_t)slot * 16;
    const double u0 = U[0], u1 = U[1], u2 = U[2], u4 = U[4], u5 = U[5], u6 = U[6], u8 = U[8], u9 = U[9], u10 = U[10], u12 = U[12],
                 u13 = U[13], u14 = U[14];
    double e = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n_src; i += kValBlock) {
      const P4 p = src[i];
      const double px = p.x, py = p.y, pz = p.z;
      const double qx = u0 * px + u4 * py + u8 * pz + u12, qy = u1 * px + u5 * py + u9 * pz + u13, qz = u2 * px + u6 * py + u10 * pz + u14;
      const QueryCell c = locate(g, qx, qy, qz);
      double best = r2;
      long long bi = -1;
      for (int dz = -K; dz <= K; ++dz) {
        const int z = c.iz + dz;
        if ((unsigned)z >= (unsigned)g.nz) continue;
        for (int dy = -K; dy <= K; ++dy) {
          const int y = c.iy + dy;
          if ((unsigned)y >= (unsigned)g.ny) continue;
          const int xa = max(c.ix - K, 0), xb = min(c.ix + K, g.nx - 1);
          if (xa > xb) continue;
          const int row = (z * g.ny + y) * g.sx;
          const int s = g.cell_start[row + xa], en = g.cell_start[row + xb + 1];
          for (int q = s; q < en; ++q) {
            const P4 t = tp[q];
            const double dx = (double)t.x - qx, dy2 = (double)t.y - qy, dz2 = (double)t.z - qz;
            const double d2 = dx * dx + dy2 * dy2 + dz2 * dz2;
            const long long ti = (long long)t.i;
            if (d2 < best || (d2 == best && bi >= 0 && ti < bi)) {
              best = d2;
              bi = ti;
            }
          }
        }
      }
      if (bi >= 0) {
        e += best;
        ++cnt;
      }
    }
    s_e[threadIdx.x] = e;
    s_c[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = kValBlock / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) {
        s_e[threadIdx.x] += s_e[threadIdx.x + w];
        s_c[threadIdx.x] += s_c[threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out[3 * (size_t)k] = (double)slot;
      out[3 * (size_t)k + 1] = (double)s_c[0];
      out[3 * (size_t)k + 2] = s_e[0];
    }
    __syncthreads();
  }
}

#pragma clang fp contract(fast)

}  // namespace o3ds
