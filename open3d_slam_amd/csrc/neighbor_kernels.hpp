// neighbor_kernels.hpp -- neighbour queries between device clouds: [O3D] KDTreeFlann::SearchKNN / SearchRadius / SearchHybrid, and the
// pieces of RemoveStatisticalOutliers / RemoveRadiusOutliers that come after the search (o3ds_neighbor_search and the two filters).
//
// The result of one query is defined without reference to any search structure (tests/neighbor_restatement.py is the same text in numpy):
//   * the query is the stored point, or storage(T s) with T s formed in f64 as ((T00 x + T01 y) + T02 z) + T03, no contraction;
//   * d2 = (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own (nrm_d2);
//   * a candidate is ACCEPTED iff d2 is finite and (radius <= 0 or d2 < storage(radius * radius)), the product formed in f64;
//   * the list is the first max_nn accepted candidates in the order (d2, original target index); `total` counts all of them.
//
// SIXTEEN LANES PER QUERY, four queries per wavefront, selection by RANKING as in normals_kernel.hpp: a batch of sixteen candidates (one
// per lane) that pass the current bound and the kept keys are ranked against each other with broadcast LDS reads, and whoever ranks below
// max_nn stores itself at slot [rank].  Keys are unique, so the list is sorted at all times and does not depend on the order the points
// of a cell arrive in.
//
// The walk goes SHELL BY SHELL around the query's cell -- the cell of the grid nearest to a query that lies outside it: shell R is the
// block of half-width R less the block of half-width R - 1, clipped to the grid, its (y, z) rows dealt out sixteen per round, a row being
// one range of the cell-sorted points (a row through the inside of the block: its two end cells).  After shell R the walk STOPS iff nothing
// outside the block can matter: B < lb^2, with lb a lower bound of the distance from the query to the nearest face of the block that has
// cells beyond it, and B the largest d2 that still changes the result -- storage(r^2) while `total` is wanted or the list is not full,
// the max_nn-th key once it is, +inf for an unbounded query whose list is not full.  No face left: the whole grid has been covered.
// Bounds are LOWER bounds, shrunk by 1e-6 -- far more than the rounding of a d2 in either storage -- so the test errs to the side of walking
// on.  The index clamps points into its grid (cell_of), so the first and last cell of an axis count as unbounded outwards: they are
// never "beyond a face" of a block that holds them, and a row in them has no gap on that side.
//
// `total` of an unbounded query is the number of targets with a finite d2.  Where no d2 can overflow (the query is within 1e18 -- f64
// storage: 1e150 -- of the grid's box on every axis) that is the number of targets without a NaN coordinate, counted once per call
// (count_finite_kernel); only otherwise does an unbounded query walk the whole grid.
#pragma once
#include "cloud_kernels.hpp"
#include "common.hpp"
#include "normals_kernel.hpp"  // row_incl_scan, row_last, nrm_d2, nrm_key, nrm_less, O3DS_WAVE_SYNC

namespace o3ds {

constexpr int kNbrQueriesPerBlock = 4;  // one wavefront per workgroup, a DPP row per query

template <bool WIDE, int KMAX>
struct alignas(16) NbrGroupLds {
  unsigned long long Kk[KMAX];  // kept keys, ascending by (key, index); slots past the count hold a key nothing is smaller than
  int Ki[WIDE ? KMAX : 4];      // original indices (f64 storage; with f32 storage the index is the key's low word)
  unsigned long long Sk[16];    // the batch being ranked
  int Si[WIDE ? 16 : 4];
  int seg_off[32];              // first flat candidate number of each segment of the round (two per lane)
  int seg_base[32];             // position in the sorted cloud minus seg_off
};

// number of target points every coordinate of which is a number (an infinite one fails the index build before this matters)
template <typename P4>
__global__ __launch_bounds__(kBlock) void count_finite_kernel(const P4* __restrict__ pts, size_t n, unsigned int* __restrict__ out) {
  unsigned int c = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const P4 p = pts[i];
    c += (p.x == p.x && p.y == p.y && p.z == p.z) ? 1u : 0u;
  }
  for (int k = 32; k >= 1; k >>= 1) c += __shfl_xor(c, k, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// lower bound of the distance along one axis between the query (coordinate q, clamped cell c) and the points of cell k != c
__device__ __forceinline__ double nbr_gap_lo(double q, double o, double cell, int c, int k) {
  const double face = o + (double)(k > c ? k : k + 1) * cell;
  const double gap = k > c ? face - q : q - face;
  return fmax(gap * (1.0 - 1e-6) - 1e-12 * (fabs(face) + fabs(q) + fabs(o)), 0.0);
}

// 1 iff (ak, ai) < (bk, bi), indices non-negative.  With f64 storage the key has 96 bits: the comparison is the borrow out of the
// subtraction b from a, one chain through the carry flag -- as three compares and two mask operations per pair, the sixteen-fold unrolled
// ranking kept more lane masks alive than there are scalar registers
template <bool WIDE>
__device__ __forceinline__ int nbr_less(unsigned long long ak, int ai, unsigned long long bk, int bi) {
  if constexpr (WIDE) {
    unsigned long long borrow = 0;
    (void)__builtin_subcll(ak, bk, (unsigned int)ai < (unsigned int)bi ? 1ull : 0ull, &borrow);
    return (int)borrow;
  } else {
    return ak < bk ? 1 : 0;
  }
}

template <typename P4, int KMAX>
__global__ __launch_bounds__(64) void neighbor_kernel(const P4* __restrict__ qpts /* the query cloud, original order */,
                                                      const uint32_t* __restrict__ qidx /* null: query j is point j */, size_t nq, int has_pose, Mat34 M,
                                                      GridDev g, const P4* __restrict__ sp /* the target, sorted by cell */, int max_nn, double radius,
                                                      int want_total, const unsigned int* __restrict__ n_finite, uint32_t* __restrict__ out_idx,
                                                      double* __restrict__ out_d2, uint32_t* __restrict__ out_cnt, uint32_t* __restrict__ out_tot,
                                                      double* __restrict__ out_avg /* mean of sqrt(d2) over the list, f64 in list order; null: not wanted */) {
#pragma clang fp contract(off)
  using R = typename Scalar<P4>::type;
  constexpr bool WIDE = sizeof(P4) > 16;
  constexpr int KPL = KMAX / 16;  // kept keys per lane
  constexpr unsigned long long kNever = ~0ull;
  __shared__ NbrGroupLds<WIDE, KMAX> s_grp[kNbrQueriesPerBlock];
  const int lane = threadIdx.x, l = lane & 15, grp = lane >> 4;
  NbrGroupLds<WIDE, KMAX>& L = s_grp[grp];
  const size_t j = (size_t)blockIdx.x * kNbrQueriesPerBlock + (size_t)grp;
  const bool have = j < nq;
  const P4 s = qpts[have ? (qidx ? (size_t)qidx[j] : j) : (qidx ? (size_t)qidx[0] : 0)];
  R qx = s.x, qy = s.y, qz = s.z;
  if (has_pose) {
    const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
    qx = (R)((M.m[0] * x + M.m[1] * y) + M.m[2] * z + M.m[3]);
    qy = (R)((M.m[4] * x + M.m[5] * y) + M.m[6] * z + M.m[7]);
    qz = (R)((M.m[8] * x + M.m[9] * y) + M.m[10] * z + M.m[11]);
  }
  const double qxd = (double)qx, qyd = (double)qy, qzd = (double)qz;
  bool active = have && isfinite(qxd) && isfinite(qyd) && isfinite(qzd);
  const bool unbounded = !(radius > 0.0);
  const R r2 = (R)(radius * radius);
  // the cell of the grid nearest to the query (clamped as a number, before it becomes an integer)
  const int cx = (int)fmin(fmax(floor((qxd - g.ox) * g.inv_cell), 0.0), (double)(g.nx - 1));
  const int cy = (int)fmin(fmax(floor((qyd - g.oy) * g.inv_cell), 0.0), (double)(g.ny - 1));
  const int cz = (int)fmin(fmax(floor((qzd - g.oz) * g.inv_cell), 0.0), (double)(g.nz - 1));
  bool exhaustive = false;  // an unbounded query some d2 of which may overflow: `total` has to be counted
  if (unbounded) {
    const double hx = g.ox + (double)g.nx * g.cell, hy = g.oy + (double)g.ny * g.cell, hz = g.oz + (double)g.nz * g.cell;
    const double far = fmax(fmax(fmax(fabs(qxd - g.ox), fabs(qxd - hx)), fmax(fabs(qyd - g.oy), fabs(qyd - hy))), fmax(fabs(qzd - g.oz), fabs(qzd - hz)));
    exhaustive = !(far < (WIDE ? 1e150 : 1e18));
  }
  const int* __restrict__ cs = g.cell_start;

#pragma unroll
  for (int u = 0; u < KPL; ++u) L.Kk[l + 16 * u] = kNever;
  O3DS_WAVE_SYNC();

  // group state (the same value in all 16 lanes)
  int cnt = 0;
  unsigned int tot = 0;
  unsigned long long tau_k = kNever;
  int tau_i = 0x7fffffff;
  // B: the largest d2 that can still change the result -- fixed for an exhaustive walk and while `total` is wanted within a radius,
  // otherwise the max_nn-th key once the list is full
  const bool fixed_bound = exhaustive || (!unbounded && (want_total || max_nn == 0));
  double B = (exhaustive || unbounded) ? INFINITY : (double)r2;

  for (int ring = 0; __ballot(active) != 0ull; ++ring) {
    const int z0 = max(cz - ring, 0), z1 = min(cz + ring, g.nz - 1), y0 = max(cy - ring, 0), y1 = min(cy + ring, g.ny - 1);
    const int wy = y1 - y0 + 1;
    const int ntask = active ? wy * (z1 - z0 + 1) : 0;
    for (int t0 = 0; __ballot(t0 < ntask) != 0ull; t0 += 16) {
      // ---- one row per lane: up to two ranges of the sorted cloud
      int s0 = 0, e0 = 0, s1 = 0, e1 = 0;
      const int t = t0 + l;
      if (t < ntask) {
        const int tz = t / wy;
        const int z = z0 + tz, y = y0 + (t - tz * wy);
        const double gz = z == cz ? 0.0 : nbr_gap_lo(qzd, g.oz, g.cell, cz, z), gy = y == cy ? 0.0 : nbr_gap_lo(qyd, g.oy, g.cell, cy, y);
        if (gz * gz + gy * gy < B) {
          const int row = (z * g.ny + y) * g.nx;
          if (abs(z - cz) == ring || abs(y - cy) == ring) {  // a row of the shell's faces: every cell of it inside the block
            const int x0 = max(cx - ring, 0), x1 = min(cx + ring, g.nx - 1);
            s0 = cs[row + x0];
            e0 = cs[row + x1 + 1];
          } else {  // a row through the block searched before: its two end cells
            if (cx - ring >= 0) {
              s0 = cs[row + cx - ring];
              e0 = cs[row + cx - ring + 1];
            }
            if (cx + ring <= g.nx - 1) {
              s1 = cs[row + cx + ring];
              e1 = cs[row + cx + ring + 1];
            }
          }
        }
      }
      // ---- lay the ranges of the 16 lanes end to end
      const int len0 = e0 - s0, len1 = e1 - s1;
      const int incl = row_incl_scan(len0 + len1);
      const int T = row_last(incl);
      {
        const int off = incl - (len0 + len1);
        L.seg_off[2 * l] = off;
        L.seg_base[2 * l] = s0 - off;
        L.seg_off[2 * l + 1] = off + len0;
        L.seg_base[2 * l + 1] = s1 - (off + len0);
      }
      O3DS_WAVE_SYNC();
      for (int f0 = 0; __ballot(f0 < T) != 0ull; f0 += 64) {
        // ---- four candidates per lane: flat number -> segment (the last one whose first number is <= f; an empty segment shares
        // its successor's number, which wins)
        int pos[4] = {0, 0, 0, 0};
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int v = L.seg_off[pos[c] + step];
            if (v <= f0 + l + 16 * c) pos[c] += step;
          }
        }
        P4 cand[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int f = f0 + l + 16 * c;
          cand[c] = sp[f < T ? L.seg_base[pos[c]] + f : 0];
        }
        unsigned long long ck[4];
        int ci[4];
        int accm = 0, na = 0;  // (accepted slots as bits of a register: four lane masks would live in scalar registers)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const R d2 = nrm_d2<R>(cand[c].x, cand[c].y, cand[c].z, qx, qy, qz);
          ci[c] = (int)cand[c].i;
          ck[c] = nrm_key(d2, ci[c]);
          const int a = ((f0 + l + 16 * c < T) && isfinite(d2) && (unbounded || d2 < r2)) ? 1 : 0;
          accm |= a << c;
          na += a;
        }
        tot += (unsigned int)row_last(row_incl_scan(na));
        // ---- rank sixteen at a time
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {  // (one copy of the ranking code: the slot is picked by selects, not by unrolling)
          const unsigned long long mk = c == 0 ? ck[0] : c == 1 ? ck[1] : c == 2 ? ck[2] : ck[3];
          const int mi = c == 0 ? ci[0] : c == 1 ? ci[1] : c == 2 ? ci[2] : ci[3];
          const bool ma = ((accm >> c) & 1) != 0;
          const bool sv = ma && max_nn > 0 && (cnt < max_nn || nrm_less<WIDE>(mk, mi, tau_k, tau_i));
          const unsigned long long any = __ballot(sv);
          if (any == 0ull) continue;
          const int nsv = __popc((unsigned int)(any >> (16 * grp)) & 0xffffu);
          L.Sk[l] = sv ? mk : kNever;
          if constexpr (WIDE) L.Si[l] = mi;
          O3DS_WAVE_SYNC();
          // lane l owns the batch's entry l and the kept keys l, l + 16, ...: rank = number of smaller keys
          unsigned long long kk[KPL];
          int ki[KPL], rk[KPL];
          int rs = 0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            const int idx = l + 16 * u;
            kk[u] = L.Kk[idx];  // (kNever past the count)
            ki[u] = 0;
            if constexpr (WIDE) ki[u] = L.Ki[idx];
            rk[u] = idx;
          }
#pragma unroll
          for (int jj = 0; jj < 16; jj += 2) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&L.Sk[jj]);
            int i0 = 0, i1 = 0;
            if constexpr (WIDE) {
              const int2 t2 = *reinterpret_cast<const int2*>(&L.Si[jj]);
              i0 = t2.x, i1 = t2.y;
            }
            rs += nbr_less<WIDE>(a.x, i0, mk, mi);
            rs += nbr_less<WIDE>(a.y, i1, mk, mi);
#pragma unroll
            for (int u = 0; u < KPL; ++u) {
              rk[u] += nbr_less<WIDE>(a.x, i0, kk[u], ki[u]);
              rk[u] += nbr_less<WIDE>(a.y, i1, kk[u], ki[u]);
            }
          }
          for (int jj = 0; __ballot(jj < cnt) != 0ull; jj += 2) {  // (cnt <= KMAX, which is even: jj + 1 stays inside the table)
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(&L.Kk[jj]);
            int i0 = 0, i1 = 0;
            if constexpr (WIDE) {
              const int2 t2 = *reinterpret_cast<const int2*>(&L.Ki[jj]);
              i0 = t2.x, i1 = t2.y;
            }
            rs += nbr_less<WIDE>(a.x, i0, mk, mi);
            rs += nbr_less<WIDE>(a.y, i1, mk, mi);
          }
          O3DS_WAVE_SYNC();
          if (nsv > 0) {
#pragma unroll
            for (int u = 0; u < KPL; ++u)
              if (l + 16 * u < cnt && rk[u] < max_nn) {
                L.Kk[rk[u]] = kk[u];
                if constexpr (WIDE) L.Ki[rk[u]] = ki[u];
              }
            if (sv && rs < max_nn) {
              L.Kk[rs] = mk;
              if constexpr (WIDE) L.Ki[rs] = mi;
            }
          }
          O3DS_WAVE_SYNC();
          cnt = min(cnt + nsv, max_nn);
          if (cnt == max_nn) {  // list full: the bound becomes the max_nn-th key
            double worst;
            tau_k = L.Kk[max_nn - 1];
            if constexpr (WIDE) {
              tau_i = L.Ki[max_nn - 1];
              worst = __longlong_as_double((long long)tau_k);
            } else {
              tau_i = 0;
              worst = (double)__uint_as_float((unsigned int)(tau_k >> 32));
            }
            if (!fixed_bound) B = worst;
          }
        }
      }
      O3DS_WAVE_SYNC();  // the segment table is rewritten by the next round
    }
    // ---- shell done: does anything outside the block still matter?
    if (active) {
      double lb = INFINITY;
      if (cx + ring < g.nx - 1) lb = fmin(lb, nbr_gap_lo(qxd, g.ox, g.cell, cx, cx + ring + 1));
      if (cx - ring > 0) lb = fmin(lb, nbr_gap_lo(qxd, g.ox, g.cell, cx, cx - ring - 1));
      if (cy + ring < g.ny - 1) lb = fmin(lb, nbr_gap_lo(qyd, g.oy, g.cell, cy, cy + ring + 1));
      if (cy - ring > 0) lb = fmin(lb, nbr_gap_lo(qyd, g.oy, g.cell, cy, cy - ring - 1));
      if (cz + ring < g.nz - 1) lb = fmin(lb, nbr_gap_lo(qzd, g.oz, g.cell, cz, cz + ring + 1));
      if (cz - ring > 0) lb = fmin(lb, nbr_gap_lo(qzd, g.oz, g.cell, cz, cz - ring - 1));
      const bool covered = cx + ring >= g.nx - 1 && cx - ring <= 0 && cy + ring >= g.ny - 1 && cy - ring <= 0 && cz + ring >= g.nz - 1 && cz - ring <= 0;
      if (covered || B < lb * lb) active = false;
    }
  }

  if (have) {
    const bool fin = isfinite(qxd) && isfinite(qyd) && isfinite(qzd);
    if (fin && unbounded && !exhaustive) tot = *n_finite;
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
      const int idx = l + 16 * u;
      if (idx < max_nn) {
        const bool v = idx < cnt;
        const unsigned long long key = L.Kk[idx];
        uint32_t oi = 0;
        double dd = 0.0;
        if (v) {
          if constexpr (WIDE) {
            oi = (uint32_t)L.Ki[idx];
            dd = __longlong_as_double((long long)key);
          } else {
            oi = (uint32_t)(key & 0xffffffffull);
            dd = (double)__uint_as_float((unsigned int)(key >> 32));
          }
        }
        if (out_idx) out_idx[j * (size_t)max_nn + (size_t)idx] = oi;
        if (out_d2) out_d2[j * (size_t)max_nn + (size_t)idx] = dd;
      }
    }
    if (l == 0) {
      out_cnt[j] = (uint32_t)cnt;
      if (out_tot) out_tot[j] = tot;
      if (out_avg) {
        double sum = 0.0;
        for (int jj = 0; jj < cnt; ++jj) {
          const unsigned long long key = L.Kk[jj];
          double dd;
          if constexpr (WIDE)
            dd = __longlong_as_double((long long)key);
          else
            dd = (double)__uint_as_float((unsigned int)(key >> 32));
          sum += sqrt(dd);
        }
        out_avg[j] = cnt > 0 ? sum / (double)cnt : 0.0;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- the filters' statistics
// [O3D] RemoveStatisticalOutliers: mean and standard deviation of the average distances a_i > 0, in the fixed order of the cloud centre
// (cloud_kernels.hpp: kCenterChunks chunks, a strided sum per thread, a halving tree over the threads, the same tree over the chunks), so
// that the threshold has the same bits whatever launched it.  pass 0 sums (a_i, 1) over the valid points, pass 1 sums (a_i - mean)^2.
__device__ __forceinline__ void stat_tree(double* sa, double* sb, int t) {
  for (int s = kBlock / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (t < s) {
      sa[t] += sa[t + s];
      sb[t] += sb[t + s];
    }
  }
  __syncthreads();
}
__global__ __launch_bounds__(kBlock) void stat_partial_kernel(const double* __restrict__ a, size_t n, const double* __restrict__ stat /* null: pass 0 */,
                                                              double* __restrict__ partial /* [kCenterChunks][2] */) {
#pragma clang fp contract(off)
  __shared__ double sa[kBlock], sb[kBlock];
  const int t = threadIdx.x;
  const size_t len = (n + kCenterChunks - 1) / kCenterChunks;
  const size_t lo = (size_t)blockIdx.x * len;
  const size_t hi = lo + len < n ? lo + len : n;
  const double mean = stat ? stat[0] : 0.0;
  double x = 0.0, y = 0.0;
  for (size_t i = lo + (size_t)t; i < hi; i += kBlock) {
    const double v = a[i];
    if (v > 0.0) {
      x += stat ? (v - mean) * (v - mean) : v;
      y += 1.0;
    }
  }
  sa[t] = x;
  sb[t] = y;
  stat_tree(sa, sb, t);
  if (t == 0) {
    partial[2 * blockIdx.x] = sa[0];
    partial[2 * blockIdx.x + 1] = sb[0];
  }
}
// stat = {mean, n_valid, threshold}; pass 0 writes the first two, pass 1 the third.  n_valid < 2 gives 0 / 0: a NaN threshold.
__global__ __launch_bounds__(kBlock) void stat_finish_kernel(const double* __restrict__ partial, int pass, double std_ratio, double* __restrict__ stat) {
#pragma clang fp contract(off)
  static_assert(kCenterChunks == kBlock, "one chunk per thread");
  __shared__ double sa[kBlock], sb[kBlock];
  const int t = threadIdx.x;
  sa[t] = partial[2 * t];
  sb[t] = partial[2 * t + 1];
  stat_tree(sa, sb, t);
  if (t == 0) {
    if (pass == 0) {
      stat[0] = sa[0] / sb[0];
      stat[1] = sb[0];
    } else {
      const double sd = sqrt(sa[0] / (stat[1] - 1.0));
      stat[2] = stat[0] + std_ratio * sd;
    }
  }
}
// keep point i iff a_i > 0 and a_i < threshold (statistical), or total_i > nb_points (radius); flags[n] = 0 is the scan's sentinel
__global__ __launch_bounds__(kBlock) void stat_flag_kernel(const double* __restrict__ a, size_t n, const double* __restrict__ stat, int* __restrict__ flags) {
  const double thr = stat[2];
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) flags[i] = (a[i] > 0.0 && a[i] < thr) ? 1 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}
__global__ __launch_bounds__(kBlock) void radius_flag_kernel(const uint32_t* __restrict__ total, size_t n, uint32_t nb_points, int* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) flags[i] = total[i] > nb_points ? 1 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}
__global__ __launch_bounds__(kBlock) void kept_index_kernel(const int* __restrict__ flags, const int* __restrict__ pos, size_t n, uint32_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    if (flags[i]) out[pos[i]] = (uint32_t)i;
}

}  // namespace o3ds
