// cluster_kernels.hpp -- [O3D] PointCloud::ClusterDBSCAN(eps, min_points) on a device cloud, and the filter that drops the noise and the
// small clusters (o3ds_cluster_dbscan, o3ds_remove_small_clusters).
//
// The labels are defined without reference to any search structure (tests/cluster_restatement.py is the same text in numpy), with the
// arithmetic of neighbor_kernels.hpp:
//   * d2(i, j) = (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own (nrm_d2);
//   * j is a NEIGHBOUR of i iff d2 is finite and d2 < storage(eps * eps), strictly, the product formed in f64; N_i is the set of them in
//     i's own cloud, i included; a point with a non-finite coordinate has none;
//   * i is a CORE point iff |N_i| >= min_points;
//   * the clusters are the connected components of the graph on the core points with an edge i - j iff j is in N_i (d2 is symmetric bit
//     for bit), numbered 0 .. n_clusters - 1 in the order of each component's smallest core index;
//   * a point that is not core gets the SMALLEST cluster id among the core points of N_i (not the cluster of its lowest-index core
//     neighbour), -1 if there is none.
//
// Five steps.  |N_i| is the count-only Radius search of the cloud in itself (neighbor_kernel, max_nn = 0).  HOOKING: one walk of every
// core point's neighbourhood, sixteen lanes per point and four points per wavefront as in neighbor_kernel; for every accepted core
// candidate j < i (each edge from its larger end) i and j are united in a union-find over parent[n], indexed by original index:
//   * parent[x] <= x at all times, and parent[x] == x iff x is a root;
//   * only a root is ever re-pointed, by a device-scope compare-and-swap from itself to a smaller root;
//   * a path is only ever shortened by lowering a parent to one of its ancestors (atomicMin);
// so a chase strictly descends, and the root of a finished component is its smallest core index -- which is the cluster order.  (The
// sixteen candidates a group looks at together are united with each other first, under the smallest of their roots, and i with that.)  Inside
// the hooking kernel parent is read with relaxed agent-scope atomic loads: a plain load may be served from another XCD's stale line; a
// stale value is still an ancestor, and the compare-and-swap decides.  FLATTEN (a later launch, so every hook is visible): parent[i] =
// root of i for every core point, the roots flagged; an exclusive scan of the flags ranks them: that is the cluster id.  BORDER: a second
// walk, for the points that are not core and have a neighbour besides themselves: the minimum of parent[j] over the accepted core
// candidates j, then its rank; the same kernel writes every label.  SIZES: an integer atomicAdd per run of equal labels in consecutive
// lanes (order-free, so reproducible; one add per point onto the counter of a cluster of a million points is a million serialised adds).
//
// The walk visits the cells that meet the cube [p - eps, p + eps], clipped to the grid -- the index clamps points into its grid, so the
// first and last cell of an axis are unbounded outwards and the clipped range still holds every neighbour --, its (y, z) rows dealt out
// sixteen per round, a row being ONE range of the cell-sorted points; a row whose (y, z) gap alone reaches storage(eps^2) is skipped (the
// shrunk lower bounds of neighbor_kernel: nbr_gap_lo).  The ranges of a round are laid end to end and their candidates dealt out four per
// lane, so a neighbourhood of hundreds of points is no single lane's loop, and no list of neighbours exists anywhere: |N_i| is unbounded.
//
// EVERY LOOP OVER parent IS BOUNDED: a chase descends, so it is shorter than the number of points, and a union retries only after
// another thread re-pointed the root it held, which happens once per point.  Both are counted against n; past it the thread sets the
// error word and stops uniting, and the host reports O3DS_ERR_HIP without publishing a label.
#pragma once
#include "neighbor_kernels.hpp"

namespace o3ds {

// (Every kernel here is a template, the small ones of a parameter nobody sets: the compiler emits the plain kernels of a translation unit
// first and the instantiations in the order of their first use, and backend.hip uses these last -- so every other kernel keeps the place
// in the code object that the registration was measured with.)
struct alignas(16) ClusterGroupLds {
  int seg_off[16];   // first flat candidate number of each row of the round (one per lane)
  int seg_base[16];  // position in the sorted cloud minus seg_off
};

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x; *bad: the chase took more than `cap` steps (never expected: it descends).  On the way every node passed is pointed
// at its grandparent: points that come in scan-line order hook i under i - 1 under i - 2 ... while thousands of them are in flight
// together, and without the shortening every later chase would walk that whole line, one memory round trip per step.
__device__ __forceinline__ int cl_find(int* parent, int x, int cap, bool* bad) {
  int cur = cl_load(parent + x);
  if (cur == x) return x;
  int prev = x;
  for (int steps = 0;; ++steps) {
    const int next = cl_load(parent + cur);
    if (next == cur) break;  // a root
    if (steps >= cap) {
      *bad = true;
      break;
    }
    atomicMin(parent + prev, next);  // (next is an ancestor of prev, below its parent)
    prev = cur;
    cur = next;
  }
  return cur;
}

// unites the components of a (an ancestor of the thread's own point, or the point) and b; returns an ancestor of a's point afterwards
__device__ __forceinline__ int cl_unite(int* parent, int a, int b, int cap, bool* bad) {
  for (int tries = 0;; ++tries) {
    a = cl_find(parent, a, cap, bad);
    b = cl_find(parent, b, cap, bad);
    if (*bad || a == b) break;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) {  // hi was still a root: it hangs under the smaller root now
      a = lo;
      break;
    }
    if (tries >= cap) {  // (a failed swap means another thread re-pointed hi: once per point at most)
      *bad = true;
      break;
    }
    a = hi, b = lo;
  }
  return a;
}

template <int = 0>
__global__ __launch_bounds__(kBlock) void cluster_init_kernel(int* __restrict__ parent, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) parent[i] = (int)i;
}

// BORDER false: the hooking walk of the core points.  BORDER true: the walk of the non-core points with a neighbour besides themselves,
// and the label of every point.
template <typename P4, bool BORDER>
__global__ __launch_bounds__(64) void cluster_walk_kernel(const P4* __restrict__ pts /* the cloud, original order */, size_t n, GridDev g,
                                                          const P4* __restrict__ sp /* the same cloud, sorted by cell */, double eps, uint32_t min_points,
                                                          const uint32_t* __restrict__ total /* |N_i| */, int* parent,
                                                          const int* __restrict__ rank /* BORDER: exclusive scan of the root flags */,
                                                          int* __restrict__ labels, int* __restrict__ err) {
#pragma clang fp contract(off)
  using R = typename Scalar<P4>::type;
  __shared__ ClusterGroupLds s_grp[kNbrQueriesPerBlock];
  const int lane = threadIdx.x, l = lane & 15, grp = lane >> 4;
  ClusterGroupLds& L = s_grp[grp];
  const size_t iq = (size_t)blockIdx.x * kNbrQueriesPerBlock + (size_t)grp;
  const bool have = iq < n;
  const int i = have ? (int)iq : 0;
  const int cap = (int)n;
  const P4 s = pts[i];
  const R qx = s.x, qy = s.y, qz = s.z;
  const double qxd = (double)qx, qyd = (double)qy, qzd = (double)qz;
  const uint32_t tot_i = total[i];
  const bool core_i = tot_i >= min_points;
  // (a point with a non-finite coordinate has |N_i| = 0: it is neither core nor walked)
  const bool active = have && (BORDER ? (!core_i && tot_i >= 2u) : core_i);
  const R r2 = (R)(eps * eps);
  // the query's cell (clamped as a number, before it becomes an integer) and the cells of the cube around it: floor((x - o) * inv_cell)
  // is monotonic in x and is what the index computed (cell_of), so a neighbour's cell lies between the cells of the cube's two faces;
  // the faces are pushed outwards by far more than the rounding of a d2 in either storage
  const int cx = (int)fmin(fmax(floor((qxd - g.ox) * g.inv_cell), 0.0), (double)(g.nx - 1));
  const int cy = (int)fmin(fmax(floor((qyd - g.oy) * g.inv_cell), 0.0), (double)(g.ny - 1));
  const int cz = (int)fmin(fmax(floor((qzd - g.oz) * g.inv_cell), 0.0), (double)(g.nz - 1));
  const double ew = eps * (1.0 + 1e-5) + 1e-18;
  const double ex = ew + 1e-12 * (fabs(qxd) + fabs(g.ox)), ey = ew + 1e-12 * (fabs(qyd) + fabs(g.oy)), ez = ew + 1e-12 * (fabs(qzd) + fabs(g.oz));
  int x0 = 0, x1 = 0, y0 = 0, y1 = -1, z0 = 0, z1 = -1;
  if (active) {
    x0 = (int)fmin(fmax(floor((qxd - ex - g.ox) * g.inv_cell), 0.0), (double)(g.nx - 1));
    x1 = (int)fmin(fmax(floor((qxd + ex - g.ox) * g.inv_cell), 0.0), (double)(g.nx - 1));
    y0 = (int)fmin(fmax(floor((qyd - ey - g.oy) * g.inv_cell), 0.0), (double)(g.ny - 1));
    y1 = (int)fmin(fmax(floor((qyd + ey - g.oy) * g.inv_cell), 0.0), (double)(g.ny - 1));
    z0 = (int)fmin(fmax(floor((qzd - ez - g.oz) * g.inv_cell), 0.0), (double)(g.nz - 1));
    z1 = (int)fmin(fmax(floor((qzd + ez - g.oz) * g.inv_cell), 0.0), (double)(g.nz - 1));
  }
  const int wy = y1 - y0 + 1;
  const int ntask = active ? wy * (z1 - z0 + 1) : 0;
  const int* __restrict__ cs = g.cell_start;
  const double B = (double)r2;

  int mine = i;            // hooking, lane 0 of the group: an ancestor of i, as far down as it has seen
  int best = 0x7fffffff;   // border: the smallest root among the core neighbours this lane has seen
  bool bad = false;

  for (int t0 = 0; __ballot(t0 < ntask) != 0ull; t0 += 16) {
    // ---- one row per lane: one range of the sorted cloud
    int s0 = 0, e0 = 0;
    const int t = t0 + l;
    if (t < ntask) {
      const int tz = t / wy;
      const int z = z0 + tz, y = y0 + (t - tz * wy);
      const double gz = z == cz ? 0.0 : nbr_gap_lo(qzd, g.oz, g.cell, cz, z), gy = y == cy ? 0.0 : nbr_gap_lo(qyd, g.oy, g.cell, cy, y);
      if (gz * gz + gy * gy < B) {
        const int row = (z * g.ny + y) * g.nx;
        s0 = cs[row + x0];
        e0 = cs[row + x1 + 1];
      }
    }
    // ---- lay the ranges of the 16 lanes end to end
    const int len0 = e0 - s0;
    const int incl = row_incl_scan(len0);
    const int T = row_last(incl);
    L.seg_off[l] = incl - len0;
    L.seg_base[l] = s0 - (incl - len0);
    O3DS_WAVE_SYNC();
    for (int f0 = 0; __ballot(f0 < T) != 0ull; f0 += 64) {
      // ---- four candidates per lane: flat number -> row (the last one whose first number is <= f; an empty row shares its successor's
      // number, which wins)
      int pos[4] = {0, 0, 0, 0};
#pragma unroll
      for (int step = 8; step >= 1; step >>= 1) {
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
      int cj[4];
      int accm = 0;  // (accepted slots as bits of a register)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const R d2 = nrm_d2<R>(cand[c].x, cand[c].y, cand[c].z, qx, qy, qz);
        cj[c] = (int)cand[c].i;
        accm |= ((f0 + l + 16 * c < T) && isfinite(d2) && d2 < r2) ? 1 << c : 0;
      }
#pragma unroll 1
      for (int c = 0; c < 4; ++c) {  // (one copy of the union code: the slot is picked by selects, not by unrolling)
        const int j = c == 0 ? cj[0] : c == 1 ? cj[1] : c == 2 ? cj[2] : cj[3];
        const bool acc = ((accm >> c) & 1) != 0;
        if constexpr (BORDER) {
          if (acc && total[j] >= min_points) best = min(best, parent[j]);  // (flattened: parent of a core point is its root)
        } else {
          // The sixteen lanes do not each unite i with their candidate: all of them would swap at parent[i], one would win and fifteen
          // would chase again (twelve failed swaps per successful one were counted on a lidar scan).  Each lane finds the root above its
          // candidate, the group takes the smallest of them, every other root found is hooked under that one -- swaps at sixteen
          // different words -- and lane 0 hooks i.
          int r = 0x7fffffff;
          if (acc && j < i && !bad && total[j] >= min_points) r = cl_find(parent, j, cap, &bad);
          int m = r;
#pragma unroll
          for (int k = 8; k >= 1; k >>= 1) m = min(m, __shfl_xor(m, k, 16));
          if (m != 0x7fffffff && !bad) {
            if (r != 0x7fffffff && r != m) (void)cl_unite(parent, r, m, cap, &bad);
            if (l == 0 && m != mine) mine = cl_unite(parent, mine, m, cap, &bad);  // (m == mine: i hangs under m already)
          }
        }
      }
    }
    O3DS_WAVE_SYNC();  // the row table is rewritten by the next round
  }

  if constexpr (BORDER) {
#pragma unroll
    for (int k = 8; k >= 1; k >>= 1) best = min(best, __shfl_xor(best, k, 16));
    if (have && l == 0) {
      int lab = -1;
      if (core_i)
        lab = rank[parent[i]];
      else if (best != 0x7fffffff)
        lab = rank[best];
      labels[i] = lab;
    }
  } else {
    if (active && !bad && mine < i) atomicMin(parent + i, mine);  // mine is an ancestor of i: the path of i gets shorter
    if (bad) *err = 1;
  }
}

// parent[i] = the root of i for every core point (whoever reads an entry meanwhile reads an ancestor of its point: either value serves),
// flags[i] = 1 iff i is a core point and a root; flags[n] = 0 is the scan's sentinel.  Roots are final: nothing hooks in this launch.
template <int = 0>
__global__ __launch_bounds__(kBlock) void cluster_flatten_kernel(int* parent, const uint32_t* __restrict__ total, uint32_t min_points, size_t n,
                                                                 int* __restrict__ flags, int* __restrict__ err) {
  const int cap = (int)n;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    int f = 0;
    if (total[i] >= min_points) {
      bool bad = false;
      const int r = cl_find(parent, (int)i, cap, &bad);
      if (bad) *err = 1;
      if (r != (int)i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      f = r == (int)i ? 1 : 0;
    }
    flags[i] = f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}

// sizes[c] += the points labelled c: a run of equal labels in consecutive lanes (clouds come in scan-line or voxel order: neighbours in the
// array are neighbours in space) is served by one atomic of its first lane (cell_run)
template <int = 0>
__global__ __launch_bounds__(kBlock) void cluster_sizes_kernel(const int* __restrict__ labels, size_t n, uint32_t* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  for (size_t i0 = (size_t)blockIdx.x * kBlock; i0 < n; i0 += (size_t)gridDim.x * kBlock) {  // whole wavefronts iterate together
    const size_t i = i0 + threadIdx.x;
    const int lab = i < n ? labels[i] : -1;
    int len, lead_lane;
    if (cell_run(lab, lane, &len, &lead_lane)) atomicAdd(sizes + lab, (uint32_t)len);
  }
}

// keep point i iff it has a label and its cluster holds at least min_size points; flags[n] = 0 is the scan's sentinel
template <int = 0>
__global__ __launch_bounds__(kBlock) void cluster_size_flag_kernel(const int* __restrict__ labels, const uint32_t* __restrict__ sizes, size_t n,
                                                                   uint32_t min_size, int* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const int lab = labels[i];
    flags[i] = (lab >= 0 && sizes[lab] >= min_size) ? 1 : 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}

}  // namespace o3ds
