// list_icp_kernels.hpp -- the pass body and the tail of the LIST forms of the ICP pass: icp_multi_accumulate_kernel (multi_icp_kernels.hpp,
// a list of targets) and icp_batch_accumulate_kernel (batch_icp_kernels.hpp, a list of registrations), DESIGN.md sections 7.4 and 7.5.
//
// Both kernels serve one batch of kPassBlock / kGroup queries per workgroup and call, per query, the pieces below: place the query,
// search one target from a bound, write the record, sum the records into the workgroup's row.  Each piece is the arithmetic of
// icp_pass_body (icp_kernels.hpp) without candidate sets, keys, stats and trace, built on the same nn_search_group / nn_search_wave_far /
// write_record, so a list form's workgroup record is the record the one-pair kernels write for the same correspondences.
//
// icp_pass_body does NOT call these functions: the one-pair kernels (the benchmark's path, at their register limit: see kSingle there)
// keep their own copy of the search pass in icp_kernels.hpp.  A change to the stage-3 drain loop, to the parking of a far query, to the
// record write or to the slice arithmetic is made in two places: there and here.
#pragma once
#include "icp_kernels.hpp"

#pragma clang fp contract(off)  // as icp_kernels.hpp: the same source must round the same way in every kernel it is inlined into

namespace o3ds {

// a query as its lanes hold it: the pose in scalar registers, the transformed point in f64 (the record's) and rounded to storage type
// (the search's)
template <typename R>
struct ListQuery {
  double t00, t10, t20, t01, t11, t21, t02, t12, t22, t03, t13, t23;
  double px, py, pz;
  R qx, qy, qz;
};

template <typename P4>
__device__ __forceinline__ ListQuery<typename Scalar<P4>::type> list_place_query(const IcpPassArgs& a, bool live, size_t i) {
  using R = typename Scalar<P4>::type;
  const double* Tm = a.state->T;
  ListQuery<R> q;
  q.t00 = to_sgpr(Tm[0]), q.t10 = to_sgpr(Tm[1]), q.t20 = to_sgpr(Tm[2]), q.t01 = to_sgpr(Tm[4]), q.t11 = to_sgpr(Tm[5]),
  q.t21 = to_sgpr(Tm[6]), q.t02 = to_sgpr(Tm[8]), q.t12 = to_sgpr(Tm[9]), q.t22 = to_sgpr(Tm[10]), q.t03 = to_sgpr(Tm[12]),
  q.t13 = to_sgpr(Tm[13]), q.t23 = to_sgpr(Tm[14]);
  q.px = 0, q.py = 0, q.pz = 0;
  if (a.method == O3DS_ICP_POINT_TO_POINT && threadIdx.x == 0) {  // the record's pivot, for list_sum_row (behind the callers' barriers)
    double c[3] = {0.0, 0.0, 0.0};
    if (deal_count(a) > 0) p2p_pivot(Tm, a.src, (int)(sizeof(R) == 8), c);
    double* s_pivot = p2p_pivot_lds();
    s_pivot[0] = c[0], s_pivot[1] = c[1], s_pivot[2] = c[2];
  }
  if (live) {
    const P4 s = ((const P4*)a.src)[a.first + i];
    q.px = q.t00 * (double)s.x + q.t01 * (double)s.y + q.t02 * (double)s.z + q.t03;  // [O3D] PointCloud::Transform, as icp_pass_body
    q.py = q.t10 * (double)s.x + q.t11 * (double)s.y + q.t12 * (double)s.z + q.t13;
    q.pz = q.t20 * (double)s.x + q.t21 * (double)s.y + q.t22 * (double)s.z + q.t23;
  }
  q.qx = (R)q.px, q.qy = (R)q.py, q.qz = (R)q.pz;
  return q;
}

// The nearest point of one target to this group's query, from the bound `best`: stages 1 and 2 by the query's group, stage 3 pooled
// over the workgroup (as icp_pass_body).  Called by every thread of the workgroup (it holds barriers); s_far ([0] count, [1] next,
// [2..] query slots parked for stage 3) is zero on entry and is reset by the caller, behind a barrier, before the next call.
template <typename P4, bool kCrop, int kGroup, int kStride>
__device__ __forceinline__ NNBest<P4> list_search_target(const GridDev& grid, const P4* __restrict__ tp, int kmax, const CropDev& crop, bool live,
                                                         const ListQuery<typename Scalar<P4>::type>& q, const NNBest<P4>& best, double* s_rec,
                                                         int2* s_seg, int* s_far) {
  using R = typename Scalar<P4>::type;
  static_assert((64 / kGroup) * kSegMax >= kFarList, "a wavefront's share of s_seg holds the stage-3 list");
  static_assert(sizeof(FarItem<P4>) <= kStride * sizeof(double), "a parked far query fits its record slot");
  const int gl = threadIdx.x & (kGroup - 1), ql = threadIdx.x / kGroup;
  NNBest<P4> nn = best;
  bool resolved = true;
  if (live) {
    int kdone;
    Collect<R> col;
    col.tau2 = (R)0;
    col.cnt = nullptr;
    col.list = nullptr;
    int gl_b = gl;
    asm volatile("" : "+v"(gl_b));
    nn = nn_search_group<P4, kCrop, kGroup, false>(grid, tp, q.qx, q.qy, q.qz, kmax, crop, gl_b, s_seg + ql * kSegMax, best, (R)0, col, &resolved, &kdone);
    if (!resolved && gl == 0) {  // park the query for stage 3 (its record slot is unused while a target is searched)
      FarItem<P4>* it = (FarItem<P4>*)(s_rec + ql * kStride);
      it->x = q.qx;
      it->y = q.qy;
      it->z = q.qz;
      it->d2 = nn.d2;
      it->m = (R)0;
      it->tau2 = (R)0;
      it->idx = nn.idx;
      it->pos = nn.pos;
      const int f = atomicAdd(&s_far[0], 1);
      s_far[2 + f] = ql;
    }
  }
  lds_barrier();
  const int n_far = __builtin_amdgcn_readfirstlane(s_far[0]);
  if (n_far > 0) {  // workgroup-uniform
    const int lane = threadIdx.x & 63;
    int2* list = s_seg + (threadIdx.x >> 6) * (64 / kGroup) * kSegMax;
    const int side_recip = far_side_recip(kmax);
    for (int f = wave_pop(&s_far[1], lane); f < n_far; f = wave_pop(&s_far[1], lane)) {  // f is scalar: a uniform loop
      const int slot = s_far[2 + f];
      FarItem<P4>* it = (FarItem<P4>*)(s_rec + slot * kStride);
      NNBest<P4> bq;
      bq.d2 = it->d2;
      bq.pos = it->pos;
      bq.idx = it->idx;
      Collect<R> col;
      col.tau2 = (R)0;
      col.cnt = nullptr;
      col.list = nullptr;
      nn_search_wave_far<P4, kCrop, false>(grid, tp, it->x, it->y, it->z, kmax, crop, bq, lane, side_recip, list, (R)0, col);
      // every lane holds the same winner and stores it (same address, same value): no lane-0 branch inside this loop --
      // with one, the structurised code re-ran the body for the other lanes forever (seen on ROCm 7.2)
      it->d2 = bq.d2;
      it->pos = bq.pos;
      it->idx = bq.idx;
    }
    lds_barrier();
    if (!resolved) {
      const FarItem<P4>* it = (const FarItem<P4>*)(s_rec + ql * kStride);
      nn.d2 = it->d2;
      nn.pos = it->pos;
      nn.idx = it->idx;  // (the group's lane 0 overwrites this slot with the record: same wavefront, after this read)
    }
  }
  return nn;
}

// the record of query i against position `pos` of a target's cell-sorted arrays, or zeros (no match, no query): lane 0 of the group
template <typename P4, bool kGicp, int kStride>
__device__ __forceinline__ void list_write_record(const IcpPassArgs& a, double* rec, bool p2p, bool live, size_t i,
                                                  const ListQuery<typename Scalar<P4>::type>& q, const void* tpts, const void* tnrm, int pos) {
  if (live && pos != -1) {
    const P4 t = ((const P4*)tpts)[pos];
    const P4 nt = (!kGicp && p2p) ? P4{} : ((const P4*)tnrm)[pos];
    write_record<P4, kGicp>(a, rec, p2p, q.px, q.py, q.pz, t, nt, i, q.t00, q.t01, q.t02, q.t10, q.t11, q.t12, q.t20, q.t21, q.t22);
  } else {
#pragma unroll
    for (int s = 0; s < kStride; ++s) rec[s] = 0.0;
  }
}

// the workgroup's record from its queries' records (complete: behind a barrier): 32 terms x kPassBlock / 32 query slices, then the
// slices in fixed order (icp_pass_body's arithmetic), stored to `row`
template <int kPassBlock, int kGroup, bool kGicp>
__device__ __forceinline__ void list_sum_row(const double* s_rec, double (*s_red)[kRec], bool p2p, double* __restrict__ row) {
  constexpr int kQPB = kPassBlock / kGroup;
  constexpr int kStride = kGicp ? kRec : kRecSlots;
  constexpr int kSlices = kPassBlock / 32;
  const int term = threadIdx.x & 31, qs = threadIdx.x >> 5;
  const int ta = term_slot(p2p ? kPackA_p2p.lo : kPackA.lo, p2p ? kPackA_p2p.hi : kPackA.hi, term);
  const int tb = term_slot(p2p ? kPackB_p2p.lo : kPackB.lo, p2p ? kPackB_p2p.hi : kPackB.hi, term);
  double acc = 0.0;
  if (!kGicp && p2p) {  // uniform: the slots relative to the pivot list_place_query left (as icp_pass_body)
    const double* s_pivot = p2p_pivot_lds();
    const double pa = p2p_pivot_of_slot(s_pivot, ta), pb = p2p_pivot_of_slot(s_pivot, tb);
#pragma unroll
    for (int qq = 0; qq < kQPB / kSlices; ++qq) {
      const double* rec = s_rec + (qs * (kQPB / kSlices) + qq) * kStride;
      const double one = rec[7];
      acc = fma(fma(-pa, one, rec[ta]), fma(-pb, one, rec[tb]), acc);
    }
  } else {
#pragma unroll
    for (int qq = 0; qq < kQPB / kSlices; ++qq) {
      const double* rec = s_rec + (qs * (kQPB / kSlices) + qq) * kStride;
      if (kGicp)
        acc += rec[term];
      else
        acc = fma(rec[ta], rec[tb], acc);
    }
  }
  s_red[qs][term] = acc;
  lds_barrier();
  if (threadIdx.x < kRec) {
    double v = 0.0;
#pragma unroll
    for (int s = 0; s < kSlices; ++s) v += s_red[s][threadIdx.x];
    if (threadIdx.x >= 30) v = 0.0;
    // (the store's address is formed HERE: left to itself the compiler forms row + threadIdx.x in the prologue and keeps the pair of
    // registers across the whole search, which the crop + generalized multi-target kernel does not have -- it spilt them)
    int tx = threadIdx.x;
    asm volatile("" : "+v"(tx));
    row[tx] = v;
  }
}

// The serial tail of a pass, one workgroup of kUpdBlock threads per state: sum the partial rows exactly (reduce_partials, with the
// quanta q_hi), convergence test, solve, T <- U * T (icp_step_block) -- what icp_reduce_update_kernel does for one pair.  `den` is the
// fitness denominator.
__device__ __forceinline__ void list_reduce_update(const double* __restrict__ partials, int nrows, const double* q_hi, IcpStateDev* state,
                                                   unsigned long long den, int max_iter, double rel_fitness, double rel_rmse, int method,
                                                   const void* src, int src_f64) {
  __shared__ double s_part[2 * (kUpdBlock / 32) * kRec];
  __shared__ double s_out[kRec];
  __shared__ double s_x[8], s_sc[8], s_U[16];
  __shared__ int s_go;
  reduce_partials(partials, nrows, q_hi, s_part, s_out);
  icp_step_block(s_out, state, den, max_iter, rel_fitness, rel_rmse, s_x, s_sc, s_U, &s_go, nullptr, method, nullptr, false, src, src_f64);
}

}  // namespace o3ds
#pragma clang fp contract(fast)
