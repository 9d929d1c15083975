// batch_icp_kernels.hpp -- the ICP pass of SEVERAL INDEPENDENT registrations in one launch (o3ds_icp_register_batch).
//
// A table in device memory holds one IcpPassArgs per live entry -- what a one-pair session holds: source, target index, crop, radius,
// quanta, state -- with `partials` the base of the entry's own partial rows and `nn_cache` its own match cache.  Beside it sits the
// exclusive prefix of the entries' workgroup counts (ceil(count / kQPB), at least one).  A workgroup finds its entry from blockIdx.x in
// the prefix, its batch inside the entry as blockIdx.x - start, and from there is the one-target path of icp_multi_accumulate_kernel:
// the device functions of icp_kernels.hpp (the bound-pruned grid search, the record terms, the per-workgroup accumulation), called and
// not changed, over the entry's own count, in the order pass_order gives for the entry's own pass number.  So the workgroup records of an
// entry are the records its one-pair registration sums, and the sums are exact (reduce_partials): every entry ends with the bits of
// o3ds_icp_register_dev.  Candidate sets are not kept: every pass searches, from the match of the previous pass as its bound.
// The table and the prefix are written by one host copy before the loop and by no kernel, so their uniform (scalar-cache) reads see
// nothing in flight; an entry's state is written by the update launch, which is another kernel.
#pragma once
#include "icp_kernels.hpp"

#pragma clang fp contract(off)  // as icp_kernels.hpp: the same source must round the same way in every kernel it is inlined into

namespace o3ds {

constexpr int kBatchMaxEntries = O3DS_BATCH_MAX_ENTRIES;
static_assert(kBatchMaxEntries <= 64, "one lane of a wavefront per entry in the search of the prefix");

struct IcpBatchArgs {
  const IcpPassArgs* entry;  // [n_entries], device memory: the live entries' sessions; partials / nn_cache are the entry's own
  const int* start;          // [n_entries + 1], device memory: exclusive prefix of the entries' workgroup counts
  int n_entries;
};

template <typename P4, bool kCrop, int kPassBlock, int kGroup, bool kGicp>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void icp_batch_accumulate_kernel(IcpBatchArgs ba) {
  constexpr int kQPB = kPassBlock / kGroup;
  constexpr int kStride = kGicp ? kRec : kRecSlots;
  constexpr int kSlices = kPassBlock / 32;
  using R = typename Scalar<P4>::type;
  static_assert((64 / kGroup) * kSegMax >= kFarList, "a wavefront's share of s_seg holds the stage-3 list");
  static_assert(sizeof(FarItem<P4>) <= kStride * sizeof(double), "a parked far query fits its record slot");
  // ---- whose workgroup is this: the number of entries that end at or before it (one prefix element per lane, one ballot; the same in
  // every wavefront of the workgroup)
  const int lane64 = threadIdx.x & 63;
  const int end = lane64 < ba.n_entries ? ba.start[lane64 + 1] : 0x7fffffff;
  const int e = __popcll(__ballot(end <= (int)blockIdx.x));  // uniform
  if (e >= ba.n_entries) return;                             // (the grid is start[n_entries] workgroups)
  const IcpPassArgs& a = ba.entry[e];
  const int first_wg = ba.start[e];
  const size_t b = (size_t)((int)blockIdx.x - first_wg);  // this workgroup's batch of the entry's queries
  if (a.state->done) return;  // this entry's loop has terminated: keep its previous partials
  __shared__ double s_rec[kQPB * kStride];
  __shared__ double s_red[kSlices][kRec];
  __shared__ int2 s_seg[kQPB * kSegMax];
  __shared__ int s_far[2 + kQPB];  // [0] count, [1] next, [2..] query slots parked for stage 3
  double* __restrict__ row = a.partials + b * kRec;
  const int pass = a.state->pass;
  const bool use_cache = pass > 0;
  const int order = pass_order(pass);
  const size_t n_live = deal_count(a);
  const size_t n_batches = (n_live + kQPB - 1) / kQPB;
  if (b >= n_batches) {  // (the entry's workgroups are sized by the upper bound of its count, and there is always one) no query: zeros
    if (threadIdx.x < kRec) row[threadIdx.x] = 0.0;
    return;
  }
  const double* Tm = a.state->T;
  const double t00 = to_sgpr(Tm[0]), t10 = to_sgpr(Tm[1]), t20 = to_sgpr(Tm[2]), t01 = to_sgpr(Tm[4]), t11 = to_sgpr(Tm[5]),
               t21 = to_sgpr(Tm[6]), t02 = to_sgpr(Tm[8]), t12 = to_sgpr(Tm[9]), t22 = to_sgpr(Tm[10]), t03 = to_sgpr(Tm[12]),
               t13 = to_sgpr(Tm[13]), t23 = to_sgpr(Tm[14]);
  const int gl = threadIdx.x & (kGroup - 1), ql = threadIdx.x / kGroup;
  const int term = threadIdx.x & 31, qs = threadIdx.x >> 5;
  const bool p2p = a.method == O3DS_ICP_POINT_TO_POINT;
  const int ta = term_slot(p2p ? kPackA_p2p.lo : kPackA.lo, p2p ? kPackA_p2p.hi : kPackA.hi, term);
  const int tb = term_slot(p2p ? kPackB_p2p.lo : kPackB.lo, p2p ? kPackB_p2p.hi : kPackB.hi, term);
  if (threadIdx.x == 0) s_far[0] = s_far[1] = 0;
  lds_barrier();
  const size_t i = query_index<kQPB, 64 / kGroup>(n_live, b, ql, order);
  const bool live = i < n_live;  // uniform across the lanes of a group
  double px = 0, py = 0, pz = 0;
  if (live) {
    const P4 s = ((const P4*)a.src)[a.first + i];
    px = t00 * (double)s.x + t01 * (double)s.y + t02 * (double)s.z + t03;  // [O3D] PointCloud::Transform, as icp_pass_body
    py = t10 * (double)s.x + t11 * (double)s.y + t12 * (double)s.z + t13;
    pz = t20 * (double)s.x + t21 * (double)s.y + t22 * (double)s.z + t23;
  }
  const R qx = (R)px, qy = (R)py, qz = (R)pz;
  const P4* __restrict__ tp = (const P4*)a.tpts;
  const GridDev grid = a.grid;  // (a uniform copy: the descriptor lives in scalar registers while the target is searched)
  const CropDev crop = a.crop;
  const int kmax = a.kmax;
  // ---- the starting bound: the match of the previous pass
  NNBest<P4> best;
  best.d2 = (R)a.r2max;
  best.pos = -1;
  best.idx = -1;
  if (live && use_cache) {
    const int prev = a.nn_cache[a.first + i];
    if (prev >= 0 && prev < a.n_tgt) consider<P4, kCrop>(tp[prev], prev, true, qx, qy, qz, crop, best);  // never trust the cache with an address
  }
  // ---- stages 1 and 2 by the query's group, stage 3 pooled over the workgroup (as icp_pass_body)
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
    nn = nn_search_group<P4, kCrop, kGroup, false>(grid, tp, qx, qy, qz, kmax, crop, gl_b, s_seg + ql * kSegMax, best, (R)0, col, &resolved, &kdone);
    if (!resolved && gl == 0) {  // park the query for stage 3 (its record slot is unused while the target is searched)
      FarItem<P4>* it = (FarItem<P4>*)(s_rec + ql * kStride);
      it->x = qx;
      it->y = qy;
      it->z = qz;
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
    int2* list = s_seg + (threadIdx.x >> 6) * (64 / kGroup) * kSegMax;
    for (int f = wave_pop(&s_far[1], lane64); f < n_far; f = wave_pop(&s_far[1], lane64)) {  // f is scalar: a uniform loop
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
      nn_search_wave_far<P4, kCrop, false>(grid, tp, it->x, it->y, it->z, kmax, crop, bq, lane64, list, (R)0, col);
      // (every lane stores the same winner: no lane-0 branch inside this loop, see icp_pass_body)
      it->d2 = bq.d2;
      it->pos = bq.pos;
      it->idx = bq.idx;
    }
    lds_barrier();
    if (!resolved) {
      const FarItem<P4>* it = (const FarItem<P4>*)(s_rec + ql * kStride);
      nn.d2 = it->d2;
      nn.pos = it->pos;
      nn.idx = it->idx;  // (the group's lane 0 overwrites this slot with the record below: same wavefront, after this read)
    }
  }
  // ---- records: one per query
  if (gl == 0) {
    if (live) a.nn_cache[a.first + i] = nn.pos;
    double* rec = s_rec + ql * kStride;
    if (live && nn.pos != -1) {
      const P4 q = tp[nn.pos];
      const P4 nq = (!kGicp && p2p) ? P4{} : ((const P4*)a.tnrm)[nn.pos];
      write_record<P4, kGicp>(a, rec, p2p, px, py, pz, q, nq, i, t00, t01, t02, t10, t11, t12, t20, t21, t22);
    } else {
#pragma unroll
      for (int s = 0; s < kStride; ++s) rec[s] = 0.0;
    }
  }
  lds_barrier();
  // ---- the workgroup's record: 32 terms x kSlices query slices, then the slices in fixed order (icp_pass_body's arithmetic)
  double acc = 0.0;
#pragma unroll
  for (int qq = 0; qq < kQPB / kSlices; ++qq) {
    const double* rec = s_rec + (qs * (kQPB / kSlices) + qq) * kStride;
    if (kGicp)
      acc += rec[term];
    else
      acc = fma(rec[ta], rec[tb], acc);
  }
  s_red[qs][term] = acc;
  lds_barrier();
  if (threadIdx.x < kRec) {
    double v = 0.0;
#pragma unroll
    for (int s = 0; s < kSlices; ++s) v += s_red[s][threadIdx.x];
    if (threadIdx.x >= 30) v = 0.0;
    row[threadIdx.x] = v;
  }
}

// The serial tail of a pass for every entry: workgroup k sums entry k's partial rows exactly (reduce_partials, with the entry's quanta),
// then convergence test, solve, T <- U * T on the entry's state (icp_step_block) -- what icp_reduce_update_kernel does for one pair, with
// the fitness denominator taken from the device-held source count where the host has an upper bound only.
__global__ __launch_bounds__(kUpdBlock) void icp_batch_reduce_update_kernel(IcpBatchArgs ba, int max_iter, double rel_fitness, double rel_rmse,
                                                                            int method) {
  const IcpPassArgs& a = ba.entry[blockIdx.x];
  IcpStateDev* state = const_cast<IcpStateDev*>(a.state);
  if (state->done) return;
  __shared__ double s_part[2 * (kUpdBlock / 32) * kRec];
  __shared__ double s_out[kRec];
  __shared__ double s_x[8], s_sc[8], s_U[16], s_T[16];
  __shared__ int s_go;
  const int nrows = ba.start[blockIdx.x + 1] - ba.start[blockIdx.x];
  const size_t n = deal_count(a);
  reduce_partials(a.partials, nrows, a.q_hi, s_part, s_out);
  icp_step_block(s_out, state, (unsigned long long)n, max_iter, rel_fitness, rel_rmse, s_x, s_sc, s_U, s_T, &s_go, nullptr, method);
}

}  // namespace o3ds
#pragma clang fp contract(fast)
