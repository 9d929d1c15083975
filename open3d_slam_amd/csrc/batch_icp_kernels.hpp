// batch_icp_kernels.hpp -- the ICP pass of SEVERAL INDEPENDENT registrations in one launch (o3ds_icp_register_batch).
//
// A table in device memory holds one IcpPassArgs per live entry -- what a one-pair session holds: source, target index, crop, radius,
// quanta, state -- with `partials` the base of the entry's own partial rows and `nn_cache` its own match cache.  Beside it sits the
// exclusive prefix of the entries' workgroup counts (ceil(count / kQPB), at least one).  A workgroup finds its entry from blockIdx.x in
// the prefix, its batch inside the entry as blockIdx.x - start, and from there makes one call of each piece of the list-form pass body
// (list_icp_kernels.hpp: place the query, search the target from a bound, write the record, sum the row) over the entry's own count,
// in the order pass_order gives for the entry's own pass number.  So the workgroup records of an entry are the records its one-pair
// registration sums, and the sums are exact (reduce_partials): every entry ends with the bits of o3ds_icp_register_dev.  Candidate
// sets are not kept: every pass searches, from the match of the previous pass as its bound.
// The table and the prefix are written by one host copy before the loop and by no kernel, so their uniform (scalar-cache) reads see
// nothing in flight; an entry's state is written by the update launch, which is another kernel.
#pragma once
#include "list_icp_kernels.hpp"

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
  const int gl = threadIdx.x & (kGroup - 1), ql = threadIdx.x / kGroup;
  const bool p2p = a.method == O3DS_ICP_POINT_TO_POINT;
  const size_t i = query_index<kQPB, 64 / kGroup>(n_live, b, ql, order);
  const bool live = i < n_live;  // uniform across the lanes of a group
  // (in front of the first barrier: behind it the compiler no longer reads the pose through the scalar cache)
  const ListQuery<R> q = list_place_query<P4>(a, live, i);
  if (threadIdx.x == 0) s_far[0] = s_far[1] = 0;
  lds_barrier();
  const P4* __restrict__ tp = (const P4*)a.tpts;
  const GridDev grid = a.grid;  // (a uniform copy: the descriptor lives in scalar registers while the target is searched)
  const CropDev crop = a.crop;
  // ---- the starting bound: the match of the previous pass
  NNBest<P4> best;
  best.d2 = (R)a.r2max;
  best.pos = -1;
  best.idx = NNBest<P4>::kNoIdx;
  if (live && use_cache) {
    const int prev = a.nn_cache[a.first + i];
    if (prev >= 0 && prev < a.n_tgt) consider<P4, kCrop>(tp[prev], prev, true, q.qx, q.qy, q.qz, crop, best);  // never trust the cache with an address
  }
  const NNBest<P4> nn = list_search_target<P4, kCrop, kGroup, kStride>(grid, tp, a.kmax, crop, live, q, best, s_rec, s_seg, s_far);
  // ---- records: one per query
  if (gl == 0) {
    if (live) a.nn_cache[a.first + i] = nn.pos;
    list_write_record<P4, kGicp, kStride>(a, s_rec + ql * kStride, p2p, live, i, q, a.tpts, a.tnrm, nn.pos);
  }
  lds_barrier();
  list_sum_row<kPassBlock, kGroup, kGicp>(s_rec, s_red, p2p, row);
}

// The serial tail of a pass for every entry: workgroup k runs list_reduce_update over entry k's partial rows, with the entry's quanta, on
// the entry's state, with the fitness denominator taken from the device-held source count where the host has an upper bound only.
__global__ __launch_bounds__(kUpdBlock) void icp_batch_reduce_update_kernel(IcpBatchArgs ba, int max_iter, double rel_fitness, double rel_rmse,
                                                                            int method) {
  const IcpPassArgs& a = ba.entry[blockIdx.x];
  IcpStateDev* state = const_cast<IcpStateDev*>(a.state);
  if (state->done) return;
  list_reduce_update(a.partials, ba.start[blockIdx.x + 1] - ba.start[blockIdx.x], a.q_hi, state, (unsigned long long)deal_count(a), max_iter, rel_fitness,
                     rel_rmse, method, a.src, a.src_f64);
}

}  // namespace o3ds
#pragma clang fp contract(fast)
