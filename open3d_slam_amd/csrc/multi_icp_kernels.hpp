// multi_icp_kernels.hpp -- the ICP pass against a LIST of resident targets (o3ds_icp_register_multi).
//
// One launch per pass: every query walks the target list inside the kernel and searches each target with the list-form pass body of
// list_icp_kernels.hpp (place the query, search one target from a bound, write the record, sum the row); what is here is what a list
// of targets adds: the carried match of UNION, the per-slot cache of JOINT, the slot loop and when a record is emitted.
//   UNION  the best (d2, slot, position) so far is carried in registers and is the STARTING BOUND of the search in the next target: the
//          search only touches cells inside the ball of its bound, so a query matched at 5 cm in one target visits next to nothing in the
//          others.  Equal d2: the lower slot wins, inside a slot the smaller original index (the one-target rule) -- the order of the
//          cloud the targets would form when appended in slot order.  One record per query, one partial row per workgroup.
//   JOINT  every target is searched from its own bound and contributes its own record; a workgroup writes ONE PARTIAL ROW PER TARGET
//          (row = slot * gridDim.x + workgroup), each the very row icp_accumulate_kernel writes for that target alone.  The rows are
//          summed exactly by reduce_partials (split_exact), so K copies of one target give K times the one-target record, bit for bit.
// The queries are dealt out over the device-held source count (deal_count), one batch of kPassBlock / kGroup queries per workgroup, in
// the order pass_order gives: the partition of icp_fused_kernel, hence the same workgroup records wherever the correspondences agree.
// Candidate sets (Collect / SetRef) are not kept by this form: every pass searches, from the match of the previous pass as its bound
// (`cache`).
#pragma once
#include "list_icp_kernels.hpp"

#pragma clang fp contract(off)  // as icp_kernels.hpp: the same source must round the same way in every kernel it is inlined into

namespace o3ds {

constexpr int kMultiMaxTargets = O3DS_MULTI_MAX_TARGETS;
constexpr int kMultiPosBits = 28;  // UNION match cache: slot << 28 | position in that slot's cell-sorted arrays

// what the search and the record need of one target (IcpPassArgs::tpts / tnrm / grid / kmax / n_tgt of a one-target session)
struct MultiTargetDev {
  const void* tpts;
  const void* tnrm;
  GridDev grid;
  int kmax;
  int n_tgt;
};

struct IcpMultiArgs {
  IcpPassArgs pass;           // source, crop, radius, quanta, method, state, partials; its one-target fields (tpts, grid, nn_cache ...) are unused
  const MultiTargetDev* tgt;  // [n_slots], device memory: the non-empty targets in slot order
  int n_slots;
  int joint;                  // 0: UNION, 1: JOINT
  int* cache;                 // UNION [count]: slot << kMultiPosBits | position; JOINT [n_slots][cache_stride]: position; -1: none
  size_t cache_stride;
};

template <typename P4, bool kCrop, int kPassBlock, int kGroup, bool kGicp>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(4))) void icp_multi_accumulate_kernel(IcpMultiArgs ma) {
  constexpr int kQPB = kPassBlock / kGroup;
  constexpr int kStride = kGicp ? kRec : kRecSlots;
  constexpr int kSlices = kPassBlock / 32;
  using R = typename Scalar<P4>::type;
  using I = typename Scalar<P4>::index;
  const IcpPassArgs& a = ma.pass;
  if (a.state->done) return;  // device-side loop already terminated: keep the previous partials
  __shared__ double s_rec[kQPB * kStride];
  __shared__ double s_red[kSlices][kRec];
  __shared__ int2 s_seg[kQPB * kSegMax];
  __shared__ int s_far[2 + kQPB];  // [0] count, [1] next, [2..] query slots parked for stage 3
  const int pass = a.state->pass;
  const bool use_cache = pass > 0;
  const int order = pass_order(pass);
  const size_t n_live = deal_count(a);
  const size_t n_batches = (n_live + kQPB - 1) / kQPB;
  const bool joint = ma.joint != 0;
  const int K = ma.n_slots;
  if ((size_t)blockIdx.x >= n_batches) {  // (the launch is sized by the upper bound of the count) no query: rows of zeros
    if (threadIdx.x < kRec) {
      const int rows = joint ? K : 1;
      for (int k = 0; k < rows; ++k) a.partials[((size_t)k * gridDim.x + blockIdx.x) * kRec + threadIdx.x] = 0.0;
    }
    return;
  }
  const int gl = threadIdx.x & (kGroup - 1), ql = threadIdx.x / kGroup;
  const bool p2p = a.method == O3DS_ICP_POINT_TO_POINT;
  const size_t i = query_index<kQPB, 64 / kGroup>(n_live, blockIdx.x, ql, order);
  const bool live = i < n_live;  // uniform across the lanes of a group
  // (in front of the first barrier: behind it the compiler no longer reads the pose through the scalar cache)
  const ListQuery<R> q = list_place_query<P4>(a, live, i);
  if (threadIdx.x == 0) s_far[0] = s_far[1] = 0;
  lds_barrier();
  // UNION: the best match over the slots walked so far.  Its bound for the first slot is the match of the previous pass, whichever slot
  // that was in (any target point is a valid bound).
  NNBest<P4> cur;
  cur.d2 = (R)a.r2max;
  cur.pos = -1;
  cur.idx = NNBest<P4>::kNoIdx;
  int cur_slot = -1;
  if (!joint && live && use_cache) {
    const int c = ma.cache[a.first + i];
    const int cs = c >> kMultiPosBits, cp = c & ((1 << kMultiPosBits) - 1);
    if (c >= 0 && cs < K && cp < ma.tgt[cs].n_tgt) {  // never trust the cache with an address
      const P4 t = ((const P4*)ma.tgt[cs].tpts)[cp];
      consider<P4, kCrop>(t, cp, true, q.qx, q.qy, q.qz, a.crop, cur);
      if (cur.pos != -1) cur_slot = cs;
    }
  }
  for (int k = 0; k < K; ++k) {  // uniform
    const MultiTargetDev tdv = ma.tgt[k];  // (a uniform copy: the descriptor lives in scalar registers while its slot is searched)
    const MultiTargetDev* td = &tdv;
    const P4* __restrict__ tp = (const P4*)td->tpts;
    // ---- this slot's starting bound
    NNBest<P4> best;
    best.d2 = (R)a.r2max;
    best.pos = -1;
    best.idx = NNBest<P4>::kNoIdx;
    if (joint) {
      if (live && use_cache) {
        const int prev = ma.cache[(size_t)k * ma.cache_stride + a.first + i];
        if (prev >= 0 && prev < td->n_tgt) consider<P4, kCrop>(tp[prev], prev, true, q.qx, q.qy, q.qz, a.crop, best);
      }
    } else {
      // a candidate of this slot beats the carried match if it is strictly nearer, or equally near and from a LOWER slot than the match
      // (index "infinity": consider() then lets the tie win); against a match of this very slot the one-target rule applies
      best.d2 = cur.d2;
      if (cur_slot == k) {
        best.pos = cur.pos;
        best.idx = cur.idx;
      } else if (cur_slot > k) {
        best.idx = sizeof(I) == 8 ? (I)0x7fffffffffffffffll : (I)0x7fffffff;
      }
    }
    const NNBest<P4> nn = list_search_target<P4, kCrop, kGroup, kStride>(td->grid, tp, td->kmax, a.crop, live, q, best, s_rec, s_seg, s_far);
    if (!joint && live) {
      if (cur_slot == k) {
        cur = nn;
      } else if (nn.pos != -1) {
        cur = nn;
        cur_slot = k;
      }
    }
    const bool emit = joint || k == K - 1;  // uniform
    if (emit) {
      // ---- records: one per query (UNION: of the winner over all slots; JOINT: of this slot's match)
      if (gl == 0) {
        const int w_slot = joint ? k : cur_slot;
        const int w_pos = joint ? nn.pos : cur.pos;
        if (live) {
          if (joint)
            ma.cache[(size_t)k * ma.cache_stride + a.first + i] = w_pos;
          else
            ma.cache[a.first + i] = w_pos == -1 ? -1 : ((w_slot << kMultiPosBits) | w_pos);
        }
        const MultiTargetDev* __restrict__ tw = ma.tgt + max(w_slot, 0);  // (no match: slot -1, and the record is zeros)
        list_write_record<P4, kGicp, kStride>(a, s_rec + ql * kStride, p2p, live, i, q, tw->tpts, tw->tnrm, w_pos);
      }
    }
    lds_barrier();
    if (threadIdx.x == 0) s_far[0] = s_far[1] = 0;  // everyone is past the far list (ordered before its next use by the barrier below)
    if (emit) list_sum_row<kPassBlock, kGroup, kGicp>(s_rec, s_red, p2p, a.partials + ((size_t)(joint ? k : 0) * gridDim.x + blockIdx.x) * kRec);
    lds_barrier();  // s_rec, s_red and the far list are reused by the next slot
  }
}

// The serial tail of a pass (list_reduce_update), one workgroup, with the fitness denominator taken from the device-held source count:
// den_mult x count (JOINT: the number of targets, fitness is the mean over them).
__global__ __launch_bounds__(kUpdBlock) void icp_multi_reduce_update_kernel(const double* __restrict__ partials, int nrows, IcpStateDev* state,
                                                                            size_t count, const int* count_dev, unsigned long long den_mult,
                                                                            int max_iter, double rel_fitness, double rel_rmse, int method,
                                                                            QuantumTable qt, const void* src, int src_f64) {
  if (state->done) return;
  const size_t n = count_dev ? min((size_t)*count_dev, count) : count;
  list_reduce_update(partials, nrows, qt.q, state, (unsigned long long)n * den_mult, max_iter, rel_fitness, rel_rmse, method, src, src_f64);
}

}  // namespace o3ds
#pragma clang fp contract(fast)
