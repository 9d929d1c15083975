// multi_icp_kernels.hpp -- the ICP pass against a LIST of resident targets (o3ds_icp_register_multi).
//
// One launch per pass: every query walks the target list inside the kernel, with the device functions of icp_kernels.hpp (the bound-pruned
// grid search, the record terms, the per-workgroup accumulation), called and not changed.
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
#include "icp_kernels.hpp"

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
  static_assert((64 / kGroup) * kSegMax >= kFarList, "a wavefront's share of s_seg holds the stage-3 list");
  static_assert(sizeof(FarItem<P4>) <= kStride * sizeof(double), "a parked far query fits its record slot");
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
  const size_t i = query_index<kQPB, 64 / kGroup>(n_live, blockIdx.x, ql, order);
  const bool live = i < n_live;  // uniform across the lanes of a group
  double px = 0, py = 0, pz = 0;
  if (live) {
    const P4 s = ((const P4*)a.src)[a.first + i];
    px = t00 * (double)s.x + t01 * (double)s.y + t02 * (double)s.z + t03;  // [O3D] PointCloud::Transform, as icp_pass_body
    py = t10 * (double)s.x + t11 * (double)s.y + t12 * (double)s.z + t13;
    pz = t20 * (double)s.x + t21 * (double)s.y + t22 * (double)s.z + t23;
  }
  const R qx = (R)px, qy = (R)py, qz = (R)pz;
  // UNION: the best match over the slots walked so far.  Its bound for the first slot is the match of the previous pass, whichever slot
  // that was in (any target point is a valid bound).
  NNBest<P4> cur;
  cur.d2 = (R)a.r2max;
  cur.pos = -1;
  cur.idx = -1;
  int cur_slot = -1;
  if (!joint && live && use_cache) {
    const int c = ma.cache[a.first + i];
    const int cs = c >> kMultiPosBits, cp = c & ((1 << kMultiPosBits) - 1);
    if (c >= 0 && cs < K && cp < ma.tgt[cs].n_tgt) {  // never trust the cache with an address
      const P4 t = ((const P4*)ma.tgt[cs].tpts)[cp];
      consider<P4, kCrop>(t, cp, true, qx, qy, qz, a.crop, cur);
      if (cur.pos != -1) cur_slot = cs;
    }
  }
  for (int k = 0; k < K; ++k) {  // uniform
    const MultiTargetDev tdv = ma.tgt[k];  // (a uniform copy: the descriptor lives in scalar registers while its slot is searched)
    const MultiTargetDev* td = &tdv;
    const P4* __restrict__ tp = (const P4*)td->tpts;
    const int kmax = td->kmax;
    // ---- this slot's starting bound
    NNBest<P4> best;
    best.d2 = (R)a.r2max;
    best.pos = -1;
    best.idx = -1;
    if (joint) {
      if (live && use_cache) {
        const int prev = ma.cache[(size_t)k * ma.cache_stride + a.first + i];
        if (prev >= 0 && prev < td->n_tgt) consider<P4, kCrop>(tp[prev], prev, true, qx, qy, qz, a.crop, best);
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
      nn = nn_search_group<P4, kCrop, kGroup, false>(td->grid, tp, qx, qy, qz, kmax, a.crop, gl_b, s_seg + ql * kSegMax, best, (R)0, col, &resolved, &kdone);
      if (!resolved && gl == 0) {  // park the query for stage 3 (its record slot is unused while the slots are searched)
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
      const int lane = threadIdx.x & 63;
      int2* list = s_seg + (threadIdx.x >> 6) * (64 / kGroup) * kSegMax;
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
        nn_search_wave_far<P4, kCrop, false>(td->grid, tp, it->x, it->y, it->z, kmax, a.crop, bq, lane, list, (R)0, col);
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
        nn.idx = it->idx;
      }
    }
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
        double* rec = s_rec + ql * kStride;
        if (live && w_pos != -1) {
          const MultiTargetDev* __restrict__ tw = ma.tgt + w_slot;
          const P4 q = ((const P4*)tw->tpts)[w_pos];
          const P4 nq = (!kGicp && p2p) ? P4{} : ((const P4*)tw->tnrm)[w_pos];
          write_record<P4, kGicp>(a, rec, p2p, px, py, pz, q, nq, i, t00, t01, t02, t10, t11, t12, t20, t21, t22);
        } else {
#pragma unroll
          for (int s = 0; s < kStride; ++s) rec[s] = 0.0;
        }
      }
    }
    lds_barrier();
    if (threadIdx.x == 0) s_far[0] = s_far[1] = 0;  // everyone is past the far list (ordered before its next use by the barrier below)
    if (emit) {
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
        a.partials[((size_t)(joint ? k : 0) * gridDim.x + blockIdx.x) * kRec + threadIdx.x] = v;
      }
    }
    lds_barrier();  // s_rec, s_red and the far list are reused by the next slot
  }
}

// The serial tail of a pass: sum the partial rows exactly (reduce_partials), convergence test, solve, T <- U * T (icp_step_block) -- one
// workgroup, as icp_reduce_update_kernel, with the fitness denominator taken from the device-held source count: den_mult x count
// (JOINT: the number of targets, fitness is the mean over them).
__global__ __launch_bounds__(kUpdBlock) void icp_multi_reduce_update_kernel(const double* __restrict__ partials, int nrows, IcpStateDev* state,
                                                                            size_t count, const int* count_dev, unsigned long long den_mult,
                                                                            int max_iter, double rel_fitness, double rel_rmse, int method,
                                                                            QuantumTable qt) {
  if (state->done) return;
  __shared__ double s_part[2 * (kUpdBlock / 32) * kRec];
  __shared__ double s_out[kRec];
  __shared__ double s_x[8], s_sc[8], s_U[16], s_T[16];
  __shared__ int s_go;
  const size_t n = count_dev ? min((size_t)*count_dev, count) : count;
  reduce_partials(partials, nrows, qt.q, s_part, s_out);
  icp_step_block(s_out, state, (unsigned long long)n * den_mult, max_iter, rel_fitness, rel_rmse, s_x, s_sc, s_U, s_T, &s_go, nullptr, method);
}

}  // namespace o3ds
#pragma clang fp contract(fast)
