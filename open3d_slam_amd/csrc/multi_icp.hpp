// multi_icp.hpp -- o3ds_icp_register_multi: one registration against a list of resident targets (o3ds_backend.h).
// Included at the end of backend.hip: it opens one ordinary session per target (begin_session: validation, index, grid, quanta) and
// collects what the search needs of each into the descriptor table the pass kernel of multi_icp_kernels.hpp walks.
#pragma once
#include "multi_icp_kernels.hpp"

namespace {

template <typename P4>
void launch_multi_accumulate_t(o3ds_handle h, const IcpMultiArgs& ma, int nblocks) {
  with_crop_and_estimator(h->session_crop, h->session_method == O3DS_ICP_GENERALIZED, [&](auto crop, auto gicp) {
    icp_multi_accumulate_kernel<P4, decltype(crop)::value, kIcpBlock, 4, decltype(gicp)::value><<<nblocks, kIcpBlock, 0, h->stream>>>(ma);
  });
}

void launch_multi_accumulate(o3ds_handle h, const IcpMultiArgs& ma, int nblocks) {
  DISPATCH(h->session_precision, launch_multi_accumulate_t, h, ma, nblocks);
}

}  // namespace

extern "C" {

int o3ds_icp_register_multi(o3ds_handle h, int form, o3ds_cloud source, const o3ds_cloud* targets, size_t n_targets,
                            const o3ds_crop* target_crop, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: null init/out");
  if (!params) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: null params");
  if (form != O3DS_MULTI_UNION && form != O3DS_MULTI_JOINT) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: unknown form");
  if (!targets) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: null target list");
  if (n_targets == 0 || n_targets > (size_t)kMultiMaxTargets)
    return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: between 1 and 16 targets");
  CloudRec* src = find_cloud_lazy(h, source);
  if (!src) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: unknown source cloud id");
  // ---- the list, before anything is touched: every id a cloud of this handle; a non-empty target with its index and normals
  bool empty[kMultiMaxTargets];
  size_t n_slots = 0;
  for (size_t k = 0; k < n_targets; ++k) {
    CloudRec* t = find_cloud_lazy(h, targets[k]);
    if (!t) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: target " + std::to_string(k) + " is not a cloud of this handle");
    if (t->lazy_slot >= 0) {  // "is it empty" needs the exact size
      const int rr = resolve_count(h, *t, true);
      if (rr) return rr;
    }
    empty[k] = t->n == 0;
    if (empty[k]) continue;
    ++n_slots;
    if (t->precision != src->precision) return fail(h, O3DS_ERR_INVALID_ARG, "icp: source/target precision mismatch");
    if (!t->has_index) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: target " + std::to_string(k) + " has no index (o3ds_cloud_build_index)");
    if (!t->nrm && params->method != O3DS_ICP_POINT_TO_POINT)
      return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_multi: target " + std::to_string(k) + " has no normals (the estimator needs them)");
  }
  if (n_targets == 1) return register_one_pair(h, source, targets[0], target_crop, init, params, out);
  if (n_slots == 0) return fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)");
  const bool joint = form == O3DS_MULTI_JOINT;
  // ---- capacity: one batch of kIcpQ queries per workgroup (the partition of the fused loop), one partial row per workgroup (UNION) or per
  // workgroup and target (JOINT); the exact sums of reduce_partials hold for kMaxPassBlocks rows
  if (src->n > kFusedMaxQueries)
    return fail(h, O3DS_ERR_CAPACITY, "icp_register_multi: at most O3DS_ICP_PASS_MAX_QUERIES (262144) source points");
  const int nb = fused_blocks(src->n);
  if (joint && n_targets * (size_t)nb > (size_t)kMaxPassBlocks)
    return fail(h, O3DS_ERR_CAPACITY, "icp_register_multi: JOINT holds n_targets * ceil(n_src / 128) <= 4096 workgroup records per pass");
  // ---- one session per non-empty target: its descriptor; the quanta of the exact sums are the coarsest of the targets' (the bound of
  // the box that holds them all)
  MultiTargetDev desc[kMultiMaxTargets];
  IcpMultiArgs ma{};
  size_t s = 0;
  for (size_t k = 0; k < n_targets; ++k) {
    if (empty[k]) continue;
    const int rc = begin_session(h, source, targets[k], target_crop, init, params, true);
    h->session = false;  // the loop below owns the state
    if (rc) return rc;
    const IcpPassArgs& a = h->pass;
    if ((size_t)a.n_tgt > ((size_t)1 << kMultiPosBits))
      return fail(h, O3DS_ERR_CAPACITY, "icp_register_multi: more than 2^28 index positions in one target");
    desc[s].tpts = a.tpts;
    desc[s].tnrm = a.tnrm;
    desc[s].grid = a.grid;
    desc[s].kmax = a.kmax;
    desc[s].n_tgt = a.n_tgt;
    if (s == 0) {
      ma.pass = a;
    } else {
      for (int t = 0; t < kRec; ++t) ma.pass.q_hi[t] = std::max(ma.pass.q_hi[t], a.q_hi[t]);
    }
    ++s;
  }
  src = find_cloud_lazy(h, source);  // (a persistent-form source was folded by the first session)
  ma.pass.src = h->pass.src;
  ma.pass.src_f64 = h->pass.src_f64;
  ma.pass.count = h->pass.count;
  ma.pass.count_dev = h->pass.count_dev;
  ma.pass.snrm = h->pass.snrm;
  ma.pass.nn_cache = nullptr;
  ma.pass.set_pos = nullptr;
  ma.pass.stats = nullptr;
  ma.pass.debug = 0;
  ma.n_slots = (int)n_slots;
  ma.joint = joint ? 1 : 0;
  const size_t n_upper = ma.pass.count;
  ma.cache_stride = (n_upper + 63) & ~(size_t)63;
  MultiTargetDev* d_desc = nullptr;
  double* d_rows = nullptr;
  const int nrows = joint ? (int)n_slots * nb : nb;
  TMP_ALLOC(d_desc, sizeof(MultiTargetDev) * kMultiMaxTargets);
  TMP_ALLOC(ma.cache, sizeof(int) * std::max<size_t>(ma.cache_stride, 64) * (joint ? n_slots : 1));
  TMP_ALLOC(d_rows, sizeof(double) * kRec * (size_t)nrows);
  int rc = h2d_copy(h, d_desc, desc, sizeof(MultiTargetDev) * n_slots);
  if (rc) return rc;
  ma.tgt = d_desc;
  ma.pass.partials = d_rows;
  const unsigned long long den_mult = joint ? (unsigned long long)n_targets : 1ull;
  const int total_passes = params->max_iteration + 1;  // max_iter updates need max_iter + 1 correspondence passes
  return two_launch_loop(h, total_passes, look_at_session_state(h, out), [&] {  // the host loop of o3ds_icp_register_dev's two-launch form
    launch_multi_accumulate(h, ma, nb);
    icp_multi_reduce_update_kernel<<<1, kUpdBlock, 0, h->stream>>>(d_rows, nrows, h->d_state, n_upper, ma.pass.count_dev, den_mult, params->max_iteration,
                                                                params->relative_fitness, params->relative_rmse, params->method, quantum_table(ma.pass), ma.pass.src,
                                                                ma.pass.src_f64);
  });
}

}  // extern "C"
