// batch_icp.hpp -- o3ds_icp_register_batch: several independent registrations, one launch per pass (o3ds_backend.h).
// Included at the end of backend.hip: it opens one ordinary session per entry (begin_session: validation, index, grid, quanta), keeps
// what the session holds as the entry's row of the table the pass kernel of batch_icp_kernels.hpp reads, and drives all entries with
// the two-launch host loop until every one of them has terminated on the device.
#pragma once
#include "batch_icp_kernels.hpp"

namespace {

constexpr size_t kBatchMaxWorkgroups = O3DS_BATCH_MAX_WORKGROUPS;

template <typename P4>
void launch_batch_accumulate_t(o3ds_handle h, const IcpBatchArgs& ba, int nblocks, bool crop, bool gicp) {
  with_crop_and_estimator(crop, gicp, [&](auto crop_c, auto gicp_c) {
    icp_batch_accumulate_kernel<P4, decltype(crop_c)::value, kIcpBlock, 4, decltype(gicp_c)::value><<<nblocks, kIcpBlock, 0, h->stream>>>(ba);
  });
}

void launch_batch_accumulate(o3ds_handle h, int precision, const IcpBatchArgs& ba, int nblocks, bool crop, bool gicp) {
  DISPATCH(precision, launch_batch_accumulate_t, h, ba, nblocks, crop, gicp);
}

}  // namespace

extern "C" {

int o3ds_icp_register_batch(o3ds_handle h, const o3ds_icp_batch_entry* entries, size_t n_entries, const o3ds_icp_params* params,
                            o3ds_icp_result* out, int* status) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!entries || !out || !status) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: null entries/out/status");
  if (!params) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: null params");
  if (n_entries == 0 || n_entries > (size_t)kBatchMaxEntries) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: between 1 and 64 entries");
  if (!(params->max_correspondence_distance > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");
  if (params->method != O3DS_ICP_POINT_TO_PLANE && params->method != O3DS_ICP_GENERALIZED && params->method != O3DS_ICP_POINT_TO_POINT)
    return fail(h, O3DS_ERR_INVALID_ARG, "icp: unknown method");
  if (params->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp: negative max_iteration");
  // ---- the list, before anything is touched: every id a cloud of this handle, all of one precision; a non-empty target with the
  // normals the estimator needs
  bool empty[kBatchMaxEntries];
  int precision = h->precision;  // (of the clouds: a handle's setting may have changed since they were made)
  for (size_t k = 0; k < n_entries; ++k) {
    const CloudRec* s = find_cloud_lazy(h, entries[k].source);
    CloudRec* t = find_cloud_lazy(h, entries[k].target);
    if (!s || !t) return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: entry " + std::to_string(k) + ": source or target is not a cloud of this handle");
    if (t->lazy_slot >= 0) {  // "is it empty" needs the exact size
      const int rr = resolve_count(h, *t, true);
      if (rr) return rr;
    }
    if (k == 0) precision = s->precision;
    if (s->precision != precision || t->precision != precision)
      return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: entry " + std::to_string(k) + ": source/target precision mismatch (one precision per batch)");
    empty[k] = t->n == 0;
    if (!empty[k] && !t->nrm && params->method != O3DS_ICP_POINT_TO_POINT)
      return fail(h, O3DS_ERR_INVALID_ARG, "icp_register_batch: entry " + std::to_string(k) + ": target has no normals (the estimator needs them)");
  }
  if (n_entries == 1) {
    status[0] = register_one_pair(h, entries[0].source, entries[0].target, entries[0].target_crop, entries[0].init, params, &out[0]);
    if (status[0]) memset(&out[0], 0, sizeof(o3ds_icp_result));
    return O3DS_OK;
  }
  // ---- capacity: one batch of kIcpQ queries per workgroup (the partition of the fused loop), one partial row per workgroup
  size_t total_wg = 0;
  for (size_t k = 0; k < n_entries; ++k) {
    if (empty[k]) continue;
    const CloudRec* s = find_cloud_lazy(h, entries[k].source);
    if (s->n > kFusedMaxQueries)
      return fail(h, O3DS_ERR_CAPACITY, "icp_register_batch: entry " + std::to_string(k) + ": at most 262144 source points per entry");
    total_wg += (size_t)fused_blocks(s->n);
  }
  if (total_wg > kBatchMaxWorkgroups)
    return fail(h, O3DS_ERR_CAPACITY, "icp_register_batch: the entries hold sum of ceil(n_src / 128) <= 65536 workgroups per pass");
  // ---- a persistent-form source is folded by its session, which drops the index another entry may already have taken as its target:
  // fold them all first
  for (size_t k = 0; k < n_entries; ++k) {
    CloudRec* s = find_cloud_lazy(h, entries[k].source);
    if (!empty[k] && s->pm) {
      const int re = pm_exit(h, *s);
      if (re) return re;
    }
  }
  // ---- one session per runnable entry: what it holds is the entry's row of the table
  std::vector<IcpPassArgs> table;
  std::vector<IcpStateDev> states;
  std::vector<int> start(1, 0), entry_of;
  std::vector<size_t> cache_off(1, 0);
  bool any_crop = false;
  for (size_t k = 0; k < n_entries; ++k) {
    status[k] = empty[k] ? fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)")
                         : begin_session(h, entries[k].source, entries[k].target, entries[k].target_crop, entries[k].init, params, false);
    h->session = false;  // the loop below owns the states
    if (status[k]) {
      memset(&out[k], 0, sizeof(o3ds_icp_result));
      continue;
    }
    IcpPassArgs a = h->pass;
    a.set_pos = nullptr;
    a.set_ref = nullptr;
    a.stats = nullptr;
    a.debug = 0;
    if (a.count > kFusedMaxQueries) {  // (cannot grow between the check above and here; the rows below are sized by it)
      status[k] = fail(h, O3DS_ERR_CAPACITY, "icp_register_batch: at most 262144 source points per entry");
      memset(&out[k], 0, sizeof(o3ds_icp_result));
      continue;
    }
    table.push_back(a);
    states.push_back(*h->h_state);  // (begin_session: zero state, T = init)
    entry_of.push_back((int)k);
    start.push_back(start.back() + fused_blocks(a.count));
    cache_off.push_back(cache_off.back() + std::max<size_t>((a.count + 63) & ~(size_t)63, 64));
    any_crop = any_crop || h->session_crop;  // an entry without a crop holds the volume that contains everything: the same matches
  }
  const size_t n_live = table.size();
  if (n_live == 0) return O3DS_OK;
  const int total_blocks = start.back();
  IcpPassArgs* d_table = nullptr;
  IcpStateDev* d_states = nullptr;
  int* d_start = nullptr;
  int* d_cache = nullptr;
  double* d_rows = nullptr;
  TMP_ALLOC(d_table, sizeof(IcpPassArgs) * n_live);
  TMP_ALLOC(d_states, sizeof(IcpStateDev) * n_live);
  TMP_ALLOC(d_start, sizeof(int) * (n_live + 1));
  TMP_ALLOC(d_cache, sizeof(int) * cache_off.back());
  TMP_ALLOC(d_rows, sizeof(double) * kRec * (size_t)total_blocks);
  for (size_t s = 0; s < n_live; ++s) {
    table[s].state = d_states + s;
    table[s].partials = d_rows + (size_t)start[s] * kRec;
    table[s].nn_cache = d_cache + cache_off[s];
  }
  int rc = h2d_copy(h, d_table, table.data(), sizeof(IcpPassArgs) * n_live);
  if (!rc) rc = h2d_copy(h, d_states, states.data(), sizeof(IcpStateDev) * n_live);
  if (!rc) rc = h2d_copy(h, d_start, start.data(), sizeof(int) * (n_live + 1));
  if (rc) return rc;
  IcpBatchArgs ba{};
  ba.entry = d_table;
  ba.start = d_start;
  ba.n_entries = (int)n_live;
  const bool gicp = params->method == O3DS_ICP_GENERALIZED;
  const int total_passes = params->max_iteration + 1;  // max_iter updates need max_iter + 1 correspondence passes
  const auto look = [&](bool* done) {  // all states in one pinned copy; done: every entry's loop has terminated
    const int rb = read_back(h, {{states.data(), d_states, sizeof(IcpStateDev) * n_live}});
    *done = std::all_of(states.begin(), states.end(), [](const IcpStateDev& s) { return s.done != 0; });
    return rb;
  };
  rc = two_launch_loop(h, total_passes, look, [&] {
    launch_batch_accumulate(h, precision, ba, total_blocks, any_crop, gicp);
    icp_batch_reduce_update_kernel<<<(int)n_live, kUpdBlock, 0, h->stream>>>(ba, params->max_iteration, params->relative_fitness, params->relative_rmse,
                                                                            params->method);
  });
  if (rc) return rc;
  for (size_t s = 0; s < n_live; ++s) state_result(states[s], &out[entry_of[s]]);
  return O3DS_OK;
}

}  // extern "C"
