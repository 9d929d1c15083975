// backend.hip -- C-ABI (include/o3ds_backend.h) of the gfx950 scan-matching / map-fusion backend.
// Host-side orchestration only; all arithmetic is in icp_kernels.hpp / cloud_kernels.hpp.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <initializer_list>
#include <map>

#include <rocprim/device/device_radix_sort.hpp>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "cloud_kernels.hpp"
#include "common.hpp"
#include "feature_kernels.hpp"
#include "icp_kernels.hpp"
#include "map_kernels.hpp"
#include "neighbor_kernels.hpp"
#include "normals_kernel.hpp"
#include "pose_graph_kernels.hpp"
#include "cluster_kernels.hpp"  // (last: its kernels follow every other one in the code object, whose layout the registration was measured with)
#include "plane_kernels.hpp"    // (and these follow the clustering's)
#include "colored_icp_kernels.hpp"  // (and these the plane's)
#include "robust_icp_kernels.hpp"   // (and this one the coloured step's)
#include "degeneracy_kernels.hpp"   // (and this one the robust step's)
#include "ndt_kernels.hpp"          // (and these the degeneracy tail's)

using namespace o3ds;

namespace {

thread_local std::string g_thread_error;

// A/B levers, tuning knobs and debugging aids (O3DS_ICP_MODE, O3DS_ICP_SETS, O3DS_SUM_NO_SPLIT, O3DS_VOXEL_SORT, O3DS_CARVE_SORT, ...) exist
// only in the library built with -DO3DS_AB_SWITCHES (lib/libo3ds_backend_ab.so: what the A/B tests and the experiment scripts load); every one
// of them is listed in tests/test_abi.py, which fails on a name that is not: a lever is kept while a test, the benchmark or a kernel uses it.  The
// shipped library reads three environment variables, two of memory sizing and the file name of RCCL: O3DS_POOL_CAP_MB, O3DS_ARENA_MB, O3DS_RCCL_LIB -- a drop-in library's results
// and code paths must not depend on its host process's environment.
#ifdef O3DS_AB_SWITCHES
inline const char* ab_getenv(const char* name) { return getenv(name); }
#else
inline const char* ab_getenv(const char*) { return nullptr; }
#endif

struct CloudRec {
  size_t n = 0;
  int precision = 0;
  void* pts = nullptr;  // P4[n]
  void* nrm = nullptr;  // P4[n] or null
  void* col = nullptr;  // P4[n] or null: PointCloud::colors_ (carried by the cloud operations, never read by registration)
  size_t cap = 0;       // points the pts / nrm arrays have room for when that is more than n (a map after its merge: the next scan is placed
                        // behind the last point instead of copying the map into larger arrays); 0 = exactly n
  // nearest-neighbour index
  bool has_index = false;
  bool index_byproduct = false;  // the index was left by the normal estimation (its cell size suits THAT search): a registration
                                 // keeps it if the cell is within [r / 8, 0.75 r] of its own radius and rebuilds otherwise
  GridDev grid{};
  int* cell_start = nullptr;
  void* spts = nullptr;
  void* snrm = nullptr;
  void* rpts = nullptr;     // the neighbourhood-major replica of spts (GridDev::rpts) and its tables; null: none
  int* rstart = nullptr;
  int* rpos = nullptr;
  int index_regs = 0;       // registrations against this index so far (maybe_build_replica)
  size_t spts_slack = 0;    // bytes allocated behind the last element of spts, and of rpts: the search's scan loop loads up to
  size_t rpts_slack = 0;    // kScanSlackBytes beyond the end of a range (scan_strided) and is refused a target that has less
  // A box that is known to contain every point (not necessarily tight): set where a bounding box has been computed anyway
  // (VoxelDownSample, an index build) and carried to clouds derived from it (subsets, voxel means, rigid placements, unions), so
  // that the next index build of the per-scan pipeline does not pay a reduction kernel + read-back + host sync for it again.
  // layout left by the map merge: [pass-through block | voxel block in ascending key order]; vox_first < 0 = unknown (any other
  // operation that reorders or moves points resets it), see voxel_reduce_t
  long long vox_first = -1;
  size_t vox_count = 0;
  struct PMapRec* pm = nullptr;  // non-null: the cloud is a submap in its PERSISTENT form (map_kernels.hpp): pts / nrm are slot arrays, n an
                                 // upper bound of the slots in use, the index is row-paged and kept up to date by the insertions
  size_t index_positions = 0;    // positions the cell-sorted arrays of the index span (0: n; the row-paged index has gaps)
  // A count the host has not seen yet (common.hpp, CountPub): `n` is then an UPPER bound -- the arrays have room for it, launches are
  // sized by it -- and the exact number is in the device word of record `lazy_slot` once the producing kernel has run (and in the pinned
  // record, stamped `lazy_seq`, for the host: resolve_count).  -1: n is exact.
  int lazy_slot = -1;
  int lazy_seq = 0;
  size_t n_lower = 0;  // ... and a lower bound of it (o3ds_cloud_size_bound: "is it empty" rarely needs the exact number)
  // An ingest that is still in flight on the handle's copy stream (o3ds_cloud_upload_f32): the first use of the cloud on the handle's
  // stream waits for this event (cloud_ready); `ingest_buf` is the ingest buffer the points live in (not a pool block), -1 = none.
  hipEvent_t ingest_ev = nullptr;
  int ingest_buf = -1;
  // ... and the box of the points inside `pre_crop` that the ingest kernel reduced on the way (pinned record `pre_slot`, stamp `pre_seq`)
  int pre_slot = -1;
  int pre_seq = 0;
  CropDev pre_crop{};
  bool has_box = false;
  bool box_padded = false;  // the box already has a margin against the rounding of derived values (never padded twice: a map is
                            // re-voxelised at every insertion and its box must not creep outwards over a long mission)
  double bmn[3] = {0, 0, 0}, bmx[3] = {0, 0, 0};
  // FPFH features (o3ds_compute_fpfh): n x 33 doubles, row-major; dropped by every operation that changes the points or normals in place
  double* fpfh = nullptr;
  bool has_fpfh = false;
  size_t fpfh_n = 0;
  // colour gradients (o3ds_compute_color_gradients): n x 3 doubles, remembered with the (radius, max_nn) that made them; dropped by every
  // operation that changes the points, normals or colours in place, carried into no other cloud
  double* cgrad = nullptr;
  bool has_cgrad = false;
  size_t cgrad_n = 0;
  double cgrad_radius = 0.0;
  int cgrad_max_nn = 0;
};

void box_inflate(CloudRec& c) {  // stored values are rounded (f32 storage, f64 -> f32 of means / placements): keep the box conservative
  if (c.box_padded) return;
  c.box_padded = true;
  for (int a = 0; a < 3; ++a) {
    const double pad = 1e-5 * (std::fabs(c.bmn[a]) + std::fabs(c.bmx[a]) + (c.bmx[a] - c.bmn[a])) + 1e-9;
    c.bmn[a] -= pad;
    c.bmx[a] += pad;
  }
}
void box_copy(CloudRec& to, const CloudRec& from) {
  to.has_box = from.has_box;
  to.box_padded = from.box_padded;
  for (int a = 0; a < 3; ++a) to.bmn[a] = from.bmn[a], to.bmx[a] = from.bmx[a];
}
void box_union(CloudRec& to, const CloudRec& a, const CloudRec& b) {  // of two non-empty clouds; an empty one contributes nothing
  if (a.n == 0) return box_copy(to, b);
  if (b.n == 0) return box_copy(to, a);
  to.has_box = a.has_box && b.has_box;
  to.box_padded = a.box_padded && b.box_padded;
  for (int k = 0; k < 3; ++k) to.bmn[k] = std::min(a.bmn[k], b.bmn[k]), to.bmx[k] = std::max(a.bmx[k], b.bmx[k]);
}
void box_transform(CloudRec& to, const CloudRec& from, const double T[16]) {  // box of the 8 placed corners, inflated
  to.has_box = from.has_box;
  to.box_padded = false;  // the placed values are rounded again
  if (!from.has_box) return;
  for (int a = 0; a < 3; ++a) to.bmn[a] = 1e300, to.bmx[a] = -1e300;
  for (int k = 0; k < 8; ++k) {
    const double x = (k & 1) ? from.bmx[0] : from.bmn[0], y = (k & 2) ? from.bmx[1] : from.bmn[1], z = (k & 4) ? from.bmx[2] : from.bmn[2];
    const double w = T[3] * x + T[7] * y + T[11] * z + T[15];
    for (int a = 0; a < 3; ++a) {
      const double v = (T[a] * x + T[4 + a] * y + T[8 + a] * z + T[12 + a]) / w;
      to.bmn[a] = std::min(to.bmn[a], v);
      to.bmx[a] = std::max(to.bmx[a], v);
    }
  }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(to.bmn[a]) || !std::isfinite(to.bmx[a])) to.has_box = false;
  if (to.has_box) box_inflate(to);
}

// host side of a submap in its persistent form (map_kernels.hpp)
struct PMapRec {
  PmDev dev{};
  CropDev* d_hist = nullptr;
  int t = 0;              // insertions since the map entered this form (their volumes: d_hist[1..t])
  size_t n_upper = 0;     // slots in use: the host's upper bound (exact value: dev.counters[kPmN])
  size_t live_lower = 0;  // live points: a lower bound
  double clamped = 0;     // slots that entered the index outside its grid, as of the last record
  double multi_total = 0; // entries of the multi list so far (appended to, never compacted), as of the last record
  double pool_top = 0;    // first free position of the index pool: an upper bound (the last record the host saw + the worst case of
                          // every insertion since)
  int rec_slot = -1, rec_seq = 0;  // pinned record the insertions publish {slots, pool top, dead, error} into; stamp of the latest
  size_t rows = 0;
  std::vector<void*> blocks;  // every pool block of the form except the slot arrays and the index arrays (those hang on the CloudRec)
};

constexpr int kMaxPassBlocks = 4096;  // capacity of the partial-record buffer (rows per pass <= pass_rows <= this)
constexpr size_t kMaxCells = (size_t)1 << 27;  // 512 MiB of cell_start at most
// The neighbourhood-major replica of a registration target's index (GridDev::rpts) is built when its points, their position map and its
// table of super-row starts fit in this many bytes, the Infinity Cache, and the table has at most kMaxCells entries.  9 copies of every point: 180 MB
// for the 1 M-point map with f32 storage (built: configs[1] +8 %); 1.44 GB for an 8 M-point map, whose stage-1 gathers then come from HBM
// and lost 3 % (not built), 324 MB with f64 storage (no gain measured: not built).
constexpr size_t kReplicaMaxBytes = (size_t)256 << 20;
// How many elements of P4 a searched array may hold (build_grid_t, the persistent map's pool): kScanMaxBytes of them, i.e. 2^32 bytes less
// the scan loop's slack.  A/B library: O3DS_SCAN_SPACE_BYTES=<b> stands in for the 2^32 (the slack still comes off it), so that a test
// reaches the limit with a small cloud.
template <typename P4>
size_t scan_capacity() {
  static_assert(kScanMaxBytes + kScanSlackBytes == (size_t)1 << 32, "capacity and slack share the 32-bit offset space");
  const char* e = ab_getenv("O3DS_SCAN_SPACE_BYTES");
  const size_t space = e ? (size_t)strtoull(e, nullptr, 10) : kScanMaxBytes + kScanSlackBytes;
  return space > kScanSlackBytes ? (std::min(space, kScanMaxBytes + kScanSlackBytes) - kScanSlackBytes) / sizeof(P4) : 0;
}
// the slack an index array is allocated with; A/B library: O3DS_NO_SCAN_SLACK allocates as a caller unaware of the scan loop would
inline size_t scan_slack_alloc() { return ab_getenv("O3DS_NO_SCAN_SLACK") ? 0 : kScanSlackBytes; }
static_assert(kReplicaMaxBytes <= kScanMaxBytes, "scan_strided addresses a searched array by 32-bit byte offsets");

}  // namespace

// dense voxel map (VoxelizedPointCloud): a device hash table, see cloud_kernels.hpp
struct DenseRec {
  double voxel = 0.0;
  size_t cap = 0;          // power of two
  o3ds::DenseDev dev{};
  bool has_normals = false;
  bool has_colors = false;
  size_t used_upper = 0;   // upper bound on the OCCUPIED slots = live voxels + tombstones (exact count fetched only when the table
                           // looks too full); the load factor of the open-addressing table is about these, not about live voxels
};

// the voxel Gaussians of a cloud (ndt_kernels.hpp): a snapshot, every array n_vox long and in ascending packed-key order
struct NdtRec {
  double voxel = 0.0;
  size_t n_vox = 0;
  o3ds_voxel_gaussians_info info{};
  unsigned long long* keys = nullptr;
  uint32_t* counts = nullptr;
  double *mean = nullptr, *cov = nullptr, *information = nullptr;
  uint8_t* valid = nullptr;
  o3ds::NdtVoxel* rec = nullptr;  // what a pass reads
};

struct o3ds_context {
  int device = 0;
  hipStream_t stream = nullptr;
  int precision = O3DS_PRECISION_F32;
  std::string err, deferred_err;
  std::unordered_map<uint64_t, CloudRec> clouds;
  std::unordered_map<uint64_t, DenseRec> dense_maps;
  std::unordered_map<uint64_t, NdtRec> voxel_gaussians;
  uint64_t next_id = 1;
  // ICP scratch
  double* d_partials = nullptr;     // [kMaxPassBlocks][kRec]
  IcpStateDev* d_state = nullptr;
  IcpStateDev* h_state = nullptr;   // pinned, mapped
  char* h_pin = nullptr;            // pinned block the small device -> host read-backs land in (read_back)
  char* h_pin_dev = nullptr;        // the same block as kernels address it: a kernel that produces a size / count / box the host is about
                                    // to wait for stores it here itself (no copy on the stream, the host only synchronises)
  char* h_stage[2] = {nullptr, nullptr};  // pinned ring the large host <-> device copies of caller buffers go through (staged_copy)
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  IcpStateDev* h_state_dev = nullptr;  // the device's view of h_state
  // step-wise ICP session
  bool session = false;
  IcpPassArgs pass{};
  o3ds_icp_params params{};
  size_t session_n_src = 0;
  int session_launches = 0;                     // fused step-wise form: launches issued in this session
  const IcpStateDev* session_state = nullptr;   // ... and the state the latest one wrote (null: d_state)
  int session_precision = 0;
  bool session_crop = false;
  int session_method = O3DS_ICP_POINT_TO_PLANE;
  double gicp_epsilon = 1e-3;  // [O3D] TransformationEstimationForGeneralizedICP default
  hipStream_t own_stream = nullptr;
  // device memory of the handle: a caching allocator over hipMalloc (dev_alloc / dev_free below)
  std::multimap<size_t, void*> pool_free;        // cached blocks by size
  std::unordered_map<void*, size_t> pool_size;   // every block this handle obtained from hipMalloc -> its size
  size_t pool_bytes = 0;   // everything obtained from hipMalloc
  size_t pool_cached = 0;  // of which in the free lists
  // bump arena for the temporaries of one top-level ABI call (stream-ordered reuse: everything runs on one stream)
  std::vector<std::pair<char*, size_t>> arena_blocks;
  size_t arena_cur = 0, arena_off = 0;
  int arena_depth = 0;
  // rows (workgroups) per pass are capped at pass_rows (O3DS_PASS_ROWS, for experiments and the geometry-independence test)
  // ONE launch per pass with the previous pass's tail in its prologue (O3DS_ICP_MODE=fused), see icp_fused_kernel
  // normal estimation: remembered cell size of the ring search (see normals_t)
  double nrm_cell = 0.0, nrm_radius = 0.0;
  int nrm_knn = 0, nrm_age = 0;
  size_t nrm_n = 0;
  bool fused = true;  // O3DS_ICP_MODE=launch selects the two-kernel form (same results bit for bit)
  int* d_nn_cache = nullptr;  // per-query match of the previous pass (bound for the pruned search); grown on demand
  size_t nn_cache_cap = 0;
  // candidate sets of the fused loop (icp_kernels.hpp, Collect): one allocation of nn_cache_cap x (kSetCap ints + {p_ref, L} at f64 width)
  int* d_set_pos = nullptr;
  void* d_set_ref = nullptr;
  bool sets = true;                                      // O3DS_ICP_SETS=0: every pass searches (same results bit for bit)
  float set_gain = 2.0f, set_min = 1e-3f, set_cap = 0.04f;  // O3DS_SET_GAIN / _MIN / _CAP (metres)
  char* d_fused = nullptr;  // [2 states | 3 x kFusedSlots slot records (hi and lo sums)]
  unsigned long long fused_launches = 0;
  unsigned long long fused_seq = 0;  // stamp of the last launch that was asked to write the pinned state (wait_fused_state)
  o3ds_overlap_fn overlap_fn = nullptr;  // o3ds_icp_overlap_next: called once behind the next registration's launches
  void* overlap_arg = nullptr;
  // Scratch that its users leave the way they found it, so that no launch is spent on clearing it: the per-cell counters of an index
  // build (the scatter counts them back down to zero) and the voxel table of VoxelDownSample (vox_mean_kernel empties the slots it
  // used).  `*_clean` is false while an operation is in flight or after one failed: the next user clears the block first.
  int* d_cells = nullptr;
  size_t cells_cap = 0;
  bool cells_clean = false;
  unsigned char* d_voxtab = nullptr;
  o3ds::DrawState* d_draw = nullptr;  // RandomDownSample on the device (cloud_kernels.hpp): histograms zero between calls
  size_t voxtab_cap = 0;  // slots
  bool voxtab_clean = false;
  // ---- values kernels publish for the host without a copy or a wait on the stream: kPinRecs records {count, stamp, box} in pinned
  // memory (h_rec; the device's view h_rec_dev), the counts also in device words (d_cnt) for the kernels that consume a cloud whose size
  // the host has not seen yet.  A record belongs to one cloud at a time (rec_owner: cloud id, 0 = free).
  struct PinRec {
    int cnt, seq;
    double box[6];
    double pad;  // box[6] to the kernels that publish seven values (pm_carve_finish_kernel: the number of carved points)
  };
  PinRec* h_rec = nullptr;
  PinRec* h_rec_dev = nullptr;
  int* d_cnt = nullptr;  // [kPinRecs * 16]: one word per record, 64 bytes apart
  uint64_t rec_owner[64] = {0};
  int rec_next = 0, rec_seq = 0;
  size_t voxel_count_hint = 0;  // the last VoxelDownSample size the host saw: the estimate heuristics use while the current one is in flight
  // ---- ingest (o3ds_cloud_upload_f32): its own stream, so that scan k + 1 crosses PCIe and is unpacked while frame k runs; buffers of
  // its own (not pool blocks: the pool's reuse is ordered by the handle's ONE stream), handed back behind an event on that stream
  struct IngestBuf {
    void* pts = nullptr;
    size_t pts_bytes = 0;
    unsigned long long* box = nullptr;  // device box record (order_bits images), armed
    hipEvent_t freed = nullptr;         // recorded on the handle's stream when the cloud was freed: the next ingest into the buffer waits for it
    bool in_use = false;
  };
  std::vector<IngestBuf> ingest_bufs;
  hipStream_t copy_stream = nullptr;
  unsigned char* d_raw = nullptr;  // the records as they crossed PCIe (copy-stream ordered: one buffer)
  size_t raw_cap = 0;
  std::vector<hipEvent_t> ev_pool;  // disable-timing events for ingest_ev
  bool pre_crop_valid = false;      // the volume of the last crop + VoxelDownSample: what the next ingest reduces its box for
  CropDev pre_crop{};
  // chained scan of vox_order_kernel: tile records (never cleared: they carry the call's number) and the running ticket counter
  unsigned long long* d_tiles = nullptr;
  size_t tiles_cap = 0;
  unsigned int* d_ticket = nullptr;
  unsigned int ticket_base = 0, scan_gen = 0;
  int fused_chunk_hint[2] = {12, 12};  // [registration against a cropped target?]: scan-to-map and scan-to-scan alternate on a handle  // launches queued before the host first looks at the state: what the previous registration needed, plus one
  int debug_update = 0;  // O3DS_DEBUG_UPDATE: timing experiments only
  int pass_rows = 1024;
  // sharded registrations inside the library (sharded.hpp): the RCCL communicator (created by o3ds_comm_init: owned; attached: the
  // caller's), this handle's place in it, and the buffers the collectives run on
  void* nccl_comm = nullptr;
  bool nccl_owned = false;
  int comm_rank = 0, comm_world = 1;
  double* d_shard_sums = nullptr;  // 3 x O3DS_ICP_SUMS_DOUBLES
  unsigned long long* d_shard_keys = nullptr;
  size_t shard_keys_cap = 0;
  // profiling (bench.py roofline): 1 = event pairs around every accumulate launch + tagged spans, 2 = tagged spans only (a span around
  // a whole registration then holds its kernels and nothing else)
  int profiling = 0;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  // ... and tagged spans (o3ds_profile_span): pairs of events around whatever the caller -- or, for the internal tags, a kernel
  // sequence inside a call -- encloses
  static constexpr int kSpanTags = 20;  // 0..7 the caller's (o3ds_profile_span), 8..19 marked inside the library
  std::vector<hipEvent_t> span_ev[kSpanTags];
  size_t span_used[kSpanTags] = {0};
};

namespace {

int fail(o3ds_handle h, int code, const std::string& msg) {
  std::string text = msg;
  if (h && !h->deferred_err.empty()) {  // what went wrong inside find_cloud (a size that never arrived, a map that could not be folded)
    text += " [" + h->deferred_err + "]";
    h->deferred_err.clear();
  }
  g_thread_error = text;
  if (h) h->err = text;
  return code;
}

#define HIP_TRY(expr)                                                                                       \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess)                                                                                   \
      return fail(h, _e == hipErrorOutOfMemory ? O3DS_ERR_OOM : O3DS_ERR_HIP,                               \
                  std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

// Every entry point makes the handle's device the calling thread's current device: the current device is per thread and defaults to
// 0, handles are shared across the caller's worker threads (host/o3ds_mapping.hpp) and one process may drive one handle per GPU.
#define CHECK_HANDLE(h)                                                        \
  if (!(h)) return fail(nullptr, O3DS_ERR_BAD_HANDLE, "null handle");          \
  if (hipSetDevice((h)->device) != hipSuccess) return fail((h), O3DS_ERR_HIP, "hipSetDevice failed")

// ---- small read-backs ---------------------------------------------------------------------------------------------
// Sizes, counts and bounding boxes that the host needs go through a pinned block owned by the handle: a D2H copy into pageable
// memory is staged and waited for inside the runtime (tens of microseconds for four bytes -- a dozen of them per lidar frame);
// into pinned memory it is an ordinary stream operation, and one synchronisation serves all items of a call.
constexpr size_t kPinBytes = 64 << 10;
constexpr size_t kPubOff = kPinBytes - 256;  // the last 256 bytes: slots for values kernels publish themselves (pub_slot)
struct D2H {
  void* dst;
  const void* src;
  size_t bytes;
};
int read_back(o3ds_handle h, std::initializer_list<D2H> items) {
  size_t off = 0;
  for (const D2H& it : items) {
    if (off + it.bytes > kPubOff) return fail(h, O3DS_ERR_INVALID_ARG, "read_back: item list exceeds the pinned block");
    HIP_TRY(hipMemcpyAsync(h->h_pin + off, it.src, it.bytes, hipMemcpyDeviceToHost, h->stream));
    off += (it.bytes + 15) & ~(size_t)15;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  off = 0;
  for (const D2H& it : items) {
    memcpy(it.dst, h->h_pin + off, it.bytes);
    off += (it.bytes + 15) & ~(size_t)15;
  }
  return O3DS_OK;
}

// ---- large copies of caller buffers ------------------------------------------------------------------------------
// A caller's cloud is pageable memory (std::vector<Eigen::Vector3d>, a numpy array).  What the runtime does with a multi-megabyte
// pageable copy depends on its mood: seen on the same box, the same 3 MB download took 0.3 ms in one process and 8 ms in the next
// (tests/cpp/stream_mapping.cpp: 0.9 vs 24 ms per scan).  So copies above kStageMin go through two pinned buffers owned by the
// handle: memcpy into / out of the ring on the host, DMA between the ring and the device, one chunk in flight while the other is
// copied.  The host-to-device form returns with the last DMA queued (callers synchronise as before); device-to-host is complete.
constexpr size_t kStageBytes = 1 << 20, kStageMin = 128 << 10;  // 1 MB chunks: a 3 MB cloud is three chunks, DMA and host memcpy overlap
int stage_init(o3ds_handle h) {
  if (h->h_stage[1] && h->stage_ev[1]) return O3DS_OK;
  HIP_TRY(hipSetDevice(h->device));  // the events must belong to the device of the handle's stream
  for (int k = 0; k < 2; ++k) {
    if (!h->h_stage[k]) HIP_TRY(hipHostMalloc((void**)&h->h_stage[k], kStageBytes, hipHostMallocDefault));
    if (!h->stage_ev[k]) HIP_TRY(hipEventCreateWithFlags(&h->stage_ev[k], hipEventDisableTiming));
  }
  return O3DS_OK;
}
int h2d_copy(o3ds_handle h, void* d_dst, const void* h_src, size_t bytes, hipStream_t stream = nullptr /* the handle's */) {
  if (!stream) stream = h->stream;
  if (bytes < kStageMin) {
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, stream));
    return O3DS_OK;
  }
  int rc = stage_init(h);
  if (rc) return rc;
  int k = 0;
  for (size_t off = 0; off < bytes; off += kStageBytes, k ^= 1) {
    const size_t n = std::min(kStageBytes, bytes - off);
    HIP_TRY(hipEventSynchronize(h->stage_ev[k]));  // the DMA that last read this buffer is done (a fresh event is complete)
    memcpy(h->h_stage[k], (const char*)h_src + off, n);
    HIP_TRY(hipMemcpyAsync((char*)d_dst + off, h->h_stage[k], n, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(h->stage_ev[k], stream));
  }
  return O3DS_OK;
}
int d2h_copy(o3ds_handle h, void* h_dst, const void* d_src, size_t bytes) {  // synchronous: h_dst is filled on return
  if (bytes < kStageMin) {
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return O3DS_OK;
  }
  int rc = stage_init(h);
  if (rc) return rc;
  const size_t chunks = (bytes + kStageBytes - 1) / kStageBytes;
  for (size_t c = 0; c <= chunks; ++c) {
    if (c < chunks) {  // queue chunk c into buffer c & 1 (its previous content, chunk c - 2, was copied out one step ago)
      const size_t off = c * kStageBytes, n = std::min(kStageBytes, bytes - off);
      HIP_TRY(hipMemcpyAsync(h->h_stage[c & 1], (const char*)d_src + off, n, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipEventRecord(h->stage_ev[c & 1], h->stream));
    }
    if (c > 0) {  // while it flies, hand chunk c - 1 to the caller
      const size_t off = (c - 1) * kStageBytes, n = std::min(kStageBytes, bytes - off);
      HIP_TRY(hipEventSynchronize(h->stage_ev[(c - 1) & 1]));
      memcpy((char*)h_dst + off, h->h_stage[(c - 1) & 1], n);
    }
  }
  return O3DS_OK;
}

// ---- device memory -------------------------------------------------------------------------------------------------
// Every device buffer of a handle (clouds, indices, arena blocks) comes from this cache over plain hipMalloc.  All work of a handle
// is ordered on ONE stream (o3ds_set_stream synchronises the stream it leaves), so a block handed back by dev_free may be handed out
// again at once: whatever still reads it was enqueued earlier on the same stream -- the semantics of a stream-ordered pool without
// the runtime's.  Round 1 used hipMallocAsync / hipFreeAsync; under alloc / free churn of blocks of tens to hundreds of MB
// (estimate_normals with a fine pilot grid: a 150 MB scratch block, 40 MB cell tables per call) ROCm 7.2's pool intermittently
// handed out memory whose contents were then lost -- cell_start came back zeroed from some cell on, or the GPU faulted on it
// (scripts/stress_normals.py reproduced it; a host-side check showed the broken table before the kernel that reads it ran; the scratch arena
// had met the same thing in round 1 and stopped returning its blocks).  Sizes are rounded up to 1/8 of their power of two, so the
// slowly varying sizes of a lidar stream hit the same classes; blocks go back to the driver only when the handle is destroyed.
hipError_t dev_alloc(o3ds_handle h, void** out, size_t bytes) {
  if (bytes < 256) bytes = 256;
  size_t gran = 256;
  while (gran * 8 < bytes) gran <<= 1;
  const size_t want = (bytes + gran - 1) / gran * gran;
  auto it = h->pool_free.lower_bound(want);
  if (it != h->pool_free.end() && it->first <= want + want / 4) {
    *out = it->second;
    h->pool_cached -= it->first;
    h->pool_free.erase(it);
    return hipSuccess;
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess && !h->pool_free.empty()) {  // out of memory: give the cached blocks back and retry
    (void)hipStreamSynchronize(h->stream);
    for (auto& b : h->pool_free) {
      h->pool_bytes -= b.first;
      h->pool_size.erase(b.second);
      (void)hipFree(b.second);
    }
    h->pool_free.clear();
    h->pool_cached = 0;
    e = hipMalloc(&p, want);
  }
  if (e != hipSuccess) return e;
  h->pool_size.emplace(p, want);
  h->pool_bytes += want;
  *out = p;
  return hipSuccess;
}
void dev_free(o3ds_handle h, void* p) {
  if (!p) return;
  auto it = h->pool_size.find(p);
  if (it == h->pool_size.end()) return;  // not ours (never happens)
  h->pool_free.emplace(it->second, p);
  h->pool_cached += it->second;
  // The cache is bounded: size classes drift as a map grows, and blocks of outgrown classes are never asked for again.  Beyond the cap
  // (O3DS_POOL_CAP_MB, default 32 GB of the 288) everything cached goes back to the driver -- after a stream synchronisation, because a
  // cached block may still be read by work enqueued before its dev_free.
  static const size_t cap = (getenv("O3DS_POOL_CAP_MB") ? (size_t)atoll(getenv("O3DS_POOL_CAP_MB")) : (size_t)32768) << 20;
  if (h->pool_cached > cap) {
    (void)hipStreamSynchronize(h->stream);
    for (auto& b : h->pool_free) {
      h->pool_bytes -= b.first;
      h->pool_size.erase(b.second);
      (void)hipFree(b.second);
    }
    h->pool_free.clear();
    h->pool_cached = 0;
  }
}
void dev_release_all(o3ds_handle h) {  // o3ds_destroy: the stream has been synchronised
  for (auto& b : h->pool_size) (void)hipFree(b.first);
  h->pool_size.clear();
  h->pool_free.clear();
  h->pool_bytes = 0;
  h->pool_cached = 0;
}

// device blocks obtained in a function that may still fail: handed back to the cache on every early return, kept on release()
struct DevGuard {
  o3ds_handle h;
  std::vector<void**> held;
  explicit DevGuard(o3ds_handle hh) : h(hh) {}
  ~DevGuard() {
    for (void** q : held)
      if (*q) {
        dev_free(h, *q);
        *q = nullptr;
      }
  }
  void add(void** q) { held.push_back(q); }
  void release() { held.clear(); }
};

// ---- scratch arena ------------------------------------------------------------------------------------------------
// Temporaries (scan block sums, flags, sort buffers, staging copies ...) are bump-allocated from blocks that persist
// for the life of the handle: a per-scan pipeline makes ~120 allocations otherwise (4.6 us each + free).  The bump
// pointer is reset at the start of every outermost ABI call; safe without synchronisation because all work of a handle
// is ordered on one stream.
int arena_alloc(o3ds_handle h, void** out, size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes == 0) bytes = 256;
  for (;;) {
    if (h->arena_cur < h->arena_blocks.size()) {
      auto& b = h->arena_blocks[h->arena_cur];
      if (h->arena_off + bytes <= b.second) {
        *out = b.first + h->arena_off;
        h->arena_off += bytes;
        return O3DS_OK;
      }
      ++h->arena_cur;
      h->arena_off = 0;
      continue;
    }
    static const size_t first_mb = getenv("O3DS_ARENA_MB") ? (size_t)atoi(getenv("O3DS_ARENA_MB")) : 32;
    size_t want = std::max<size_t>(bytes, first_mb << 20);
    if (!h->arena_blocks.empty()) want = std::max(want, 2 * h->arena_blocks.back().second);
    char* p = nullptr;
    hipError_t e = dev_alloc(h, (void**)&p, want);
    if (e != hipSuccess) return fail(h, O3DS_ERR_OOM, std::string("arena: ") + hipGetErrorString(e));
    h->arena_blocks.emplace_back(p, want);
  }
}
struct ArenaScope {
  o3ds_handle h;
  explicit ArenaScope(o3ds_handle hh) : h(hh) {
    if (h && h->arena_depth++ == 0) {
      // Blocks are never returned or merged while the handle lives: they grow geometrically, so there are at most a
      // handful, and a call simply walks through them.  (Freeing a 32 MB and a 64 MB block and immediately requesting
      // one 96 MB block from the stream-ordered pool corrupted live data on ROCm 7.2 -- timing dependent, reproduced
      // with scripts/debug_stream.py -- so the arena avoids free/alloc churn altogether.)
      h->arena_cur = 0;
      h->arena_off = 0;
    }
  }
  ~ArenaScope() {
    if (h) --h->arena_depth;
  }
};
// tagged span marks on the handle's stream (only while profiling is enabled): begin and end alternate per tag
void span_mark(o3ds_handle h, int tag) {
  if (!h->profiling || tag < 0 || tag >= o3ds_context::kSpanTags) return;
  auto& v = h->span_ev[tag];
  if (h->span_used[tag] >= v.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    v.push_back(e);
  }
  (void)hipEventRecord(v[h->span_used[tag]++], h->stream);
}
constexpr int kSpanNormalsKernels = 8, kSpanIndexBuild = 9, kSpanNeighborKernel = 10;  // internal tags

#define TMP_ALLOC(ptr, bytes)                                   \
  do {                                                          \
    int _rc = arena_alloc(h, (void**)&(ptr), (size_t)(bytes));  \
    if (_rc) return _rc;                                        \
  } while (0)

inline int grid_for(size_t n, int cap = 4096) {
  size_t g = (n + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > (size_t)cap) g = cap;
  return (int)g;
}

size_t p4_size(int precision) { return precision == O3DS_PRECISION_F64 ? sizeof(P4d) : sizeof(P4f); }
// fn<P4> of the storage precision
#define DISPATCH(prec, fn, ...) ((prec) == O3DS_PRECISION_F64 ? fn<P4d>(__VA_ARGS__) : fn<P4f>(__VA_ARGS__))
// ... and a launch that is not worth a function of its own: statements that name the type as P4 (not a generic lambda: its kernels would be
// instantiated behind every other one instead of where they are first used, and the order of the kernels in the code object follows that)
#define WITH_P4(prec, ...)              \
  do {                                  \
    if ((prec) == O3DS_PRECISION_F64) { \
      using P4 = P4d;                   \
      __VA_ARGS__;                      \
    } else {                            \
      using P4 = P4f;                   \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

void cloud_ready(o3ds_handle h, CloudRec& c);
int resolve_count(o3ds_handle h, CloudRec& c, bool block);
// A cloud for an operation on the handle's stream.  find_cloud: with its exact size (waits for a size a kernel has yet to publish -- the
// default, every operation that sizes anything on the host by the cloud); find_cloud_lazy: for the operations of the per-scan chain that
// take the size as it is (an upper bound + the device word, count_ref): normal estimation, registration, map insertion.
int pm_poll(o3ds_handle h, PMapRec* pm, bool block);
int pm_exit(o3ds_handle h, CloudRec& c);  // a persistent submap back into the reference's array form (defined with the map functions)
CloudRec* find_cloud_lazy(o3ds_handle h, o3ds_cloud id) {
  auto it = h->clouds.find(id);
  if (it == h->clouds.end()) return nullptr;
  cloud_ready(h, it->second);
  (void)resolve_count(h, it->second, false);
  return &it->second;
}
CloudRec* find_cloud(o3ds_handle h, o3ds_cloud id) {
  auto it = h->clouds.find(id);
  if (it == h->clouds.end()) return nullptr;
  cloud_ready(h, it->second);
  if (resolve_count(h, it->second, true) != O3DS_OK || (it->second.pm && pm_exit(h, it->second) != O3DS_OK)) {  // whoever wants the map as an
    h->deferred_err = h->err;                                                                                     // array gets the reference's array
    return nullptr;
  }
  return &it->second;
}

void free_index(o3ds_handle h, CloudRec& c) {
  if (c.cell_start) dev_free(h, c.cell_start);
  if (c.spts) dev_free(h, c.spts);
  if (c.snrm) dev_free(h, c.snrm);
  if (c.rpts) dev_free(h, c.rpts);
  if (c.rstart) dev_free(h, c.rstart);
  if (c.rpos) dev_free(h, c.rpos);
  c.cell_start = nullptr;
  c.spts = c.snrm = c.rpts = nullptr;
  c.rstart = c.rpos = nullptr;
  c.index_regs = 0;
  c.spts_slack = c.rpts_slack = 0;
  c.has_index = false;
  c.index_byproduct = false;
}
// ---- records kernels publish into, events, ingest buffers ---------------------------------------------------------------------------
constexpr int kPinRecs = 64;
inline int* cnt_word(o3ds_handle h, int slot) { return h->d_cnt + 16 * slot; }
int resolve_count(o3ds_handle h, CloudRec& c, bool block);

// a free record; when all are held (64 clouds with a size or a box in flight) the oldest holder among the CLOUDS is settled first.  A
// record of a persistent map (kRecOwnerMap) or of a cloud still being made (~0) is never taken from its owner; -1 if every record is one
// of those (sixty-odd persistent maps on one handle: the callers fail or do without)
constexpr uint64_t kRecOwnerMap = ~0ull - 1;
int take_rec(o3ds_handle h) {
  for (int tries = 0; tries < kPinRecs; ++tries) {
    const int slot = h->rec_next;
    h->rec_next = (h->rec_next + 1) % kPinRecs;
    if (h->rec_owner[slot] == 0) {
      h->rec_owner[slot] = ~0ull;  // (taken; add_cloud writes the id)
      return slot;
    }
  }
  for (int tries = 0; tries < kPinRecs; ++tries) {
    const int slot = h->rec_next;
    h->rec_next = (h->rec_next + 1) % kPinRecs;
    auto it = h->clouds.find(h->rec_owner[slot]);
    if (it == h->clouds.end()) continue;  // a map's record, or a cloud in the making
    if (it->second.lazy_slot == slot && resolve_count(h, it->second, true) != O3DS_OK) continue;
    if (it->second.pre_slot == slot && it->second.ingest_ev) continue;  // its box_publish_kernel may still be queued on the copy stream: it would write over the new owner
    if (it->second.pre_slot == slot) it->second.pre_slot = -1;  // the box is reduced again when it is asked for
    h->rec_owner[slot] = ~0ull;
    return slot;
  }
  return -1;
}
// the points of a cloud changed in place, or its point array was replaced: the box the asynchronous ingest reduced (pre_slot / pre_crop) is
// the box of points that no longer exist -- VoxelDownSample's grid origin, the 'nothing inside the volume' return and the index's clamping
// must not be fed from it (advisor, round 5).  The callers have used the cloud on the handle's stream, i.e. its ingest is ordered before
// whatever the record is used for next.
void drop_ingest_box(o3ds_handle h, CloudRec& c) {
  if (c.pre_slot >= 0) {
    h->rec_owner[c.pre_slot] = 0;
    c.pre_slot = -1;
  }
}
hipEvent_t take_event(o3ds_handle h) {
  if (!h->ev_pool.empty()) {
    hipEvent_t e = h->ev_pool.back();
    h->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  return e;
}
// the first use of an ingested cloud on the handle's stream: queue the wait for its copy + unpack (no host wait)
void cloud_ready(o3ds_handle h, CloudRec& c) {
  if (!c.ingest_ev) return;
  (void)hipStreamWaitEvent(h->stream, c.ingest_ev, 0);
  h->ev_pool.push_back(c.ingest_ev);
  c.ingest_ev = nullptr;
}
// the size of a cloud whose count a kernel published: taken from the pinned record if its stamp is there; `block`: wait for it
int resolve_count(o3ds_handle h, CloudRec& c, bool block) {
  if (c.lazy_slot < 0) return O3DS_OK;
  volatile o3ds_context::PinRec* r = h->h_rec + c.lazy_slot;
  if (r->seq != c.lazy_seq) {
    if (!block) return O3DS_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (r->seq != c.lazy_seq) return fail(h, O3DS_ERR_HIP, "the size of a cloud was never published by the kernel that decides it");
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  const int cnt = r->cnt;
  if (cnt < 0 || (size_t)cnt > c.n) return fail(h, O3DS_ERR_HIP, "published cloud size outside its bound");
  c.n = (size_t)cnt;
  h->voxel_count_hint = c.n;
  h->rec_owner[c.lazy_slot] = 0;
  c.lazy_slot = -1;
  return O3DS_OK;
}
// what a consumer kernel is handed for the cloud's size
inline CountRef count_ref(o3ds_handle h, const CloudRec& c) { return CountRef{c.n, c.lazy_slot >= 0 ? cnt_word(h, c.lazy_slot) : nullptr}; }

// the point array of a cloud goes back where it came from: the pool, or the ingest buffers (behind an event on the handle's stream, so
// that the next ingest into the buffer -- on the copy stream -- comes after everything that still reads it here)
void free_points(o3ds_handle h, CloudRec& c) {
  if (c.ingest_ev) cloud_ready(h, c);
  if (c.ingest_buf >= 0) {
    o3ds_context::IngestBuf& b = h->ingest_bufs[(size_t)c.ingest_buf];
    if (!b.freed) (void)hipEventCreateWithFlags(&b.freed, hipEventDisableTiming);
    (void)hipEventRecord(b.freed, h->stream);
    b.in_use = false;
    c.ingest_buf = -1;
  } else if (c.pts) {
    dev_free(h, c.pts);
  }
  c.pts = nullptr;
}
void pm_release(o3ds_handle h, CloudRec& c) {  // the persistent form's own blocks (slot arrays and index arrays stay with the cloud)
  if (!c.pm) return;
  for (void* b : c.pm->blocks) dev_free(h, b);
  if (c.pm->rec_slot >= 0) h->rec_owner[c.pm->rec_slot] = 0;
  delete c.pm;
  c.pm = nullptr;
  c.index_positions = 0;
}
void free_fpfh(o3ds_handle h, CloudRec& c) {
  if (c.fpfh) dev_free(h, c.fpfh);
  c.fpfh = nullptr;
  c.has_fpfh = false;
  c.fpfh_n = 0;
}
void free_cgrad(o3ds_handle h, CloudRec& c) {
  if (c.cgrad) dev_free(h, c.cgrad);
  c.cgrad = nullptr;
  c.has_cgrad = false;
  c.cgrad_n = 0;
}
void drop_cgrad(o3ds_handle h, o3ds_cloud id) {  // the entry points that change a cloud's colours in place
  auto it = h->clouds.find(id);
  if (it != h->clouds.end()) free_cgrad(h, it->second);
}
void drop_fpfh(o3ds_handle h, o3ds_cloud id) {  // the entry points that change a cloud's points or normals in place: the colour gradients go too
  auto it = h->clouds.find(id);
  if (it != h->clouds.end()) {
    free_fpfh(h, it->second);
    free_cgrad(h, it->second);
  }
}
void free_cloud(o3ds_handle h, CloudRec& c) {
  free_fpfh(h, c);
  free_cgrad(h, c);
  pm_release(h, c);
  free_index(h, c);
  free_points(h, c);
  if (c.nrm) dev_free(h, c.nrm);
  if (c.col) dev_free(h, c.col);
  c.nrm = c.col = nullptr;
  if (c.lazy_slot >= 0) h->rec_owner[c.lazy_slot] = 0;
  if (c.pre_slot >= 0) h->rec_owner[c.pre_slot] = 0;
  c.lazy_slot = c.pre_slot = -1;
  c.n = 0;
  c.cap = 0;
}

// a cloud under construction in a function that may still fail: freed on every early return, handed over by release()
struct CloudGuard {
  o3ds_handle h;
  CloudRec* c;
  CloudGuard(o3ds_handle hh, CloudRec& cc) : h(hh), c(&cc) {}
  ~CloudGuard() {
    if (c) free_cloud(h, *c);
  }
  void release() { c = nullptr; }
};
// ... and an index under construction over points its record only borrows: the index is freed on every early return, kept by release()
struct IndexGuard {
  o3ds_handle h;
  CloudRec* c;
  IndexGuard(o3ds_handle hh, CloudRec& cc) : h(hh), c(&cc) {}
  ~IndexGuard() {
    if (c) free_index(h, *c);
  }
  void release() { c = nullptr; }
};

// exclusive scan of m ints (in -> out) with the hand-written 3-phase scan; in may alias out
// pub: null, or a device-visible address (the handle's pinned block) that also receives out[m - 1] -- the total, when the input ends in a
// zero sentinel -- from the kernel that finishes that element
// local(nb, sums, pub): the launch of the first phase, which reads the input (an array: exclusive_scan_t, a functor: exclusive_scan_fn)
template <typename T, typename L>
int exclusive_scan_phases(o3ds_handle h, T* out, size_t m, T* pub, L&& local) {
  if (m == 0) return O3DS_OK;
  const int nb = (int)((m + kScanPerBlock - 1) / kScanPerBlock);
  T* sums = nullptr;
  TMP_ALLOC(sums, sizeof(T) * (size_t)nb);
  local(nb, sums, nb == 1 ? pub : nullptr);
  if (nb > 1 && nb <= kScanFusedBlocks) {
    scan_add_fused_kernel<T><<<nb, kBlock, 0, h->stream>>>(out, sums, m, pub);
  } else if (nb > 1) {
    scan_sums_kernel<T><<<1, kBlock, 0, h->stream>>>(sums, nb);
    scan_add_kernel<T><<<nb, kBlock, 0, h->stream>>>(out, sums, m, pub);
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;  // results are stream-ordered; callers that need a value on the host copy it back and synchronise
}
template <typename T>
int exclusive_scan_t(o3ds_handle h, const T* in, T* out, size_t m, T* pub = nullptr) {
  return exclusive_scan_phases<T>(h, out, m, pub, [&](int nb, T* sums, T* p) { scan_local_kernel<T><<<nb, kBlock, 0, h->stream>>>(in, out, sums, m, p); });
}
template <typename T, typename Fn>
int exclusive_scan_fn(o3ds_handle h, Fn in, T* out, size_t m, T* pub = nullptr) {  // the input is in(i), i < m
  return exclusive_scan_phases<T>(h, out, m, pub, [&](int nb, T* sums, T* p) { scan_local_fn_kernel<T, Fn><<<nb, kBlock, 0, h->stream>>>(in, out, sums, m, p); });
}
int exclusive_scan_int(o3ds_handle h, const int* in, int* out, size_t m, int* pub = nullptr) { return exclusive_scan_t<int>(h, in, out, m, pub); }

// slots of the pinned block for values kernels publish themselves (the front of the block belongs to bbox_of / read_back)
template <typename T>
T* pub_slot(o3ds_handle h, int k) { return (T*)(h->h_pin_dev + kPubOff + 16 * (size_t)k); }
template <typename T>
T pub_value(o3ds_handle h, int k) { return *(const volatile T*)(h->h_pin + kPubOff + 16 * (size_t)k); }
int wait_stream(o3ds_handle h) {
  HIP_TRY(hipStreamSynchronize(h->stream));
  return O3DS_OK;
}

// ---- what the cloud and map operations share ------------------------------------------------------------------------
// n (key, value) pairs in ascending order of the key bits [0, end_bit), equal keys in their order of arrival: rocPRIM's radix sort,
// its temporary (its own ping-pong buffers of n keys and values among it: about 12 bytes per pair) from the arena.  `keep`: a caller
// that sorts the same number of pairs again hands the same SortTemp to both calls, and the second sort runs in the first one's temporary
struct SortTemp {
  void* p = nullptr;
  size_t bytes = 0;
};
int sort_pairs(o3ds_handle h, unsigned long long* k_in, unsigned long long* k_out, uint32_t* v_in, uint32_t* v_out, size_t n, unsigned int end_bit = 64,
               SortTemp* keep = nullptr) {
  SortTemp own;
  SortTemp& t = keep ? *keep : own;
  if (!t.p) {
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, t.bytes, k_in, k_out, v_in, v_out, n, 0, end_bit, h->stream));
    TMP_ALLOC(t.p, t.bytes ? t.bytes : 16);
  }
  HIP_TRY(rocprim::radix_sort_pairs(t.p, t.bytes, k_in, k_out, v_in, v_out, n, 0, end_bit, h->stream));
  return O3DS_OK;
}

// head[0..n] (1 where a segment starts, head[n] = 0: the sentinel) -> seg_id[0..n], its exclusive scan, which ends with the number of
// segments: read back into *n_seg (null: not wanted)
int segment_ids(o3ds_handle h, const int* head, int* seg_id, size_t n, int* n_seg) {
  const int rc = exclusive_scan_int(h, head, seg_id, n + 1);
  if (rc || !n_seg) return rc;
  return read_back(h, {{n_seg, seg_id + n, sizeof(int)}});
}
// ... of keys in ascending order: a segment is a run of equal keys
int key_segments(o3ds_handle h, const unsigned long long* sorted_keys, size_t n, int* head, int* seg_id, int* n_seg) {
  segment_head_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(sorted_keys, n, head);  // also writes the sentinel head[n] = 0
  return segment_ids(h, head, seg_id, n, n_seg);
}

// the upper three rows of a pose (4 x 4, column-major) as the kernels take them; null: the identity
Mat34 mat34(const double* T) {
  Mat34 M;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M.m[r * 4 + c] = T ? T[c * 4 + r] : (r == c ? 1.0 : 0.0);
  return M;
}

// Scratch the handle owns and grows on demand (d_cells, d_voxtab, d_tiles, d_nn_cache): room for `want` elements in *ptr.  A block that
// is too small is given back -- behind a synchronisation: work in flight may still use it -- and one of `new_cap` elements (`new_bytes`
// bytes) is allocated; *fresh: the block is new, nothing is known of its contents.  An allocation that fails is the caller's to report
// (or to live with: build_replica_t): it finds *ptr null.
template <typename T>
int handle_scratch(o3ds_handle h, T** ptr, size_t* cap, size_t want, size_t new_cap, size_t new_bytes, bool* fresh) {
  *fresh = false;
  if (*cap >= want) return O3DS_OK;
  if (*ptr) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
  }
  if (hipMalloc((void**)ptr, new_bytes) != hipSuccess) {
    *ptr = nullptr;
    return O3DS_OK;
  }
  *cap = new_cap;
  *fresh = true;
  return O3DS_OK;
}
// per-cell counters for a table of ncell cells: the handle's block of zeros (ncell + 1: the scan's sentinel stays zero), counted up by
// a count kernel, read by the scan, counted back down to zero by the scatter -- after which the caller sets cells_clean again (stream
// order: whoever counts next runs after that scatter).  h->d_cells is null when the allocation failed.
int cell_counters(o3ds_handle h, size_t ncell) {
  bool fresh = false;
  const int rc = handle_scratch(h, &h->d_cells, &h->cells_cap, ncell + 1, ncell + 1 + ncell / 4, sizeof(int) * (ncell + 1 + ncell / 4), &fresh);
  if (rc || !h->d_cells) return rc;
  if (fresh) h->cells_clean = false;
  if (!h->cells_clean) HIP_TRY(hipMemsetAsync(h->d_cells, 0, sizeof(int) * h->cells_cap, h->stream));
  h->cells_clean = false;
  return O3DS_OK;
}
// the scratch of vox_insert_kernel / pm_place_kernel and vox_order_kernel for n points.  The handle's voxel table: all 0xff between calls
// (vox_mean_kernel / pm_group_kernel empty the slots a call used, after which the caller sets voxtab_clean again), grown to the largest
// cloud seen.  The chained scan's tile records: kept across calls, never cleared (they carry the call's number, see vox_order_kernel)
int vox_scratch(o3ds_handle h, size_t n, const char* what, VoxTable* table, size_t* n_tiles) {
  size_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  bool fresh = false;
  int rc = handle_scratch(h, &h->d_voxtab, &h->voxtab_cap, cap, cap, kVoxSlotBytes * cap + 16, &fresh);
  if (rc) return rc;
  if (!h->d_voxtab) return fail(h, O3DS_ERR_OOM, std::string(what) + ": voxel table allocation failed");
  if (fresh) h->voxtab_clean = false;
  cap = h->voxtab_cap;
  unsigned char* tab = h->d_voxtab;
  *table = VoxTable{(VoxSlot*)tab, (unsigned int*)(tab + kVoxSlotBytes * cap), (unsigned int)(cap - 1)};
  if (!h->voxtab_clean) HIP_TRY(hipMemsetAsync(tab, 0xff, kVoxSlotBytes * cap + 16, h->stream));
  h->voxtab_clean = false;
  *n_tiles = (n + kVoxTile - 1) / kVoxTile;
  const size_t tiles = std::max<size_t>(*n_tiles + *n_tiles / 4, 1024);
  rc = handle_scratch(h, &h->d_tiles, &h->tiles_cap, *n_tiles, tiles, sizeof(unsigned long long) * tiles, &fresh);
  if (rc) return rc;
  if (!h->d_tiles) return fail(h, O3DS_ERR_OOM, std::string(what) + ": scan state allocation failed");
  if (fresh) {
    const hipError_t e = hipMemsetAsync(h->d_tiles, 0, sizeof(unsigned long long) * tiles, h->stream);
    if (e != hipSuccess) h->tiles_cap = 0;  // (never zeroed: the next call must not take it for a block in use)
    HIP_TRY(e);
  }
  return O3DS_OK;
}

// the points (+ normals) of `in` whose flag is `which` -- m of its first n, to the positions `pos` -- and then its colours, which ride along
// as a second attribute array through the same kernel; the arrays are allocated here, unless the caller has done so before its own launches
template <typename P4>
int compact_cloud(o3ds_handle h, const CloudRec& in, size_t n, const int* flags, const int* pos, int which, size_t m, void** pts, void** nrm, void** col) {
  if (!*pts) HIP_TRY(dev_alloc(h, pts, sizeof(P4) * m));
  if (in.nrm && !*nrm) HIP_TRY(dev_alloc(h, nrm, sizeof(P4) * m));
  compact_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.pts, (const P4*)in.nrm, n, flags, pos, which, (P4*)*pts, (P4*)*nrm);
  if (in.col) {
    if (!*col) HIP_TRY(dev_alloc(h, col, sizeof(P4) * m));
    compact_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.col, nullptr, n, flags, pos, which, (P4*)*col, nullptr);
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}
// ... and the points idx[0..m) of `in`, in that order, as the arrays of `out`
template <typename P4>
int gather_cloud(o3ds_handle h, const CloudRec& in, const uint32_t* idx, size_t m, CloudRec& out) {
  HIP_TRY(dev_alloc(h, &out.pts, sizeof(P4) * m));
  if (in.nrm) HIP_TRY(dev_alloc(h, &out.nrm, sizeof(P4) * m));
  gather_kernel<P4><<<grid_for(m), kBlock, 0, h->stream>>>((const P4*)in.pts, (const P4*)in.nrm, idx, m, (P4*)out.pts, (P4*)out.nrm);
  if (in.col) {
    HIP_TRY(dev_alloc(h, &out.col, sizeof(P4) * m));
    gather_kernel<P4><<<grid_for(m), kBlock, 0, h->stream>>>((const P4*)in.col, nullptr, idx, m, (P4*)out.col, nullptr);
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

// a cloud's arrays are replaced by new ones (a carve, an append, a fold): n points in arrays with room for `cap` (0: exactly n); its
// index goes, the vox_first / vox_count layout is the caller's to set
void replace_arrays(o3ds_handle h, CloudRec& c, void* pts, void* nrm, void* col, size_t n, size_t cap) {
  free_index(h, c);
  free_points(h, c);
  if (c.nrm) dev_free(h, c.nrm);
  if (c.col) dev_free(h, c.col);
  c.pts = pts;
  c.nrm = nrm;
  c.col = col;
  c.n = n;
  c.cap = cap;
}

// The fused registration loop's wait.  The launch the host waits for writes the state into pinned memory and then, with a system-scope
// release, the stamp `seq` into a pinned word (icp_fused_kernel); every earlier launch of the stream has completed by then, and once the
// loop is done the rest of that launch is workgroups returning.  Watching the word hands the result over as it is written instead of
// after the kernel's completion signal has made its way through the runtime (a few microseconds per registration of ~200).  A stamp
// that does not show up within 50 ms (a faulted queue) falls back to the stream wait, which reports the error.
constexpr int kSeqSlot = 8;
constexpr int kWaitSpinUs = 20;
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}
hipError_t wait_fused_state(o3ds_handle h, unsigned long long seq) {
  const volatile unsigned long long* w = (const volatile unsigned long long*)(h->h_pin + kPubOff + 16 * (size_t)kSeqSlot);
  // spin for ~20 us (a steady pass launch is 10 us: the stamp of a registration that is about to finish shows up inside that), then
  // give the core away between looks: SlamWrapper runs four to seven threads (SlamWrapper.cpp:227-236) and a GPU box grants its
  // container a CPU quota -- a core that spins through a whole registration is a core the other worker does not get
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned int spins = 1;; ++spins) {
    if (*w == seq) {
      std::atomic_thread_fence(std::memory_order_acquire);
      return hipSuccess;
    }
    cpu_relax();
    if ((spins & 0x3fu) == 0) {
      const auto dt = std::chrono::steady_clock::now() - t0;
      if (dt > std::chrono::milliseconds(50)) break;
      if (dt > std::chrono::microseconds(kWaitSpinUs)) sched_yield();
    }
  }
  return hipStreamSynchronize(h->stream);
}

template <typename P4>
int bbox_of(o3ds_handle h, const P4* pts, size_t n, double mn[3], double mx[3], const CropDev* crop = nullptr) {
  const int g = grid_for(n, 1024);  // 1024 x 48 B fit the pinned block below the published slots
  static_assert(1024 * 6 * sizeof(double) <= kPinBytes - 256, "bbox partials fit the pinned block");
  CropDev all{};
  bbox_kernel<P4><<<g, kBlock, 0, h->stream>>>(pts, n, crop ? *crop : all, (double*)h->h_pin_dev);  // every block stores its box there itself
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  const double* hb = (const double*)h->h_pin;
  for (int a = 0; a < 3; ++a) {
    mn[a] = 1e300;
    mx[a] = -1e300;
  }
  for (int b = 0; b < g; ++b)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], hb[(size_t)b * 6 + a]);
      mx[a] = std::max(mx[a], hb[(size_t)b * 6 + 3 + a]);
    }
  return O3DS_OK;
}

// Build one uniform grid over `pts`: cell_start (exclusive scan of the per-cell counts) and the points (+ normals when
// given) re-stored in cell order.  Output buffers are allocated here; the caller owns them.
template <typename P4>
int build_grid_t(o3ds_handle h, const P4* pts, const P4* nrm, size_t n, double cell, GridDev* out_grid, int** out_cell_start, void** out_spts,
                 void** out_snrm, size_t* out_slack /* bytes allocated behind spts[n - 1] */,
                 CloudRec* box /* in: a known box, if has_box; out: the box used */,
                 const int* n_dev = nullptr /* n is an upper bound, the exact count is here (a cloud whose size the host has not seen: it then brings its box) */) {
  if (n == 0) return fail(h, O3DS_ERR_EMPTY, "build_index: empty cloud");
  if (n > scan_capacity<P4>())
    return fail(h, O3DS_ERR_CAPACITY, "build_index: the cell-sorted points exceed 2^32 bytes less the scan loop's slack (the search addresses them by 32-bit byte offsets)");
  double mn[3], mx[3];
  int rc = O3DS_OK;
  if (box && box->has_box) {
    for (int a = 0; a < 3; ++a) mn[a] = box->bmn[a], mx[a] = box->bmx[a];
  } else {
    if (n_dev) return fail(h, O3DS_ERR_INVALID_ARG, "build_index: a cloud whose size is still in flight must bring its box");
    rc = bbox_of<P4>(h, pts, n, mn, mx);
    if (rc) return rc;
    if (box) {
      box->has_box = true;
      box->box_padded = false;  // exact bounds of the stored values
      for (int a = 0; a < 3; ++a) box->bmn[a] = mn[a], box->bmx[a] = mx[a];
    }
  }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) return fail(h, O3DS_ERR_INVALID_ARG, "build_index: non-finite coordinates");
  size_t nx, ny, nz;
  for (;;) {
    nx = (size_t)std::floor((mx[0] - mn[0]) / cell) + 1;
    ny = (size_t)std::floor((mx[1] - mn[1]) / cell) + 1;
    nz = (size_t)std::floor((mx[2] - mn[2]) / cell) + 1;
    if (nx * ny * nz <= kMaxCells) break;
    cell *= 1.26;  // ~ x2 fewer cells per step
  }
  const size_t ncell = nx * ny * nz;
  GridDev g{};
  g.ox = mn[0];
  g.oy = mn[1];
  g.oz = mn[2];
  g.cell = cell;
  g.inv_cell = 1.0 / cell;
  g.nx = (int)nx;
  g.sx = (int)nx;
  g.ny = (int)ny;
  g.nz = (int)nz;
  int *counts = nullptr, *cell_id = nullptr, *cell_start = nullptr;
  void *spts = nullptr, *snrm = nullptr;
  rc = cell_counters(h, ncell);  // counted up by cell_count_kernel, counted back down to zero by scatter_kernel
  if (rc) return rc;
  if (!h->d_cells) return fail(h, O3DS_ERR_OOM, "build_index: cell counters allocation failed");
  counts = h->d_cells;
  TMP_ALLOC(cell_id, sizeof(int) * n);
  HIP_TRY(dev_alloc(h, (void**)&cell_start, sizeof(int) * (ncell + 1 + 4)));  // +4: the search reads rows as unaligned 16-B vectors
  // (the slack is never written and never looked at: scan_strided)
  const size_t slack = scan_slack_alloc();
  HIP_TRY(dev_alloc(h, (void**)&spts, sizeof(P4) * n + slack));
  if (nrm) HIP_TRY(dev_alloc(h, (void**)&snrm, sizeof(P4) * n));
  span_mark(h, kSpanIndexBuild);
  cell_count_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(pts, n, g, counts, cell_id, n_dev);
  rc = exclusive_scan_int(h, counts, cell_start, ncell + 1);
  if (rc) return rc;
  scatter_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(pts, nrm, n, cell_id, cell_start, counts, (P4*)spts, (P4*)snrm, n_dev);
  span_mark(h, kSpanIndexBuild);
  HIP_TRY(hipGetLastError());
  h->cells_clean = true;  // (stream order: whoever counts next runs after the scatter)
  g.cell_start = cell_start;
  *out_grid = g;
  *out_cell_start = cell_start;
  *out_spts = spts;
  *out_slack = slack;
  if (out_snrm) *out_snrm = snrm;
  return O3DS_OK;
}

template <typename P4>
int build_index_t(o3ds_handle h, CloudRec& c, double cell) {
  free_index(h, c);
  if (c.lazy_slot >= 0 && !c.has_box) {
    const int rr = resolve_count(h, c, true);
    if (rr) return rr;
  }
  int rc = build_grid_t<P4>(h, (const P4*)c.pts, (const P4*)c.nrm, c.n, cell, &c.grid, &c.cell_start, &c.spts, &c.snrm, &c.spts_slack, &c,
                            c.lazy_slot >= 0 ? cnt_word(h, c.lazy_slot) : nullptr);
  if (rc) return rc;
  c.has_index = true;
  return O3DS_OK;
}

constexpr double kIndexCellDiv = 4.0;  // grid cell of a registration target = max_correspondence_distance / this

int build_index(o3ds_handle h, CloudRec& c, double cell) { return DISPATCH(c.precision, build_index_t, h, c, cell); }

// The neighbourhood-major replica of an index (GridDev::rpts), built from its cell-sorted points: one count, one scan and one scatter
// (replica_count_kernel / replica_scatter_kernel).  Not built when it does not fit (kReplicaMaxBytes, kMaxCells) or the memory is not there:
// the index then stays without one and the search takes the rows of cell_start.
template <typename P4>
int build_replica_t(o3ds_handle h, CloudRec& c) {
  GridDev g = c.grid;
  const size_t n = c.n, rcell = (size_t)g.nx * (size_t)(g.ny + 2) * (size_t)(g.nz + 2);  // super-row cells
  if (rcell > kMaxCells || 9 * n > (size_t)INT_MAX || 9 * n * (sizeof(P4) + sizeof(int)) + sizeof(int) * (rcell + 1) > kReplicaMaxBytes) return O3DS_OK;
  void* rpts = nullptr;
  int *rstart = nullptr, *rpos = nullptr;
  if (dev_alloc(h, (void**)&rstart, sizeof(int) * (rcell + 1)) != hipSuccess || dev_alloc(h, &rpts, sizeof(P4) * 9 * n + scan_slack_alloc()) != hipSuccess ||
      dev_alloc(h, (void**)&rpos, sizeof(int) * 9 * n) != hipSuccess) {
    (void)hipGetLastError();
    if (rstart) dev_free(h, rstart);
    if (rpts) dev_free(h, rpts);
    return O3DS_OK;
  }
  const int rs = cell_counters(h, rcell);  // as in build_grid_t
  if (rs || !h->d_cells) {  // (no memory for the counters: no replica, no error)
    (void)hipGetLastError();
    dev_free(h, rstart), dev_free(h, rpts), dev_free(h, rpos);
    return rs;
  }
  int* rcounts = h->d_cells;
  const int* n_dev = c.lazy_slot >= 0 ? cnt_word(h, c.lazy_slot) : nullptr;
  replica_count_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)c.spts, n, g, rcounts, n_dev);
  const int rc = exclusive_scan_int(h, rcounts, rstart, rcell + 1);
  if (rc) {
    dev_free(h, rstart), dev_free(h, rpts), dev_free(h, rpos);
    return rc;
  }
  replica_scatter_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)c.spts, n, g, rstart, rcounts, (P4*)rpts, rpos, n_dev);
  HIP_TRY(hipGetLastError());
  h->cells_clean = true;
  c.rpts = rpts;
  c.rpts_slack = scan_slack_alloc();
  c.rstart = rstart;
  c.rpos = rpos;
  c.grid.rpts = rpts;
  c.grid.rstart = rstart;
  c.grid.rpos = rpos;
  return O3DS_OK;
}

// The replica pays for itself only over repeated registrations against one index (its build costs about what seven or eight 10-pass
// registrations of configs[1] save), so it is built at the kReplicaAfterRegs-th registration against an index, not with the index: the
// indexes a stream rebuilds every frame (the scan a registration targets, a submap after each insertion) are registered against once and
// never pay for it.  Row-paged (persistent-map) indexes have none.  O3DS_NN_REPLICA_AFTER=<k> (A/B library): at the k-th registration.
constexpr int kReplicaAfterRegs = 4;
int maybe_build_replica(o3ds_handle h, CloudRec& c) {
  if (!c.has_index || c.rpts || c.pm || c.index_positions) return O3DS_OK;
  const char* e = ab_getenv("O3DS_NN_REPLICA_AFTER");
  const int after = e ? std::max(1, atoi(e)) : kReplicaAfterRegs;
  if (++c.index_regs < after) return O3DS_OK;
  return DISPATCH(c.precision, build_replica_t, h, c);
}

// f32 storage: the caller's doubles are narrowed on their way into the pinned ring (the narrowing the device would do: round to nearest
// even) and widened on their way out, so half the bytes cross PCIe and the host touches every value once either way
int h2d_copy_narrow(o3ds_handle h, float* d_dst, const double* h_src, size_t count) {
  int rc = stage_init(h);
  if (rc) return rc;
  const size_t per = kStageBytes / sizeof(float);
  int k = 0;
  for (size_t off = 0; off < count; off += per, k ^= 1) {
    const size_t n = std::min(per, count - off);
    HIP_TRY(hipEventSynchronize(h->stage_ev[k]));
    float* dst = (float*)h->h_stage[k];
    const double* src = h_src + off;
    for (size_t i = 0; i < n; ++i) dst[i] = (float)src[i];
    HIP_TRY(hipMemcpyAsync(d_dst + off, dst, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->stage_ev[k], h->stream));
  }
  return O3DS_OK;
}
int d2h_copy_widen(o3ds_handle h, double* h_dst, const float* d_src, size_t count) {  // synchronous
  int rc = stage_init(h);
  if (rc) return rc;
  const size_t per = kStageBytes / sizeof(float);
  const size_t chunks = (count + per - 1) / per;
  for (size_t c = 0; c <= chunks; ++c) {
    if (c < chunks) {
      const size_t off = c * per, n = std::min(per, count - off);
      HIP_TRY(hipMemcpyAsync(h->h_stage[c & 1], d_src + off, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipEventRecord(h->stage_ev[c & 1], h->stream));
    }
    if (c > 0) {
      const size_t off = (c - 1) * per, n = std::min(per, count - off);
      HIP_TRY(hipEventSynchronize(h->stage_ev[(c - 1) & 1]));
      const float* src = (const float*)h->h_stage[(c - 1) & 1];
      double* dst = h_dst + off;
      for (size_t i = 0; i < n; ++i) dst[i] = (double)src[i];
    }
  }
  return O3DS_OK;
}
template <typename P4>
int upload_array_t(o3ds_handle h, const double* host, size_t n, P4* d_out) {  // host double[3n] -> device P4[n]
  if (std::is_same<P4, P4f>::value && sizeof(double) * 3 * n >= kStageMin) {
    float* stage = nullptr;
    TMP_ALLOC(stage, sizeof(float) * 3 * n);
    const int rcc = h2d_copy_narrow(h, stage, host, 3 * n);
    if (rcc) return rcc;
    pack_kernel<P4, float><<<grid_for(n), kBlock, 0, h->stream>>>(stage, n, d_out);
    return O3DS_OK;
  }
  double* stage = nullptr;
  TMP_ALLOC(stage, sizeof(double) * 3 * n);
  const int rcc = h2d_copy(h, stage, host, sizeof(double) * 3 * n);
  if (rcc) return rcc;
  pack_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(stage, n, d_out);
  return O3DS_OK;
}
template <typename P4>
int download_array_t(o3ds_handle h, const P4* d_in, size_t n, double* host) {  // device P4[n] -> host double[3n]; complete on return
  if (std::is_same<P4, P4f>::value && sizeof(double) * 3 * n >= kStageMin) {
    float* stage = nullptr;
    TMP_ALLOC(stage, sizeof(float) * 3 * n);
    unpack_kernel<P4, float><<<grid_for(n), kBlock, 0, h->stream>>>(d_in, n, stage);
    return d2h_copy_widen(h, host, stage, 3 * n);
  }
  double* stage = nullptr;
  TMP_ALLOC(stage, sizeof(double) * 3 * n);
  unpack_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(d_in, n, stage);
  return d2h_copy(h, host, stage, sizeof(double) * 3 * n);
}

template <typename P4>
int upload_t(o3ds_handle h, const double* xyz, const double* normals, size_t n, CloudRec& c) {
  c.n = n;
  c.precision = h->precision;
  if (n == 0) return O3DS_OK;
  HIP_TRY(dev_alloc(h, (void**)&c.pts, sizeof(P4) * n));
  int rcc = upload_array_t<P4>(h, xyz, n, (P4*)c.pts);
  if (rcc) return rcc;
  if (normals) {
    HIP_TRY(dev_alloc(h, (void**)&c.nrm, sizeof(P4) * n));
    rcc = upload_array_t<P4>(h, normals, n, (P4*)c.nrm);
    if (rcc) return rcc;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));  // the caller may release its host buffers as soon as this returns
  return O3DS_OK;
}

template <typename P4>
int download_t(o3ds_handle h, const CloudRec& c, double* xyz, double* normals) {
  if (c.n == 0) return O3DS_OK;
  if (xyz) {
    const int rcc = download_array_t<P4>(h, (const P4*)c.pts, c.n, xyz);
    if (rcc) return rcc;
  }
  if (normals && c.nrm) {
    const int rcc = download_array_t<P4>(h, (const P4*)c.nrm, c.n, normals);
    if (rcc) return rcc;
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

o3ds_cloud add_cloud(o3ds_handle h, CloudRec&& c) {
  const uint64_t id = h->next_id++;
  if (c.lazy_slot >= 0) h->rec_owner[c.lazy_slot] = id;
  if (c.pre_slot >= 0) h->rec_owner[c.pre_slot] = id;
  h->clouds.emplace(id, std::move(c));
  return id;
}
// a new cloud as the result of a call: fill(cloud) makes it; freed if that fails, registered under a new id in *out otherwise
template <typename F>
int new_cloud(o3ds_handle h, o3ds_cloud* out, F&& fill) {
  CloudRec c;
  CloudGuard c_guard(h, c);
  const int rc = fill(c);
  if (rc) return rc;
  if (out) {  // (null: an output the caller did not ask for)
    c_guard.release();
    *out = add_cloud(h, std::move(c));
  }
  return O3DS_OK;
}
// device copies of a cloud's arrays (n elements each; nrm and col may be null) into the arrays of the new cloud `o`, which they are allocated for
int copy_arrays(o3ds_handle h, CloudRec& o, size_t n, const void* pts, const void* nrm, const void* col) {
  const size_t bytes = p4_size(o.precision) * n;
  const void* from[3] = {pts, nrm, col};
  void** to[3] = {&o.pts, &o.nrm, &o.col};
  for (int k = 0; k < 3; ++k)
    if (from[k]) {
      HIP_TRY(dev_alloc(h, to[k], bytes));
      HIP_TRY(hipMemcpyAsync(*to[k], from[k], bytes, hipMemcpyDeviceToDevice, h->stream));
    }
  return O3DS_OK;
}

const double kIdentity16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// ---- dense voxel map helpers -----------------------------------------------------------------------
void dense_release(o3ds_handle h, DenseRec& d) {
  if (d.dev.keys) dev_free(h, d.dev.keys);
  if (d.dev.cnt) dev_free(h, d.dev.cnt);
  if (d.dev.sp) dev_free(h, d.dev.sp);
  if (d.dev.sn) dev_free(h, d.dev.sn);
  if (d.dev.sc) dev_free(h, d.dev.sc);
  d.dev = o3ds::DenseDev{};
  d.cap = 0;
}

void ndt_release(o3ds_handle h, NdtRec& g) {
  for (void* p : {(void*)g.keys, (void*)g.counts, (void*)g.mean, (void*)g.cov, (void*)g.information, (void*)g.valid, (void*)g.rec})
    if (p) dev_free(h, p);
  g = NdtRec{};
}

int dense_alloc(o3ds_handle h, size_t cap, o3ds::DenseDev* out) {
  o3ds::DenseDev d{};
  HIP_TRY(dev_alloc(h, (void**)&d.keys, sizeof(unsigned long long) * cap));
  HIP_TRY(dev_alloc(h, (void**)&d.cnt, sizeof(int) * cap));
  HIP_TRY(dev_alloc(h, (void**)&d.sp, sizeof(long long) * 3 * cap));
  HIP_TRY(dev_alloc(h, (void**)&d.sn, sizeof(long long) * 3 * cap));
  HIP_TRY(dev_alloc(h, (void**)&d.sc, sizeof(long long) * 3 * cap));
  HIP_TRY(hipMemsetAsync(d.keys, 0xFF, sizeof(unsigned long long) * cap, h->stream));
  HIP_TRY(hipMemsetAsync(d.cnt, 0, sizeof(int) * cap, h->stream));
  HIP_TRY(hipMemsetAsync(d.sp, 0, sizeof(long long) * 3 * cap, h->stream));
  HIP_TRY(hipMemsetAsync(d.sn, 0, sizeof(long long) * 3 * cap, h->stream));
  HIP_TRY(hipMemsetAsync(d.sc, 0, sizeof(long long) * 3 * cap, h->stream));
  d.mask = (unsigned int)(cap - 1);
  *out = d;
  return O3DS_OK;
}

// number of live voxels and of occupied slots (one scan + two small read backs)
int dense_count(o3ds_handle h, DenseRec& d, size_t* n_live, int** flag_out = nullptr, int** pos_out = nullptr, size_t* n_occupied = nullptr) {
  *n_live = 0;
  if (n_occupied) *n_occupied = 0;
  if (d.cap == 0) return O3DS_OK;
  int *flag = nullptr, *pos = nullptr;
  unsigned long long* d_occ = nullptr;
  TMP_ALLOC(flag, sizeof(int) * (d.cap + 1));
  TMP_ALLOC(pos, sizeof(int) * (d.cap + 1));
  TMP_ALLOC(d_occ, sizeof(unsigned long long));
  HIP_TRY(hipMemsetAsync(flag + d.cap, 0, sizeof(int), h->stream));
  HIP_TRY(hipMemsetAsync(d_occ, 0, sizeof(unsigned long long), h->stream));
  dense_used_flag_kernel<<<grid_for(d.cap), kBlock, 0, h->stream>>>(d.dev, d.cap, flag, d_occ);
  int rc = exclusive_scan_int(h, flag, pos, d.cap + 1);
  if (rc) return rc;
  int total = 0;
  unsigned long long occ = 0;
  rc = read_back(h, {{&total, pos + d.cap, sizeof(int)}, {&occ, d_occ, sizeof(occ)}});
  if (rc) return rc;
  *n_live = (size_t)total;
  if (n_occupied) *n_occupied = (size_t)occ;
  d.used_upper = (size_t)occ;  // exact now
  if (flag_out) *flag_out = flag;
  if (pos_out) *pos_out = pos;
  return O3DS_OK;
}

// make room for up to n_new more voxels: occupied slots (live + tombstones) stay <= cap / 2, so a probe always finds a free slot
int dense_reserve(o3ds_handle h, DenseRec& d, size_t n_new) {
  if (d.cap && (d.used_upper + n_new) * 2 <= d.cap) {
    d.used_upper += n_new;
    return O3DS_OK;
  }
  size_t live = 0, occupied = 0;
  if (d.cap) {
    int rc = dense_count(h, d, &live, nullptr, nullptr, &occupied);  // the bound was pessimistic (most points fall into existing voxels)
    if (rc) return rc;
    if ((occupied + n_new) * 2 <= d.cap) {
      d.used_upper = occupied + n_new;
      return O3DS_OK;
    }
  }
  // rehash: only live voxels move, tombstones are dropped -- so the new table may even be the same size as the old one
  size_t cap = 1024;
  while (cap < 4 * (live + n_new)) cap <<= 1;
  if (cap > ((size_t)1 << 31)) return fail(h, O3DS_ERR_OOM, "dense map: table would exceed 2^31 slots");
  o3ds::DenseDev nd{};
  int rc = dense_alloc(h, cap, &nd);
  if (rc) return rc;
  if (d.cap) {
    dense_rehash_kernel<<<grid_for(d.cap), kBlock, 0, h->stream>>>(d.dev, d.cap, nd);
    HIP_TRY(hipGetLastError());
    DenseRec old = d;
    dense_release(h, old);
  }
  d.dev = nd;
  d.cap = cap;
  d.used_upper = live + n_new;
  return O3DS_OK;
}

template <typename P4>
int dense_insert_t(o3ds_handle h, DenseRec& d, const CloudRec& c, const double T[16]) {
  if (c.n == 0) return O3DS_OK;
  int rc = dense_reserve(h, d, c.n);
  if (rc) return rc;
  dense_insert_kernel<P4><<<grid_for(c.n), kBlock, 0, h->stream>>>((const P4*)c.pts, (const P4*)c.nrm, (const P4*)c.col, c.n, mat34(T), 1.0 / d.voxel, d.dev);
  HIP_TRY(hipGetLastError());
  if (c.nrm) d.has_normals = true;  // isHasNormals_, Voxel.cpp:80-83
  if (c.col) d.has_colors = true;   // isHasColors_, Voxel.cpp:84-87
  return O3DS_OK;
}

template <typename P4>
int dense_to_cloud_t(o3ds_handle h, DenseRec& d, CloudRec& out) {
  out.precision = h->precision;
  out.n = 0;
  size_t used = 0;
  int *flag = nullptr, *pos = nullptr;
  int rc = dense_count(h, d, &used, &flag, &pos);
  if (rc || used == 0) return rc;
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  uint32_t *s0 = nullptr, *s1 = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * used);
  TMP_ALLOC(k1, sizeof(unsigned long long) * used);
  TMP_ALLOC(s0, sizeof(uint32_t) * used);
  TMP_ALLOC(s1, sizeof(uint32_t) * used);
  dense_list_kernel<<<grid_for(d.cap), kBlock, 0, h->stream>>>(d.dev, d.cap, flag, pos, k0, s0);
  rc = sort_pairs(h, k0, k1, s0, s1, used);  // ascending key order: the table order depends on how insertions interleaved, the output must not
  if (rc) return rc;
  out.n = used;
  HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * used));
  if (d.has_normals) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * used));
  if (d.has_colors) HIP_TRY(dev_alloc(h, (void**)&out.col, sizeof(P4) * used));
  dense_emit_kernel<P4><<<grid_for(used), kBlock, 0, h->stream>>>(d.dev, s1, used, (P4*)out.pts, (P4*)out.nrm, (P4*)out.col);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

inline QuantumTable quantum_table(const IcpPassArgs& a) {
  QuantumTable t;
  for (int k = 0; k < kRec; ++k) t.q[k] = a.q_hi[k];
  return t;
}

// ---- ICP launch helpers -------------------------------------------------------------------------
// threads per workgroup of the pass kernels (4 lanes per query): every form of the pass uses the same number, so that the queries are
// partitioned into the same batches -- a batch's record is one rounded f64 reduction -- and the forms agree bit for bit
#ifndef O3DS_ICP_BLOCK
#define O3DS_ICP_BLOCK 512
#endif
constexpr int kIcpBlock = O3DS_ICP_BLOCK, kIcpQ = kIcpBlock / 4;

// profiling (o3ds_profile_enable(1)): one pass launch between two events of h->ev, taken from the handle or created on first use (a
// failed creation is skipped silently: that launch goes unmeasured)
struct LaunchBracket {
  o3ds_handle h;
  hipEvent_t e1 = nullptr;
  LaunchBracket(o3ds_handle h_, bool on) : h(h_) {
    if (h->profiling != 1 || !on) return;
    if (h->ev_used + 2 > h->ev.size()) {
      hipEvent_t a0, a1;
      if (hipEventCreate(&a0) == hipSuccess && hipEventCreate(&a1) == hipSuccess) {
        h->ev.push_back(a0);
        h->ev.push_back(a1);
      }
    }
    if (h->ev_used + 2 <= h->ev.size()) {
      const hipEvent_t e0 = h->ev[h->ev_used];
      e1 = h->ev[h->ev_used + 1];
      h->ev_used += 2;
      (void)hipEventRecord(e0, h->stream);
    }
  }
  ~LaunchBracket() {
    if (e1) (void)hipEventRecord(e1, h->stream);
  }
};

// The pass kernels are instantiated per target crop and estimator (generalized ICP or not): launch(crop, gicp) is called with the two as
// compile-time constants, std::true_type / std::false_type
template <typename F>
void with_crop_and_estimator(bool crop, bool gicp, F&& launch) {
  if (gicp)
    crop ? launch(std::true_type{}, std::true_type{}) : launch(std::false_type{}, std::true_type{});
  else
    crop ? launch(std::true_type{}, std::false_type{}) : launch(std::false_type{}, std::false_type{});
}

// the launchers pick the instantiation from the session: storage precision (launch_*), target crop, estimator
template <typename P4>
void launch_accumulate_t(o3ds_handle h, const IcpPassArgs& a, int nblocks) {
  // one geometry: kIcpBlock threads = kIcpBlock / 4 queries x 4 lanes (G = 2 / 8 were swept and dropped; 512 threads against 256: a launch costs 2.7 ns per
  // workgroup beyond the first 256 -- scripts/ubench/launch_shape.hip -- and a steady pass is 9.7 us instead of 10.2)
  with_crop_and_estimator(h->session_crop, h->session_method == O3DS_ICP_GENERALIZED, [&](auto crop, auto gicp) {
    if (a.keys_mode != 0)  // target-sharded registration (o3ds_icp_nn_keys / o3ds_icp_accumulate_keys): the instantiation with the key code
      icp_accumulate_kernel<P4, decltype(crop)::value, kIcpBlock, 4, decltype(gicp)::value, true><<<nblocks, kIcpBlock, 0, h->stream>>>(a);
    else
      icp_accumulate_kernel<P4, decltype(crop)::value, kIcpBlock, 4, decltype(gicp)::value><<<nblocks, kIcpBlock, 0, h->stream>>>(a);
  });
}

void launch_accumulate(o3ds_handle h, const IcpPassArgs& a, int nblocks) {
  LaunchBracket scope(h, true);
  DISPATCH(h->session_precision, launch_accumulate_t, h, a, nblocks);
}

// fused form: byte offsets inside d_fused
constexpr size_t kFusedStateStride = 256;
constexpr size_t kFusedSlotsOff = 2 * kFusedStateStride;
constexpr size_t kFusedSlotBufBytes = (size_t)kFusedSlots * kSlotDoubles * sizeof(double);
constexpr size_t kFusedBytes = kFusedSlotsOff + 3 * kFusedSlotBufBytes;
static_assert(sizeof(IcpStateDev) <= kFusedStateStride, "state slot too small");

template <typename P4>
void launch_fused_t(o3ds_handle h, const IcpFusedArgs& fa, int nblocks) {
  with_crop_and_estimator(h->session_crop, h->session_method == O3DS_ICP_GENERALIZED, [&](auto crop, auto gicp) {
    icp_fused_kernel<P4, decltype(crop)::value, kIcpBlock, 4, decltype(gicp)::value><<<nblocks, kIcpBlock, 0, h->stream>>>(fa.state_in, fa.slots_in, fa.first, fa);
  });
}

void launch_fused(o3ds_handle h, const IcpFusedArgs& fa, int nblocks, bool bracket) {  // (a tail-only launch is not a pass: no bracket)
  LaunchBracket scope(h, bracket);
  DISPATCH(h->session_precision, launch_fused_t, h, fa, nblocks);
}

// the fused kernel serves ONE batch of kIcpQ queries per workgroup (no batch loop: icp_pass_body, kSingle); its records go to slot
// blockIdx % kFusedSlots, so the grid has no capacity to respect (the exact sums hold for 4 096 workgroup records: 2 048 at most here)
constexpr size_t kFusedMaxQueries = (size_t)4096 * 64;
static_assert(kFusedMaxQueries == O3DS_ICP_PASS_MAX_QUERIES, "the limit the header documents");
int fused_blocks(size_t count) { return (int)std::max<size_t>((count + kIcpQ - 1) / kIcpQ, 1); }

int pass_blocks(o3ds_handle h, size_t count) {
  const size_t qpb = kIcpQ;  // one batch of kIcpBlock / 4 queries per workgroup iteration
  size_t g = (count + qpb - 1) / qpb;
  if (g < 1) g = 1;
  if (g > (size_t)h->pass_rows) g = h->pass_rows;
  return (int)g;
}

int validate_icp(o3ds_handle h, const CloudRec* src, const CloudRec* tgt, const o3ds_icp_params* p) {
  if (!src || !tgt) return fail(h, O3DS_ERR_INVALID_ARG, "icp: unknown cloud id");
  if (!p) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null params");
  if (tgt->n == 0) return fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)");  // ScanToMapRegistration.cpp:60
  if (!(p->max_correspondence_distance > 0.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");  // [O3D] RegistrationICP
  if (p->method != O3DS_ICP_POINT_TO_PLANE && p->method != O3DS_ICP_GENERALIZED && p->method != O3DS_ICP_POINT_TO_POINT)
    return fail(h, O3DS_ERR_INVALID_ARG, "icp: unknown method");
  if (!tgt->nrm && p->method != O3DS_ICP_POINT_TO_POINT)
    return fail(h, O3DS_ERR_NO_NORMALS, p->method == O3DS_ICP_GENERALIZED ? "generalized ICP: target has no normals (covariances are built from normals)"
                                                                           : "TransformationEstimationPointToPlane requires target normals");
  if (p->method == O3DS_ICP_GENERALIZED && src->n > 0 && !src->nrm)
    return fail(h, O3DS_ERR_NO_NORMALS, "generalized ICP: source has no normals (covariances are built from normals)");
  if (src->precision != tgt->precision) return fail(h, O3DS_ERR_INVALID_ARG, "icp: source/target precision mismatch");
  if (p->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp: negative max_iteration");
  return O3DS_OK;
}

// per-term bounds on the sums of |record terms| -> per-term quanta of the exact record sums (split_exact): 2^53 q >= 8 B_k.  g: the
// target's grid (its box holds the matched points), r: the correspondence distance, n_src: the source's size as the host knows it
void record_quanta(const GridDev& g, double r, int method, double gicp_epsilon, size_t n_src, double q_hi[kRec]) {
  const double ex = std::max(std::fabs(g.ox), std::fabs(g.ox + g.nx * g.cell)), ey = std::max(std::fabs(g.oy), std::fabs(g.oy + g.ny * g.cell)),
               ez = std::max(std::fabs(g.oz), std::fabs(g.oz + g.nz * g.cell));
  const double P = std::max(1.0, std::sqrt(ex * ex + ey * ey + ez * ez) + r);  // a matched source point lies within r of the target's box
  const double rr = std::max(r, 1e-3);
  // headroom: 64 ranks of a sharded run may add up ("submap" mode: every rank contributes up to n correspondences).  The number of
  // queries enters as a CONSTANT (2^24, or the next power of two above a larger scan), not as n_src: for the head of a lazy chain
  // that is the exact count or the chain's upper bound, whichever the host happens to know when the registration starts, and a
  // quantum that follows it makes the dropped bits -- below 2^-85 of a term's bound, but the whole last place of J^T r once that sum
  // has converged to nothing -- a matter of timing: two-handle runs of the stream differed from one-handle runs by an ulp of a pose entry
  // in every third run (round 6, scripts/debug_wobble.py), the two-kernel form, which waits for the count, never did.  (The other half
  // of the same story is in the kernels: the queries are dealt out over the exact number the DEVICE holds, icp_kernels.hpp deal_count.)
  size_t n_for_quantum = (size_t)1 << 24;
  while (n_for_quantum < n_src) n_for_quantum <<= 1;
  const double nn = 64.0 * (double)n_for_quantum;
  double bound[kRec];
  if (method == O3DS_ICP_GENERALIZED) {
    const double gw = 4.0 * std::max(1.0, 0.5 / gicp_epsilon);  // |M^-1| <= 1 / (2 eps)
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) bound[k++] = gw * (i < 3 ? P : 1.0) * (j < 3 ? P : 1.0);  // A^T M^-1 A, A = [-[p]x | I]
    for (int i = 0; i < 6; ++i) bound[21 + i] = gw * (i < 3 ? P : 1.0) * rr;                 // A^T M^-1 d
    bound[27] = gw * rr * rr;
    bound[28] = 1.0;
    bound[29] = rr * rr;
    bound[30] = bound[31] = 1.0;
  } else {
    // the record terms are products of two per-query slots; slot magnitudes per method (icp_kernels.hpp, kTermA/B tables)
    double slot[10];
    const unsigned char *ta, *tb;
    if (method == O3DS_ICP_POINT_TO_POINT) {  // also the information-matrix pass (same slots, q q^T terms bounded by p q^T's)
      for (int i = 0; i < 6; ++i) slot[i] = P;  // p, q
      slot[6] = 0.0, slot[7] = 1.0, slot[8] = rr * rr, slot[9] = 0.0;
      ta = kTermA_p2p, tb = kTermB_p2p;
    } else {
      for (int i = 0; i < 3; ++i) slot[i] = P, slot[3 + i] = 1.0;  // J = [p x n ; n], unit normals
      slot[6] = rr, slot[7] = 1.0, slot[8] = rr * rr, slot[9] = 0.0;
      ta = kTermA, tb = kTermB;
    }
    for (int k = 0; k < kRec; ++k) bound[k] = std::max(slot[ta[k]] * slot[tb[k]], 1e-30);
    if (method == O3DS_ICP_POINT_TO_POINT)
      for (int k = 0; k < 9; ++k) bound[k] = P * P;  // information matrix: terms 0..8 are q_a q_b or q_a (<= P^2 either way)
  }
  const bool no_split = ab_getenv("O3DS_SUM_NO_SPLIT") != nullptr;  // diagnostic: plain f64 sums
  for (int k = 0; k < kRec; ++k) {
    int e = 0;
    (void)std::frexp(nn * bound[k], &e);                    // n * bound < 2^e
    q_hi[k] = no_split ? 0.0 : std::ldexp(1.0, e + 3 - 53);  // 2^53 q = 8 * 2^e
  }
}

int begin_session(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* crop, const double init[16],
                  const o3ds_icp_params* params, bool upload_state = true) {
  // (sizes as they are: a source or target whose size a kernel has yet to publish enters with its upper bound and the device word)
  CloudRec* src = find_cloud_lazy(h, source);
  CloudRec* tgt = find_cloud_lazy(h, target);
  // a persistent submap stays persistent as the TARGET (its row-paged index is what the pass kernel reads); as the SOURCE its slot array
  // -- dead and never-written slots among the live ones -- would become queries and the fitness denominator: it is folded first
  if (src && src->pm) {
    const int re = pm_exit(h, *src);
    if (re) return re;
    tgt = find_cloud_lazy(h, target);  // (source == target: the fold dropped the index)
  }
  int rc = validate_icp(h, src, tgt, params);
  if (rc) return rc;
  const double r_hint = params->max_correspondence_distance;
  if (!tgt->has_index || (tgt->nrm && !tgt->snrm) || (tgt->index_byproduct && (tgt->grid.cell < r_hint / 8.0 || tgt->grid.cell > r_hint * 0.75))) {
    rc = build_index(h, *tgt, params->max_correspondence_distance / kIndexCellDiv);
    if (rc) return rc;
  }
  rc = maybe_build_replica(h, *tgt);
  if (rc) return rc;
  // the scan loop loads candidates beyond the end of a range without looking at them (scan_strided): behind the last element of either
  // array there must be memory of the same allocation.  Refused before anything of the handle is touched
  if (tgt->spts_slack < kScanSlackBytes || (tgt->rpts && tgt->rpts_slack < kScanSlackBytes))
    return fail(h, O3DS_ERR_INVALID_ARG, "icp: the target's index arrays end without the kScanSlackBytes the search's scan loop may load beyond a range");
  const size_t cap = (std::max<size_t>(src->n + src->n / 4, 1 << 16) + 7) & ~(size_t)7;
  bool fresh_cache = false;
  rc = handle_scratch(h, &h->d_nn_cache, &h->nn_cache_cap, src->n, cap, cap * sizeof(int), &fresh_cache);
  if (rc) return rc;
  if (!h->d_nn_cache) return fail(h, O3DS_ERR_OOM, "icp: match cache allocation failed");
  if (fresh_cache) {  // the candidate sets are sized with it (the synchronisation above covers them)
    if (h->d_set_pos) (void)hipFree(h->d_set_pos);
    h->d_set_pos = nullptr;
    h->d_set_ref = nullptr;
    if (hipMalloc((void**)&h->d_set_pos, cap * (kSetCap * sizeof(int) + 4 * sizeof(double))) != hipSuccess) {
      (void)hipFree(h->d_nn_cache);
      h->d_nn_cache = nullptr;
      h->nn_cache_cap = 0;
      return fail(h, O3DS_ERR_OOM, "icp: candidate-set allocation failed");
    }
    h->d_set_ref = (char*)h->d_set_pos + cap * kSetCap * sizeof(int);  // (cap is a multiple of 4: 32-byte aligned)
  }
  IcpStateDev st{};
  memcpy(st.T, init, sizeof(double) * 16);
  *h->h_state = st;
  if (upload_state) HIP_TRY(hipMemcpyAsync(h->d_state, h->h_state, sizeof(IcpStateDev), hipMemcpyHostToDevice, h->stream));
  IcpPassArgs a{};
  a.src = src->pts;
  a.src_f64 = src->precision == O3DS_PRECISION_F64 ? 1 : 0;
  a.first = 0;
  a.count = src->n;
  a.tpts = tgt->spts;
  a.tnrm = tgt->snrm;
  a.grid = tgt->grid;
  {  // A/B switch: O3DS_NN_REPLICA=0 searches the rows of cell_start although the index has a replica (read at every registration)
    const char* e = ab_getenv("O3DS_NN_REPLICA");
    if (e && atoi(e) == 0) a.grid.rpts = nullptr, a.grid.rstart = a.grid.rpos = nullptr;
  }
  a.crop = to_dev(crop);
  const double r = params->max_correspondence_distance;
  a.r2max = r * r;
  a.method = params->method;
  record_quanta(tgt->grid, r, params->method, h->gicp_epsilon, src->n, a.q_hi);
  a.kmax = std::max(1, (int)std::ceil(r / tgt->grid.cell));  // a neighbour within r is at most this many cells away
  a.nn_cache = h->d_nn_cache;
  a.set_pos = h->fused && h->sets ? h->d_set_pos : nullptr;
  a.set_ref = h->d_set_ref;
  a.set_gain = h->set_gain;
  a.set_min = h->set_min;
  a.set_cap = h->set_cap;
  a.n_tgt = (int)(tgt->index_positions ? tgt->index_positions : tgt->n);
  a.snrm = src->nrm;
  a.count_dev = src->lazy_slot >= 0 ? cnt_word(h, src->lazy_slot) : nullptr;
  a.gicp_k = 1.0 - h->gicp_epsilon;
  a.state = h->d_state;
  a.partials = h->d_partials;
  a.debug = ab_getenv("O3DS_DEBUG_ACC") ? atoi(ab_getenv("O3DS_DEBUG_ACC")) : 0;
  h->pass = a;
  h->params = *params;
  h->session = true;
  h->session_n_src = src->n;
  h->session_launches = 0;
  h->session_state = nullptr;
  h->session_precision = src->precision;
  h->session_crop = crop && (crop->kind != O3DS_CROP_NONE || crop->invert);
  h->session_method = params->method;
  return O3DS_OK;
}

void state_result(const IcpStateDev& s, o3ds_icp_result* out) {
  memcpy(out->transformation, s.T, sizeof(double) * 16);
  out->fitness = s.fitness;
  out->inlier_rmse = s.rmse;
  out->iterations = s.iterations;
  out->converged = s.converged;
  out->n_corr = s.n_corr;
}

void copy_result(o3ds_handle h, o3ds_icp_result* out) {
  if (out) state_result(*h->h_state, out);
}

int read_state(o3ds_handle h, o3ds_icp_result* out, const IcpStateDev* d_from = nullptr) {
  HIP_TRY(hipMemcpyAsync(h->h_state, d_from ? d_from : h->d_state, sizeof(IcpStateDev), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  copy_result(h, out);
  return O3DS_OK;
}

// the session's part of a fused launch's arguments (init, written by begin_session, is read by the first launch only); the caller adds
// its own: range, slots, first, pass_index, states, seq, trace, stats
IcpFusedArgs fused_args(o3ds_handle h, size_t n_src_total) {
  IcpFusedArgs fa{};
  fa.pass = h->pass;
  fa.n_src_total = (unsigned long long)n_src_total;
  fa.max_iter = h->params.max_iteration;
  fa.rel_fitness = h->params.relative_fitness;
  fa.rel_rmse = h->params.relative_rmse;
  fa.init = *h->h_state;
  return fa;
}

// launch j of a session writes its state here: the two slots at the head of d_fused alternate, launch j + 1 reads what launch j wrote
IcpStateDev* fused_state_out(o3ds_handle h, int j) { return (IcpStateDev*)(h->d_fused + (size_t)(j & 1) * kFusedStateStride); }

// one pass over a's range and, where d_record is given, the reduction of its workgroup rows into that record
int accumulate_pass(o3ds_handle h, const IcpPassArgs& a, double* d_record) {
  const int nb = pass_blocks(h, a.count);
  launch_accumulate(h, a, nb);
  if (d_record) icp_reduce_kernel<<<1, kUpdBlock, 0, h->stream>>>(h->d_partials, nb, h->d_state, d_record, quantum_table(a));
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

// behind o3ds_icp_accumulate, o3ds_icp_nn_keys and o3ds_icp_accumulate_keys, which check their arguments: the session's pass over
// source points first .. first + count.  keys_mode 0: search and accumulate, 1: search -> keys (no record), 2: keys -> accumulate
int stepwise_pass(o3ds_handle h, size_t first, size_t count, int keys_mode, int rank, unsigned long long* d_keys, double* d_record) {
  IcpPassArgs a = h->pass;
  a.first = first;
  a.count = count;
  a.keys_mode = keys_mode;
  a.keys_rank = rank;
  a.keys = d_keys;
  return accumulate_pass(h, a, d_record);
}

// the host-array forms: uploads both clouds, runs fn(source, target) on their ids and frees them; the error text of what failed first
// survives the frees
template <typename F>
int with_uploaded_clouds(o3ds_handle h, const double* src_xyz, const double* src_normals, size_t n_src, const double* tgt_xyz,
                         const double* tgt_normals, size_t n_tgt, F&& fn) {
  o3ds_cloud s = 0, t = 0;
  int rc = o3ds_cloud_upload(h, src_xyz, src_normals, n_src, &s);
  if (rc) return rc;
  rc = o3ds_cloud_upload(h, tgt_xyz, tgt_normals, n_tgt, &t);
  if (!rc) rc = fn(s, t);
  const std::string keep = h->err;
  (void)o3ds_cloud_free(h, s);
  if (t) (void)o3ds_cloud_free(h, t);
  if (rc) h->err = keep;
  return rc;
}

// the host loop of the two-launch forms: queue_pass() queues one correspondence pass and its tail.  The device loops terminate
// themselves (done flags); the host only looks between chunks of queued passes -- after 12 passes, then every 8 -- with look(&done),
// which reads the state(s) back and answers whether every loop has terminated
template <typename L, typename F>
int two_launch_loop(o3ds_handle h, int total_passes, L&& look, F&& queue_pass) {
  int launched = 0;
  while (launched < total_passes) {
    const int chunk = std::min(total_passes - launched, launched == 0 ? 12 : 8);
    for (int k = 0; k < chunk; ++k) queue_pass();
    launched += chunk;
    HIP_TRY(hipGetLastError());
    bool done = false;
    const int rc = look(&done);
    if (rc || done) return rc;
  }
  return O3DS_OK;
}

// the look of the forms with one state, the handle's: into h->h_state and, as a result, into out
auto look_at_session_state(o3ds_handle h, o3ds_icp_result* out) {
  return [h, out](bool* done) {
    const int rc = read_state(h, out);
    *done = h->h_state->done;
    return rc;
  };
}

// one pair through o3ds_icp_register_dev from inside another entry point (a list of one is the existing call, bit for bit): a function
// armed with o3ds_icp_overlap_next is put aside for the call and stays armed
int register_one_pair(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                      const o3ds_icp_params* params, o3ds_icp_result* out) {
  const o3ds_overlap_fn fn = h->overlap_fn;
  void* const arg = h->overlap_arg;
  h->overlap_fn = nullptr;
  h->overlap_arg = nullptr;
  const int rc = o3ds_icp_register_dev(h, source, target, target_crop, init, params, out);
  h->overlap_fn = fn;
  h->overlap_arg = arg;
  return rc;
}

}  // namespace

// =================================================================================================

namespace {
int gicp_knn_normals(o3ds_handle h, CloudRec& c);  // defined after normals_t
}

extern "C" {

const char* o3ds_version(void) {
#ifdef O3DS_AB_SWITCHES
  return "o3ds_backend 0.2 (gfx950, hip, f32/f64 storage, f64 accumulate; A/B switches compiled in)";
#else
  return "o3ds_backend 0.2 (gfx950, hip, f32/f64 storage, f64 accumulate)";
#endif
}

const char* o3ds_last_error(o3ds_handle h) { return h ? h->err.c_str() : g_thread_error.c_str(); }

int o3ds_create(int device_id, o3ds_handle* out) {
  if (!out) return fail(nullptr, O3DS_ERR_INVALID_ARG, "o3ds_create: null out");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, O3DS_ERR_HIP, std::string("o3ds_create: no HIP device (") + hipGetErrorString(e) + ")");
  if (device_id < 0 || device_id >= count) return fail(nullptr, O3DS_ERR_INVALID_ARG, "o3ds_create: bad device id");
  o3ds_handle h = new o3ds_context();
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      (h->own_stream = h->stream, false) || hipMalloc(&h->d_partials, sizeof(double) * kRec * kMaxPassBlocks) != hipSuccess ||
      hipMalloc(&h->d_state, sizeof(IcpStateDev)) != hipSuccess ||
      hipHostMalloc((void**)&h->h_state, sizeof(IcpStateDev), hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&h->h_state_dev, h->h_state, 0) != hipSuccess ||
      hipHostMalloc((void**)&h->h_pin, kPinBytes, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&h->h_pin_dev, h->h_pin, 0) != hipSuccess) {
    o3ds_destroy(h);  // frees whatever part of the context exists (every member is null-checked there)
    return fail(nullptr, O3DS_ERR_HIP, "o3ds_create: device initialisation failed");
  }
  {
    if (hipMalloc((void**)&h->d_fused, kFusedBytes) != hipSuccess || hipMemset(h->d_fused, 0, kFusedBytes) != hipSuccess) {
      o3ds_destroy(h);
      return fail(nullptr, O3DS_ERR_OOM, "o3ds_create: scratch allocation failed");
    }
    if (const char* e = ab_getenv("O3DS_ICP_SETS")) h->sets = atoi(e) != 0;
    if (const char* e = ab_getenv("O3DS_SET_GAIN")) h->set_gain = (float)atof(e);
    if (const char* e = ab_getenv("O3DS_SET_MIN")) h->set_min = (float)atof(e);
    if (const char* e = ab_getenv("O3DS_SET_CAP")) h->set_cap = (float)atof(e);
    if (const char* e = ab_getenv("O3DS_ICP_MODE")) {
      h->fused = std::string(e) != "launch";
    }
  }
  {
    static_assert(sizeof(o3ds_context::PinRec) == 64, "one pinned record per cache line");
    if (hipHostMalloc((void**)&h->h_rec, sizeof(o3ds_context::PinRec) * kPinRecs, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->h_rec_dev, h->h_rec, 0) != hipSuccess ||
        hipMalloc((void**)&h->d_cnt, sizeof(int) * 16 * kPinRecs) != hipSuccess || hipMemset(h->d_cnt, 0, sizeof(int) * 16 * kPinRecs) != hipSuccess ||
        hipMalloc((void**)&h->d_ticket, 64) != hipSuccess || hipMemset(h->d_ticket, 0, 64) != hipSuccess ||
        hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess) {
      o3ds_destroy(h);
      return fail(nullptr, O3DS_ERR_OOM, "o3ds_create: record allocation failed");
    }
    memset(h->h_rec, 0, sizeof(o3ds_context::PinRec) * kPinRecs);
  }
  if (const char* e = ab_getenv("O3DS_DEBUG_UPDATE")) h->debug_update = atoi(e);
  if (const char* e = ab_getenv("O3DS_PASS_ROWS")) h->pass_rows = std::min(std::max(atoi(e), 1), kMaxPassBlocks);
  *out = h;
  return O3DS_OK;
}

int o3ds_destroy(o3ds_handle h) {
  CHECK_HANDLE(h);
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamSynchronize(h->own_stream);
  if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  for (auto& kv : h->clouds) free_cloud(h, kv.second);
  for (auto& kv : h->dense_maps) dense_release(h, kv.second);
  for (auto& kv : h->voxel_gaussians) ndt_release(h, kv.second);
  for (auto& b : h->arena_blocks) dev_free(h, b.first);
  (void)hipStreamSynchronize(h->stream);
  dev_release_all(h);
  for (auto& b : h->ingest_bufs) {
    if (b.pts) (void)hipFree(b.pts);
    if (b.box) (void)hipFree(b.box);
    if (b.freed) (void)hipEventDestroy(b.freed);
  }
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->d_raw) (void)hipFree(h->d_raw);
  if (h->d_tiles) (void)hipFree(h->d_tiles);
  if (h->d_ticket) (void)hipFree(h->d_ticket);
  if (h->d_cnt) (void)hipFree(h->d_cnt);
  if (h->h_rec) (void)hipHostFree(h->h_rec);
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  (void)o3ds_comm_destroy(h);
  if (h->d_shard_sums) (void)hipFree(h->d_shard_sums);
  if (h->d_shard_keys) (void)hipFree(h->d_shard_keys);
  if (h->d_fused) (void)hipFree(h->d_fused);
  if (h->d_nn_cache) (void)hipFree(h->d_nn_cache);
  if (h->d_set_pos) (void)hipFree(h->d_set_pos);
  if (h->d_cells) (void)hipFree(h->d_cells);
  if (h->d_voxtab) (void)hipFree(h->d_voxtab);
  if (h->d_draw) (void)hipFree(h->d_draw);
  if (h->d_partials) (void)hipFree(h->d_partials);
  if (h->d_state) (void)hipFree(h->d_state);
  if (h->h_state) (void)hipHostFree(h->h_state);
  if (h->h_pin) (void)hipHostFree(h->h_pin);
  for (int k = 0; k < 2; ++k) {
    if (h->h_stage[k]) (void)hipHostFree(h->h_stage[k]);
    if (h->stage_ev[k]) (void)hipEventDestroy(h->stage_ev[k]);
  }
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  for (auto& v : h->span_ev)
    for (hipEvent_t e : v) (void)hipEventDestroy(e);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return O3DS_OK;
}

int o3ds_set_precision(o3ds_handle h, int precision) {
  CHECK_HANDLE(h);
  if (precision != O3DS_PRECISION_F32 && precision != O3DS_PRECISION_F64) return fail(h, O3DS_ERR_INVALID_ARG, "bad precision");
  h->precision = precision;
  return O3DS_OK;
}

int o3ds_synchronize(o3ds_handle h) {
  CHECK_HANDLE(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return O3DS_OK;
}

void* o3ds_stream(o3ds_handle h) { return h ? (void*)h->stream : nullptr; }

int o3ds_set_stream(o3ds_handle h, void* hip_stream) {
  CHECK_HANDLE(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return O3DS_OK;
}

int o3ds_profile_enable(o3ds_handle h, int on) {
  CHECK_HANDLE(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->profiling = on == 2 ? 2 : (on != 0);
  h->ev_used = 0;
  for (auto& u : h->span_used) u = 0;
  return O3DS_OK;
}

int o3ds_profile_span(o3ds_handle h, int tag, int end) {
  CHECK_HANDLE(h);
  if (tag < 0 || tag >= 8) return fail(h, O3DS_ERR_INVALID_ARG, "profile_span: caller tags are 0..7");
  if ((int)(h->span_used[tag] & 1) != (end ? 1 : 0)) return fail(h, O3DS_ERR_INVALID_ARG, "profile_span: begin / end out of order");
  span_mark(h, tag);
  return O3DS_OK;
}

int o3ds_profile_span_read(o3ds_handle h, int tag, uint64_t* n_spans, double* total_ms) {
  CHECK_HANDLE(h);
  if (tag < 0 || tag >= o3ds_context::kSpanTags) return fail(h, O3DS_ERR_INVALID_ARG, "profile_span_read: bad tag");
  HIP_TRY(hipStreamSynchronize(h->stream));
  double tot = 0.0;
  const size_t used = h->span_used[tag] & ~(size_t)1;
  for (size_t i = 0; i + 1 < used; i += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->span_ev[tag][i], h->span_ev[tag][i + 1]));
    tot += (double)ms;
  }
  if (n_spans) *n_spans = used / 2;
  if (total_ms) *total_ms = tot;
  h->span_used[tag] = 0;
  return O3DS_OK;
}

int o3ds_profile_read(o3ds_handle h, uint64_t* n_launches, double* total_ms) {
  CHECK_HANDLE(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  double tot = 0.0;
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    tot += (double)ms;
  }
  if (n_launches) *n_launches = h->ev_used / 2;
  if (total_ms) *total_ms = tot;
  h->ev_used = 0;
  return O3DS_OK;
}

// ---- clouds ------------------------------------------------------------------------------------
int o3ds_cloud_upload(o3ds_handle h, const double* xyz, const double* normals, size_t n, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!out || (n > 0 && !xyz)) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_upload: null argument");
  if (n > 0x7fffffffull) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_upload: more than 2^31-1 points");
  HIP_TRY(hipSetDevice(h->device));
  return new_cloud(h, out, [&](CloudRec& c) { return DISPATCH(h->precision, upload_t, h, xyz, normals, n, c); });
}

int o3ds_cloud_upload_f32(o3ds_handle h, const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y, size_t off_z,
                          o3ds_cloud* out) {
  CHECK_HANDLE(h);
  if (!out || (n > 0 && !data)) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_upload_f32: null argument");
  if (n > 0x7fffffffull) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_upload_f32: more than 2^31-1 points");
  if (point_step < 12 || off_x + 4 > point_step || off_y + 4 > point_step || off_z + 4 > point_step)
    return fail(h, O3DS_ERR_INVALID_ARG, "cloud_upload_f32: x/y/z fields do not fit the point step");
  HIP_TRY(hipSetDevice(h->device));
  return new_cloud(h, out, [&](CloudRec& c) -> int {
    c.n = n;
    c.precision = h->precision;
    if (n > 0) {
      // The whole ingest runs on the handle's COPY stream -- DMA of the records, unpack, box -- and the call returns with it queued: the
      // scan crosses PCIe while the frame before it is still being registered and merged on the handle's stream, whose first use of the
      // cloud waits for an event (cloud_ready), not the host.  The points live in an ingest buffer (free_points).
      const size_t psz = p4_size(h->precision), bytes = n * point_step;
      // a buffer nothing on the handle's stream still reads (its "freed" event has passed): the ingest must not queue behind the frame
      // that used the buffer last -- that frame is exactly what it is meant to overlap with.  Up to four buffers before one is waited for.
      int bi = -1, idle = -1;
      for (size_t k = 0; k < h->ingest_bufs.size(); ++k) {
        o3ds_context::IngestBuf& cand = h->ingest_bufs[k];
        if (cand.in_use) continue;
        if (idle < 0) idle = (int)k;
        if (cand.pts_bytes >= psz * n && (!cand.freed || hipEventQuery(cand.freed) == hipSuccess)) {
          bi = (int)k;
          break;
        }
      }
      (void)hipGetLastError();  // (hipErrorNotReady of a pending event is not an error)
      if (bi < 0) {
        if (h->ingest_bufs.size() < 4 || idle < 0) {
          h->ingest_bufs.emplace_back();
          bi = (int)h->ingest_bufs.size() - 1;
        } else {
          bi = idle;  // too small (grown below) or still being read (waited for on the copy stream)
        }
      }
      o3ds_context::IngestBuf& b = h->ingest_bufs[(size_t)bi];
      if (b.pts_bytes < psz * n) {
        if (b.pts) {
          if (b.freed) HIP_TRY(hipEventSynchronize(b.freed));
          HIP_TRY(hipStreamSynchronize(h->copy_stream));
          (void)hipFree(b.pts);
          b.pts = nullptr;
          b.pts_bytes = 0;
        }
        const size_t want = psz * (n + n / 8);
        if (hipMalloc(&b.pts, want) != hipSuccess) return fail(h, O3DS_ERR_OOM, "cloud_upload_f32: ingest buffer allocation failed");
        b.pts_bytes = want;
      }
      if (!b.box) {
        if (hipMalloc((void**)&b.box, 64) != hipSuccess) return fail(h, O3DS_ERR_OOM, "cloud_upload_f32: box record allocation failed");
        unsigned long long arm[8] = {0};
        for (int a = 0; a < 6; ++a) arm[a] = order_bits(a < 3 ? 1e300 : -1e300);
        HIP_TRY(hipMemcpy(b.box, arm, sizeof(arm), hipMemcpyHostToDevice));
      }
      if (h->raw_cap < bytes) {
        HIP_TRY(hipStreamSynchronize(h->copy_stream));
        if (h->d_raw) (void)hipFree(h->d_raw);
        h->d_raw = nullptr;
        h->raw_cap = 0;
        if (hipMalloc((void**)&h->d_raw, bytes + bytes / 8) != hipSuccess) return fail(h, O3DS_ERR_OOM, "cloud_upload_f32: staging allocation failed");
        h->raw_cap = bytes + bytes / 8;
      }
      if (b.freed) HIP_TRY(hipStreamWaitEvent(h->copy_stream, b.freed, 0));  // whatever still read the buffer's last cloud on the handle's stream
      // the records: straight DMA from memory the runtime knows as pinned (o3ds_pinned_alloc, hipHostRegister: read asynchronously, see the
      // header), through the handle's pinned ring otherwise (the caller's buffer is consumed when this returns)
      hipPointerAttribute_t attr{};
      const bool pinned = hipPointerGetAttributes(&attr, data) == hipSuccess && attr.type == hipMemoryTypeHost;
      (void)hipGetLastError();  // (a pageable pointer makes the query fail: not an error of ours)
      if (pinned) {
        HIP_TRY(hipMemcpyAsync(h->d_raw, data, bytes, hipMemcpyHostToDevice, h->copy_stream));
      } else {
        const int rcc = h2d_copy(h, h->d_raw, data, bytes, h->copy_stream);
        if (rcc) return rcc;
      }
      b.in_use = true;
      c.pts = b.pts;
      c.ingest_buf = bi;
      // the box of the points inside the volume the handle last cropped with rides on the unpack (pack_strided_f32_box_kernel)
      const int box_slot = h->pre_crop_valid ? take_rec(h) : -1;  // (-1: every record is held by a map -- the box is reduced when it is asked for)
      if (box_slot >= 0) {
        c.pre_slot = box_slot;
        c.pre_seq = ++h->rec_seq;
        c.pre_crop = h->pre_crop;
        o3ds_context::PinRec* rec = h->h_rec_dev + c.pre_slot;
        WITH_P4(h->precision, pack_strided_f32_box_kernel<P4><<<grid_for(n, 1024), kBlock, 0, h->copy_stream>>>(h->d_raw, n, point_step, off_x, off_y, off_z,
                                                                                                                 (P4*)c.pts, c.pre_crop, b.box));
        box_publish_kernel<<<1, 64, 0, h->copy_stream>>>(b.box, rec->box, &rec->seq, c.pre_seq);
      } else {
        WITH_P4(h->precision, pack_strided_f32_kernel<P4><<<grid_for(n), kBlock, 0, h->copy_stream>>>(h->d_raw, n, point_step, off_x, off_y, off_z, (P4*)c.pts));
      }
      HIP_TRY(hipGetLastError());
      c.ingest_ev = take_event(h);
      if (!c.ingest_ev) return fail(h, O3DS_ERR_HIP, "cloud_upload_f32: event creation failed");
      HIP_TRY(hipEventRecord(c.ingest_ev, h->copy_stream));
    }
    return O3DS_OK;
  });
}

int o3ds_pinned_alloc(o3ds_handle h, size_t bytes, void** out) {
  CHECK_HANDLE(h);
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "pinned_alloc: null out");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return O3DS_OK;
}
int o3ds_pinned_free(o3ds_handle h, void* p) {
  CHECK_HANDLE(h);
  if (h->copy_stream) HIP_TRY(hipStreamSynchronize(h->copy_stream));  // an ingest may still be reading it
  if (p) HIP_TRY(hipHostFree(p));
  return O3DS_OK;
}
int o3ds_cloud_wait_ingest(o3ds_handle h, o3ds_cloud id) {
  CHECK_HANDLE(h);
  auto it = h->clouds.find(id);
  if (it == h->clouds.end()) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_wait_ingest: unknown cloud id");
  if (it->second.ingest_ev) HIP_TRY(hipEventSynchronize(it->second.ingest_ev));
  return O3DS_OK;
}

int o3ds_cloud_free(o3ds_handle h, o3ds_cloud id) {
  CHECK_HANDLE(h);
  auto it = h->clouds.find(id);
  if (it == h->clouds.end()) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_free: unknown cloud id");
  // no host synchronisation: the buffers go back to the handle's allocator behind whatever still reads them on this stream
  // (o3ds_set_stream synchronises the stream it leaves)
  free_cloud(h, it->second);
  h->clouds.erase(it);
  return O3DS_OK;
}

int o3ds_cloud_size(o3ds_handle h, o3ds_cloud id, size_t* n, int* has_normals) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud_lazy(h, id);  // (whether a cloud has normals is known without waiting for its size)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_size: unknown cloud id");
  if (n && c->pm) {  // a submap in its persistent form stays in it: its live points = slots in use - dead slots, from the device's counters
    int counters[kPmCounters];
    ArenaScope arena_scope(h);
    const int rb = read_back(h, {{counters, c->pm->dev.counters, sizeof(counters)}});
    if (rb) return rb;
    *n = (size_t)(counters[kPmN] - counters[kPmDeadCnt]);
    if (has_normals) *has_normals = c->nrm != nullptr;
    return O3DS_OK;
  }
  if (n) {
    const int rr = resolve_count(h, *c, true);
    if (rr) return rr;
  }
  if (n) *n = c->n;
  if (has_normals) *has_normals = c->nrm != nullptr;
  return O3DS_OK;
}

int o3ds_cloud_index_replica(o3ds_handle h, o3ds_cloud id, size_t* elements) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud_lazy(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_index_replica: unknown cloud id");
  if (!elements) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_index_replica: null output");
  *elements = c->rpts ? 9 * c->n : 0;
  return O3DS_OK;
}

int o3ds_cloud_is_persistent_map(o3ds_handle h, o3ds_cloud id, int* persistent) {
  CHECK_HANDLE(h);
  auto it = h->clouds.find(id);  // (not even find_cloud_lazy: nothing is waited for, nothing changes)
  if (it == h->clouds.end()) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_is_persistent_map: unknown cloud id");
  if (!persistent) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_is_persistent_map: null output");
  *persistent = it->second.pm != nullptr;
  return O3DS_OK;
}

int o3ds_cloud_size_bound(o3ds_handle h, o3ds_cloud id, size_t* lower, size_t* upper) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud_lazy(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_size_bound: unknown cloud id");
  if (c->pm) {
    (void)pm_poll(h, c->pm, false);
    if (lower) *lower = c->pm->live_lower;
    if (upper) *upper = c->pm->n_upper;
    return O3DS_OK;
  }
  if (lower) *lower = c->lazy_slot >= 0 ? std::min(c->n_lower, c->n) : c->n;
  if (upper) *upper = c->n;
  return O3DS_OK;
}

int o3ds_cloud_download(o3ds_handle h, o3ds_cloud id, double* xyz, double* normals, size_t capacity) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download: unknown cloud id");
  if (capacity < c->n) return fail(h, O3DS_ERR_CAPACITY, "cloud_download: capacity < cloud size");
  return DISPATCH(c->precision, download_t, h, *c, xyz, normals);
}

int o3ds_cloud_download_f32(o3ds_handle h, o3ds_cloud id, void* data, size_t capacity, size_t point_step, size_t off_x, size_t off_y,
                            size_t off_z, size_t off_normal, size_t off_rgb, int rgb_rounding) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: unknown cloud id");
  if (capacity < c->n) return fail(h, O3DS_ERR_CAPACITY, "cloud_download_f32: capacity < cloud size");
  if (c->n > 0 && !data) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: null buffer");
  if (point_step < 12 || off_x + 4 > point_step || off_y + 4 > point_step || off_z + 4 > point_step)
    return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: x/y/z fields do not fit the point step");
  if (off_normal != O3DS_NO_FIELD) {
    if (off_normal + 12 > point_step) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: normal fields do not fit the point step");
    if (!c->nrm) return fail(h, O3DS_ERR_NO_NORMALS, "cloud_download_f32: normals requested but the cloud has none");
  }
  if (off_rgb != O3DS_NO_FIELD) {
    if (off_rgb + 4 > point_step) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: rgb field does not fit the point step");
    if (!c->col) return fail(h, O3DS_ERR_EMPTY, "cloud_download_f32: rgb requested but the cloud has no colours");
    if (rgb_rounding != 0 && rgb_rounding != 1) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_f32: rgb_rounding must be 0 or 1");
  }
  if (c->n == 0) return O3DS_OK;
  HIP_TRY(hipSetDevice(h->device));
  unsigned char* d_raw = nullptr;
  const size_t bytes = c->n * point_step;
  TMP_ALLOC(d_raw, bytes);
  HIP_TRY(hipMemsetAsync(d_raw, 0, bytes, h->stream));  // padding and the fields this path does not carry
  const size_t on = off_normal == O3DS_NO_FIELD ? kNoField : off_normal;
  const size_t oc = off_rgb == O3DS_NO_FIELD ? kNoField : off_rgb;
  WITH_P4(c->precision, unpack_strided_f32_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>((const P4*)c->pts, (const P4*)c->nrm, (const P4*)c->col, c->n,
                                                                                                 point_step, off_x, off_y, off_z, on, oc, rgb_rounding, d_raw));
  HIP_TRY(hipGetLastError());
  return d2h_copy(h, data, d_raw, bytes);
}

int o3ds_cloud_set_colors_from_records(o3ds_handle h, o3ds_cloud id, const void* data, size_t point_step, size_t off_field, int kind) {
  CHECK_HANDLE(h);
  drop_cgrad(h, id);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_set_colors_from_records: unknown cloud id");
  if (kind != O3DS_COLOR_FIELD_RGB && kind != O3DS_COLOR_FIELD_INTENSITY)
    return fail(h, O3DS_ERR_INVALID_ARG, "cloud_set_colors_from_records: unknown field kind");
  if (off_field + 4 > point_step) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_set_colors_from_records: the field does not fit the point step");
  if (c->n > 0 && !data) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_set_colors_from_records: null buffer");
  HIP_TRY(hipSetDevice(h->device));
  if (c->col) dev_free(h, c->col);
  c->col = nullptr;
  if (c->n == 0) return O3DS_OK;
  unsigned char* d_raw = nullptr;
  TMP_ALLOC(d_raw, c->n * point_step);
  {
    const int rcc = h2d_copy(h, d_raw, data, c->n * point_step);
    if (rcc) return rcc;
  }
  HIP_TRY(dev_alloc(h, (void**)&c->col, p4_size(c->precision) * c->n));
  WITH_P4(c->precision, colors_from_records_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>(d_raw, c->n, point_step, off_field, kind, (P4*)c->col));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));  // `data` may be reused by the caller
  return O3DS_OK;
}

int o3ds_cloud_set_colors(o3ds_handle h, o3ds_cloud id, const double* rgb) {
  CHECK_HANDLE(h);
  drop_cgrad(h, id);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_set_colors: unknown cloud id");
  HIP_TRY(hipSetDevice(h->device));
  if (c->col) dev_free(h, c->col);
  c->col = nullptr;
  if (!rgb || c->n == 0) return O3DS_OK;  // colors_.clear()
  double* stage = nullptr;
  TMP_ALLOC(stage, sizeof(double) * 3 * c->n);
  {
    const int rcc = h2d_copy(h, stage, rgb, sizeof(double) * 3 * c->n);
    if (rcc) return rcc;
  }
  HIP_TRY(dev_alloc(h, (void**)&c->col, p4_size(c->precision) * c->n));
  WITH_P4(c->precision, pack_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>(stage, c->n, (P4*)c->col));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));  // rgb may be released by the caller
  return O3DS_OK;
}

int o3ds_cloud_has_colors(o3ds_handle h, o3ds_cloud id, int* has_colors) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud_lazy(h, id);  // (known without the cloud's size, and without folding a persistent map)
  if (!c || !has_colors) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_has_colors: bad argument");
  *has_colors = c->col != nullptr;
  return O3DS_OK;
}

int o3ds_cloud_get_colors(o3ds_handle h, o3ds_cloud id, double* rgb, size_t capacity) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c || !rgb) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_get_colors: bad argument");
  if (!c->col) return fail(h, O3DS_ERR_EMPTY, "cloud_get_colors: the cloud has no colours");
  if (capacity < c->n) return fail(h, O3DS_ERR_CAPACITY, "cloud_get_colors: capacity < cloud size");
  double* stage = nullptr;
  TMP_ALLOC(stage, sizeof(double) * 3 * c->n);
  WITH_P4(c->precision, unpack_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>((const P4*)c->col, c->n, stage));
  HIP_TRY(hipGetLastError());
  return d2h_copy(h, rgb, stage, sizeof(double) * 3 * c->n);
}

int o3ds_cloud_build_index(o3ds_handle h, o3ds_cloud id, double max_corr_hint, double cell_size) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "build_index: unknown cloud id");
  double cell = cell_size > 0.0 ? cell_size : max_corr_hint / kIndexCellDiv;
  if (!(cell > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "build_index: need cell_size > 0 or max_corr_hint > 0");
  int rc = build_index(h, *c, cell);
  return rc;
}

// ---- ICP ---------------------------------------------------------------------------------------
int o3ds_icp_begin(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                   const o3ds_icp_params* params) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init) return fail(h, O3DS_ERR_INVALID_ARG, "icp_begin: null init");
  (void)find_cloud(h, source);  // the step-wise forms address source RANGES: they take the exact size
  return begin_session(h, source, target, target_crop, init, params);
}

int o3ds_icp_accumulate(o3ds_handle h, size_t first, size_t count, double* d_record) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate: no session (call o3ds_icp_begin)");
  if (!d_record) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate: null record");
  if (first + count > h->session_n_src) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate: range outside source");
  return stepwise_pass(h, first, count, 0, 0, nullptr, d_record);
}

// Partitioning B (one map split over the GPUs of a node): search pass -> keys; the caller MIN-all-reduces them; accumulate pass
int o3ds_icp_nn_keys(o3ds_handle h, size_t first, size_t count, int rank, unsigned long long* d_keys) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_nn_keys: no session (call o3ds_icp_begin)");
  if (!d_keys) return fail(h, O3DS_ERR_INVALID_ARG, "icp_nn_keys: null keys");
  if (rank < 0 || rank > 15) return fail(h, O3DS_ERR_INVALID_ARG, "icp_nn_keys: rank must be 0..15 (4 bits of the key)");
  if (first + count > h->session_n_src) return fail(h, O3DS_ERR_INVALID_ARG, "icp_nn_keys: range outside source");
  if ((size_t)h->pass.n_tgt > ((size_t)1 << 28)) return fail(h, O3DS_ERR_INVALID_ARG, "icp_nn_keys: more than 2^28 target points per shard");
  return stepwise_pass(h, first, count, 1, rank, d_keys, nullptr);
}

int o3ds_icp_accumulate_keys(o3ds_handle h, size_t first, size_t count, int rank, const unsigned long long* d_keys, double* d_record) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate_keys: no session (call o3ds_icp_begin)");
  if (!d_keys || !d_record) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate_keys: null argument");
  if (rank < 0 || rank > 15) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate_keys: rank must be 0..15");
  if (first + count > h->session_n_src) return fail(h, O3DS_ERR_INVALID_ARG, "icp_accumulate_keys: range outside source");
  return stepwise_pass(h, first, count, 2, rank, const_cast<unsigned long long*>(d_keys), d_record);
}

int o3ds_icp_update(o3ds_handle h, const double* d_record, uint64_t n_src_total) {
  CHECK_HANDLE(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_update: no session");
  if (!d_record) return fail(h, O3DS_ERR_INVALID_ARG, "icp_update: null record");
  icp_update_kernel<<<1, 128, 0, h->stream>>>(d_record, h->d_state, (unsigned long long)n_src_total, h->params.max_iteration,
                                             h->params.relative_fitness, h->params.relative_rmse, h->session_method, h->pass.src, h->pass.src_f64);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

int o3ds_icp_pass(o3ds_handle h, size_t first, size_t count, size_t n_src_total, const double* d_sums_in, double* d_sums_out,
                  double* d_sums_next) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass: no session (call o3ds_icp_begin)");
  if (!d_sums_out || !d_sums_next || (h->session_launches > 0 && !d_sums_in)) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass: null sums buffer");
  if (first + count > h->session_n_src) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass: range outside source");
  if (count > kFusedMaxQueries)
    return fail(h, O3DS_ERR_CAPACITY, "icp_pass: at most O3DS_ICP_PASS_MAX_QUERIES (262144) source points per call: use o3ds_icp_accumulate / o3ds_icp_update for larger shards");
  IcpFusedArgs fa = fused_args(h, n_src_total);
  fa.pass.first = first;
  fa.pass.count = count;
  const int j = h->session_launches++;
  fa.first = j == 0;
  fa.pass_index = j;
  fa.state_in = h->session_state ? h->session_state : h->d_state;
  fa.state_out = fused_state_out(h, j);
  fa.state_host = nullptr;
  fa.slots_in = d_sums_in ? d_sums_in : d_sums_next;  // unused by the first launch
  fa.slots_out = d_sums_out;
  fa.slots_clear = d_sums_next;
  fa.trace = nullptr;
  launch_fused(h, fa, fused_blocks(count), true);
  h->session_state = fa.state_out;
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

int o3ds_icp_pass_finish(o3ds_handle h, size_t n_src_total, const double* d_sums_in, double* d_sums_scratch, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass_finish: no session");
  if (!out || !d_sums_in || !d_sums_scratch) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass_finish: null argument");
  if (h->session_launches == 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp_pass_finish: no pass was issued");
  IcpFusedArgs fa = fused_args(h, n_src_total);  // the one-workgroup tail launch: folds the last pass, never reaches the body
  fa.pass.count = 0;
  fa.first = 0;
  fa.state_in = h->session_state;
  fa.state_out = fused_state_out(h, h->session_launches++);
  fa.state_host = h->h_state_dev;
  fa.seq_host = pub_slot<unsigned long long>(h, kSeqSlot);
  fa.seq = ++h->fused_seq;
  fa.slots_in = d_sums_in;
  fa.slots_out = d_sums_scratch;  // a launch that still has iterations left would add an (empty) pass here
  fa.slots_clear = d_sums_scratch;
  launch_fused(h, fa, 1, false);
  HIP_TRY(hipGetLastError());
  HIP_TRY(wait_fused_state(h, fa.seq));
  h->session = false;
  h->session_state = nullptr;
  copy_result(h, out);
  return O3DS_OK;
}

int o3ds_icp_done(o3ds_handle h, int* done) {
  CHECK_HANDLE(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_done: no session");
  int rc = read_state(h, nullptr, h->session_state);
  if (rc) return rc;
  if (done) *done = h->h_state->done;
  return O3DS_OK;
}

int o3ds_icp_finish(o3ds_handle h, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  if (!h->session) return fail(h, O3DS_ERR_INVALID_ARG, "icp_finish: no session");
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_finish: null out");
  h->session = false;
  return read_state(h, out);
}

int o3ds_set_gicp_epsilon(o3ds_handle h, double epsilon) {
  CHECK_HANDLE(h);
  if (!(epsilon > 0.0 && epsilon <= 1.0)) return fail(h, O3DS_ERR_INVALID_ARG, "gicp epsilon must be in (0, 1]");
  h->gicp_epsilon = epsilon;
  return O3DS_OK;
}

int o3ds_icp_point_to_plane_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop,
                                const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  if (!params) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null params");
  o3ds_icp_params p = *params;
  p.method = O3DS_ICP_POINT_TO_PLANE;
  return o3ds_icp_register_dev(h, source, target, target_crop, init, &p, out);
}

int o3ds_information_matrix_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double T[16],
                                double max_correspondence_distance, double information[36]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !information) return fail(h, O3DS_ERR_INVALID_ARG, "information_matrix: null argument");
  o3ds_icp_params p{};
  p.max_correspondence_distance = max_correspondence_distance;
  p.max_iteration = 0;
  p.method = O3DS_ICP_POINT_TO_POINT;  // validation as for point-to-point: no normals needed
  (void)find_cloud(h, source);
  int rc = begin_session(h, source, target, target_crop, T, &p);
  if (rc) return rc;
  h->session = false;
  IcpPassArgs a = h->pass;
  a.method = kMethodInformation;
  double* d_record = nullptr;
  TMP_ALLOC(d_record, sizeof(double) * kRec);
  rc = accumulate_pass(h, a, d_record);
  if (rc) return rc;
  double rec[kRec];
  rc = read_back(h, {{rec, d_record, sizeof(rec)}});
  if (rc) return rc;
  // Lambda = [[ |q|^2 I - q q^T , [q]x ], [ [q]x^T , I ]] summed over the matched target points
  const double xx = rec[0], xy = rec[1], xz = rec[2], yy = rec[3], yz = rec[4], zz = rec[5], sx = rec[6], sy = rec[7], sz = rec[8];
  const double m = rec[kRecCount];
  const double L[6][6] = {{yy + zz, -xy, -xz, 0.0, -sz, sy}, {-xy, xx + zz, -yz, sz, 0.0, -sx}, {-xz, -yz, xx + yy, -sy, sx, 0.0},
                          {0.0, sz, -sy, m, 0.0, 0.0},       {-sz, 0.0, sx, 0.0, m, 0.0},      {sy, -sx, 0.0, 0.0, 0.0, m}};
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) information[r * 6 + c] = L[r][c];
  return O3DS_OK;
}

int o3ds_information_matrix(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, size_t n_tgt, const double T[16],
                            double max_correspondence_distance, double information[36]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !information) return fail(h, O3DS_ERR_INVALID_ARG, "information_matrix: null argument");
  if (!(max_correspondence_distance > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");
  if (n_tgt == 0) return fail(h, O3DS_ERR_EMPTY, "information_matrix: empty target");
  return with_uploaded_clouds(h, src_xyz, nullptr, n_src, tgt_xyz, nullptr, n_tgt, [&](o3ds_cloud s, o3ds_cloud t) {
    return o3ds_information_matrix_dev(h, s, t, nullptr, T, max_correspondence_distance, information);
  });
}

int o3ds_icp_point_to_point_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                                const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  if (!params) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null params");
  o3ds_icp_params p = *params;
  p.method = O3DS_ICP_POINT_TO_POINT;
  return o3ds_icp_register_dev(h, source, target, target_crop, init, &p, out);
}

int o3ds_icp_point_to_point(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, size_t n_tgt, const double init[16],
                            const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!params || !out || !init) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null argument");
  if (!(params->max_correspondence_distance > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");
  if (n_tgt == 0) return fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)");
  return with_uploaded_clouds(h, src_xyz, nullptr, n_src, tgt_xyz, nullptr, n_tgt,
                              [&](o3ds_cloud s, o3ds_cloud t) { return o3ds_icp_point_to_point_dev(h, s, t, nullptr, init, params, out); });
}

int o3ds_icp_generalized_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                             const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  if (!params) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null params");
  o3ds_icp_params p = *params;
  p.method = O3DS_ICP_GENERALIZED;
  // [O3D] InitializePointCloudForGeneralizedICP (call site CloudRegistration.cpp:16-21): a cloud that carries no normals gets
  // EstimateNormals(KDTreeSearchParamKNN(20)) on a COPY -- the caller's cloud stays without normals
  o3ds_cloud use[2] = {source, target}, own[2] = {0, 0};
  int rc = O3DS_OK;
  static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int k = 0; k < 2 && !rc; ++k) {
    const CloudRec* c = find_cloud_lazy(h, use[k]);
    if (!c || c->n == 0 || c->nrm) continue;
    rc = o3ds_transform_cloud(h, use[k], kIdentity, &own[k]);  // x * 1 + 0: a bit-exact copy
    if (rc) break;
    use[k] = own[k];
    CloudRec* cc = find_cloud(h, own[k]);
    ArenaScope arena_scope(h);
    rc = gicp_knn_normals(h, *cc);
  }
  if (!rc) rc = o3ds_icp_register_dev(h, use[0], use[1], target_crop, init, &p, out);
  const std::string keep = h->err;
  for (int k = 0; k < 2; ++k)
    if (own[k]) (void)o3ds_cloud_free(h, own[k]);
  if (rc) h->err = keep;
  return rc;
}

int o3ds_icp_generalized(o3ds_handle h, const double* src_xyz, const double* src_normals, size_t n_src, const double* tgt_xyz,
                         const double* tgt_normals, size_t n_tgt, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!params || !out || !init) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null argument");
  if (!(params->max_correspondence_distance > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");
  if (n_tgt == 0) return fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)");
  return with_uploaded_clouds(h, src_xyz, src_normals, n_src, tgt_xyz, tgt_normals, n_tgt,
                              [&](o3ds_cloud s, o3ds_cloud t) { return o3ds_icp_generalized_dev(h, s, t, nullptr, init, params, out); });
}

int o3ds_icp_overlap_next(o3ds_handle h, o3ds_overlap_fn fn, void* arg) {
  CHECK_HANDLE(h);
  h->overlap_fn = fn;
  h->overlap_arg = fn ? arg : nullptr;
  return O3DS_OK;
}

int o3ds_icp_register_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                          const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  struct OverlapOnce {  // the callback belongs to THIS registration: whatever happens, the next one does not inherit it
    o3ds_handle h;
    ~OverlapOnce() { h->overlap_fn = nullptr, h->overlap_arg = nullptr; }
  } overlap_once{h};
  if (!init || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null init/out");
  // the fused loop runs one workgroup per kIcpQ queries; its exact record sums are order-independent for up to 4096 workgroup records
  // (split_exact), so sources beyond kFusedMaxQueries points take the two-launch form (same results, looped pass kernel)
  CloudRec* src_rec = find_cloud_lazy(h, source);
  const bool use_fused = h->fused && src_rec && src_rec->n <= kFusedMaxQueries;
  if (src_rec && !use_fused) {  // the two-launch form hands the source size to its update kernel by value
    const int rr = resolve_count(h, *src_rec, true);
    if (rr) return rr;
  }
  int rc = begin_session(h, source, target, target_crop, init, params, !use_fused);
  if (rc) return rc;
  h->session = false;  // the loop below owns the state
  const IcpPassArgs a = h->pass;
  if (use_fused) {
    // launch j = [tail of pass j-1 in every workgroup's prologue] + pass j; launch max_iter+1 is prologue-only (one workgroup)
    IcpFusedArgs fa = fused_args(h, a.count);
    const int nb = fused_blocks(a.count);
    const int total = params->max_iteration + 2;
    // O3DS_FUSED_TRACE=<file>: phase timestamps of every workgroup of launch 5 (development aid, see scripts/fused_trace.py)
    const char* trace_path = ab_getenv("O3DS_FUSED_TRACE");
    unsigned long long* d_trace = nullptr;
    const int trace_launch = ab_getenv("O3DS_FUSED_TRACE_LAUNCH") ? atoi(ab_getenv("O3DS_FUSED_TRACE_LAUNCH")) : 5;
    if (trace_path && total > trace_launch + 1) {
      HIP_TRY(hipMalloc((void**)&d_trace, sizeof(unsigned long long) * 16 * nb));
      HIP_TRY(hipMemset(d_trace, 0, sizeof(unsigned long long) * 16 * nb));
    }
    // O3DS_ICP_STATS=1: per-launch counters of how the queries were served (verified from their candidate set / searched / sets left /
    // stage-3 queries), printed to stderr after the registration (development aid)
    static const bool want_stats = ab_getenv("O3DS_ICP_STATS") != nullptr;
    unsigned long long* d_stats = nullptr;
    if (want_stats) {
      HIP_TRY(hipMalloc((void**)&d_stats, sizeof(unsigned long long) * 4 * (size_t)total));
      HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * 4 * (size_t)total, h->stream));
    }
    int j = 0;
    const IcpStateDev* last = h->d_state;
    while (j < total) {
      // A launch after the loop has ended costs its launch (~4.6 us each, a dozen of them per registration of a stream whose scans
      // converge in four or five iterations), a look at the state costs a host round trip: queue what the previous registration on this
      // handle needed plus one, then four at a time
      const int chunk = std::min(total - j, j == 0 ? h->fused_chunk_hint[target_crop ? 1 : 0] : 4);
      for (int k = 0; k < chunk; ++k, ++j) {
        fa.first = j == 0;
        fa.pass_index = j;
        fa.state_in = last;
        fa.state_out = fused_state_out(h, j);
        // slot buffers rotate with a launch counter that runs across registrations: launch g reads (g-1)%3, adds into g%3, clears (g+1)%3
        const unsigned long long g = h->fused_launches++;
        fa.slots_in = (const double*)(h->d_fused + kFusedSlotsOff + ((g + 2) % 3) * kFusedSlotBufBytes);
        fa.slots_out = (double*)(h->d_fused + kFusedSlotsOff + (g % 3) * kFusedSlotBufBytes);
        fa.slots_clear = (double*)(h->d_fused + kFusedSlotsOff + ((g + 1) % 3) * kFusedSlotBufBytes);
        const bool tail_only = j == total - 1;
        fa.trace = j == trace_launch ? d_trace : nullptr;
        fa.pass.stats = d_stats ? d_stats + 4 * (size_t)j : nullptr;
        fa.state_host = k == chunk - 1 ? h->h_state_dev : nullptr;  // the launch the host waits for also writes the pinned copy
        fa.seq_host = pub_slot<unsigned long long>(h, kSeqSlot);
        if (fa.state_host) fa.seq = ++h->fused_seq;
        launch_fused(h, fa, tail_only ? 1 : nb, !tail_only);
        last = fa.state_out;
      }
      {
        // a failed launch or stream breaks the "slot buffer g % 3 was cleared by launch g - 1" rotation: clear all three and restart
        // the counter, so that the next registration does not add into records that were never cleared
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && h->overlap_fn) {  // o3ds_icp_overlap_next: the caller's work for the time this thread would wait (nested
          const o3ds_overlap_fn fn = h->overlap_fn;  // ABI calls bump-allocate behind this call's temporaries: the arena is reset by the
          void* const arg = h->overlap_arg;          // outermost call only)
          h->overlap_fn = nullptr;
          fn(arg);
          (void)hipSetDevice(h->device);
          e = hipGetLastError();
        }
        if (e == hipSuccess) e = wait_fused_state(h, h->fused_seq);
        if (e != hipSuccess) {
          (void)hipStreamSynchronize(h->stream);
          (void)hipMemset(h->d_fused + kFusedSlotsOff, 0, 3 * kFusedSlotBufBytes);
          h->fused_launches = 0;
          if (d_trace) (void)hipFree(d_trace);
          return fail(h, O3DS_ERR_HIP, std::string("icp (fused loop): ") + hipGetErrorString(e));
        }
      }
      copy_result(h, out);
      if (h->h_state->done) break;
    }
    h->fused_chunk_hint[target_crop ? 1 : 0] = std::min(std::max(h->h_state->iterations + 3, 4), 12);  // iterations + 2 launches were needed
    // (development aids below read device memory with null-stream copies: the handle's stream is non-blocking and the pinned stamp may have
    // been seen while the last launch was still draining)
    if (d_stats || d_trace) (void)hipStreamSynchronize(h->stream);
    if (d_stats) {
      std::vector<unsigned long long> t((size_t)4 * total);
      (void)hipMemcpy(t.data(), d_stats, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      (void)hipFree(d_stats);
      fprintf(stderr, "icp stats (n_src %zu):", (size_t)a.count);
      for (int k = 0; k < j; ++k) fprintf(stderr, " [%d v%llu s%llu k%llu f%llu]", k, t[4 * k], t[4 * k + 1], t[4 * k + 2], t[4 * k + 3]);
      fprintf(stderr, "\n");
    }
    if (d_trace) {
      std::vector<unsigned long long> t((size_t)16 * nb);
      (void)hipMemcpy(t.data(), d_trace, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      (void)hipFree(d_trace);
      if (FILE* f = fopen(trace_path, "w")) {
        for (int b = 0; b < nb; ++b) {
          for (int k = 0; k < 16; ++k) fprintf(f, "%llu ", t[(size_t)b * 16 + k]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
    return O3DS_OK;
  }
  const int nb = pass_blocks(h, a.count);
  const int total_passes = params->max_iteration + 1;  // max_iter updates need max_iter+1 correspondence passes
  return two_launch_loop(h, total_passes, look_at_session_state(h, out), [&] {
    launch_accumulate(h, a, nb);
    icp_reduce_update_kernel<<<1, kUpdBlock, 0, h->stream>>>(h->d_partials, nb, h->d_state, (unsigned long long)a.count,
                                                          params->max_iteration, params->relative_fitness, params->relative_rmse,
                                                          h->debug_update, h->session_method, quantum_table(a), a.src, a.src_f64);
  });
}

int o3ds_icp_point_to_plane(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, const double* tgt_normals,
                            size_t n_tgt, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!params || !out || !init) return fail(h, O3DS_ERR_INVALID_ARG, "icp: null argument");
  if (!(params->max_correspondence_distance > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");
  if (n_tgt == 0) return fail(h, O3DS_ERR_EMPTY, "icp: empty target (map patch size is zero)");
  if (!tgt_normals) return fail(h, O3DS_ERR_NO_NORMALS, "TransformationEstimationPointToPlane requires target normals");
  return with_uploaded_clouds(h, src_xyz, nullptr, n_src, tgt_xyz, tgt_normals, n_tgt,
                              [&](o3ds_cloud s, o3ds_cloud t) { return o3ds_icp_point_to_plane_dev(h, s, t, nullptr, init, params, out); });
}


// ---- pre-processing -----------------------------------------------------------------------------
}  // extern "C" (helpers below are C++)

namespace {

template <typename P4>
__global__ __launch_bounds__(kBlock) void reindex_copy_kernel(const P4* __restrict__ in, size_t n, P4* __restrict__ out, size_t off, int set_index) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    P4 p = in[i];
    if (set_index) p.i = (typename Scalar<P4>::index)(off + i);
    out[off + i] = p;
  }
}

// occupied cells of a grid index = cells whose start differs from the next start
__global__ __launch_bounds__(kBlock) void count_occupied_kernel(const int* __restrict__ cs, size_t m, unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (size_t)gridDim.x * kBlock) c += cs[i + 1] != cs[i];
  for (int k = 32; k >= 1; k >>= 1) c += __shfl_xor(c, k, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// first position whose key has the pass-through bit (keys sorted ascending) -> number of in-volume points
__global__ void first_pass_kernel(const unsigned long long* __restrict__ keys, size_t n, unsigned long long* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (keys[mid] & kPassBit)
      hi = mid;
    else
      lo = mid + 1;
  }
  *out = lo;
}

template <typename P4>
int crop_t(o3ds_handle h, const CloudRec& in, const CropDev& crop, CloudRec& out) {
  out.precision = in.precision;
  out.n = 0;
  box_copy(out, in);  // a subset
  if (in.n == 0) return O3DS_OK;
  int *flags = nullptr, *pos = nullptr;
  TMP_ALLOC(flags, sizeof(int) * (in.n + 1));
  TMP_ALLOC(pos, sizeof(int) * (in.n + 1));
  crop_flag_kernel<P4><<<grid_for(in.n), kBlock, 0, h->stream>>>((const P4*)in.pts, in.n, crop, flags);  // also writes the sentinel flags[n] = 0
  int rc = exclusive_scan_int(h, flags, pos, in.n + 1, pub_slot<int>(h, 0));
  if (rc) return rc;
  rc = wait_stream(h);
  if (rc) return rc;
  const int total = pub_value<int>(h, 0);
  out.n = (size_t)total;
  if (total > 0) {
    rc = compact_cloud<P4>(h, in, in.n, flags, pos, 1, out.n, &out.pts, &out.nrm, &out.col);
    if (rc) return rc;
  }
  return O3DS_OK;
}

// shared by VoxelDownSample (mode 0) and voxelizeWithinCroppingVolume (mode 1)
template <typename P4>
int voxel_reduce_t(o3ds_handle h, const CloudRec& in, int mode, double voxel, const CropDev& crop, CloudRec& out, bool filter = false,
                   long long merge_np = -1 /* >= 0: `in` is [pass block: merge_np | voxel block in key order: merge_nv | new points] */,
                   size_t merge_nv = 0) {
  // filter (mode 0 only): CroppingVolume::crop followed by VoxelDownSample in one go -- the points outside `crop` are keyed as
  // pass-through, sort behind the voxels and are not emitted; same grid anchor (the box of the INSIDE points), same keys, same
  // summation order as cropping first, without the compaction, its scan and its size read-back
  out.precision = in.precision;
  out.n = 0;
  const size_t n = in.n;
  if (n == 0) return O3DS_OK;
  double ox = 0, oy = 0, oz = 0;
  // VoxelDownSample proper: no sort (cloud_kernels.hpp, VoxTable); O3DS_VOXEL_SORT=1 keeps the sort-based path below for A/B runs
  static const bool voxel_sort = ab_getenv("O3DS_VOXEL_SORT") != nullptr;
  const bool table_path = mode == 0 && !voxel_sort && n < ((size_t)1 << 30);
  if (mode == 0) {  // [O3D] voxel_min_bound = GetMinBound() - voxel_size * 0.5
    double mn[3], mx[3];
    // the box of the points inside the volume: reduced by the ingest of this very cloud if it assumed the volume asked for now (a lidar
    // stream: always) -- the pinned record is normally there long before anyone asks; reduced now otherwise (one launch + a wait)
    CropDev want{};
    if (filter) want = crop;
    bool have_box = false;
    if (in.pre_slot >= 0 && memcmp(&in.pre_crop, &want, sizeof(CropDev)) == 0) {
      volatile o3ds_context::PinRec* r = h->h_rec + in.pre_slot;
      if (r->seq != in.pre_seq) HIP_TRY(hipStreamSynchronize(h->copy_stream));
      if (r->seq == in.pre_seq) {
        std::atomic_thread_fence(std::memory_order_acquire);
        for (int a = 0; a < 3; ++a) mn[a] = r->box[a], mx[a] = r->box[3 + a];
        have_box = true;
      }
    }
    if (!have_box) {
      int rc = bbox_of<P4>(h, (const P4*)in.pts, n, mn, mx, filter ? &crop : nullptr);
      if (rc) return rc;
    }
    if (filter) {  // the next ingest of this handle reduces its box for this volume
      h->pre_crop = crop;
      h->pre_crop_valid = true;
    }
    if (filter && mn[0] > mx[0]) return O3DS_OK;  // nothing inside the volume: an empty cloud
    if (voxel * 2147483647.0 < std::max({mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]}) + voxel)
      return fail(h, O3DS_ERR_INVALID_ARG, "[VoxelDownSample] voxel_size is too small.");
    ox = mn[0] - voxel * 0.5;
    oy = mn[1] - voxel * 0.5;
    oz = mn[2] - voxel * 0.5;
    out.has_box = true;  // voxel means lie in the box of the points they average
    out.box_padded = false;
    for (int a = 0; a < 3; ++a) out.bmn[a] = mn[a], out.bmx[a] = mx[a];
    if (!std::isfinite(mn[0] + mn[1] + mn[2] + mx[0] + mx[1] + mx[2])) out.has_box = false;
  } else {
    box_copy(out, in);
  }
  if (out.has_box) box_inflate(out);
  if (table_path) {
    VoxTable t{};
    size_t n_tiles = 0;
    const int rs = vox_scratch(h, n, "VoxelDownSample", &t, &n_tiles);
    if (rs) return rs;
    int *lead_slot = nullptr, *run_next = nullptr, *run_len = nullptr, *order = nullptr;
    uint32_t* starts = nullptr;
    int2* piece = nullptr;
    TMP_ALLOC(lead_slot, sizeof(int) * n);
    TMP_ALLOC(run_next, sizeof(int) * n);
    TMP_ALLOC(run_len, sizeof(int) * n);
    TMP_ALLOC(order, sizeof(int) * n);
    TMP_ALLOC(starts, sizeof(uint32_t) * n);
    if (in.col) TMP_ALLOC(piece, sizeof(int2) * n);
    // the size of the result: an upper bound here, the number of voxels in a device word and a pinned record when vox_order_kernel has run
    out.n = n;
    out.n_lower = 1;  // (the box is not empty: at least one point lies inside the volume, hence at least one voxel)
    out.lazy_slot = take_rec(h);
    if (out.lazy_slot < 0) return fail(h, O3DS_ERR_CAPACITY, "VoxelDownSample: no record free for the size of the result (every one is held by a persistent map)");
    out.lazy_seq = ++h->rec_seq;
    CountPub pub{cnt_word(h, out.lazy_slot), &(h->h_rec_dev + out.lazy_slot)->cnt, out.lazy_seq};
    const CountRef m_ref{n, pub.dev};
    HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * n));
    if (in.nrm) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * n));
    if (in.col) HIP_TRY(dev_alloc(h, (void**)&out.col, sizeof(P4) * n));
    if (++h->scan_gen == 0) h->scan_gen = 1;
    vox_insert_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.pts, n, ox, oy, oz, voxel, crop, filter ? 1 : 0, t, lead_slot, run_next, run_len);
    vox_order_kernel<<<(unsigned int)n_tiles, kBlock, 0, h->stream>>>(lead_slot, CountRef{n, nullptr}, t, h->d_tiles, h->d_ticket, h->ticket_base, h->scan_gen, order, pub);
    h->ticket_base += (unsigned int)n_tiles;
    vox_mean_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.pts, (const P4*)in.nrm, m_ref, order, run_next, run_len, starts, piece, 0,
                                                             (P4*)out.pts, (P4*)out.nrm, t);
    h->voxtab_clean = true;
    if (in.col)  // [O3D] VoxelDownSample: AccumulatedPoint averages the colours
      vox_mean_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.col, nullptr, m_ref, order, run_next, run_len, starts, piece, 1, (P4*)out.col,
                                                               nullptr, t);
    HIP_TRY(hipGetLastError());
    return O3DS_OK;
  }
  unsigned long long *k0 = nullptr, *k1 = nullptr, *d_scalar = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  size_t merged_n_inside = 0;
  int *head = nullptr, *seg_id = nullptr, *seg_start = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(head, sizeof(int) * (n + 1));
  TMP_ALLOC(seg_id, sizeof(int) * (n + 1));
  TMP_ALLOC(d_scalar, sizeof(unsigned long long));
  // The sorted (key, index) list: by merging when the input is a map the previous merge left in key order plus new points (only the
  // new keys are sorted), by one radix sort of everything otherwise.  Same arrays either way (cloud_kernels.hpp, merge_class_kernel).
  static const bool no_incremental = ab_getenv("O3DS_NO_INCREMENTAL_MERGE") != nullptr;  // A/B and debugging
  bool merged = false;
  if (mode == 1 && !filter && merge_np >= 0 && !no_incremental && n < ((size_t)1 << 31) && (size_t)merge_np + merge_nv <= n) {
    const size_t np = (size_t)merge_np, nv = merge_nv;
    unsigned long long *cls = nullptr, *rank = nullptr, *vk = nullptr, *xk = nullptr, *xk2 = nullptr;
    uint32_t *vv = nullptr, *xv = nullptr, *xv2 = nullptr;
    int* d_unsorted = nullptr;
    const size_t nx_cap = n - nv;  // the pass block and the new points
    TMP_ALLOC(cls, sizeof(unsigned long long) * (n + 1));
    TMP_ALLOC(rank, sizeof(unsigned long long) * (n + 1));
    TMP_ALLOC(vk, sizeof(unsigned long long) * (nv + 1));
    TMP_ALLOC(vv, sizeof(uint32_t) * (nv + 1));
    TMP_ALLOC(xk, sizeof(unsigned long long) * (nx_cap + 1));
    TMP_ALLOC(xv, sizeof(uint32_t) * (nx_cap + 1));
    // the "not in key order" flag and the three totals are stored into the pinned block by the kernels themselves (slot 2: the host
    // clears it here -- nothing is in flight that writes it, every use ends in a synchronisation)
    d_unsorted = pub_slot<int>(h, 2);
    *(volatile int*)(h->h_pin + kPubOff + 32) = 0;
    merge_class_kernel<P4><<<grid_for(n + 1), kBlock, 0, h->stream>>>((const P4*)in.pts, n, voxel, crop, np, nv, k0, cls, d_unsorted);
    int rcs = exclusive_scan_t<unsigned long long>(h, cls, rank, n + 1, pub_slot<unsigned long long>(h, 1));
    if (rcs) return rcs;
    rcs = wait_stream(h);
    if (rcs) return rcs;
    const unsigned long long tot = pub_value<unsigned long long>(h, 1);
    const int unsorted = pub_value<int>(h, 2);
    if (!unsorted) {
      const size_t npass_ = (size_t)(tot & kCntMask), nvin = (size_t)(tot >> 32), nx = n - npass_ - nvin;
      int *xpos = nullptr, *cnt = nullptr, *before = nullptr;
      TMP_ALLOC(xpos, sizeof(int) * (nx + 1));
      TMP_ALLOC(cnt, sizeof(int) * (nvin + 2));
      TMP_ALLOC(before, sizeof(int) * (nvin + 2));
      merge_split_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(k0, rank, n, np, nv, k1, v1, vk, vv, xk, xv, cnt, nvin + 2);
      const unsigned long long* xks = xk;
      const uint32_t* xvs = xv;
      if (nx > 1) {  // the only sort: the points that are new to the volume -- tile sort in LDS, then merge passes (cloud_kernels.hpp)
        TMP_ALLOC(xk2, sizeof(unsigned long long) * nx);
        TMP_ALLOC(xv2, sizeof(uint32_t) * nx);
        static const bool lib_sort = ab_getenv("O3DS_MERGE_LIBRARY_SORT") != nullptr;  // A/B: rocPRIM's radix sort of the same pairs
        if (lib_sort) {
          rcs = sort_pairs(h, xk, xk2, xv, xv2, nx, 63);
          if (rcs) return rcs;
          xks = xk2, xvs = xv2;
        } else {
          unsigned long long *ka = xk2, *kb = xk;  // the tile sort reads xk / xv and writes the second pair of buffers; passes ping-pong
          uint32_t *va = xv2, *vb = xv;
          sort_tile_kernel<<<(unsigned int)((nx + kSortTile - 1) / kSortTile), kBlock, 0, h->stream>>>(xk, xv, nx, ka, va);
          static const int ways = [] {  // tuning experiments: 2, 4, 8 or 16 runs merged per pass; anything else is ignored (a width that
            const int w = ab_getenv("O3DS_SORT_WAYS") ? atoi(ab_getenv("O3DS_SORT_WAYS")) : kSortWays;  // grows by 3 under an 8-way kernel sorts wrongly)
            return (w == 2 || w == 4 || w == 8 || w == 16) ? w : kSortWays;
          }();
          for (size_t width = kSortTile; width < nx; width *= (size_t)ways) {  // nx < 2^31 on this path
            const unsigned int gsz = (unsigned int)grid_for(nx);
            if (ways == 2)
              sort_merge_pass_kernel<2><<<gsz, kBlock, 0, h->stream>>>(ka, va, (uint32_t)nx, (uint32_t)width, kb, vb);
            else if (ways == 4)
              sort_merge_pass_kernel<4><<<gsz, kBlock, 0, h->stream>>>(ka, va, (uint32_t)nx, (uint32_t)width, kb, vb);
            else if (ways == 16)
              sort_merge_pass_kernel<16><<<gsz, kBlock, 0, h->stream>>>(ka, va, (uint32_t)nx, (uint32_t)width, kb, vb);
            else
              sort_merge_pass_kernel<8><<<gsz, kBlock, 0, h->stream>>>(ka, va, (uint32_t)nx, (uint32_t)width, kb, vb);
            std::swap(ka, kb);
            std::swap(va, vb);
          }
          xks = ka, xvs = va;
        }
      }
      if (nx) merge_rank_kernel<<<grid_for(nx), kBlock, 0, h->stream>>>(xks, xvs, nx, vk, nvin, np, xpos, cnt);
      rcs = exclusive_scan_int(h, cnt, before, nvin + 2);
      if (rcs) return rcs;
      if (nvin + nx) merge_place_kernel<<<grid_for(nvin + nx), kBlock, 0, h->stream>>>(vk, vv, nvin, before, xks, xvs, xpos, nx, k1, v1);
      (void)npass_;
      merged = true;
      merged_n_inside = nvin + nx;
    }
  }
  if (!merged) {
    voxel_key_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)in.pts, n, mode, ox, oy, oz, voxel, crop, k0, v0, filter ? 1 : 0);
    const int rs = sort_pairs(h, k0, k1, v0, v1, n);
    if (rs) return rs;
  }
  segment_head_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(k1, n, head);  // also writes the sentinel head[n] = 0
  if (!merged) first_pass_kernel<<<1, 64, 0, h->stream>>>(k1, n, pub_slot<unsigned long long>(h, 3));
  int rc = exclusive_scan_int(h, head, seg_id, n + 1, pub_slot<int>(h, 0));
  if (rc) return rc;
  rc = wait_stream(h);
  if (rc) return rc;
  const int n_seg = pub_value<int>(h, 0);
  const unsigned long long n_inside = merged ? (unsigned long long)merged_n_inside : pub_value<unsigned long long>(h, 3);
  (void)d_scalar;
  const size_t n_pass = n - (size_t)n_inside;
  if (mode == 1 && !filter) {  // the layout the next merge can rely on
    out.vox_first = (long long)n_pass;
    out.vox_count = (size_t)n_seg - n_pass;
  }
  TMP_ALLOC(seg_start, sizeof(int) * ((size_t)n_seg + 1));
  segment_start_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(head, seg_id, n, seg_start);
  const int drop = filter ? 1 : 0;
  out.n = filter ? (size_t)n_seg - n_pass : (size_t)n_seg;
  if (out.n == 0) return O3DS_OK;
  // a map (mode 1) gets room for the scans to come: Submap::insertScan appends one before every merge, and with the room in place the
  // append is one kernel that places the scan's points behind the map's instead of two allocations and a copy of the whole map
  const size_t room = (mode == 1 && !filter) ? out.n + std::max<size_t>(out.n / 4, (size_t)1 << 18) : out.n;
  HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * room));
  if (in.nrm) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * room));
  if (room > out.n && !in.col) out.cap = room;
  segment_mean_kernel<P4><<<grid_for((size_t)n_seg), kBlock, 0, h->stream>>>((const P4*)in.pts, (const P4*)in.nrm, k1, v1, seg_start, (size_t)n_seg, n,
                                                                            mode == 1 ? 1 : 0, n_pass, (P4*)out.pts, (P4*)out.nrm, drop);
  if (in.col) {
    HIP_TRY(dev_alloc(h, (void**)&out.col, sizeof(P4) * out.n));
    if (mode == 0)  // [O3D] VoxelDownSample: AccumulatedPoint averages the colours
      segment_mean_kernel<P4><<<grid_for((size_t)n_seg), kBlock, 0, h->stream>>>((const P4*)in.col, nullptr, k1, v1, seg_start, (size_t)n_seg, n, 0, n_pass,
                                                                                (P4*)out.col, nullptr, drop);
    else  // the map merge keeps the colour of the LAST point of a voxel (helpers.cpp:40-42,61-63: `color_ = ...`, not `+=`)
      segment_last_kernel<P4><<<grid_for(out.n), kBlock, 0, h->stream>>>((const P4*)in.col, k1, v1, seg_start, out.n, n, n_pass, (P4*)out.col);
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

template <typename P4>
int normals_t(o3ds_handle h, CloudRec& c, double radius, int max_nn, bool knn_raw = false) {
  if (c.n == 0) return O3DS_OK;
  if (knn_raw || !c.has_box) {  // (paths that reduce a box on the host need the exact size first)
    const int rr = resolve_count(h, c, true);
    if (rr) return rr;
    if (c.n == 0) return O3DS_OK;
  }
  if (knn_raw) {  // [O3D] EstimateNormals(KDTreeSearchParamKNN(max_nn)) and nothing after it: a radius no pair of points exceeds
    double mn[3], mx[3];
    const int rb = bbox_of<P4>(h, (const P4*)c.pts, c.n, mn, mx);
    if (rb) return rb;
    const double dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    radius = std::sqrt(dx * dx + dy * dy + dz * dz) * 1.001 + 1e-3;
    if (!std::isfinite(radius)) return fail(h, O3DS_ERR_INVALID_ARG, "estimate_normals: non-finite points");
  }
  // The cell size only steers the cost of the (exact) ring search: aim at max_nn / pi points per occupied cell, so that the
  // max_nn-th neighbour typically lies inside the first 3x3x3 ring.  The density comes from a pilot grid at radius/8 -- one
  // extra index build, one counting kernel and a host round trip -- so it is remembered per (radius, max_nn) and reused
  // while the cloud size stays within 25 % (a lidar stream: every scan), refreshed every 32 calls.
  // (a cloud whose size is still in flight: the heuristics below go by the size of the handle's previous VoxelDownSample result -- a lidar
  // stream's scans are alike --, the kernels by the device word; the density pilot needs the real size and waits for it)
  size_t n_est = c.lazy_slot >= 0 ? std::min(c.n, h->voxel_count_hint) : c.n;
  bool reuse = h->nrm_cell > 0.0 && h->nrm_radius == radius && h->nrm_knn == max_nn && h->nrm_age < 32 && n_est > 0 &&
               (double)n_est <= 1.25 * (double)h->nrm_n && (double)n_est >= 0.75 * (double)h->nrm_n;
  if (!reuse && c.lazy_slot >= 0) {
    const int rr = resolve_count(h, c, true);
    if (rr) return rr;
    if (c.n == 0) return O3DS_OK;
    n_est = c.n;
    reuse = h->nrm_cell > 0.0 && h->nrm_radius == radius && h->nrm_knn == max_nn && h->nrm_age < 32 &&
            (double)n_est <= 1.25 * (double)h->nrm_n && (double)n_est >= 0.75 * (double)h->nrm_n;
  }
  const int* n_dev = c.lazy_slot >= 0 ? cnt_word(h, c.lazy_slot) : nullptr;
  CloudRec tmp;
  tmp.n = c.n;
  tmp.precision = c.precision;
  tmp.pts = c.pts;  // borrowed
  tmp.lazy_slot = c.lazy_slot;  // (borrowed as well: build_index_t hands the device word to its kernels)
  box_copy(tmp, c);
  IndexGuard tmp_guard(h, tmp);
  int rc = O3DS_OK;
  if (reuse) {
    ++h->nrm_age;
    rc = build_index_t<P4>(h, tmp, h->nrm_cell);
    if (rc) return rc;
  } else {
    rc = build_index_t<P4>(h, tmp, radius / 8.0);
    if (rc) return rc;
    const size_t ncell = (size_t)tmp.grid.nx * tmp.grid.ny * tmp.grid.nz;
    unsigned long long* d_cnt = nullptr;
    TMP_ALLOC(d_cnt, sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), h->stream));
    count_occupied_kernel<<<grid_for(ncell), kBlock, 0, h->stream>>>(tmp.cell_start, ncell, d_cnt);
    unsigned long long occ = 0;
    rc = read_back(h, {{&occ, d_cnt, sizeof(occ)}});
    if (rc) return rc;
    const double avg = occ ? (double)c.n / (double)occ : 1.0;
    double cell = tmp.grid.cell * std::sqrt(std::max(1.0, (double)max_nn) / (3.14159265358979 * avg));
    cell = std::min(std::max(cell, radius / 64.0), radius);
    rc = build_index_t<P4>(h, tmp, cell);
    if (rc) return rc;
    h->nrm_cell = tmp.grid.cell;
    h->nrm_radius = radius;
    h->nrm_knn = max_nn;
    h->nrm_n = c.n;
    h->nrm_age = 0;
  }
  // (a map keeps room behind its points, CloudRec::cap: normals that arrive later get the same room, the in-place append of
  // o3ds_map_insert_scan writes both arrays behind the last point)
  if (!c.nrm) HIP_TRY(dev_alloc(h, (void**)&c.nrm, sizeof(P4) * std::max(c.n, c.cap)));
  const int rmax = std::max(1, (int)std::ceil(radius / tmp.grid.cell));
  // 16 lanes per point, 16 points per 256-thread workgroup (normals_kernel.hpp), then a thread per point for the eigen-solve; the instantiation is picked by max_nn
  {
    const P4* p_pts = (const P4*)c.pts;
    const P4* p_sp = (const P4*)tmp.spts;
    P4* p_out = (P4*)c.nrm;
    const unsigned int gsz = (unsigned int)((c.n + o3ds::kNrmPointsPerBlock - 1) / o3ds::kNrmPointsPerBlock);
    double* d_sums = nullptr;
    int* d_cnts = nullptr;
    TMP_ALLOC(d_sums, sizeof(double) * 9 * c.n);
    TMP_ALLOC(d_cnts, sizeof(int) * c.n);
    span_mark(h, kSpanNormalsKernels);
    if (max_nn <= 32) {  // the shipped configs' knn is 20
      if constexpr (sizeof(P4) == 16)
        normals_kernel_occ5<P4, 32><<<gsz, 64 * o3ds::kNrmWaves, 0, h->stream>>>(p_pts, c.n, tmp.grid, p_sp, radius, max_nn, rmax, d_sums, d_cnts, n_dev);
      else
        normals_kernel<P4, 32><<<gsz, 64 * o3ds::kNrmWaves, 0, h->stream>>>(p_pts, c.n, tmp.grid, p_sp, radius, max_nn, rmax, d_sums, d_cnts, n_dev);
    } else
      normals_kernel<P4, 128><<<gsz, 64 * o3ds::kNrmWaves, 0, h->stream>>>(p_pts, c.n, tmp.grid, p_sp, radius, max_nn, rmax, d_sums, d_cnts, n_dev);
    // the grid, the cell-ordered points and (written here) the cell-ordered normals are a complete nearest-neighbour index of the cloud:
    // kept, so that a registration against this cloud (scan-to-scan odometry: the previous scan) does not build another one
    if (dev_alloc(h, (void**)&tmp.snrm, sizeof(P4) * c.n) != hipSuccess) return fail(h, O3DS_ERR_OOM, "estimate_normals: out of device memory");
    normals_finish_kernel<P4><<<(unsigned int)((c.n + 255) / 256), 256, 0, h->stream>>>(p_sp, c.n, d_sums, d_cnts, p_out, knn_raw ? 1 : 0, (P4*)tmp.snrm, n_dev);
    span_mark(h, kSpanNormalsKernels);
  }
  HIP_TRY(hipGetLastError());
  tmp_guard.release();
  box_copy(c, tmp);  // the box an index build reduced is kept for the cloud
  free_index(h, c);  // the cloud's own index (if any) no longer matches its normals
  c.grid = tmp.grid, c.cell_start = tmp.cell_start, c.spts = tmp.spts, c.snrm = tmp.snrm;
  c.spts_slack = tmp.spts_slack;
  c.has_index = true;
  c.index_byproduct = true;
  return O3DS_OK;
}

int gicp_knn_normals(o3ds_handle h, CloudRec& c) {
  return DISPATCH(c.precision, normals_t, h, c, 0.0, 20, true);
}

template <typename P4>
int transform_t(o3ds_handle h, const CloudRec& in, const double T[16], CloudRec& out) {
  out.precision = in.precision;
  out.n = in.n;
  box_transform(out, in, T);
  if (in.n == 0) return O3DS_OK;
  HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * in.n));
  if (in.nrm) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * in.n));
  transform_kernel<P4><<<grid_for(in.n), kBlock, 0, h->stream>>>((const P4*)in.pts, (const P4*)in.nrm, in.n, mat34(T), T[3], T[7], T[11], T[15],
                                                               (P4*)out.pts, (P4*)out.nrm, 0);
  if (in.col) {
    HIP_TRY(dev_alloc(h, (void**)&out.col, sizeof(P4) * in.n));
    HIP_TRY(hipMemcpyAsync(out.col, in.col, sizeof(P4) * in.n, hipMemcpyDeviceToDevice, h->stream));
  }
  if (in.has_fpfh && in.fpfh_n == in.n && in.fpfh) {  // [O3D] PointCloud::Transform leaves a Feature as it is (Submap::transform moves the
    const size_t bytes = in.n * kFeatDim * sizeof(double);  // sparse map, Submap.cpp:96, and keeps feature_)
    HIP_TRY(dev_alloc(h, (void**)&out.fpfh, bytes));
    HIP_TRY(hipMemcpyAsync(out.fpfh, in.fpfh, bytes, hipMemcpyDeviceToDevice, h->stream));
    out.has_fpfh = true;
    out.fpfh_n = in.n;
  }
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

// Submap::carve (Submap.cpp:109-125): remove from `map` the points that the rays of `scan` (sensor frame, placed by T) see through
template <typename P4>
int carve_t(o3ds_handle h, CloudRec& map, const CloudRec& scan, const double T[16], const CropDev& crop, const o3ds_carving_params& cp,
            size_t* n_removed, CloudRec* removed = nullptr /* the carved points, in map order (Submap::toRemove_) */) {
  *n_removed = 0;
  const size_t n = map.n;
  if (n == 0 || scan.n == 0) return O3DS_OK;
  unsigned long long *k0 = nullptr, *k1 = nullptr, *tkey = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  int *head = nullptr, *seg_id = nullptr, *seg_start = nullptr, *tseg = nullptr, *keep = nullptr, *pos = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(head, sizeof(int) * (n + 1));
  TMP_ALLOC(seg_id, sizeof(int) * (n + 1));
  // VoxelMap of the map points inside the wide cropping volume (cropper.getIndicesWithinVolume + insertCloud): same key as the merge
  voxel_key_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)map.pts, n, 1, 0.0, 0.0, 0.0, cp.voxel_size, crop, k0, v0);
  // The sorted (key, index) list.  A map that the merge of an insertion left is [outside points | voxel block in ascending key order], and the
  // carving volume is the volume of that insertion (Submap.cpp:56-71: the cropper still holds its pose): the inside entries are then already in
  // key order, and a stable PARTITION by "inside" (one scan, one scatter) gives what the stable sort gives.  Whether they really were in order
  // -- another voxel size, a map assembled otherwise, a mean that rounding put across a voxel boundary -- is checked on the device while the
  // segment heads are formed; if not, the library sort runs as before (O3DS_CARVE_SORT=1 forces it, for A/B runs).
  static const bool carve_sort = ab_getenv("O3DS_CARVE_SORT") != nullptr;
  const bool try_partition = !carve_sort && map.vox_first >= 0 && (size_t)map.vox_first + map.vox_count == n && n < ((size_t)1 << 31);
  int rc = O3DS_OK;
  int n_seg = 0;
  bool sorted_ok = false;
  if (try_partition) {
    int* rank = nullptr;
    TMP_ALLOC(rank, sizeof(int) * (n + 1));
    rc = exclusive_scan_fn<int>(h, KeyInsideFlag{k0, n}, rank, n + 1);
    if (rc) return rc;
    partition_keys_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(k0, rank, n, k1, v1);
    int* d_unsorted = pub_slot<int>(h, 2);
    *(volatile int*)(h->h_pin + kPubOff + 32) = 0;  // (nothing in flight writes the slot: every use ends in a synchronisation)
    segment_head_check_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(k1, n, head, d_unsorted);
    rc = segment_ids(h, head, seg_id, n, &n_seg);
    if (rc) return rc;
    sorted_ok = pub_value<int>(h, 2) == 0;
  }
  if (!sorted_ok) {
    rc = sort_pairs(h, k0, k1, v0, v1, n);
    if (!rc) rc = key_segments(h, k1, n, head, seg_id, &n_seg);
    if (rc) return rc;
  }
  TMP_ALLOC(seg_start, sizeof(int) * ((size_t)n_seg + 1));
  segment_start_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(head, seg_id, n, seg_start);
  size_t tsize = 1024;
  while (tsize < 2 * (size_t)n_seg) tsize <<= 1;
  TMP_ALLOC(tkey, sizeof(unsigned long long) * tsize);
  TMP_ALLOC(tseg, sizeof(int) * tsize);
  HIP_TRY(hipMemsetAsync(tkey, 0xFF, sizeof(unsigned long long) * tsize, h->stream));
  unsigned int* block_bits = nullptr;  // one bit per hashed 4 x 4 x 4 block of voxels (cloud_kernels.hpp, carve_block_bit)
  TMP_ALLOC(block_bits, sizeof(unsigned int) << (kCarveBitsLog2 - 5));
  HIP_TRY(hipMemsetAsync(block_bits, 0, sizeof(unsigned int) << (kCarveBitsLog2 - 5), h->stream));
  carve_table_insert_kernel<<<grid_for((size_t)n_seg), kBlock, 0, h->stream>>>(k1, seg_start, (size_t)n_seg, tkey, tseg, (unsigned int)(tsize - 1),
                                                                               block_bits);
  TMP_ALLOC(keep, sizeof(int) * (n + 1));
  TMP_ALLOC(pos, sizeof(int) * (n + 1));
  fill_int_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(keep, n, 1);
  HIP_TRY(hipMemsetAsync(keep + n, 0, sizeof(int), h->stream));
  carve_rays_kernel<P4><<<grid_for(scan.n), kBlock, 0, h->stream>>>((const P4*)scan.pts, scan.n, mat34(T), T[12], T[13], T[14], cp.voxel_size,
                                                                   cp.max_raytracing_length, cp.truncation_distance,
                                                                   cp.min_dot_product_with_normal, tkey, tseg, (unsigned int)(tsize - 1), seg_start,
                                                                   (size_t)n_seg, n, v1, (const P4*)map.nrm, keep, block_bits);
  rc = exclusive_scan_int(h, keep, pos, n + 1);
  if (rc) return rc;
  int total = 0, kept_outside = 0;
  // with the merge's layout known, the number of kept points of its first block comes back with the total: both blocks shrink in place, in
  // order, and the next insertion still finds [outside points | voxel block in key order] -- no sort of the whole map after a carve
  const bool layout = map.vox_first >= 0 && (size_t)map.vox_first + map.vox_count == n;
  rc = layout ? read_back(h, {{&total, pos + n, sizeof(int)}, {&kept_outside, pos + (size_t)map.vox_first, sizeof(int)}})
              : read_back(h, {{&total, pos + n, sizeof(int)}});
  if (rc) return rc;
  *n_removed = n - (size_t)total;
  if (*n_removed == 0) return O3DS_OK;  // removeByIds: nothing to do (helpers.cpp:221-223)
  if (removed) {  // map->SelectByIndex(idxsToRemove) (Submap.cpp:119): the same flags and positions, the other side of the compaction
    removed->precision = map.precision;
    removed->n = *n_removed;
    rc = compact_cloud<P4>(h, map, n, keep, pos, 0, removed->n, &removed->pts, &removed->nrm, &removed->col);
    if (rc) return rc;
    box_copy(*removed, map);
  }
  void *np = nullptr, *nn = nullptr, *nc = nullptr;
  if (total > 0) {
    rc = compact_cloud<P4>(h, map, n, keep, pos, 1, (size_t)total, &np, &nn, &nc);
    if (rc) return rc;
  }
  replace_arrays(h, map, np, nn, nc, (size_t)total, 0);
  drop_ingest_box(h, map);
  if (layout) {
    map.vox_first = (long long)kept_outside;
    map.vox_count = (size_t)total - (size_t)kept_outside;
  } else {
    map.vox_first = -1;
  }
  return O3DS_OK;
}

// computeIndicesOfOverlappingPoints (helpers.cpp:307-332)
template <typename P4>
int overlap_t(o3ds_handle h, const CloudRec& src, const CloudRec& tgt, const double T[16], double voxel, size_t min_points,
              unsigned long long* idx_src, size_t* n_src_out, unsigned long long* idx_tgt, size_t* n_tgt_out) {
  *n_src_out = *n_tgt_out = 0;
  const size_t ns = src.n, nt = tgt.n, n = ns + nt;
  if (ns == 0 || nt == 0) return O3DS_OK;  // no voxel can hold points of both clouds
  CloudRec moved;
  CloudGuard moved_guard(h, moved);
  int rc = transform_t<P4>(h, src, T, moved);  // sourceTransformed.Transform(sourceToTarget)
  if (rc) return rc;
  unsigned long long *k0 = nullptr, *k1 = nullptr, *d_out = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  int *head = nullptr, *seg_id = nullptr, *cnt = nullptr, *flag = nullptr, *pos = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(head, sizeof(int) * (n + 1));
  TMP_ALLOC(seg_id, sizeof(int) * (n + 1));
  CropDev none{};
  voxel_key_kernel<P4><<<grid_for(nt), kBlock, 0, h->stream>>>((const P4*)tgt.pts, nt, 1, 0.0, 0.0, 0.0, voxel, none, k0, v0);
  voxel_key_kernel<P4><<<grid_for(ns), kBlock, 0, h->stream>>>((const P4*)moved.pts, ns, 1, 0.0, 0.0, 0.0, voxel, none, k0 + nt, v0 + nt);
  overlap_tag_kernel<<<grid_for(ns), kBlock, 0, h->stream>>>(v0 + nt, ns);
  rc = sort_pairs(h, k0, k1, v0, v1, n);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(head + n, 0, sizeof(int), h->stream));
  rc = key_segments(h, k1, n, head, seg_id, nullptr);
  if (rc) return rc;
  TMP_ALLOC(cnt, sizeof(int) * 2 * n);  // at most n segments: [0, n) source counts, [n, 2n) target counts
  HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int) * 2 * n, h->stream));
  overlap_count_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(v1, head, seg_id, n, cnt, cnt + n);
  TMP_ALLOC(flag, sizeof(int) * (n + 2));  // [0, ns] source flags (+ terminator), then [ns + 1, ns + 1 + nt] target flags
  TMP_ALLOC(pos, sizeof(int) * (n + 2));
  HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int) * (n + 2), h->stream));
  int* flag_s = flag;
  int* flag_t = flag + ns + 1;
  overlap_flag_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(v1, head, seg_id, n, cnt, cnt + n, (int)std::min<size_t>(min_points, 0x7fffffff), flag_s,
                                                             flag_t);
  rc = exclusive_scan_int(h, flag_s, pos, ns + 1);
  if (!rc) rc = exclusive_scan_int(h, flag_t, pos + ns + 1, nt + 1);
  if (rc) return rc;
  int tot[2] = {0, 0};
  rc = read_back(h, {{&tot[0], pos + ns, sizeof(int)}, {&tot[1], pos + ns + 1 + nt, sizeof(int)}});
  if (rc) return rc;
  TMP_ALLOC(d_out, sizeof(unsigned long long) * (size_t)(tot[0] + tot[1] + 1));
  index_compact_kernel<<<grid_for(ns), kBlock, 0, h->stream>>>(flag_s, pos, ns, d_out);
  index_compact_kernel<<<grid_for(nt), kBlock, 0, h->stream>>>(flag_t, pos + ns + 1, nt, d_out + tot[0]);
  HIP_TRY(hipGetLastError());
  if (tot[0]) HIP_TRY(hipMemcpyAsync(idx_src, d_out, sizeof(unsigned long long) * (size_t)tot[0], hipMemcpyDeviceToHost, h->stream));
  if (tot[1]) HIP_TRY(hipMemcpyAsync(idx_tgt, d_out + tot[0], sizeof(unsigned long long) * (size_t)tot[1], hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *n_src_out = (size_t)tot[0];
  *n_tgt_out = (size_t)tot[1];
  return O3DS_OK;
}

template <typename P4>
int append_t(o3ds_handle h, CloudRec& map, const CloudRec& add) {
  // [O3D] PointCloud::operator+= : normals survive only if (map empty or map has normals) and add has normals
  const bool keep_nrm = (map.n == 0 || map.nrm) && add.nrm;
  const bool keep_col = (map.n == 0 || map.col) && add.col;  // the same rule for colors_
  const size_t n = map.n + add.n;
  CloudRec joined;
  box_union(joined, map, add);
  void *np = nullptr, *nn = nullptr, *nc = nullptr;
  DevGuard guard(h);
  guard.add(&np), guard.add(&nn), guard.add(&nc);
  if (n > 0) HIP_TRY(dev_alloc(h, (void**)&np, sizeof(P4) * n));
  if (keep_nrm && n > 0) HIP_TRY(dev_alloc(h, (void**)&nn, sizeof(P4) * n));
  if (keep_col && n > 0) HIP_TRY(dev_alloc(h, (void**)&nc, sizeof(P4) * n));
  if (map.n) {
    HIP_TRY(hipMemcpyAsync(np, map.pts, sizeof(P4) * map.n, hipMemcpyDeviceToDevice, h->stream));
    if (keep_nrm) HIP_TRY(hipMemcpyAsync(nn, map.nrm, sizeof(P4) * map.n, hipMemcpyDeviceToDevice, h->stream));
    if (keep_col) HIP_TRY(hipMemcpyAsync(nc, map.col, sizeof(P4) * map.n, hipMemcpyDeviceToDevice, h->stream));
  }
  if (add.n) {
    reindex_copy_kernel<P4><<<grid_for(add.n), kBlock, 0, h->stream>>>((const P4*)add.pts, add.n, (P4*)np, map.n, 1);
    if (keep_nrm) reindex_copy_kernel<P4><<<grid_for(add.n), kBlock, 0, h->stream>>>((const P4*)add.nrm, add.n, (P4*)nn, map.n, 0);
    if (keep_col) reindex_copy_kernel<P4><<<grid_for(add.n), kBlock, 0, h->stream>>>((const P4*)add.col, add.n, (P4*)nc, map.n, 0);
  }
  HIP_TRY(hipGetLastError());
  guard.release();
  replace_arrays(h, map, np, nn, nc, n, 0);
  drop_ingest_box(h, map);
  box_copy(map, joined);
  return O3DS_OK;
}

// [O3D] PointCloud::RandomDownSample(ratio) (Odometry.cpp:29, ScanToMapRegistration.cpp:39) as a draw on the device (cloud_kernels.hpp,
// DrawState): nothing of it -- not the size of the input, not the number kept -- passes through the host
template <typename P4>
int random_down_sample_t(o3ds_handle h, const CloudRec& in, double ratio, unsigned long long seed, CloudRec& out) {
  out.precision = in.precision;
  out.n = 0;
  box_copy(out, in);  // a subset
  if (in.n == 0 || (int)(ratio * (double)in.n) <= 0) return O3DS_OK;  // (k is monotone in the size: nothing is kept of the bound, nothing of the exact size)
  if (in.n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_INVALID_ARG, "random_down_sample: more than 2^31 points");
  constexpr int kDrawErrSlot = 9;  // pinned word draw_pick_kernel raises when its candidate list overflowed (sticky, like DrawState::error)
  if (!h->d_draw) {
    if (hipMalloc((void**)&h->d_draw, sizeof(o3ds::DrawState)) != hipSuccess) return fail(h, O3DS_ERR_OOM, "random_down_sample: state allocation failed");
    HIP_TRY(hipMemsetAsync(h->d_draw, 0, sizeof(o3ds::DrawState), h->stream));
    *(volatile int*)(h->h_pin + kPubOff + 16 * (size_t)kDrawErrSlot) = 0;
  }
  if (pub_value<int>(h, kDrawErrSlot) != 0)
    return fail(h, O3DS_ERR_CAPACITY, "random_down_sample: an earlier draw on this handle found more than 2048 keys sharing 22 leading bits and kept nothing");
  o3ds::DrawState* st = h->d_draw;
  // The number kept is published like a VoxelDownSample's -- also when the input's size is known and the host could compute it: the record
  // is how a draw that failed on the device (draw_pick_kernel) reaches whoever asks for the result's size.
  // (the record FIRST: with all of them held, take_rec settles the oldest holder -- possibly `in`, whose size is exact from then on and
  // whose device word may be the very record handed out here; everything below reads `in` as it is afterwards)
  out.lazy_slot = take_rec(h);
  if (out.lazy_slot < 0) return fail(h, O3DS_ERR_CAPACITY, "random_down_sample: no record free for the size of the result");
  out.lazy_seq = ++h->rec_seq;
  const CountPub pub{cnt_word(h, out.lazy_slot), &(h->h_rec_dev + out.lazy_slot)->cnt, out.lazy_seq};
  const size_t bound = in.n;  // (an upper bound while the input's size is in flight)
  const size_t k_bound = (size_t)std::max(0, (int)(ratio * (double)bound));  // monotone in the size: at least the exact number
  const CountRef n_ref = count_ref(h, in);
  out.n = k_bound;
  out.n_lower = in.lazy_slot >= 0 ? (size_t)std::max(0, (int)(ratio * (double)in.n_lower)) : k_bound;
  if (k_bound == 0) {  // (the settled size keeps nothing)
    h->rec_owner[out.lazy_slot] = 0, out.lazy_slot = -1;
    return O3DS_OK;
  }
  int *flags = nullptr, *pos = nullptr;
  TMP_ALLOC(flags, sizeof(int) * (bound + 1));
  TMP_ALLOC(pos, sizeof(int) * (bound + 1));
  HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * k_bound));  // (before anything is launched: a draw whose result has nowhere to go is not started)
  if (in.nrm) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * k_bound));
  if (in.col) HIP_TRY(dev_alloc(h, (void**)&out.col, sizeof(P4) * k_bound));
  const unsigned int g = grid_for(bound);
  // (O3DS_DRAW_LIST_CAP in the A/B library: a smaller list, so that the overflow path can be walked by a test)
  // (read at every call, not once per process: the test that sets it shares its process with tests that draw before it)
  const char* cap_env = ab_getenv("O3DS_DRAW_LIST_CAP");
  const unsigned int list_cap = cap_env ? (unsigned int)std::max(0, std::min(atoi(cap_env), o3ds::kDrawListCap)) : (unsigned int)o3ds::kDrawListCap;
  draw_hist1_kernel<<<g, kBlock, 0, h->stream>>>(n_ref, seed, st);
  draw_hist2_kernel<<<g, kBlock, 0, h->stream>>>(n_ref, seed, ratio, st);
  draw_collect_kernel<<<g, kBlock, 0, h->stream>>>(n_ref, seed, st, list_cap);
  draw_pick_kernel<<<1, kBlock, 0, h->stream>>>(st, pub, pub_slot<int>(h, kDrawErrSlot), list_cap);
  draw_flag_kernel<<<grid_for(bound + 1), kBlock, 0, h->stream>>>(n_ref, seed, st, flags);
  int rc = exclusive_scan_int(h, flags, pos, bound + 1);
  if (rc) return rc;
  rc = compact_cloud<P4>(h, in, bound, flags, pos, 1, k_bound, &out.pts, &out.nrm, &out.col);
  if (rc) return rc;
  return O3DS_OK;
}

// behind o3ds_dense_map_carve, which checks its arguments: the voxels of `d` that the rays of scan `c` (placed by scan_pose; null: as it is) see through are erased
template <typename P4>
int dense_carve_t(o3ds_handle h, DenseRec& d, const CloudRec& c, const double* scan_pose, const double sp[3], double neighborhood_radius,
                  double max_raytracing_length, double truncation_distance, size_t* n_removed) {
  const size_t n = c.n;
  // removeDuplicatePointsWithinSameVoxels on the PLACED scan: keys of the placed points, stable sort, heads of the key segments
  CloudRec placed;
  CloudGuard placed_guard(h, placed);
  int rc = transform_t<P4>(h, c, scan_pose ? scan_pose : kIdentity16, placed);
  if (rc) return rc;
  unsigned long long *k0 = nullptr, *k1 = nullptr, *d_removed = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  int *first = nullptr, *mark = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(first, sizeof(int) * n);
  TMP_ALLOC(mark, sizeof(int) * d.cap);
  TMP_ALLOC(d_removed, sizeof(unsigned long long));
  CropDev none{};
  voxel_key_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)placed.pts, n, 1, 0.0, 0.0, 0.0, d.voxel, none, k0, v0);
  rc = sort_pairs(h, k0, k1, v0, v1, n);
  if (rc) return rc;
  first_of_voxel_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(k1, v1, n, first);
  HIP_TRY(hipMemsetAsync(mark, 0, sizeof(int) * d.cap, h->stream));
  HIP_TRY(hipMemsetAsync(d_removed, 0, sizeof(unsigned long long), h->stream));
  // rays are cast from the ALREADY PLACED points (identity here), so that the de-duplication and the rays see the same coordinates
  dense_carve_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)placed.pts, first, n, mat34(nullptr), sp[0], sp[1], sp[2], d.voxel,
                                                                neighborhood_radius, max_raytracing_length, truncation_distance, d.dev, mark);
  dense_erase_marked_kernel<<<grid_for(d.cap), kBlock, 0, h->stream>>>(d.dev, d.cap, mark, d_removed);
  HIP_TRY(hipGetLastError());
  unsigned long long removed = 0;
  rc = read_back(h, {{&removed, d_removed, sizeof(removed)}});
  if (rc) return rc;
  if (n_removed) *n_removed = (size_t)removed;
  return O3DS_OK;
}

// ---- neighbour queries and the outlier filters (neighbor_kernels.hpp) ---------------------------------------------------------------
// The classic grid index of a search target: the one the cloud has, whatever its cell (any cell gives the same lists, only slower), or a
// new one whose cell is chosen as normals_t chooses one -- a pilot grid, the mean number of points per occupied pilot cell, cell = pilot *
// sqrt(max_nn / (pi * mean)) -- with the pilot at radius / 8 and the clamp to [radius / 64, radius] of a bounded search, and for an
// unbounded one a pilot of the box's longest side / min(128, max(4, sqrt(n))) -- a small cloud gets a small grid: a list that cannot be
// filled walks all of it --, clamped to [pilot / 16, 16 pilot].  The new index stays with the cloud, marked as a by-product: a
// registration keeps it only if its cell suits.
template <typename P4>
int neighbor_index_t(o3ds_handle h, CloudRec& c, double radius, int max_nn) {
  if (c.has_index && c.cell_start && c.spts && c.grid.sx == c.grid.nx) return O3DS_OK;
  double pilot = radius / 8.0;
  if (!(radius > 0.0)) {
    if (!c.has_box) {
      double mn[3], mx[3];
      const int rb = bbox_of<P4>(h, (const P4*)c.pts, c.n, mn, mx);
      if (rb) return rb;
      c.has_box = true;
      c.box_padded = false;
      for (int a = 0; a < 3; ++a) c.bmn[a] = mn[a], c.bmx[a] = mx[a];
    }
    pilot = std::max(std::max(c.bmx[0] - c.bmn[0], c.bmx[1] - c.bmn[1]), c.bmx[2] - c.bmn[2]) / std::min(128.0, std::max(4.0, std::sqrt((double)c.n)));
    if (!(pilot > 0.0) || !std::isfinite(pilot)) pilot = 1.0;
  }
  int rc = build_index_t<P4>(h, c, pilot);
  if (rc) return rc;
  const size_t ncell = (size_t)c.grid.nx * c.grid.ny * c.grid.nz;
  unsigned long long* d_occ = nullptr;
  TMP_ALLOC(d_occ, sizeof(unsigned long long));
  HIP_TRY(hipMemsetAsync(d_occ, 0, sizeof(unsigned long long), h->stream));
  count_occupied_kernel<<<grid_for(ncell), kBlock, 0, h->stream>>>(c.cell_start, ncell, d_occ);
  unsigned long long occ = 0;
  rc = read_back(h, {{&occ, d_occ, sizeof(occ)}});
  if (rc) return rc;
  const double avg = occ ? (double)c.n / (double)occ : 1.0;
  double cell = c.grid.cell * std::sqrt(std::max(1.0, (double)max_nn) / (3.14159265358979 * avg));
  cell = radius > 0.0 ? std::min(std::max(cell, radius / 64.0), radius) : std::min(std::max(cell, pilot / 16.0), pilot * 16.0);
  rc = build_index_t<P4>(h, c, cell);
  if (rc) return rc;
  c.index_byproduct = true;
  return O3DS_OK;
}

// The search of `nq` queries (points d_qidx[0..nq) of `q`, null: its points in order; moved by T if given) in `t`, results in device arrays:
// d_idx / d_d2 [nq * max_nn] (either may be null), d_cnt [nq], d_tot [nq] (null: not wanted, and a bounded search may stop at its
// max_nn-th key), d_avg [nq] (null: not wanted).  *empty: the target has no point with three finite coordinates -- nothing was launched,
// every list is empty.  It comes in two halves (neighbor_launch_t is both), for a caller that searches one target many times (the coloured
// registration's passes): neighbor_prepare_t, what the target needs once -- the count of its finite points, read back, and its index --,
// and neighbor_run_t, the launch.
template <typename P4>
int neighbor_prepare_t(o3ds_handle h, CloudRec& t, size_t nq, int max_nn, double radius, unsigned int** d_fin_out, bool* empty) {
  *empty = true;
  *d_fin_out = nullptr;
  if (t.n == 0 || nq == 0) return O3DS_OK;
  unsigned int* d_fin = nullptr;
  TMP_ALLOC(d_fin, sizeof(unsigned int));
  HIP_TRY(hipMemsetAsync(d_fin, 0, sizeof(unsigned int), h->stream));
  count_finite_kernel<P4><<<grid_for(t.n), kBlock, 0, h->stream>>>((const P4*)t.pts, t.n, d_fin);
  unsigned int n_fin = 0;
  int rc = read_back(h, {{&n_fin, d_fin, sizeof(n_fin)}});
  if (rc) return rc;
  if (n_fin == 0) return O3DS_OK;
  rc = neighbor_index_t<P4>(h, t, radius, max_nn);
  if (rc) return rc;
  *d_fin_out = d_fin;
  *empty = false;
  return O3DS_OK;
}
template <typename P4>
int neighbor_run_t(o3ds_handle h, const CloudRec& q, const CloudRec& t, const double* T, const uint32_t* d_qidx, size_t nq, int max_nn, double radius,
                   const unsigned int* d_fin, uint32_t* d_idx, double* d_d2, uint32_t* d_cnt, uint32_t* d_tot, double* d_avg) {
  const unsigned int gsz = (unsigned int)((nq + kNbrQueriesPerBlock - 1) / kNbrQueriesPerBlock);
  const Mat34 M = mat34(T);
  const P4* qp = (const P4*)q.pts;  // (q may be t: its points did not move)
  const P4* sp = (const P4*)t.spts;
  span_mark(h, kSpanNeighborKernel);
  if (max_nn <= 32)
    neighbor_kernel<P4, 32><<<gsz, 64, 0, h->stream>>>(qp, d_qidx, nq, T ? 1 : 0, M, t.grid, sp, max_nn, radius, d_tot ? 1 : 0, d_fin, d_idx, d_d2, d_cnt,
                                                      d_tot, d_avg);
  else
    neighbor_kernel<P4, 128><<<gsz, 64, 0, h->stream>>>(qp, d_qidx, nq, T ? 1 : 0, M, t.grid, sp, max_nn, radius, d_tot ? 1 : 0, d_fin, d_idx, d_d2, d_cnt,
                                                       d_tot, d_avg);
  span_mark(h, kSpanNeighborKernel);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}
template <typename P4>
int neighbor_launch_t(o3ds_handle h, const CloudRec& q, CloudRec& t, const double* T, const uint32_t* d_qidx, size_t nq, int max_nn, double radius,
                      uint32_t* d_idx, double* d_d2, uint32_t* d_cnt, uint32_t* d_tot, double* d_avg, bool* empty) {
  unsigned int* d_fin = nullptr;
  const int rc = neighbor_prepare_t<P4>(h, t, nq, max_nn, radius, &d_fin, empty);
  if (rc || *empty) return rc;
  return neighbor_run_t<P4>(h, q, t, T, d_qidx, nq, max_nn, radius, d_fin, d_idx, d_d2, d_cnt, d_tot, d_avg);
}

// The subset of `in` that flags[0..n) keeps (flags[n] = 0, the scan's sentinel), as the new cloud `out`: the croppers' scan and stable
// compaction (points, normals and colours in cloud order), the kept indices on request.  pos: n + 1 ints of scratch.
template <typename P4>
int compact_kept_t(o3ds_handle h, CloudRec& in, size_t n, const int* flags, int* pos, const char* what, CloudRec& out, uint32_t* kept_idx, size_t capacity,
                   size_t* n_kept) {
  out.precision = in.precision;
  out.n = 0;
  box_copy(out, in);  // a subset
  *n_kept = 0;
  if (n == 0) return O3DS_OK;
  uint32_t* d_kept = nullptr;
  int rc = exclusive_scan_int(h, flags, pos, n + 1, pub_slot<int>(h, 0));
  if (rc) return rc;
  rc = wait_stream(h);
  if (rc) return rc;
  const int total = pub_value<int>(h, 0);
  *n_kept = (size_t)total;
  if (kept_idx && (size_t)total > capacity)
    return fail(h, O3DS_ERR_CAPACITY, std::string(what) + ": kept_idx is too small for the kept points (*n_kept holds their number)");
  out.n = (size_t)total;
  if (total > 0) {
    rc = compact_cloud<P4>(h, in, n, flags, pos, 1, out.n, &out.pts, &out.nrm, &out.col);
    if (rc) return rc;
    if (kept_idx) {
      TMP_ALLOC(d_kept, sizeof(uint32_t) * (size_t)total);
      kept_index_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(flags, pos, n, d_kept);
      HIP_TRY(hipGetLastError());
      rc = d2h_copy(h, kept_idx, d_kept, sizeof(uint32_t) * (size_t)total);
      if (rc) return rc;
    }
  }
  return O3DS_OK;
}
// A filter that judges point by point states its rule, rule(n, flags) for n > 0 points: flags[0..n) = 1 where a point stays
template <typename P4, typename Rule>
int filter_cloud_t(o3ds_handle h, CloudRec& in, const char* what, CloudRec& out, uint32_t* kept_idx, size_t capacity, size_t* n_kept, Rule&& rule) {
  const size_t n = in.n;
  int *flags = nullptr, *pos = nullptr;
  *n_kept = 0;  // (also when the rule fails)
  if (n) {
    TMP_ALLOC(flags, sizeof(int) * (n + 1));
    TMP_ALLOC(pos, sizeof(int) * (n + 1));
    const int rc = rule(n, flags);
    if (rc) return rc;
  }
  return compact_kept_t<P4>(h, in, n, flags, pos, what, out, kept_idx, capacity, n_kept);
}

// [O3D] RemoveStatisticalOutliers (mode 0: k = nb_neighbors, v = std_ratio) and RemoveRadiusOutliers (mode 1: k = nb_points, v = radius):
// the search with the cloud as its own target, the mask, the croppers' stable compaction
template <typename P4>
int outlier_filter_t(o3ds_handle h, CloudRec& in, int mode, int k, double v, CloudRec& out, uint32_t* kept_idx, size_t capacity, size_t* n_kept) {
  return filter_cloud_t<P4>(h, in, "outlier filter", out, kept_idx, capacity, n_kept, [&](size_t n, int* flags) -> int {
    uint32_t *d_cnt = nullptr, *d_tot = nullptr;
    double *d_avg = nullptr, *partial = nullptr, *stat = nullptr;
    TMP_ALLOC(d_cnt, sizeof(uint32_t) * n);
    bool empty = false;
    int rc;
    if (mode == 0) {
      TMP_ALLOC(d_avg, sizeof(double) * n);
      TMP_ALLOC(partial, sizeof(double) * 2 * kCenterChunks);
      TMP_ALLOC(stat, sizeof(double) * 4);
      rc = neighbor_launch_t<P4>(h, in, in, nullptr, nullptr, n, k, 0.0, nullptr, nullptr, d_cnt, nullptr, d_avg, &empty);
      if (rc) return rc;
      if (empty) HIP_TRY(hipMemsetAsync(d_avg, 0, sizeof(double) * n, h->stream));  // no list, no valid point
      stat_partial_kernel<<<kCenterChunks, kBlock, 0, h->stream>>>(d_avg, n, nullptr, partial);
      stat_finish_kernel<<<1, kBlock, 0, h->stream>>>(partial, 0, v, stat);
      stat_partial_kernel<<<kCenterChunks, kBlock, 0, h->stream>>>(d_avg, n, stat, partial);
      stat_finish_kernel<<<1, kBlock, 0, h->stream>>>(partial, 1, v, stat);
      stat_flag_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(d_avg, n, stat, flags);
    } else {
      TMP_ALLOC(d_tot, sizeof(uint32_t) * n);
      rc = neighbor_launch_t<P4>(h, in, in, nullptr, nullptr, n, 0, v, nullptr, nullptr, d_cnt, d_tot, nullptr, &empty);
      if (rc) return rc;
      if (empty) HIP_TRY(hipMemsetAsync(d_tot, 0, sizeof(uint32_t) * n, h->stream));
      radius_flag_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(d_tot, n, (uint32_t)k, flags);
    }
    HIP_TRY(hipGetLastError());
    return O3DS_OK;
  });
}

int outlier_filter(o3ds_handle h, o3ds_cloud in, int mode, int k, double v, const char* what, o3ds_cloud* out, uint32_t* kept_idx, size_t capacity,
                   size_t* n_kept) {
  CloudRec* c = find_cloud(h, in);  // (with its exact size; a persistent map as its array)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown cloud id");
  if (!out || !n_kept) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": out and n_kept are required");
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(c->precision, outlier_filter_t, h, *c, mode, k, v, o, kept_idx, capacity, n_kept); });
}
}  // namespace

extern "C" {

int o3ds_crop_cloud(o3ds_handle h, o3ds_cloud in, const o3ds_crop* crop, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, in);
  if (!c || !out) return fail(h, O3DS_ERR_INVALID_ARG, "crop_cloud: bad argument");
  const CropDev cd = to_dev(crop);
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(c->precision, crop_t, h, *c, cd, o); });
}

int o3ds_voxel_down_sample(o3ds_handle h, o3ds_cloud in, double voxel_size, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, in);
  if (!c || !out) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_down_sample: bad argument");
  return new_cloud(h, out, [&](CloudRec& o) {
    if (voxel_size <= 0.0) {  // o3d_slam::voxelize returns the cloud unchanged (helpers.cpp:108-110)
      o.precision = c->precision;
      return DISPATCH(c->precision, append_t, h, o, *c);
    }
    CropDev none{};
    return DISPATCH(c->precision, voxel_reduce_t, h, *c, 0, voxel_size, none, o);
  });
}

int o3ds_crop_voxel_down_sample(o3ds_handle h, o3ds_cloud in, const o3ds_crop* crop, double voxel_size, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  if (!(voxel_size > 0.0)) return o3ds_crop_cloud(h, in, crop, out);  // o3d_slam::voxelize leaves the cropped cloud as it is
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, in);
  if (!c || !out) return fail(h, O3DS_ERR_INVALID_ARG, "crop_voxel_down_sample: bad argument");
  const CropDev cd = to_dev(crop);
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(c->precision, voxel_reduce_t, h, *c, 0, voxel_size, cd, o, true); });
}

int o3ds_estimate_normals(o3ds_handle h, o3ds_cloud id, double radius, int max_nn) {
  CHECK_HANDLE(h);
  drop_fpfh(h, id);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud_lazy(h, id);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "estimate_normals: unknown cloud id");
  if (!(radius > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "maxRadiusNormalEstimation_ must be > 0");  // CloudRegistration.cpp:50
  if (max_nn <= 0) return fail(h, O3DS_ERR_INVALID_ARG, "knnNormalEstimation_ must be > 0");              // CloudRegistration.cpp:51
  if (max_nn > 128) return fail(h, O3DS_ERR_INVALID_ARG, "estimate_normals: max_nn > 128 unsupported");
  if (c->pm) {  // normals_t reads pts[0..n) as an array: a persistent submap is folded into the reference's array first (o3ds_backend.h)
    const int re = pm_exit(h, *c);
    if (re) return re;
  }
  return DISPATCH(c->precision, normals_t, h, *c, radius, max_nn);
}

int o3ds_select_by_index(o3ds_handle h, o3ds_cloud in, const uint32_t* keep_idx, size_t m, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, in);
  if (!c || !out || (m && !keep_idx)) return fail(h, O3DS_ERR_INVALID_ARG, "select_by_index: bad argument");
  for (size_t i = 0; i < m; ++i)
    if (keep_idx[i] >= c->n) return fail(h, O3DS_ERR_INVALID_ARG, "select_by_index: index out of range");
  return new_cloud(h, out, [&](CloudRec& o) -> int {
    o.precision = c->precision;
    o.n = m;
    box_copy(o, *c);  // a subset
    if (m) {
      uint32_t* d_idx = nullptr;
      TMP_ALLOC(d_idx, sizeof(uint32_t) * m);
      HIP_TRY(hipMemcpyAsync(d_idx, keep_idx, sizeof(uint32_t) * m, hipMemcpyHostToDevice, h->stream));
      const int rc = DISPATCH(c->precision, gather_cloud, h, *c, d_idx, m, o);
      if (rc) return rc;
      HIP_TRY(hipStreamSynchronize(h->stream));  // keep_idx may be released by the caller
    }
    return O3DS_OK;
  });
}

int o3ds_random_down_sample(o3ds_handle h, o3ds_cloud in, double ratio, uint64_t seed, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud_lazy(h, in);
  if (!c || !out) return fail(h, O3DS_ERR_INVALID_ARG, "random_down_sample: bad argument");
  if (c->pm) return fail(h, O3DS_ERR_INVALID_ARG, "random_down_sample: the cloud is a map");
  if (!(ratio >= 0.0 && ratio <= 1.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "[RandomDownSample] Illegal sampling_ratio, sampling_ratio must be between 0 and 1.");  // [O3D]
  HIP_TRY(hipSetDevice(h->device));
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(c->precision, random_down_sample_t, h, *c, ratio, (unsigned long long)seed, o); });
}

int o3ds_transform_cloud(o3ds_handle h, o3ds_cloud in, const double T[16], o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, in);
  if (!c || !out || !T) return fail(h, O3DS_ERR_INVALID_ARG, "transform_cloud: bad argument");
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(c->precision, transform_t, h, *c, T, o); });
}

int o3ds_cloud_center(o3ds_handle h, o3ds_cloud cloud, double center[3]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud_lazy(h, cloud);  // (the size may still be on its way: the kernels read it from the device word)
  if (!c || !center) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_center: bad argument");
  if (c->pm) {  // a submap in its persistent form: the mean of the reference's array (the sum's order is the array's)
    const int rc = pm_exit(h, *c);
    if (rc) return rc;
  }
  if (c->n == 0) {  // (n is an upper bound: zero is exact)
    center[0] = center[1] = center[2] = 0.0;
    return O3DS_OK;
  }
  double *partial = nullptr, *d_out = nullptr;
  TMP_ALLOC(partial, sizeof(double) * 3 * kCenterChunks);
  TMP_ALLOC(d_out, sizeof(double) * 3);
  const CountRef cnt = count_ref(h, *c);
  WITH_P4(c->precision, center_partial_kernel<P4><<<kCenterChunks, kBlock, 0, h->stream>>>((const P4*)c->pts, cnt, partial));
  center_finish_kernel<<<1, kBlock, 0, h->stream>>>(partial, cnt, d_out);
  HIP_TRY(hipGetLastError());
  return read_back(h, {{center, d_out, sizeof(double) * 3}});
}

int o3ds_neighbor_search(o3ds_handle h, o3ds_cloud queries, o3ds_cloud target, const double T[16], const uint32_t* query_idx, size_t n_queries, int max_nn,
                         double radius, uint32_t* idx, double* d2, uint32_t* count, uint32_t* total) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (max_nn < 0) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: max_nn < 0");
  if (max_nn > 128) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: max_nn > 128 unsupported");
  if (radius != radius) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: the radius is not a number");
  if (max_nn == 0 && !(radius > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: a count (max_nn == 0) needs a radius > 0");
  if ((max_nn == 0) != (idx == nullptr)) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: idx is NULL iff max_nn == 0");
  if (max_nn == 0 && d2) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: d2 without a list (max_nn == 0)");
  if (n_queries && !count) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: count is required");
  CloudRec* q = find_cloud(h, queries);  // (exact sizes; a persistent map as its array)
  if (!q) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: unknown query cloud id");
  CloudRec* t = find_cloud(h, target);
  if (!t) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: unknown target cloud id");
  if (q->precision != t->precision) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: the clouds have different storage types");
  if (!query_idx && n_queries != q->n) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: without query_idx, n_queries is the size of the query cloud");
  for (size_t i = 0; query_idx && i < n_queries; ++i)
    if (query_idx[i] >= q->n) return fail(h, O3DS_ERR_INVALID_ARG, "neighbor_search: query_idx out of range");
  if (n_queries == 0) return O3DS_OK;
  const size_t rows = n_queries * (size_t)max_nn;
  uint32_t *d_qidx = nullptr, *d_idx = nullptr, *d_cnt = nullptr, *d_tot = nullptr;
  double* d_d2 = nullptr;
  if (query_idx) {
    TMP_ALLOC(d_qidx, sizeof(uint32_t) * n_queries);
    const int rc = h2d_copy(h, d_qidx, query_idx, sizeof(uint32_t) * n_queries);
    if (rc) return rc;
  }
  if (idx) TMP_ALLOC(d_idx, sizeof(uint32_t) * rows);
  if (d2) TMP_ALLOC(d_d2, sizeof(double) * rows);
  TMP_ALLOC(d_cnt, sizeof(uint32_t) * n_queries);
  if (total) TMP_ALLOC(d_tot, sizeof(uint32_t) * n_queries);
  bool empty = false;
  int rc = DISPATCH(t->precision, neighbor_launch_t, h, *q, *t, T, d_qidx, n_queries, max_nn, radius, d_idx, d_d2, d_cnt, d_tot, nullptr, &empty);
  if (rc) return rc;
  if (empty) {  // an empty target is not an error: every list is empty
    HIP_TRY(hipStreamSynchronize(h->stream));  // (query_idx may be released by the caller)
    if (idx) memset(idx, 0, sizeof(uint32_t) * rows);
    if (d2) memset(d2, 0, sizeof(double) * rows);
    memset(count, 0, sizeof(uint32_t) * n_queries);
    if (total) memset(total, 0, sizeof(uint32_t) * n_queries);
    return O3DS_OK;
  }
  if (idx) rc = d2h_copy(h, idx, d_idx, sizeof(uint32_t) * rows);
  if (!rc && d2) rc = d2h_copy(h, d2, d_d2, sizeof(double) * rows);
  if (!rc) rc = d2h_copy(h, count, d_cnt, sizeof(uint32_t) * n_queries);
  if (!rc && total) rc = d2h_copy(h, total, d_tot, sizeof(uint32_t) * n_queries);
  return rc;
}

int o3ds_remove_statistical_outliers(o3ds_handle h, o3ds_cloud in, int nb_neighbors, double std_ratio, o3ds_cloud* out, uint32_t* kept_idx, size_t capacity,
                                     size_t* n_kept) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (nb_neighbors < 1 || !(std_ratio > 0.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "[RemoveStatisticalOutliers] Illegal input parameters, the number of neighbors and standard deviation ratio must be positive.");  // [O3D]
  if (nb_neighbors > 128) return fail(h, O3DS_ERR_INVALID_ARG, "remove_statistical_outliers: nb_neighbors > 128 unsupported");
  return outlier_filter(h, in, 0, nb_neighbors, std_ratio, "remove_statistical_outliers", out, kept_idx, capacity, n_kept);
}

int o3ds_remove_radius_outliers(o3ds_handle h, o3ds_cloud in, int nb_points, double radius, o3ds_cloud* out, uint32_t* kept_idx, size_t capacity,
                                size_t* n_kept) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (nb_points < 1 || !(radius > 0.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "[RemoveRadiusOutliers] Illegal input parameters, number of points and radius must be positive.");  // [O3D]
  return outlier_filter(h, in, 1, nb_points, radius, "remove_radius_outliers", out, kept_idx, capacity, n_kept);
}

int o3ds_cloud_append(o3ds_handle h, o3ds_cloud map, o3ds_cloud add) {
  CHECK_HANDLE(h);
  drop_fpfh(h, map);
  ArenaScope arena_scope(h);
  CloudRec* m = find_cloud(h, map);
  CloudRec* a = find_cloud(h, add);
  if (!m || !a || m == a) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_append: bad cloud id");
  if (m->n && a->n && m->precision != a->precision) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_append: precision mismatch");
  if (m->n == 0) m->precision = a->precision;
  return DISPATCH(m->precision, append_t, h, *m, *a);
}

int o3ds_cloud_copy_across(o3ds_handle dst, o3ds_handle src, o3ds_cloud src_cloud, o3ds_cloud* out) {
  o3ds_handle h = dst;
  CHECK_HANDLE(h);
  if (!src || !out) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_copy_across: bad argument");
  if (src == dst) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_copy_across: source and destination handle are the same (use the cloud itself)");
  if (src->device != dst->device) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_copy_across: the handles live on different devices");
  CloudRec* c = find_cloud(src, src_cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_copy_across: unknown cloud id on the source handle");
  if (c->n && c->precision != dst->precision) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_copy_across: the handles store points in different precisions");
  return new_cloud(h, out, [&](CloudRec& o) -> int {
    o.precision = c->n ? c->precision : dst->precision;
    o.n = c->n;
    box_copy(o, *c);
    if (c->n == 0) return O3DS_OK;
    // what the source handle queued for this cloud must have happened before the copy reads it: the destination stream waits for
    // an event on the source stream (no host wait); the source cloud must stay alive until the destination stream passed the copy,
    // which the synchronisation below guarantees before this returns
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, src->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
    (void)hipEventDestroy(ev);  // released once it has completed
    HIP_TRY(e);
    const int rc = copy_arrays(h, o, c->n, c->pts, c->nrm, c->col);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return O3DS_OK;
  });
}

int o3ds_cloud_export_view(o3ds_handle h, o3ds_cloud id, o3ds_cloud_view* out) {
  CHECK_HANDLE(h);
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_export_view: null view");
  memset(out, 0, sizeof(*out));
  CloudRec* c = find_cloud(h, id);  // (the exact size; a persistent map is folded: a view is of arrays)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_export_view: unknown cloud id");
  HIP_TRY(hipSetDevice(h->device));
  out->pts = c->pts, out->nrm = c->nrm, out->col = c->col;
  out->n = c->n;
  out->precision = c->n ? c->precision : h->precision;
  out->device = h->device;
  out->has_box = c->has_box ? (c->box_padded ? 2 : 1) : 0;
  for (int a = 0; a < 3; ++a) out->box_min[a] = c->bmn[a], out->box_max[a] = c->bmx[a];
  if (c->n) {  // behind everything this handle has queued for the cloud so far
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const hipError_t e = hipEventRecord(ev, h->stream);
    if (e != hipSuccess) {
      (void)hipEventDestroy(ev);
      HIP_TRY(e);
    }
    out->event = ev;
  }
  return O3DS_OK;
}

int o3ds_cloud_view_release(o3ds_cloud_view* view) {
  if (view && view->event) (void)hipEventDestroy((hipEvent_t)view->event);
  if (view) memset(view, 0, sizeof(*view));
  return O3DS_OK;
}

int o3ds_cloud_import_view(o3ds_handle h, const o3ds_cloud_view* v, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!v || !out) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_import_view: null argument");
  if (v->device != h->device) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_import_view: the view's cloud lives on another device");
  if (v->n && v->precision != h->precision) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_import_view: the view's cloud is stored in another precision");
  if (v->n && (!v->pts || !v->event)) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_import_view: a released or incomplete view");
  HIP_TRY(hipSetDevice(h->device));
  return new_cloud(h, out, [&](CloudRec& o) -> int {
    o.precision = h->precision;
    o.n = v->n;
    o.has_box = v->has_box != 0;
    o.box_padded = v->has_box == 2;
    for (int a = 0; a < 3; ++a) o.bmn[a] = v->box_min[a], o.bmx[a] = v->box_max[a];
    if (v->n == 0) return O3DS_OK;
    HIP_TRY(hipStreamWaitEvent(h->stream, (hipEvent_t)v->event, 0));  // what the owner queued for the cloud before it exported the view
    const int rc = copy_arrays(h, o, v->n, v->pts, v->nrm, v->col);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));  // the owner may free its cloud as soon as this returns
    return O3DS_OK;
  });
}

}  // extern "C" (a helper with default arguments follows)
namespace {
// voxelizeWithinCroppingVolume of a device cloud in place; merge_np >= 0: the cloud is [pass block | voxel block in key order | new points]
int voxelize_within_volume_impl(o3ds_handle h, o3ds_cloud map, double voxel_size, const o3ds_crop* crop, long long merge_np = -1, size_t merge_nv = 0) {
  CloudRec* m = find_cloud(h, map);
  if (!m) return fail(h, O3DS_ERR_INVALID_ARG, "voxelize_within_volume: unknown cloud id");
  if (voxel_size <= 0.0 || m->n == 0) return O3DS_OK;  // helpers.cpp:119-123 / Submap.cpp:139: unchanged
  CloudRec o;
  CloudGuard o_guard(h, o);
  const CropDev cd = to_dev(crop);
  const int rc = DISPATCH(m->precision, voxel_reduce_t, h, *m, 1, voxel_size, cd, o, false, merge_np, merge_nv);
  if (rc) return rc;
  o_guard.release();
  free_cloud(h, *m);
  *m = o;
  return O3DS_OK;
}
}  // namespace

// ---- the persistent form of a submap (map_kernels.hpp): enter, insert, leave ------------------------------------------------------------
namespace {

#define PM_ALLOC(ptr, bytes)                                                                               \
  do {                                                                                                     \
    void* _p = nullptr;                                                                                    \
    if (dev_alloc(h, &_p, (size_t)(bytes)) != hipSuccess) return fail(h, O3DS_ERR_OOM, "persistent map: out of device memory"); \
    pm->blocks.push_back(_p);                                                                              \
    (ptr) = (decltype(ptr))_p;                                                                             \
  } while (0)

// cell edge of the row-paged index in voxels: the classic index uses max_corr / 4; here a whole number of voxels
int pm_cell_voxels(double max_corr_hint, double voxel) {
  const double want = max_corr_hint > 0.0 ? max_corr_hint / kIndexCellDiv : 2.5 * voxel;
  return std::max(1, (int)std::floor(want / voxel + 0.5));
}

// The map `c` -- an array [pass-through block | voxel block in key order] (vox_first / vox_count) with normals or without -- enters the
// persistent form.  O(N): history and voxel hash of every point, the row-paged search index.
template <typename P4>
int pm_enter_t(o3ds_handle h, CloudRec& c, double voxel, double max_corr_hint, size_t scan_upper) {
  const size_t n = c.n;
  PMapRec* pm = new PMapRec();
  c.pm = pm;  // (from here on free_cloud / pm_release own it)
  // room: half the map again and a few scans' worth
  const size_t want_cap = n + std::max<size_t>({n / 2, 16 * scan_upper, (size_t)1 << 18});
  if (c.cap < want_cap) {  // (entering costs a pass over the map anyway; room for half the map again makes the next capacity fold a rare event)
    void *np = nullptr, *nn = nullptr;
    HIP_TRY(dev_alloc(h, &np, sizeof(P4) * want_cap));
    HIP_TRY(hipMemcpyAsync(np, c.pts, sizeof(P4) * n, hipMemcpyDeviceToDevice, h->stream));
    if (c.nrm) {
      if (dev_alloc(h, &nn, sizeof(P4) * want_cap) != hipSuccess) {
        dev_free(h, np);
        return fail(h, O3DS_ERR_OOM, "persistent map: out of device memory");
      }
      HIP_TRY(hipMemcpyAsync(nn, c.nrm, sizeof(P4) * n, hipMemcpyDeviceToDevice, h->stream));
    }
    free_points(h, c);
    if (c.nrm) dev_free(h, c.nrm);
    c.pts = np;
    c.nrm = nn;
    c.cap = want_cap;
  }
  const size_t cap = c.cap;
  if (c.col) {  // the colour slots: always a block of their own size (an array's colours are allocated for its points, whatever room pts / nrm have)
    void* nc = nullptr;
    HIP_TRY(dev_alloc(h, &nc, sizeof(P4) * cap));
    HIP_TRY(hipMemcpyAsync(nc, c.col, sizeof(P4) * n, hipMemcpyDeviceToDevice, h->stream));
    dev_free(h, c.col);
    c.col = nc;
  }
  PmDev& d = pm->dev;
  d.pts = c.pts;
  d.nrm = c.nrm;
  d.col = c.col;
  d.cap = cap;
  PM_ALLOC(d.slot, sizeof(PmSlot) * cap);
  size_t hcap = 1024;
  while (hcap < 2 * cap) hcap <<= 1;
  PM_ALLOC(d.h, sizeof(PmHash) * hcap);
  d.hmask = (unsigned int)(hcap - 1);
  pm_hash_init_kernel<<<grid_for(hcap), kBlock, 0, h->stream>>>(d.h, hcap);
  d.list_cap = (int)std::min<size_t>(cap, 0x7fffffff);
  PM_ALLOC(d.counters, sizeof(int) * kPmCounters);
  for (int k = 0; k < 2; ++k) PM_ALLOC(d.unsettled[k], sizeof(int) * cap);
  PM_ALLOC(d.multi[0], sizeof(unsigned long long) * cap);
  d.multi[1] = nullptr;
  PM_ALLOC(d.complex_groups, sizeof(int) * cap);
  PM_ALLOC(d.outside_pts, sizeof(int) * cap);
  PM_ALLOC(d.relink, sizeof(int) * cap);
  PM_ALLOC(d.touched_rows, sizeof(int) * cap);
  PM_ALLOC(d.new_slots, sizeof(int) * cap);
  PM_ALLOC(pm->d_hist, sizeof(CropDev) * (kPmHistory + 1));
  d.hist = pm->d_hist;
  d.n_base = (int)n;
  d.np_base = (int)c.vox_first;
  d.voxel = voxel;
  d.inv_voxel = 1.0 / voxel;
  // the grid of the index: aligned with the voxel grid, over the map's box with a margin (points beyond it are clamped into the border cells,
  // as build_grid_t's cell_of does: slower to search, never wrong)
  if (!c.has_box) {
    double mn[3], mx[3];
    const int rb = bbox_of<P4>(h, (const P4*)c.pts, n, mn, mx);
    if (rb) return rb;
    c.has_box = true;
    c.box_padded = false;
    for (int a = 0; a < 3; ++a) c.bmn[a] = mn[a], c.bmx[a] = mx[a];
  }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(c.bmn[a]) || !std::isfinite(c.bmx[a])) return fail(h, O3DS_ERR_INVALID_ARG, "persistent map: non-finite coordinates");
  d.kc = pm_cell_voxels(max_corr_hint, voxel);
  double cell = d.kc * voxel;
  long long g0[3], gn[3];
  for (;;) {
    for (int a = 0; a < 3; ++a) {
      const double ext = c.bmx[a] - c.bmn[a];
      const double pad = a < 2 ? std::max(5.0, 0.1 * ext) : std::max(2.0, 0.1 * ext);
      const long long lo = (long long)std::floor((c.bmn[a] - pad) / cell), hi = (long long)std::floor((c.bmx[a] + pad) / cell);
      g0[a] = lo * d.kc;
      gn[a] = hi - lo + 1;
    }
    if ((double)gn[0] * (double)gn[1] * (double)gn[2] <= (double)kMaxCells / 2 && gn[0] < 5000) break;  // (pm_rows_kernel keeps three ints per cell of a row in LDS)
    d.kc *= 2;
    cell = d.kc * voxel;
  }
  for (int a = 0; a < 3; ++a)
    if (std::llabs(g0[a]) + gn[a] * d.kc >= (1ll << 20)) return fail(h, O3DS_ERR_INVALID_ARG, "persistent map: voxel coordinates beyond 2^20");
  d.gx0 = g0[0], d.gy0 = g0[1], d.gz0 = g0[2];
  GridDev g{};
  g.ox = (double)g0[0] * voxel;
  g.oy = (double)g0[1] * voxel;
  g.oz = (double)g0[2] * voxel;
  g.cell = cell;
  g.inv_cell = 1.0 / cell;
  g.nx = (int)gn[0], g.ny = (int)gn[1], g.nz = (int)gn[2];
  g.sx = g.nx + 1;
  pm->rows = (size_t)g.ny * g.nz;
  const size_t table = pm->rows * (size_t)g.sx;
  // the arrays of the index hang on the cloud (free_index): the registration uses them like any index
  free_index(h, c);
  int* cs = nullptr;
  HIP_TRY(dev_alloc(h, (void**)&cs, sizeof(int) * (table + 1 + 4)));
  c.cell_start = cs;
  const size_t pool = 6 * n + 16 * scan_upper + ((size_t)1 << 22);
  if (pool >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_OOM, "persistent map: index pool beyond 2^31 positions");
  if (pool > scan_capacity<P4>()) return fail(h, O3DS_ERR_CAPACITY, "persistent map: index pool beyond 2^32 bytes less the scan loop's slack (the search addresses it by 32-bit byte offsets)");
  HIP_TRY(dev_alloc(h, &c.spts, sizeof(P4) * pool + scan_slack_alloc()));
  c.spts_slack = scan_slack_alloc();
  {  // no position of the pool or of the slack behind it keeps what its block held before (pm_pool_clear_kernel)
    const size_t n_clear = pool + c.spts_slack / sizeof(P4);
    pm_pool_clear_kernel<P4><<<(unsigned)std::min<size_t>((n_clear + kBlock - 1) / kBlock, 8192), kBlock, 0, h->stream>>>((P4*)c.spts, n_clear);
  }
  if (c.nrm) HIP_TRY(dev_alloc(h, &c.snrm, sizeof(P4) * pool));
  PM_ALLOC(d.row_cap, sizeof(int) * pm->rows);
  PM_ALLOC(d.row_flag, sizeof(int) * pm->rows);
  PM_ALLOC(d.cell_add, sizeof(int) * (table + 1));
  HIP_TRY(hipMemsetAsync(d.cell_add, 0, sizeof(int) * (table + 1), h->stream));
  g.cell_start = cs;
  d.grid = g;
  d.cs = cs;
  d.spts = c.spts;
  d.snrm = c.snrm;
  d.pool_cap = (int)pool;
  int rc = cell_counters(h, table);  // build_grid_t's: counted up, scanned, counted back down to zero by the scatter
  if (rc) return rc;
  if (!h->d_cells) return fail(h, O3DS_ERR_OOM, "persistent map: cell counters allocation failed");
  HIP_TRY(hipMemsetAsync(d.counters, 0, sizeof(int) * kPmCounters, h->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(d.counters + kPmN), (int)n, 1, h->stream));
  int* cell_id = nullptr;
  TMP_ALLOC(cell_id, sizeof(int) * n);
  const int ni = (int)n;
  span_mark(h, kSpanIndexBuild);
  pm_enter_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(d, ni);
  pm_cell_count_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(d, ni, h->d_cells, cell_id);
  pm_row_slack_kernel<<<grid_for(pm->rows * 64), kBlock, 0, h->stream>>>(h->d_cells, (int)pm->rows, g.nx, d.row_cap, d.row_flag);
  rc = exclusive_scan_int(h, h->d_cells, cs, table + 1);
  if (rc) return rc;
  pm_row_finish_kernel<<<grid_for(pm->rows), kBlock, 0, h->stream>>>(h->d_cells, cs, (int)pm->rows, g.nx, d.counters + kPmPoolTop);
  pm_scatter_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(d, ni, cell_id, h->d_cells);
  // (the voxels with several members that pm_enter_kernel listed are what the first insertion looks at)
  HIP_TRY(hipMemcpyAsync(d.counters + kPmMultiIn, d.counters + kPmMultiOut, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  span_mark(h, kSpanIndexBuild);
  HIP_TRY(hipGetLastError());
  h->cells_clean = true;
  c.grid = g;
  c.has_index = true;
  c.index_byproduct = false;
  c.index_positions = pool;
  pm->t = 0;
  pm->n_upper = n;
  pm->live_lower = n;
  pm->pool_top = (double)(n + n / 2 + 8 * pm->rows);  // (an upper bound until the first record arrives: count + slack of every row)
  pm->rec_slot = take_rec(h);
  if (pm->rec_slot < 0) return fail(h, O3DS_ERR_CAPACITY, "persistent map: no record free for its counters");
  h->rec_owner[pm->rec_slot] = kRecOwnerMap;
  pm->rec_seq = 0;
  return O3DS_OK;
}

// what the latest record the insertions published says, if it has arrived (never waits unless `block`)
int pm_poll(o3ds_handle h, PMapRec* pm, bool block) {
  if (pm->rec_seq == 0) return O3DS_OK;
  volatile o3ds_context::PinRec* r = h->h_rec + pm->rec_slot;
  if (r->seq != pm->rec_seq) {
    if (!block) return O3DS_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (r->seq != pm->rec_seq) return fail(h, O3DS_ERR_HIP, "persistent map: an insertion never published its record");
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  const size_t slots = (size_t)r->cnt, dead = (size_t)r->box[1];
  if ((int)r->box[2] != 0) return fail(h, O3DS_ERR_CAPACITY, "persistent map: an internal capacity was exceeded (error " + std::to_string((int)r->box[2]) + ")");
  pm->n_upper = slots;
  pm->live_lower = slots - dead;
  pm->pool_top = r->box[0];
  pm->clamped = r->box[5];
  pm->multi_total = std::max(pm->multi_total, (double)r->box[3]);  // (a carve's record repeats the list's count; its removed points travel in PinRec::pad)
  pm->rec_seq = 0;  // consumed
  return O3DS_OK;
}

// Submap::insertScan's map += T * scan; voxelizeWithinCroppingVolume on the persistent form: six launches over the scan, nothing returns
template <typename P4>
int pm_insert_t(o3ds_handle h, CloudRec& c, const CloudRec& scan, const double T[16], const CropDev& crop) {
  PMapRec* pm = c.pm;
  PmDev d = pm->dev;
  const size_t ms = scan.n;  // (an upper bound when the scan's size is still in flight)
  const bool has_nrm = c.nrm != nullptr;
  const P4* scan_col = c.col ? (const P4*)scan.col : nullptr;  // (an uncoloured map ignores a scan's colours, as operator+= does)
  const int t_now = pm->t + 1;
  // scratch: the voxel table of VoxelDownSample, the chained scan's tiles
  VoxTable t{};
  size_t n_tiles = 0;
  const int rs = vox_scratch(h, ms, "map_insert_scan", &t, &n_tiles);
  if (rs) return rs;
  P4 *placed = nullptr, *placed_nrm = nullptr;
  int *lead_slot = nullptr, *run_next = nullptr, *run_len = nullptr, *order = nullptr, *d_groups = nullptr;
  uint32_t* starts = nullptr;
  int2* piece = nullptr;
  unsigned long long* group_key = nullptr;
  TMP_ALLOC(placed, sizeof(P4) * ms);
  if (has_nrm) TMP_ALLOC(placed_nrm, sizeof(P4) * ms);
  TMP_ALLOC(lead_slot, sizeof(int) * ms);
  TMP_ALLOC(run_next, sizeof(int) * ms);
  TMP_ALLOC(run_len, sizeof(int) * ms);
  TMP_ALLOC(order, sizeof(int) * ms);
  TMP_ALLOC(starts, sizeof(uint32_t) * ms);
  TMP_ALLOC(piece, sizeof(int2) * ms);
  TMP_ALLOC(group_key, sizeof(unsigned long long) * ms);
  TMP_ALLOC(d_groups, sizeof(int) * 16);
  const Mat34 M = mat34(T);
  if (++h->scan_gen == 0) h->scan_gen = 1;
  const CountRef n_scan = count_ref(h, scan);
  const CountPub groups_pub{d_groups, nullptr, 0};
  const CountRef groups{ms, d_groups};
  pm_place_kernel<P4><<<grid_for(ms), kBlock, 0, h->stream>>>((const P4*)scan.pts, has_nrm ? (const P4*)scan.nrm : nullptr, n_scan, M, T[3], T[7], T[11], T[15], crop, d, t,
                                                            placed, placed_nrm, lead_slot, run_next, run_len);
  vox_order_kernel<<<(unsigned int)n_tiles, kBlock, 0, h->stream>>>(lead_slot, n_scan, t, h->d_tiles, h->d_ticket, h->ticket_base, h->scan_gen, order, groups_pub);
  h->ticket_base += (unsigned int)n_tiles;
  pm_group_kernel<P4><<<grid_for(ms), kBlock, 0, h->stream>>>(d, groups, order, run_next, run_len, starts, piece, placed, placed_nrm, scan_col, t, crop, t_now, group_key);
  h->voxtab_clean = true;
  pm_merge_kernel<P4><<<512, 64, 0, h->stream>>>(d, piece, run_next, run_len, placed, placed_nrm, scan_col, group_key, crop, t_now);
  pm_misc_kernel<P4><<<256, kBlock, 0, h->stream>>>(d, placed, placed_nrm, scan_col, crop, t_now);
  const unsigned int row_blocks = (unsigned int)std::min<size_t>(std::max<size_t>(ms / 8, 64), 2048);
  pm_rows_kernel<P4><<<row_blocks, kBlock, sizeof(int) * 3 * (size_t)(d.grid.nx + 1), h->stream>>>(d);
  pm_place_new_kernel<P4><<<grid_for(ms), kBlock, 0, h->stream>>>(d);
  pm->rec_seq = ++h->rec_seq;
  o3ds_context::PinRec* rec = h->h_rec_dev + pm->rec_slot;
  const CountPub pub{cnt_word(h, pm->rec_slot), &rec->cnt, pm->rec_seq};
  pm_turn_kernel<<<1, 64, 0, h->stream>>>(d, pub, pm->d_hist, crop, t_now, rec->box);
  HIP_TRY(hipGetLastError());
  // the lists trade places for the next insertion
  std::swap(pm->dev.unsettled[0], pm->dev.unsettled[1]);
  pm->t = t_now;
  pm->n_upper += ms;
  c.n = pm->n_upper;
  return O3DS_OK;
}

// the reference's array back: [pass-through block in original order | voxel block in key order], then the ordinary cloud it was
template <typename P4>
int pm_exit_t(o3ds_handle h, CloudRec& c) {
  PMapRec* pm = c.pm;
  int rc = pm_poll(h, pm, true);
  if (rc) return rc;
  int counters[kPmCounters];
  rc = read_back(h, {{counters, pm->dev.counters, sizeof(counters)}});
  if (rc) return rc;
  if (counters[kPmError]) return fail(h, O3DS_ERR_CAPACITY, "persistent map: an internal capacity was exceeded (error " + std::to_string(counters[kPmError]) + ")");
  const size_t n = (size_t)counters[kPmN], live = n - (size_t)counters[kPmDeadCnt];
  unsigned long long *hi = nullptr, *lo = nullptr, *k1 = nullptr, *d_np = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  TMP_ALLOC(hi, sizeof(unsigned long long) * n);
  TMP_ALLOC(lo, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(d_np, sizeof(unsigned long long));
  HIP_TRY(hipMemsetAsync(d_np, 0, sizeof(unsigned long long), h->stream));
  pm_view_key_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(pm->dev, (int)n, pm->t, hi, lo, v0, d_np);
  // order by (hi, lo): two stable sorts, least significant key first
  SortTemp temp;  // (one temporary serves both sorts)
  rc = sort_pairs(h, lo, k1, v0, v1, n, 64, &temp);
  if (rc) return rc;
  pm_gather_u64_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(hi, v1, n, lo);  // lo := hi in the order of the first sort
  rc = sort_pairs(h, lo, k1, v1, v0, n, 64, &temp);
  if (rc) return rc;
  unsigned long long n_pass = 0;
  rc = read_back(h, {{&n_pass, d_np, sizeof(n_pass)}});
  if (rc) return rc;
  const size_t room = live + std::max<size_t>(live / 4, (size_t)1 << 18);
  void *np = nullptr, *nn = nullptr, *nc = nullptr;
  if (live > 0) {
    HIP_TRY(dev_alloc(h, &np, sizeof(P4) * room));
    if ((c.nrm && dev_alloc(h, &nn, sizeof(P4) * room) != hipSuccess) || (c.col && dev_alloc(h, &nc, sizeof(P4) * live) != hipSuccess)) {
      dev_free(h, np);
      if (nn) dev_free(h, nn);
      return fail(h, O3DS_ERR_OOM, "persistent map: out of device memory");
    }
    pm_permute_kernel<P4><<<grid_for(live), kBlock, 0, h->stream>>>((const P4*)c.pts, (const P4*)c.nrm, (const P4*)c.col, v0, live, (P4*)np, (P4*)nn, (P4*)nc);
    HIP_TRY(hipGetLastError());
  }
  pm_release(h, c);
  replace_arrays(h, c, np, nn, nc, live, live > 0 ? room : 0);
  c.vox_first = (long long)n_pass;
  c.vox_count = live - (size_t)n_pass;
  return O3DS_OK;
}

}  // namespace

namespace {
int pm_exit(o3ds_handle h, CloudRec& c) {
  if (!c.pm) return O3DS_OK;
  ArenaScope arena_scope(h);
  return DISPATCH(c.precision, pm_exit_t, h, c);
}
}  // namespace

extern "C" {

int o3ds_voxelize_within_volume(o3ds_handle h, o3ds_cloud map, double voxel_size, const o3ds_crop* crop) {
  CHECK_HANDLE(h);
  drop_fpfh(h, map);
  ArenaScope arena_scope(h);
  return voxelize_within_volume_impl(h, map, voxel_size, crop);
}

int o3ds_cloud_undistort(o3ds_handle h, o3ds_cloud cloud, const double linear_velocity[3], const double angular_velocity_rpy[3],
                         double scan_duration, int spinning_clockwise) {
  CHECK_HANDLE(h);
  drop_fpfh(h, cloud);
  CloudRec* c = find_cloud(h, cloud);
  if (!c || !linear_velocity || !angular_velocity_rpy) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_undistort: bad argument");
  if (!(scan_duration > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "lidar scanDuration_: must be > 0");  // MotionCompensation.cpp:62
  if (c->n == 0) return O3DS_OK;
  const double* v = linear_velocity;
  const double* w = angular_velocity_rpy;
  WITH_P4(c->precision, undistort_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>((P4*)c->pts, c->n, v[0], v[1], v[2], w[0], w[1], w[2], scan_duration,
                                                                                        spinning_clockwise));
  HIP_TRY(hipGetLastError());
  c->vox_first = -1;  // the points moved
  if (c->nrm) {
    dev_free(h, c->nrm);
    c->nrm = nullptr;
  }
  free_index(h, *c);
  c->has_box = false;  // the points moved
  drop_ingest_box(h, *c);  // ... and so did the box the ingest reduced
  return O3DS_OK;
}

int o3ds_dense_map_create(o3ds_handle h, double voxel_size, o3ds_dense_map* out) {
  CHECK_HANDLE(h);
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_create: null out");
  if (!(voxel_size > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_create: voxel_size must be > 0");
  DenseRec d;
  d.voxel = voxel_size;
  const uint64_t id = h->next_id++;
  h->dense_maps.emplace(id, d);
  *out = id;
  return O3DS_OK;
}

int o3ds_dense_map_free(o3ds_handle h, o3ds_dense_map id) {
  CHECK_HANDLE(h);
  auto it = h->dense_maps.find(id);
  if (it == h->dense_maps.end()) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_free: unknown id");
  (void)hipStreamSynchronize(h->stream);
  dense_release(h, it->second);
  h->dense_maps.erase(it);
  return O3DS_OK;
}

int o3ds_dense_map_insert(o3ds_handle h, o3ds_dense_map id, o3ds_cloud cloud, const double T[16]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  auto it = h->dense_maps.find(id);
  CloudRec* c = find_cloud(h, cloud);
  if (it == h->dense_maps.end() || !c) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_insert: unknown id");
  return DISPATCH(c->precision, dense_insert_t, h, it->second, *c, T);
}

extern "C++" {
namespace {
template <typename P4>
int export_rows_t(o3ds_handle h, const CloudRec& c, const double T[16], double voxel, int world, double* d_rows, long long* d_counts) {
  const Mat34 M = mat34(T);  // (null: the kernels are told not to place the points)
  HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(long long) * (size_t)world, h->stream));
  if (c.n == 0) return O3DS_OK;
  int* owner = nullptr;
  unsigned long long* offsets = nullptr;
  TMP_ALLOC(owner, sizeof(int) * c.n);
  TMP_ALLOC(offsets, sizeof(unsigned long long) * 2 * (size_t)world);
  owner_count_kernel<P4><<<grid_for(c.n), kBlock, 0, h->stream>>>((const P4*)c.pts, c.n, M, T ? 1 : 0, 1.0 / voxel, world, owner, d_counts);
  owner_offsets_kernel<<<1, 64, 0, h->stream>>>(d_counts, world, offsets);
  owner_scatter_kernel<P4><<<grid_for(c.n), kBlock, 0, h->stream>>>((const P4*)c.pts, (const P4*)c.nrm, c.n, M, T ? 1 : 0, world, owner, offsets, d_rows);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}
template <typename P4>
int import_rows_t(o3ds_handle h, const double* d_rows, size_t n, int has_normals, CloudRec& out) {
  out.n = n;
  out.precision = h->precision;
  if (n == 0) return O3DS_OK;
  HIP_TRY(dev_alloc(h, (void**)&out.pts, sizeof(P4) * n));
  if (has_normals) HIP_TRY(dev_alloc(h, (void**)&out.nrm, sizeof(P4) * n));
  rows_to_cloud_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(d_rows, n, (P4*)out.pts, (P4*)out.nrm);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}
}  // namespace
}  // extern "C++"

int o3ds_cloud_export_rows_by_owner(o3ds_handle h, o3ds_cloud cloud, const double T[16], double voxel_size, int world, double* d_rows,
                                    long long* d_counts) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "export_rows_by_owner: unknown cloud id");
  if (!(voxel_size > 0.0) || world < 1 || world > 64 || !d_counts || (c->n && !d_rows))
    return fail(h, O3DS_ERR_INVALID_ARG, "export_rows_by_owner: voxel_size > 0, 1 <= world <= 64, non-null buffers");
  return DISPATCH(c->precision, export_rows_t, h, *c, T, voxel_size, world, d_rows, d_counts);
}

int o3ds_cloud_import_rows(o3ds_handle h, const double* d_rows, size_t n, int has_normals, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  if (!out || (n && !d_rows)) return fail(h, O3DS_ERR_INVALID_ARG, "import_rows: null argument");
  return new_cloud(h, out, [&](CloudRec& c) { return DISPATCH(h->precision, import_rows_t, h, d_rows, n, has_normals, c); });
}

int o3ds_dense_map_size(o3ds_handle h, o3ds_dense_map id, size_t* n_voxels) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  auto it = h->dense_maps.find(id);
  if (it == h->dense_maps.end() || !n_voxels) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_size: bad argument");
  return dense_count(h, it->second, n_voxels);
}

int o3ds_dense_map_to_cloud(o3ds_handle h, o3ds_dense_map id, o3ds_cloud* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  auto it = h->dense_maps.find(id);
  if (it == h->dense_maps.end() || !out) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_to_cloud: bad argument");
  return new_cloud(h, out, [&](CloudRec& o) { return DISPATCH(h->precision, dense_to_cloud_t, h, it->second, o); });
}

int o3ds_dense_map_transform(o3ds_handle h, o3ds_dense_map id, const double T[16]) {
  CHECK_HANDLE(h);
  auto it = h->dense_maps.find(id);
  if (it == h->dense_maps.end() || !T) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_transform: bad argument");
  DenseRec& d = it->second;
  if (d.cap == 0) return O3DS_OK;
  dense_transform_kernel<<<grid_for(d.cap), kBlock, 0, h->stream>>>(d.dev, d.cap, mat34(T));
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

int o3ds_dense_map_carve(o3ds_handle h, o3ds_dense_map id, o3ds_cloud scan, const double scan_pose[16], const double sensor_position[3],
                         double neighborhood_radius, double max_raytracing_length, double truncation_distance, size_t* n_removed) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  auto it = h->dense_maps.find(id);
  CloudRec* c = find_cloud(h, scan);
  if (it == h->dense_maps.end() || !c || !sensor_position) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_carve: bad argument");
  if (!(neighborhood_radius > 0.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_carve: neighborhood radius must be > 0 (the ray step is 2 * radius)");
  if (n_removed) *n_removed = 0;
  if (it->second.cap == 0 || c->n == 0) return O3DS_OK;  // cloud->empty() (Submap.cpp:128)
  return DISPATCH(c->precision, dense_carve_t, h, it->second, *c, scan_pose, sensor_position, neighborhood_radius, max_raytracing_length, truncation_distance,
                  n_removed);
}

int o3ds_dense_map_count_occupied(o3ds_handle h, o3ds_dense_map id, o3ds_cloud cloud, const double T[16], size_t* n_hits) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  auto it = h->dense_maps.find(id);
  CloudRec* c = find_cloud(h, cloud);
  if (it == h->dense_maps.end() || !c || !n_hits) return fail(h, O3DS_ERR_INVALID_ARG, "dense_map_count_occupied: bad argument");
  *n_hits = 0;
  DenseRec& d = it->second;
  if (d.cap == 0 || c->n == 0) return O3DS_OK;
  const Mat34 M = mat34(T);
  unsigned long long* d_hits = nullptr;
  TMP_ALLOC(d_hits, sizeof(unsigned long long));
  HIP_TRY(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), h->stream));
  WITH_P4(c->precision, dense_probe_kernel<P4><<<grid_for(c->n), kBlock, 0, h->stream>>>((const P4*)c->pts, c->n, M, 1.0 / d.voxel, d.dev, d_hits));
  HIP_TRY(hipGetLastError());
  unsigned long long hits = 0;
  {
    const int rb = read_back(h, {{&hits, d_hits, sizeof(hits)}});
    if (rb) return rb;
  }
  *n_hits = (size_t)hits;
  return O3DS_OK;
}

int o3ds_overlap_indices(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double source_to_target[16], double voxel_size,
                         size_t min_points_per_voxel, uint64_t* idx_source, size_t* n_idx_source, uint64_t* idx_target, size_t* n_idx_target) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* s = find_cloud(h, source);
  CloudRec* t = find_cloud(h, target);
  if (!s || !t || !source_to_target || !n_idx_source || !n_idx_target) return fail(h, O3DS_ERR_INVALID_ARG, "overlap_indices: bad argument");
  if ((s->n && !idx_source) || (t->n && !idx_target)) return fail(h, O3DS_ERR_INVALID_ARG, "overlap_indices: null index buffer");
  if (!(voxel_size > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "overlap_indices: voxel_size must be > 0");
  if (min_points_per_voxel < 1) return fail(h, O3DS_ERR_INVALID_ARG, "minNumPointsPerVoxel must be >= 1");  // assert_ge, helpers.cpp:310
  if (s->n && t->n && s->precision != t->precision) return fail(h, O3DS_ERR_INVALID_ARG, "overlap_indices: precision mismatch");
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "index type");
  return DISPATCH(s->precision, overlap_t, h, *s, *t, source_to_target, voxel_size, min_points_per_voxel, (unsigned long long*)idx_source, n_idx_source,
                  (unsigned long long*)idx_target, n_idx_target);
}

int o3ds_map_carve(o3ds_handle h, o3ds_cloud map, o3ds_cloud raw_scan, const double map_to_range_sensor[16], const o3ds_crop* map_builder_crop,
                   const o3ds_carving_params* params, size_t* n_removed) {
  return o3ds_map_carve_removed(h, map, raw_scan, map_to_range_sensor, map_builder_crop, params, n_removed, nullptr);
}

int o3ds_map_carve_removed(o3ds_handle h, o3ds_cloud map, o3ds_cloud raw_scan, const double map_to_range_sensor[16], const o3ds_crop* map_builder_crop,
                           const o3ds_carving_params* params, size_t* n_removed, o3ds_cloud* removed_out) {
  CHECK_HANDLE(h);
  drop_fpfh(h, map);
  ArenaScope arena_scope(h);
  {  // a submap in its persistent form is carved where it is when the carving voxel is the map's (the voxel hash is the reference's table)
    CloudRec* pmc = find_cloud_lazy(h, map);
    CloudRec* sc = find_cloud(h, raw_scan);
    if (pmc && sc && pmc != sc && pmc->pm && params && map_to_range_sensor && !removed_out && params->voxel_size == pmc->pm->dev.voxel &&
        (pmc->n == 0 || sc->n == 0 || pmc->precision == sc->precision)) {
      if (n_removed) *n_removed = 0;
      if (sc->n == 0) return O3DS_OK;
      PMapRec* pm = pmc->pm;
      const PmDev d = pm->dev;
      const double* T = map_to_range_sensor;
      const Mat34 M = mat34(T);
      const CropDev cd = to_dev(map_builder_crop);
      unsigned int* block_bits = nullptr;
      TMP_ALLOC(block_bits, sizeof(unsigned int) << (kCarveBitsLog2 - 5));
      HIP_TRY(hipMemsetAsync(block_bits, 0, sizeof(unsigned int) << (kCarveBitsLog2 - 5), h->stream));
      pm_carve_bits_kernel<<<grid_for((size_t)d.hmask + 1), kBlock, 0, h->stream>>>(d.h, (size_t)d.hmask + 1, block_bits);
      pm->rec_seq = ++h->rec_seq;
      o3ds_context::PinRec* rec = h->h_rec_dev + pm->rec_slot;
      const CountPub pub{cnt_word(h, pm->rec_slot), &rec->cnt, pm->rec_seq};
      WITH_P4(pmc->precision,
              pm_carve_rays_kernel<P4><<<(unsigned int)((sc->n + kBlock - 1) / kBlock), kBlock, 0, h->stream>>>(
                  d, (const P4*)sc->pts, sc->n, M, T[12], T[13], T[14], params->max_raytracing_length, params->truncation_distance,
                  params->min_dot_product_with_normal, cd, block_bits);
              pm_carve_apply_kernel<P4><<<256, kBlock, 0, h->stream>>>(d, pub, rec->box));
      pm_carve_finish_kernel<<<1, 64, 0, h->stream>>>(d, pub, rec->box);
      HIP_TRY(hipGetLastError());
      if (n_removed) {  // (asking for the count is what waits)
        HIP_TRY(hipStreamSynchronize(h->stream));
        *n_removed = (size_t)(h->h_rec + pm->rec_slot)->pad;  // (the seventh double of the record)
        const int rp = pm_poll(h, pm, true);
        if (rp) return rp;
      }
      return O3DS_OK;
    }
  }
  CloudRec* m = find_cloud(h, map);
  CloudRec* s = find_cloud(h, raw_scan);
  if (!m || !s || !map_to_range_sensor || !params || m == s) return fail(h, O3DS_ERR_INVALID_ARG, "map_carve: bad argument");
  if (!(params->voxel_size > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "map_carve: voxel_size must be > 0");
  if (m->n > 0 && s->n > 0 && m->precision != s->precision) return fail(h, O3DS_ERR_INVALID_ARG, "map_carve: precision mismatch");
  size_t removed = 0;
  const CropDev cd = to_dev(map_builder_crop);
  const int rc = new_cloud(h, removed_out, [&](CloudRec& gone) {  // an empty cloud when nothing was carved
    gone.precision = m->precision;
    return DISPATCH(m->precision, carve_t, h, *m, *s, map_to_range_sensor, cd, *params, &removed, removed_out ? &gone : nullptr);
  });
  if (n_removed) *n_removed = removed;
  return rc;
}

int o3ds_map_insert_scan(o3ds_handle h, o3ds_cloud map, o3ds_cloud scan, const double T[16], double map_voxel_size,
                         const o3ds_crop* map_builder_crop, double max_corr_hint) {
  CHECK_HANDLE(h);
  drop_fpfh(h, map);
  ArenaScope arena_scope(h);
  CloudRec* m = find_cloud_lazy(h, map);  // (a map in its persistent form stays in it)
  CloudRec* s = find_cloud_lazy(h, scan);
  if (!m || !s || !T || m == s) return fail(h, O3DS_ERR_INVALID_ARG, "map_insert_scan: bad argument");
  if (s->pm) return fail(h, O3DS_ERR_INVALID_ARG, "map_insert_scan: the scan is a map");
  if (s->n == 0) return O3DS_OK;  // Submap.cpp:41-43: empty pre-processed scan is a no-op
  if (m->n == 0) m->precision = s->precision;
  if (m->precision != s->precision) return fail(h, O3DS_ERR_INVALID_ARG, "map_insert_scan: precision mismatch");
  int rc = O3DS_OK;
  // ---- the persistent form (map_kernels.hpp): work proportional to the scan.  It takes a map with a known layout [pass-through block | voxel
  // block in key order] -- what the first insertion into a map (below) or a fold leaves --, a search index being wanted, and map and scan
  // agreeing on normals ([O3D] operator+= drops the map's normals otherwise).  Colours follow operator+= too (append_t): a coloured map takes
  // a coloured scan with its colours, an uncoloured one takes any scan and ignores its colours, and an uncoloured scan into a coloured map
  // drops the map's colours -- the map is folded and takes the array form for that insertion (later ones re-enter, uncoloured).
  static const bool no_pm = ab_getenv("O3DS_NO_PERSISTENT_MAP") != nullptr;  // A/B and the bitwise tests: the array form at every insertion
  const bool pm_ok = !no_pm && map_voxel_size > 0.0 && max_corr_hint > 0.0 && (!m->col || s->col) && m->n > 0 && (m->nrm != nullptr) == (s->nrm != nullptr) &&
                     m->n + s->n < ((size_t)1 << 30);
  const CropDev cd = to_dev(map_builder_crop);
  CloudRec placed;
  placed.n = s->n;
  box_transform(placed, *s, T);
  if (m->pm) {
    PMapRec* pm = m->pm;
    rc = pm_poll(h, pm, false);
    if (rc) return rc;
    bool refold = !pm_ok || pm->dev.voxel != map_voxel_size || pm->dev.kc != pm_cell_voxels(max_corr_hint, map_voxel_size) || pm->t + 1 > kPmHistory;
    const double growth = 2.0 * (double)(pm->n_upper + s->n) + 8.0 * (double)s->n;  // every touched row moving to the pool's end
    if (!refold && (pm->n_upper + s->n > pm->dev.cap || pm->pool_top + growth > (double)pm->dev.pool_cap)) {
      rc = pm_poll(h, pm, true);  // the bounds were pessimistic? the exact numbers
      if (rc) return rc;
      refold = pm->n_upper + s->n > pm->dev.cap || pm->pool_top + growth > (double)pm->dev.pool_cap;
    }
    if (!refold && pm->clamped > 20000.0) refold = true;  // the map has grown well beyond the index grid: new extents (the fold re-grids)
    if (!refold && pm->multi_total + 4.0 * (double)s->n > 0.5 * (double)pm->dev.list_cap) refold = true;  // the multi list only grows (a fold starts it afresh)
    if (refold) {
      rc = pm_exit(h, *m);
      if (rc) return rc;
    }
  }
  if (!m->pm && pm_ok && m->vox_first >= 0 && (size_t)m->vox_first + m->vox_count == m->n) {
    rc = DISPATCH(m->precision, pm_enter_t, h, *m, map_voxel_size, max_corr_hint, s->n);
    if (rc) {
      pm_release(h, *m);
      m->vox_first = -1;
      return rc;
    }
  }
  if (m->pm) {
    CloudRec joined;
    box_union(joined, *m, placed);
    rc = DISPATCH(m->precision, pm_insert_t, h, *m, *s, T, cd);
    if (rc) return rc;
    box_copy(*m, joined);
    m->pm->pool_top += 2.0 * (double)(m->pm->n_upper) + 8.0 * (double)s->n;
    return O3DS_OK;
  }
  // ---- the array form (the reference's own way: everything is re-binned): the first insertions of a map, colours, a call without index ...
  rc = resolve_count(h, *s, true);
  if (rc) return rc;
  if (s->n == 0) return O3DS_OK;
  // the layout the previous insertion left (pass-through block, then the voxel block in key order): the merge below re-bins by merging
  const bool known = m->vox_first >= 0 && (size_t)m->vox_first + m->vox_count == m->n;
  const long long merge_np = known ? m->vox_first : -1;
  const size_t merge_nv = known ? m->vox_count : 0;
  if (m->n > 0 && m->cap >= m->n + s->n && m->nrm && s->nrm && !m->col && !s->col) {
    // transform (Submap.cpp:54) and operator+= (Submap.cpp:70) in one launch: the placed points go behind the map's last one, where the
    // previous merge left room -- the same kernel with the same arithmetic as transform_t, indices as append_t assigns them
    CloudRec joined;
    placed.n = s->n;
    box_union(joined, *m, placed);
    const Mat34 M = mat34(T);
    WITH_P4(m->precision, transform_kernel<P4><<<grid_for(s->n), kBlock, 0, h->stream>>>((const P4*)s->pts, (const P4*)s->nrm, s->n, M, T[3], T[7], T[11], T[15],
                                                                                          (P4*)m->pts, (P4*)m->nrm, m->n));
    HIP_TRY(hipGetLastError());
    free_index(h, *m);
    m->n += s->n;
    box_copy(*m, joined);
  } else {
    CloudRec t;
    rc = DISPATCH(s->precision, transform_t, h, *s, T, t);      // Submap.cpp:54
    if (!rc) rc = DISPATCH(m->precision, append_t, h, *m, t);   // Submap.cpp:70
    free_cloud(h, t);
  }
  if (rc) return rc;
  rc = voxelize_within_volume_impl(h, map, map_voxel_size, map_builder_crop, merge_np, merge_nv);  // Submap.cpp:71-72
  if (rc) return rc;
  m = find_cloud(h, map);
  if (max_corr_hint > 0.0) {
    rc = build_index(h, *m, max_corr_hint / kIndexCellDiv);
  }
  return rc;
}

}  // extern "C"

// ---- place recognition: FPFH, feature correspondences, RANSAC (feature_kernels.hpp) ---------------------------------------------
namespace {

size_t pool_cap_bytes() {  // the same cap dev_free applies to the handle's cached blocks
  static const size_t cap = (getenv("O3DS_POOL_CAP_MB") ? (size_t)atoll(getenv("O3DS_POOL_CAP_MB")) : (size_t)32768) << 20;
  return cap;
}

template <typename P4>
int fpfh_t(o3ds_handle h, CloudRec& c, double radius, int max_nn) {
  const size_t n = c.n;
  free_fpfh(h, c);
  if (n > (size_t)INT_MAX / 2) return fail(h, O3DS_ERR_CAPACITY, "compute_fpfh: cloud too large");
  const size_t feat_bytes = n * kFeatDim * sizeof(double), list_bytes = n * (size_t)max_nn * (sizeof(int) + sizeof(double));
  if (feat_bytes > pool_cap_bytes() || list_bytes > pool_cap_bytes())
    return fail(h, O3DS_ERR_CAPACITY, "compute_fpfh: feature buffer exceeds the pool cap (O3DS_POOL_CAP_MB)");
  double* out = nullptr;
  HIP_TRY(dev_alloc(h, (void**)&out, std::max<size_t>(feat_bytes, 8)));
  c.fpfh = out;
  if (n == 0) {
    c.has_fpfh = true;
    return O3DS_OK;
  }
  // the cloud's own index with a cell of about the radius: the neighbourhood is then the 3x3x3 block (an index with a much smaller
  // or larger cell is rebuilt; one built here is marked as a by-product, so a registration against the cloud picks its own)
  if (!c.has_index || c.grid.cell < 0.5 * radius || c.grid.cell > 2.0 * radius) {
    int rc = build_index(h, c, radius);
    if (rc) return rc;
    c.index_byproduct = true;
  }
  const int K = std::max(1, (int)std::ceil(radius / c.grid.cell));
  int *nb_idx = nullptr, *nb_cnt = nullptr;
  double *nb_d2 = nullptr, *spfh = nullptr;
  TMP_ALLOC(nb_idx, n * (size_t)max_nn * sizeof(int));
  TMP_ALLOC(nb_d2, n * (size_t)max_nn * sizeof(double));
  TMP_ALLOC(nb_cnt, n * sizeof(int));
  TMP_ALLOC(spfh, feat_bytes);
  const int ni = (int)n, nblk = (ni + 63) / 64;
  fpfh_neighbours_kernel<P4><<<std::min(ni, 65536), 64, 0, h->stream>>>(c.grid, (const P4*)c.spts, (const P4*)c.pts, ni, radius * radius,
                                                                          max_nn, K, nb_idx, nb_d2, nb_cnt);
  spfh_kernel<P4><<<nblk, 64, 0, h->stream>>>((const P4*)c.pts, (const P4*)c.nrm, ni, nb_idx, nb_cnt, max_nn, spfh);
  fpfh_kernel<<<nblk, 64, 0, h->stream>>>(spfh, ni, nb_idx, nb_d2, nb_cnt, max_nn, out);
  HIP_TRY(hipGetLastError());
  c.has_fpfh = true;
  c.fpfh_n = n;
  return O3DS_OK;
}

bool fpfh_valid(const CloudRec& c) { return c.has_fpfh && c.fpfh_n == c.n && !c.pm; }

// RegistrationRANSACBasedOnFeatureMatching's correspondences: (i, argmin_j) for every source point; with the mutual filter the pairs
// whose reverse match is i, unless there are fewer than 3 ransac_n of them (then the one-way set, fell_back = 1)
int feature_corr(o3ds_handle h, const CloudRec& s, const CloudRec& t, int mutual, int ransac_n, std::vector<uint32_t>& pairs, int* fell_back) {
  pairs.clear();
  *fell_back = 0;
  const int ns = (int)s.fpfh_n, nt = (int)t.fpfh_n;
  if (ns == 0 || nt == 0) return O3DS_OK;
  int *d_ij = nullptr, *d_ji = nullptr;
  TMP_ALLOC(d_ij, sizeof(int) * (size_t)ns);
  TMP_ALLOC(d_ji, sizeof(int) * (size_t)nt);
  feature_nn_kernel<<<(ns + kFnnBlock - 1) / kFnnBlock, kFnnBlock, 0, h->stream>>>(s.fpfh, ns, t.fpfh, nt, d_ij);
  if (mutual) feature_nn_kernel<<<(nt + kFnnBlock - 1) / kFnnBlock, kFnnBlock, 0, h->stream>>>(t.fpfh, nt, s.fpfh, ns, d_ji);
  HIP_TRY(hipGetLastError());
  std::vector<int> ij((size_t)ns), ji(mutual ? (size_t)nt : 0);
  int rc = d2h_copy(h, ij.data(), d_ij, sizeof(int) * (size_t)ns);
  if (rc) return rc;
  if (mutual) {
    rc = d2h_copy(h, ji.data(), d_ji, sizeof(int) * (size_t)nt);
    if (rc) return rc;
    for (int i = 0; i < ns; ++i) {
      const int j = ij[(size_t)i];
      if (j >= 0 && j < nt && ji[(size_t)j] == i) pairs.push_back((uint32_t)i), pairs.push_back((uint32_t)j);
    }
    if (pairs.size() / 2 >= (size_t)(3 * std::max(ransac_n, 0))) return O3DS_OK;
    *fell_back = 1;
    pairs.clear();
  }
  for (int i = 0; i < ns; ++i) pairs.push_back((uint32_t)i), pairs.push_back((uint32_t)ij[(size_t)i]);
  return O3DS_OK;
}

int ransac_batch_max() {  // hypotheses per batch at most (O3DS_RANSAC_BATCH fixes the batch size: the determinism A/B)
  static const int fixed = ab_getenv("O3DS_RANSAC_BATCH") ? std::max(1, atoi(ab_getenv("O3DS_RANSAC_BATCH"))) : 0;
  return fixed;
}

template <typename P4>
int ransac_t(o3ds_handle h, CloudRec& s, CloudRec& t, const o3ds_ransac_params* p, uint64_t seed, const std::vector<uint32_t>& pairs,
             o3ds_ransac_result* out, o3ds_ransac_trace* trace, size_t trace_cap) {
  const int n = p->ransac_n;
  const double r = p->max_correspondence_distance;
  const uint64_t m = pairs.size() / 2;
  const double conf = std::min(1.0, std::max(0.0, p->confidence));
  const long long max_iter = p->max_iteration;
  if (max_iter <= 0 || s.n == 0) return O3DS_OK;
  uint32_t* d_corr = nullptr;
  TMP_ALLOC(d_corr, pairs.size() * sizeof(uint32_t));
  int rc = h2d_copy(h, d_corr, pairs.data(), pairs.size() * sizeof(uint32_t));
  if (rc) return rc;
  if (!t.has_index || t.grid.cell < 0.5 * r || t.grid.cell > 2.0 * r) {
    rc = build_index(h, t, r);
    if (rc) return rc;
    t.index_byproduct = true;
  }
  const int K = std::max(1, (int)std::ceil(r / t.grid.cell));
  const int fixed = ransac_batch_max();
  const int bmax = fixed ? fixed : 65536;
  int batch = fixed ? fixed : 1024;  // small first batches: a good hypothesis early cuts the search short
  double *d_T = nullptr, *d_val = nullptr;
  int *d_checks = nullptr, *d_list = nullptr, *d_count = nullptr;
  uint32_t* d_samples = nullptr;
  TMP_ALLOC(d_T, (size_t)bmax * 16 * sizeof(double));
  TMP_ALLOC(d_val, (size_t)bmax * 3 * sizeof(double));
  TMP_ALLOC(d_checks, (size_t)bmax * sizeof(int));
  TMP_ALLOC(d_list, (size_t)bmax * sizeof(int));
  TMP_ALLOC(d_count, sizeof(int));
  if (trace && trace_cap) TMP_ALLOC(d_samples, (size_t)bmax * kRansacMaxN * sizeof(uint32_t));
  long long est_k = max_iter, t0 = 0, best_t = -1, validations = 0;
  long long best_pairs = 0;
  double best_rmse = 0.0, best_T[16];
  std::vector<double> val;
  std::vector<int> checks;
  std::vector<uint32_t> samples;
  std::vector<double> Ts;
  while (t0 < est_k) {
    const int cnt = (int)std::min<long long>(batch, est_k - t0);
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int), h->stream));
    RansacArgs a{};
    a.corr = d_corr;
    a.m = m;
    a.seed = seed;
    a.n = n;
    a.t0 = t0;
    a.count = cnt;
    a.edge = p->edge_length;
    a.dist = p->distance;
    a.T = d_T;
    a.checks = d_checks;
    a.samples = d_samples;
    a.list = d_list;
    a.list_count = d_count;
    ransac_hypothesis_kernel<P4><<<(cnt + 255) / 256, 256, 0, h->stream>>>((const P4*)s.pts, (const P4*)t.pts, a);
    ransac_validate_kernel<P4><<<std::min(cnt, 2048), kValBlock, 0, h->stream>>>((const P4*)s.pts, (int)s.n, t.grid, (const P4*)t.spts,
                                                                                  r * r, K, d_T, d_list, d_count, d_val);
    HIP_TRY(hipGetLastError());
    int nl = 0;
    rc = read_back(h, {{&nl, d_count, sizeof(int)}});
    if (rc) return rc;
    if (nl < 0 || nl > cnt) return fail(h, O3DS_ERR_HIP, "ransac: validation list count out of range");
    val.resize((size_t)nl * 3);
    if (nl) {
      rc = d2h_copy(h, val.data(), d_val, (size_t)nl * 3 * sizeof(double));
      if (rc) return rc;
    }
    if (trace && (size_t)t0 < trace_cap) {
      const size_t tn = std::min<size_t>((size_t)cnt, trace_cap - (size_t)t0);
      checks.resize(tn);
      samples.resize(tn * kRansacMaxN);
      Ts.resize(tn * 16);
      rc = d2h_copy(h, checks.data(), d_checks, tn * sizeof(int));
      if (!rc) rc = d2h_copy(h, samples.data(), d_samples, tn * kRansacMaxN * sizeof(uint32_t));
      if (!rc) rc = d2h_copy(h, Ts.data(), d_T, tn * 16 * sizeof(double));
      if (rc) return rc;
      for (size_t k = 0; k < tn; ++k) {
        o3ds_ransac_trace& e = trace[(size_t)t0 + k];
        for (int j = 0; j < kRansacMaxN; ++j) e.sample[j] = j < n ? samples[k * kRansacMaxN + j] : 0u;
        e.checks = checks[k];
        e.pairs = -1;
        e.error_sum = 0.0;
        memcpy(e.transformation, &Ts[k * 16], sizeof(e.transformation));
      }
      for (int k = 0; k < nl; ++k) {
        const size_t slot = (size_t)val[3 * (size_t)k];
        if (slot < tn) {
          trace[(size_t)t0 + slot].pairs = (int32_t)val[3 * (size_t)k + 1];
          trace[(size_t)t0 + slot].error_sum = val[3 * (size_t)k + 2];
        }
      }
    }
    // fold the batch's validated hypotheses in index order (the serial stopping rule)
    std::vector<std::pair<long long, int>> order((size_t)nl);
    for (int k = 0; k < nl; ++k) order[(size_t)k] = {(long long)val[3 * (size_t)k], k};
    std::sort(order.begin(), order.end());
    long long improved_slot = -1;
    for (const auto& o : order) {
      const long long tt = t0 + o.first;
      if (tt >= est_k) break;
      ++validations;
      const long long pr = (long long)val[3 * (size_t)o.second + 1];
      const double err = val[3 * (size_t)o.second + 2];
      const double rmse = pr > 0 ? std::sqrt(err / (double)pr) : 0.0;
      if (pr > best_pairs || (pr == best_pairs && rmse < best_rmse)) {  // [O3D] RegistrationResult::IsBetterRANSACThan
        best_pairs = pr;
        best_rmse = rmse;
        best_t = tt;
        improved_slot = o.first;
        const double fitness = (double)pr / (double)s.n;
        const double est = std::log(1.0 - conf) / std::log(1.0 - std::pow(fitness, n));
        if (est < (double)est_k) est_k = (long long)std::ceil(est);
      }
    }
    if (improved_slot >= 0) {
      rc = read_back(h, {{best_T, d_T + (size_t)improved_slot * 16, sizeof(best_T)}});
      if (rc) return rc;
    }
    t0 += cnt;
    if (!fixed) batch = std::min(bmax, batch * 2);
  }
  const long long run = std::max(std::min(est_k, max_iter), best_t + 1);
  out->iterations_run = run;
  out->validations = validations;
  out->best_t = best_t;
  if (best_t >= 0) {
    memcpy(out->transformation, best_T, sizeof(best_T));
    out->fitness = (double)best_pairs / (double)s.n;
    out->inlier_rmse = best_rmse;
    out->n_corr = (uint64_t)best_pairs;
  }
  if (trace)
    for (size_t k = (size_t)std::max<long long>(run, 0); k < trace_cap; ++k) {
      trace[k].checks = -1;
      trace[k].pairs = -1;
      trace[k].error_sum = 0.0;
    }
  return O3DS_OK;
}

void empty_ransac_result(o3ds_ransac_result* out) {
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 16; ++k) out->transformation[k] = (k % 5 == 0) ? 1.0 : 0.0;
  out->best_t = -1;
}

}  // namespace

extern "C" {

int o3ds_compute_fpfh(o3ds_handle h, o3ds_cloud cloud, double radius, int max_nn) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "compute_fpfh: unknown cloud id");
  if (!c->nrm) return fail(h, O3DS_ERR_INVALID_ARG, "compute_fpfh: the cloud has no normals ([O3D] ComputeFPFHFeature needs them)");
  if (!(radius > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "compute_fpfh: radius must be > 0");
  if (max_nn < 1 || max_nn > kFpfhMaxNN) return fail(h, O3DS_ERR_INVALID_ARG, "compute_fpfh: max_nn outside 1..128");
  return DISPATCH(c->precision, fpfh_t, h, *c, radius, max_nn);
}

int o3ds_cloud_has_fpfh(o3ds_handle h, o3ds_cloud cloud, int* has_fpfh) {
  CHECK_HANDLE(h);
  if (!has_fpfh) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_has_fpfh: null argument");
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_has_fpfh: unknown cloud id");
  *has_fpfh = fpfh_valid(*c) ? 1 : 0;
  return O3DS_OK;
}

int o3ds_cloud_download_fpfh(o3ds_handle h, o3ds_cloud cloud, double* out, size_t capacity) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_fpfh: unknown cloud id");
  if (!fpfh_valid(*c)) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_fpfh: the cloud has no features");
  if (capacity < c->n) return fail(h, O3DS_ERR_CAPACITY, "cloud_download_fpfh: buffer too small");
  if (c->n == 0) return O3DS_OK;
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_fpfh: null buffer");
  return d2h_copy(h, out, c->fpfh, c->n * kFeatDim * sizeof(double));
}

int o3ds_feature_correspondences(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, int mutual_filter, int ransac_n, uint32_t* pairs,
                                 size_t capacity, size_t* n_pairs, int* fell_back) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!n_pairs) return fail(h, O3DS_ERR_INVALID_ARG, "feature_correspondences: null argument");
  CloudRec* s = find_cloud(h, source);
  CloudRec* t = find_cloud(h, target);
  if (!s || !t) return fail(h, O3DS_ERR_INVALID_ARG, "feature_correspondences: unknown cloud id");
  if (!fpfh_valid(*s) || !fpfh_valid(*t)) return fail(h, O3DS_ERR_INVALID_ARG, "feature_correspondences: a cloud has no features");
  std::vector<uint32_t> v;
  int fb = 0;
  int rc = feature_corr(h, *s, *t, mutual_filter, ransac_n, v, &fb);
  if (rc) return rc;
  *n_pairs = v.size() / 2;
  if (fell_back) *fell_back = fb;
  if (capacity < v.size() / 2) return fail(h, O3DS_ERR_CAPACITY, "feature_correspondences: buffer too small");
  if (!v.empty()) {
    if (!pairs) return fail(h, O3DS_ERR_INVALID_ARG, "feature_correspondences: null buffer");
    memcpy(pairs, v.data(), v.size() * sizeof(uint32_t));
  }
  return O3DS_OK;
}

int o3ds_ransac_feature_matching(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_ransac_params* params, uint64_t seed,
                                 o3ds_ransac_result* out, o3ds_ransac_trace* trace, size_t trace_cap) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!params || !out || (trace_cap && !trace)) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_feature_matching: null argument");
  empty_ransac_result(out);
  for (size_t k = 0; k < trace_cap; ++k) {
    memset(&trace[k], 0, sizeof(trace[k]));
    trace[k].checks = -1;
    trace[k].pairs = -1;
  }
  CloudRec* s = find_cloud(h, source);
  CloudRec* t = find_cloud(h, target);
  if (!s || !t) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_feature_matching: unknown cloud id");
  if (!fpfh_valid(*s) || !fpfh_valid(*t)) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_feature_matching: a cloud has no features");
  if (params->ransac_n > kRansacMaxN) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_feature_matching: ransac_n > 8 unsupported");
  if (s->precision != t->precision) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_feature_matching: clouds of different storage precision");
  std::vector<uint32_t> pairs;
  int fb = 0;
  int rc = feature_corr(h, *s, *t, params->mutual_filter, params->ransac_n, pairs, &fb);
  if (rc) return rc;
  out->n_feature_corr = pairs.size() / 2;
  out->fell_back = fb;
  // [O3D] RegistrationRANSACBasedOnCorrespondence: the empty RegistrationResult
  if (params->ransac_n < 3 || pairs.size() / 2 < (size_t)params->ransac_n || !(params->max_correspondence_distance > 0.0)) return O3DS_OK;
  return DISPATCH(s->precision, ransac_t, h, *s, *t, params, seed, pairs, out, trace, trace_cap);
}

}  // extern "C"

// ---- pose-graph optimisation (o3ds_global_optimization) ------------------------------------------------------------------------------
namespace {

constexpr size_t kPgMaxNodes = 4096, kPgMaxEdges = (size_t)1 << 20;  // the caps o3ds_backend.h documents

struct DevBlock {  // a device block outside the arena (H and its factor are up to 4.8 GB each: they go back to the pool on return)
  o3ds_handle h;
  void* p = nullptr;
  explicit DevBlock(o3ds_handle hh) : h(hh) {}
  ~DevBlock() { dev_free(h, p); }
};

struct PgCtx {
  int n = 0, m = 0, nb = 0;
  size_t M = 0;
  double* poses[2] = {nullptr, nullptr};
  double* H = nullptr;
  double* L = nullptr;
  double *b[2] = {nullptr, nullptr}, *bw = nullptr, *y = nullptr, *x = nullptr, *part = nullptr;
  PgRecord* rec = nullptr;
  int cur = 0;  // poses[cur] are the graph's current poses
};

int pg_read(o3ds_handle h, PgCtx& C, PgRecord* r) {
  int rc = read_back(h, {{r, C.rec, sizeof(PgRecord)}});
  if (rc) return rc;
  if (r->err) return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: H + lambda I is not positive definite (pivot of row " + std::to_string(r->err - 1) + ")");
  return O3DS_OK;
}

int pg_solve(o3ds_handle h, PgCtx& C, const double* b, double lambda) {
  if (C.m <= kPgSmallMax) {
    pg_small_solve_kernel<<<1, kPgSmallThreads, 0, h->stream>>>(C.H, C.M, C.m, lambda, b, C.x, C.rec);
    HIP_TRY(hipGetLastError());
    return O3DS_OK;
  }
  const size_t MM = C.M * C.M;
  pg_shift_copy_kernel<<<(int)std::min<size_t>((MM + 255) / 256, 8192), 256, 0, h->stream>>>(C.H, C.L, C.M, lambda);
  for (int k = 0; k < C.nb; ++k) {
    pg_panel_kernel<<<1, 256, 0, h->stream>>>(C.L, C.M, k, C.rec);
    const int rest = C.nb - k - 1;
    if (rest > 0) {
      pg_trsm_kernel<<<rest, kPgNB, 0, h->stream>>>(C.L, C.M, k);
      pg_syrk_kernel<<<dim3(rest, rest), 256, 0, h->stream>>>(C.L, C.M, k);
    }
  }
  HIP_TRY(hipMemcpyAsync(C.bw, b, C.M * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  for (int k = 0; k < C.nb; ++k) pg_fwd_kernel<<<C.nb - k, kPgNB, 0, h->stream>>>(C.L, C.M, k, C.bw, C.y);
  for (int k = C.nb - 1; k >= 0; --k) pg_bwd_kernel<<<k + 1, kPgNB, 0, h->stream>>>(C.L, C.M, k, C.y, C.x);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

// One GlobalOptimizationLevenbergMarquardt::OptimizePoseGraph over the edges `ids` of `all`: the poses in C.poses[C.cur] move, conf[k]
// (indexed like ids) is updated.  The host runs Open3D's control flow on the numbers of the device record.
int pg_pass(o3ds_handle h, PgCtx& C, const o3ds_pose_graph_edge* all, const std::vector<int>& ids, std::vector<double>& conf,
            const o3ds_global_optimization_option* opt, const o3ds_global_optimization_criteria* crit, int pass, o3ds_pose_graph_result* out) {
  const int ne = (int)ids.size(), n = C.n;
  // ComputeLineProcessWeight: serial, in edge order
  double lpw = 0.0;
  if (ne > 0) {
    double avg = 0.0;
    for (int k = 0; k < ne; ++k) avg += all[ids[k]].information[5 * 6 + 5];
    avg /= (double)ne;
    lpw = opt->preference_loop_closure * std::pow(opt->max_correspondence_distance, 2) * avg;
  }
  out->line_process_weight[pass] = lpw;
  // edges, confidences, the per-block and per-node lists (the graph's structure is fixed for the pass)
  std::vector<PgEdgeIn> ein((size_t)ne);
  std::map<std::pair<int, int>, std::vector<int>> blk;
  std::vector<std::vector<int>> nod((size_t)n);
  for (int k = 0; k < ne; ++k) {
    const o3ds_pose_graph_edge& e = all[ids[k]];
    PgEdgeIn& d = ein[(size_t)k];
    memcpy(d.X, e.transformation, sizeof(d.X));
    memcpy(d.info, e.information, sizeof(d.info));
    d.src = e.source_node_id, d.tgt = e.target_node_id, d.uncertain = e.uncertain ? 1 : 0, d.pad = 0;
    const int s = d.src, t = d.tgt;  // Open3D's order: H_ss += P, H_st += -P, H_ts += -P, H_tt += P; b_s -= q, b_t -= -q
    blk[{s, s}].push_back(2 * k);
    blk[{s, t}].push_back(2 * k + 1);
    blk[{t, s}].push_back(2 * k + 1);
    blk[{t, t}].push_back(2 * k);
    nod[(size_t)s].push_back(2 * k);
    nod[(size_t)t].push_back(2 * k + 1);
  }
  std::vector<int4> blocks;
  std::vector<int> hlist, blist;
  for (auto& kv : blk) {
    blocks.push_back(make_int4(kv.first.first, kv.first.second, (int)hlist.size(), (int)kv.second.size()));
    hlist.insert(hlist.end(), kv.second.begin(), kv.second.end());
  }
  std::vector<int2> nodes((size_t)n);
  for (int i = 0; i < n; ++i) {
    nodes[(size_t)i] = make_int2((int)blist.size(), (int)nod[(size_t)i].size());
    blist.insert(blist.end(), nod[(size_t)i].begin(), nod[(size_t)i].end());
  }
  PgEdgeIn* d_e = nullptr;
  double *d_conf[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
  int4* d_blocks = nullptr;
  int2* d_nodes = nullptr;
  int *d_hl = nullptr, *d_bl = nullptr;
  TMP_ALLOC(d_e, std::max<size_t>(1, ein.size()) * sizeof(PgEdgeIn));
  for (int s = 0; s < 2; ++s) {
    TMP_ALLOC(d_conf[s], std::max(1, ne) * sizeof(double));
    TMP_ALLOC(d_out[s], (size_t)std::max(1, ne) * kPgEdgeOut * sizeof(double));
  }
  TMP_ALLOC(d_blocks, std::max<size_t>(1, blocks.size()) * sizeof(int4));
  TMP_ALLOC(d_hl, std::max<size_t>(1, hlist.size()) * sizeof(int));
  TMP_ALLOC(d_nodes, (size_t)n * sizeof(int2));
  TMP_ALLOC(d_bl, std::max<size_t>(1, blist.size()) * sizeof(int));
  int rc = O3DS_OK;
  if (ne > 0) {
    if ((rc = h2d_copy(h, d_e, ein.data(), ein.size() * sizeof(PgEdgeIn)))) return rc;
    if ((rc = h2d_copy(h, d_conf[0], conf.data(), (size_t)ne * sizeof(double)))) return rc;
    if ((rc = h2d_copy(h, d_blocks, blocks.data(), blocks.size() * sizeof(int4)))) return rc;
    if ((rc = h2d_copy(h, d_hl, hlist.data(), hlist.size() * sizeof(int)))) return rc;
    if ((rc = h2d_copy(h, d_bl, blist.data(), blist.size() * sizeof(int)))) return rc;
  }
  if ((rc = h2d_copy(h, d_nodes, nodes.data(), nodes.size() * sizeof(int2)))) return rc;
  HIP_TRY(hipMemsetAsync(C.rec, 0, sizeof(PgRecord), h->stream));
  HIP_TRY(hipMemsetAsync(C.b[0], 0, C.M * sizeof(double), h->stream));
  HIP_TRY(hipMemsetAsync(C.b[1], 0, C.M * sizeof(double), h->stream));
  pg_init_h_kernel<<<(int)std::min<size_t>((C.M * C.M + 255) / 256, 8192), 256, 0, h->stream>>>(C.H, C.M, (size_t)C.m);
  int cc = 0, co = 0, cb = 0;  // current confidences, edge outputs, b
  const int eg = (ne + 63) / 64, ng = (6 * n + 63) / 64, ug = (n + 63) / 64, nbk = (int)blocks.size();
  auto edge_pass = [&](const double* poses, int cin, int cout, int eo) {
    if (ne > 0)
      pg_edge_kernel<<<eg, 64, 0, h->stream>>>(poses, d_e, ne, d_conf[cin], d_conf[cout], d_out[eo], lpw, opt->edge_prune_threshold);
  };
  auto assemble_b = [&](int eo, int bo) {
    if (ne > 0) pg_assemble_b_kernel<<<ng, 64, 0, h->stream>>>(d_nodes, d_bl, d_out[eo], n, C.b[bo]);
  };
  // initial: the residual with the confidences as given, then UpdateConfidence, then ComputeLinearSystem
  edge_pass(C.poses[C.cur], 0, 1, 0);
  cc = ne > 0 ? 1 : 0;
  if (nbk) pg_assemble_h_kernel<<<nbk, 64, 0, h->stream>>>(d_blocks, d_hl, d_out[0], C.H, C.M);
  assemble_b(0, 0);
  pg_reduce_kernel<<<1, kPgRed, 0, h->stream>>>(d_out[0], ne, nullptr, n, C.b[0], C.H, C.M, C.m, C.rec);
  HIP_TRY(hipGetLastError());
  PgRecord R;
  if ((rc = pg_read(h, C, &R))) return rc;
  double current_residual = R.residual, new_residual = R.residual;
  double lambda = 1e-5 * R.maxdiag, ni = 2.0, rho = 0.0;
  int reason = 0, iters = 0, lm_steps = 0;
  bool stop = false;
  auto set_stop = [&](bool c, int why) {
    if (!stop && c) stop = true, reason = why;
  };
  if (R.maxb < crit->min_right_term) {
    reason = 1;
  } else {
    for (int iter = 0; !stop; ++iter) {
      int lm_count = 0;
      for (;;) {
        if ((rc = pg_solve(h, C, C.b[cb], lambda))) return rc;
        const int nw = C.cur ^ 1;
        pg_update_kernel<<<ug, 64, 0, h->stream>>>(C.poses[C.cur], C.x, C.b[cb], lambda, n, C.poses[nw], C.part);
        edge_pass(C.poses[nw], cc, cc ^ 1, co ^ 1);
        assemble_b(co ^ 1, cb ^ 1);
        pg_reduce_kernel<<<1, kPgRed, 0, h->stream>>>(d_out[co ^ 1], ne, C.part, n, C.b[cb ^ 1], nullptr, C.M, C.m, C.rec);
        HIP_TRY(hipGetLastError());
        if ((rc = pg_read(h, C, &R))) return rc;
        ++lm_steps;
        set_stop(std::sqrt(R.dn2) < crit->min_relative_increment * (std::sqrt(R.xn2) + crit->min_relative_increment), 2);
        if (!stop) {
          new_residual = R.residual;  // with the old graph's confidences
          rho = (current_residual - new_residual) / (R.ddb + 1e-3);
          if (rho > 0) {
            set_stop(current_residual - new_residual < crit->min_relative_residual_increment * current_residual, 3);
            double alpha = 1. - std::pow(2 * rho - 1, 3);
            alpha = std::min(alpha, crit->upper_scale_factor);
            lambda *= std::max(crit->lower_scale_factor, alpha);
            ni = 2;
            current_residual = new_residual;
            C.cur = nw;  // pose_graph = *pose_graph_new, its confidences updated, its linear system
            cc ^= ne > 0 ? 1 : 0;
            co ^= 1;
            cb ^= 1;
            set_stop(R.maxb < crit->min_right_term, 1);
            if (stop) break;
            if (nbk) pg_assemble_h_kernel<<<nbk, 64, 0, h->stream>>>(d_blocks, d_hl, d_out[co], C.H, C.M);
          } else {
            lambda *= ni;
            ni *= 2;
          }
        }
        ++lm_count;
        set_stop(lm_count >= crit->max_iteration_lm, 6);
        if (rho > 0 || stop) break;
      }
      set_stop(current_residual < crit->min_residual, 4);
      set_stop(iter >= crit->max_iteration, 5);
      iters = iter + 1;
    }
  }
  out->iterations[pass] = iters;
  out->lm_steps[pass] = lm_steps;
  out->stop_reason[pass] = reason;
  out->residual[pass] = current_residual;
  if (ne > 0) return d2h_copy(h, conf.data(), d_conf[cc], (size_t)ne * sizeof(double));
  return O3DS_OK;
}

void pg_inv4_host(const double* cm, double* out_cm) {  // column-major in and out, the kernel's cofactor inverse
  double m[16], o[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) m[r * 4 + c] = cm[c * 4 + r];
  double inv[16];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  const double rdet = 1.0 / (m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]);
  for (int k = 0; k < 16; ++k) o[k] = inv[k] * rdet;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out_cm[c * 4 + r] = o[r * 4 + c];
}

void pg_mul4_host(const double* a, const double* b, double* o) {  // column-major
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = a[r] * b[c * 4];
      for (int k = 1; k < 4; ++k) s += a[k * 4 + r] * b[c * 4 + k];
      o[c * 4 + r] = s;
    }
}

bool pg_connected(size_t n, const o3ds_pose_graph_edge* edges, size_t ne) {  // ValidatePoseGraphConnectivity(pose_graph, false)
  if (n == 0) return true;
  std::vector<std::vector<int>> adj(n);
  for (size_t k = 0; k < ne; ++k) {
    adj[(size_t)edges[k].source_node_id].push_back(edges[k].target_node_id);
    adj[(size_t)edges[k].target_node_id].push_back(edges[k].source_node_id);
  }
  std::vector<char> seen(n, 0);
  std::vector<int> todo{0};
  seen[0] = 1;
  size_t count = 1;
  while (!todo.empty()) {
    const int i = todo.back();
    todo.pop_back();
    for (int j : adj[(size_t)i])
      if (!seen[(size_t)j]) seen[(size_t)j] = 1, ++count, todo.push_back(j);
  }
  return count == n;
}

}  // namespace

extern "C" {

int o3ds_global_optimization(o3ds_handle h, double* node_poses, size_t n_nodes, o3ds_pose_graph_edge* edges, size_t n_edges,
                             const o3ds_global_optimization_option* opt, const o3ds_global_optimization_criteria* crit, uint8_t* edge_kept,
                             o3ds_pose_graph_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!opt || !crit || !out || (n_nodes && !node_poses) || (n_edges && !edges))
    return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: null argument");
  memset(out, 0, sizeof(*out));
  out->n_edges_kept = (int32_t)std::min<size_t>(n_edges, INT32_MAX);
  if (edge_kept)
    for (size_t k = 0; k < n_edges; ++k) edge_kept[k] = 1;
  if (n_nodes > kPgMaxNodes || n_edges > kPgMaxEdges)
    return fail(h, O3DS_ERR_CAPACITY, "global_optimization: more than 4096 nodes or 2^20 edges");
  for (size_t k = 0; k < n_edges; ++k) {
    const o3ds_pose_graph_edge& e = edges[k];
    if (e.source_node_id < 0 || (size_t)e.source_node_id >= n_nodes || e.target_node_id < 0 || (size_t)e.target_node_id >= n_nodes)
      return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: edge " + std::to_string(k) + " references a node out of range");
    bool ok = std::isfinite(e.confidence);
    for (int i = 0; i < 16; ++i) ok = ok && std::isfinite(e.transformation[i]);
    for (int i = 0; i < 36; ++i) ok = ok && std::isfinite(e.information[i]);
    if (!ok) return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: edge " + std::to_string(k) + " has a non-finite value");
  }
  for (size_t i = 0; i < n_nodes * 16; ++i)
    if (!std::isfinite(node_poses[i])) return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: a node pose has a non-finite value");
  const double o3[] = {opt->max_correspondence_distance, opt->edge_prune_threshold, opt->preference_loop_closure, crit->min_relative_increment,
                       crit->min_relative_residual_increment, crit->min_right_term, crit->min_residual, crit->upper_scale_factor,
                       crit->lower_scale_factor};
  for (double v : o3)
    if (!std::isfinite(v)) return fail(h, O3DS_ERR_INVALID_ARG, "global_optimization: a non-finite option or criterion");
  // ValidatePoseGraph: Open3D warns and returns the graph unchanged
  if (!pg_connected(n_nodes, edges, n_edges)) return O3DS_OK;
  for (size_t k = 0; k < n_edges; ++k)
    if (!edges[k].uncertain && edges[k].confidence != 1.0) return O3DS_OK;
  out->valid = 1;
  if (n_nodes <= 1) return O3DS_OK;

  PgCtx C;
  C.n = (int)n_nodes;
  C.m = 6 * C.n;
  C.M = ((size_t)C.m + kPgNB - 1) / kPgNB * kPgNB;
  C.nb = (int)(C.M / kPgNB);
  DevBlock hb(h), lb(h);
  const size_t mat = C.M * C.M * sizeof(double);
  if (dev_alloc(h, &hb.p, mat) != hipSuccess) return fail(h, O3DS_ERR_OOM, "global_optimization: out of memory for H");
  C.H = (double*)hb.p;
  if (C.m > kPgSmallMax) {
    if (dev_alloc(h, &lb.p, mat) != hipSuccess) return fail(h, O3DS_ERR_OOM, "global_optimization: out of memory for the factor");
    C.L = (double*)lb.p;
  }
  for (int s = 0; s < 2; ++s) {
    TMP_ALLOC(C.poses[s], n_nodes * 16 * sizeof(double));
    TMP_ALLOC(C.b[s], C.M * sizeof(double));
  }
  TMP_ALLOC(C.bw, C.M * sizeof(double));
  TMP_ALLOC(C.y, C.M * sizeof(double));
  TMP_ALLOC(C.x, C.M * sizeof(double));
  TMP_ALLOC(C.part, n_nodes * 3 * sizeof(double));
  TMP_ALLOC(C.rec, sizeof(PgRecord));
  int rc = h2d_copy(h, C.poses[0], node_poses, n_nodes * 16 * sizeof(double));
  if (rc) return rc;
  // pass 1 on every edge
  std::vector<int> ids(n_edges);
  std::vector<double> conf(n_edges);
  for (size_t k = 0; k < n_edges; ++k) ids[k] = (int)k, conf[k] = edges[k].confidence;
  if ((rc = pg_pass(h, C, edges, ids, conf, opt, crit, 0, out))) return rc;
  // CreatePoseGraphWithoutInvalidEdges, pass 2 with the kept edges' confidences
  std::vector<int> kept;
  std::vector<double> conf2;
  std::vector<double> final_conf(conf);
  for (size_t k = 0; k < n_edges; ++k)
    if (!edges[k].uncertain || conf[k] > opt->edge_prune_threshold) kept.push_back((int)k), conf2.push_back(conf[k]);
  if ((rc = pg_pass(h, C, edges, kept, conf2, opt, crit, 1, out))) return rc;
  for (size_t j = 0; j < kept.size(); ++j) final_conf[(size_t)kept[j]] = conf2[j];
  std::vector<double> poses(n_nodes * 16);
  if ((rc = d2h_copy(h, poses.data(), C.poses[C.cur], poses.size() * sizeof(double)))) return rc;
  // CompensateReferencePoseGraphNode
  const int ref = opt->reference_node;
  if (ref >= 0 && (size_t)ref < n_nodes) {
    double inv[16], comp[16], tmp[16];
    pg_inv4_host(&poses[(size_t)ref * 16], inv);
    pg_mul4_host(&node_poses[(size_t)ref * 16], inv, comp);
    for (size_t i = 0; i < n_nodes; ++i) {
      pg_mul4_host(comp, &poses[i * 16], tmp);
      memcpy(&poses[i * 16], tmp, sizeof(tmp));
    }
  }
  memcpy(node_poses, poses.data(), poses.size() * sizeof(double));
  for (size_t k = 0; k < n_edges; ++k) edges[k].confidence = final_conf[k];
  if (edge_kept) {
    for (size_t k = 0; k < n_edges; ++k) edge_kept[k] = 0;
    for (int k : kept) edge_kept[(size_t)k] = 1;
  }
  out->n_edges_kept = (int32_t)kept.size();
  return O3DS_OK;
}

}  // extern "C"


#include "sharded.hpp"
#include "multi_icp.hpp"
#include "batch_icp.hpp"

// The clustering sits at the end of the file: its kernels are instantiated after every other one.
namespace {
// ---- DBSCAN clustering and the small-cluster filter (cluster_kernels.hpp) -------------------------------------------------------------
// The labels of cloud `c` (n > 0 points, n < 2^31) in d_labels [n] and the number of points per label in d_sizes [n] (entries from
// *n_clusters on are zero), both device arrays; nothing is copied to the host but the number of clusters and the error word.
constexpr int kSpanClusterHook = 11, kSpanClusterFlatten = 12, kSpanClusterBorder = 13;
template <typename P4>
int cluster_labels_t(o3ds_handle h, CloudRec& c, double eps, int min_points, int* d_labels, uint32_t* d_sizes, size_t* n_clusters) {
  const size_t n = c.n;
  *n_clusters = 0;
  int *parent = nullptr, *flags = nullptr, *pos = nullptr, *d_err = nullptr;
  uint32_t *d_cnt = nullptr, *d_tot = nullptr;
  TMP_ALLOC(d_cnt, sizeof(uint32_t) * n);
  TMP_ALLOC(d_tot, sizeof(uint32_t) * n);
  TMP_ALLOC(parent, sizeof(int) * n);
  TMP_ALLOC(flags, sizeof(int) * (n + 1));
  TMP_ALLOC(pos, sizeof(int) * (n + 1));
  TMP_ALLOC(d_err, sizeof(int));
  HIP_TRY(hipMemsetAsync(d_sizes, 0, sizeof(uint32_t) * n, h->stream));
  bool empty = false;
  int rc = neighbor_launch_t<P4>(h, c, c, nullptr, nullptr, n, 0, eps, nullptr, nullptr, d_cnt, d_tot, nullptr, &empty);  // |N_i|
  if (rc) return rc;
  if (empty) {  // no point with three finite coordinates: everything is noise
    HIP_TRY(hipMemsetAsync(d_labels, 0xff, sizeof(int) * n, h->stream));
    return O3DS_OK;
  }
  HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int), h->stream));
  const unsigned int gsz = (unsigned int)((n + kNbrQueriesPerBlock - 1) / kNbrQueriesPerBlock);
  const P4 *pts = (const P4*)c.pts, *sp = (const P4*)c.spts;
  const uint32_t mp = (uint32_t)min_points;
  cluster_init_kernel<><<<grid_for(n), kBlock, 0, h->stream>>>(parent, n);
  span_mark(h, kSpanClusterHook);
  cluster_walk_kernel<P4, false><<<gsz, 64, 0, h->stream>>>(pts, n, c.grid, sp, eps, mp, d_tot, parent, nullptr, nullptr, d_err);
  span_mark(h, kSpanClusterHook);
  span_mark(h, kSpanClusterFlatten);
  cluster_flatten_kernel<><<<grid_for(n), kBlock, 0, h->stream>>>(parent, d_tot, mp, n, flags, d_err);
  HIP_TRY(hipGetLastError());
  rc = exclusive_scan_int(h, flags, pos, n + 1, pub_slot<int>(h, 0));
  if (rc) return rc;
  span_mark(h, kSpanClusterFlatten);
  span_mark(h, kSpanClusterBorder);
  cluster_walk_kernel<P4, true><<<gsz, 64, 0, h->stream>>>(pts, n, c.grid, sp, eps, mp, d_tot, parent, pos, d_labels, d_err);
  cluster_sizes_kernel<><<<grid_for(n), kBlock, 0, h->stream>>>(d_labels, n, d_sizes);
  span_mark(h, kSpanClusterBorder);
  HIP_TRY(hipGetLastError());
  int err = 0;
  rc = read_back(h, {{&err, d_err, sizeof(err)}});  // (waits for the stream: the scan's total is in its slot)
  if (rc) return rc;
  if (err) return fail(h, O3DS_ERR_HIP, "cluster_dbscan: a union-find loop exceeded its bound (never expected); no label is published");
  *n_clusters = (size_t)pub_value<int>(h, 0);
  return O3DS_OK;
}

int cluster_args(o3ds_handle h, const char* what, double eps, int min_points) {
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": eps must be a finite number greater than 0");
  if (min_points < 1) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": min_points < 1");
  return O3DS_OK;
}
constexpr const char* kClusterTooLarge = ": clouds of 2^31 points and more are unsupported (labels are 32-bit)";

template <typename P4>
int cluster_dbscan_t(o3ds_handle h, CloudRec& c, double eps, int min_points, int32_t* labels, size_t capacity, size_t* n_clusters, uint32_t* cluster_sizes,
                     size_t size_capacity) {
  const size_t n = c.n;
  int* d_labels = nullptr;
  uint32_t* d_sizes = nullptr;
  TMP_ALLOC(d_labels, sizeof(int) * n);
  TMP_ALLOC(d_sizes, sizeof(uint32_t) * n);
  size_t nc = 0;
  int rc = cluster_labels_t<P4>(h, c, eps, min_points, d_labels, d_sizes, &nc);
  if (rc) return rc;
  if (n_clusters) *n_clusters = nc;
  if (capacity < n) return fail(h, O3DS_ERR_CAPACITY, "cluster_dbscan: labels has room for fewer entries than the cloud has points");
  if (cluster_sizes && size_capacity < nc)
    return fail(h, O3DS_ERR_CAPACITY, "cluster_dbscan: cluster_sizes is too small for the clusters (*n_clusters holds their number)");
  rc = d2h_copy(h, labels, d_labels, sizeof(int32_t) * n);
  if (!rc && cluster_sizes && nc) rc = d2h_copy(h, cluster_sizes, d_sizes, sizeof(uint32_t) * nc);
  return rc;
}

template <typename P4>
int small_cluster_filter_t(o3ds_handle h, CloudRec& in, double eps, int min_points, int min_cluster_size, CloudRec& out, uint32_t* kept_idx, size_t capacity,
                           size_t* n_kept) {
  return filter_cloud_t<P4>(h, in, "remove_small_clusters", out, kept_idx, capacity, n_kept, [&](size_t n, int* flags) -> int {
    int* d_labels = nullptr;
    uint32_t* d_sizes = nullptr;
    TMP_ALLOC(d_labels, sizeof(int) * n);
    TMP_ALLOC(d_sizes, sizeof(uint32_t) * n);
    size_t nc = 0;
    const int rc = cluster_labels_t<P4>(h, in, eps, min_points, d_labels, d_sizes, &nc);
    if (rc) return rc;
    cluster_size_flag_kernel<><<<grid_for(n), kBlock, 0, h->stream>>>(d_labels, d_sizes, n, (uint32_t)min_cluster_size, flags);  // the labels stay here
    HIP_TRY(hipGetLastError());
    return O3DS_OK;
  });
}
}  // namespace

extern "C" {

int o3ds_cluster_dbscan(o3ds_handle h, o3ds_cloud cloud, double eps, int min_points, int32_t* labels, size_t capacity, size_t* n_clusters,
                        uint32_t* cluster_sizes, size_t size_capacity) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  const int ra = cluster_args(h, "cluster_dbscan", eps, min_points);
  if (ra) return ra;
  CloudRec* c = find_cloud(h, cloud);  // (with its exact size; a persistent map as its array)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cluster_dbscan: unknown cloud id");
  if (!n_clusters) return fail(h, O3DS_ERR_INVALID_ARG, "cluster_dbscan: n_clusters is required");
  *n_clusters = 0;
  if (c->n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_INVALID_ARG, std::string("cluster_dbscan") + kClusterTooLarge);
  if (c->n == 0) return O3DS_OK;  // an empty cloud has no cluster and is no error
  if (!labels) return fail(h, O3DS_ERR_INVALID_ARG, "cluster_dbscan: labels is NULL");
  return DISPATCH(c->precision, cluster_dbscan_t, h, *c, eps, min_points, labels, capacity, n_clusters, cluster_sizes, size_capacity);
}

int o3ds_remove_small_clusters(o3ds_handle h, o3ds_cloud in, double eps, int min_points, int min_cluster_size, o3ds_cloud* out, uint32_t* kept_idx,
                               size_t capacity, size_t* n_kept) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  const int ra = cluster_args(h, "remove_small_clusters", eps, min_points);
  if (ra) return ra;
  if (min_cluster_size < 1) return fail(h, O3DS_ERR_INVALID_ARG, "remove_small_clusters: min_cluster_size < 1");
  CloudRec* c = find_cloud(h, in);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "remove_small_clusters: unknown cloud id");
  if (!out || !n_kept) return fail(h, O3DS_ERR_INVALID_ARG, "remove_small_clusters: out and n_kept are required");
  if (c->n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_INVALID_ARG, std::string("remove_small_clusters") + kClusterTooLarge);
  return new_cloud(h, out, [&](CloudRec& o) {
    return DISPATCH(c->precision, small_cluster_filter_t, h, *c, eps, min_points, min_cluster_size, o, kept_idx, capacity, n_kept);
  });
}

}  // extern "C"

// The plane segmentation follows the clustering: its kernels are instantiated last of all.
namespace {
// ---- [O3D] SegmentPlane and the split by the plane (plane_kernels.hpp) -----------------------------------------------------------------
constexpr int64_t kPlaneMaxIterations = 1 << 24;
constexpr int kSpanPlaneEval = 14;

template <typename P4>
int segment_plane_t(o3ds_handle h, CloudRec& in, double thr, int ransac_n, int64_t num_iterations, uint64_t seed, o3ds_plane_result* out,
                    uint32_t* inlier_idx, size_t capacity, CloudRec* inl, CloudRec* rest) {
  const size_t n = in.n;
  const P4* pts = (const P4*)in.pts;
  PlaneState* st = nullptr;
  double *planes = nullptr, *perr = nullptr, *fit = nullptr, *rmse = nullptr, *partial = nullptr;
  uint32_t* pcnt = nullptr;
  int *flags = nullptr, *nflags = nullptr, *pos = nullptr;
  TMP_ALLOC(st, sizeof(PlaneState));
  TMP_ALLOC(planes, sizeof(double) * 4 * kPlaneBatch);
  TMP_ALLOC(perr, sizeof(double) * (size_t)kPlaneChunks * kPlaneBatch);
  TMP_ALLOC(pcnt, sizeof(uint32_t) * (size_t)kPlaneChunks * kPlaneBatch);
  TMP_ALLOC(fit, sizeof(double) * kPlaneBatch);
  TMP_ALLOC(rmse, sizeof(double) * kPlaneBatch);
  TMP_ALLOC(partial, sizeof(double) * 6 * kPlaneChunks);
  TMP_ALLOC(flags, sizeof(int) * (n + 1));
  TMP_ALLOC(nflags, sizeof(int) * (n + 1));
  TMP_ALLOC(pos, sizeof(int) * (n + 1));
  plane_init_kernel<><<<1, 1, 0, h->stream>>>(st);
  for (int64_t t0 = 0; t0 < num_iterations; t0 += kPlaneBatch) {
    const int count = (int)std::min<int64_t>(kPlaneBatch, num_iterations - t0);
    const unsigned int groups = (unsigned int)((count + 63) / 64);
    plane_hypothesis_kernel<P4><<<groups, 64, 0, h->stream>>>(pts, n, ransac_n, seed, (uint64_t)t0, count, planes);
    span_mark(h, kSpanPlaneEval);
    plane_eval_kernel<P4><<<dim3(groups, kPlaneChunks), 64, 0, h->stream>>>(pts, n, planes, thr, perr, pcnt);
    span_mark(h, kSpanPlaneEval);
    plane_finish_kernel<><<<groups * (64 / kPlaneFinishHyps), kBlock, 0, h->stream>>>(perr, pcnt, n, fit, rmse);
    plane_fold_kernel<><<<1, kBlock, 0, h->stream>>>(planes, fit, rmse, count, (long long)t0, st);
  }
  plane_mask_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>(pts, n, st, thr, flags, nflags);
  plane_sums_kernel<P4, 0><<<kPlaneChunks, 64, 0, h->stream>>>(pts, n, flags, st, partial);
  plane_sums_finish_kernel<0><<<1, kBlock, 0, h->stream>>>(partial, st);
  plane_sums_kernel<P4, 1><<<kPlaneChunks, 64, 0, h->stream>>>(pts, n, flags, st, partial);
  plane_sums_finish_kernel<1><<<1, kBlock, 0, h->stream>>>(partial, st);
  HIP_TRY(hipGetLastError());
  PlaneState s;
  int rc = read_back(h, {{&s, st, sizeof(s)}});
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) out->plane[k] = s.plane[k], out->best_plane[k] = s.best_plane[k];
  out->fitness = s.fitness;
  out->inlier_rmse = s.rmse;
  out->n_inliers = s.n_inliers;
  out->best_t = s.best_t;
  out->n_degenerate = s.n_degenerate;
  if (inlier_idx && s.n_inliers > capacity)
    return fail(h, O3DS_ERR_CAPACITY, "segment_plane: inlier_idx is too small for the inliers (n_inliers holds their number)");
  size_t m = 0;
  if (inl || inlier_idx) {  // SelectByIndex(inliers)
    CloudRec scratch;
    CloudGuard scratch_guard(h, scratch);
    CloudRec& o = inl ? *inl : scratch;
    rc = compact_kept_t<P4>(h, in, n, flags, pos, "segment_plane", o, inlier_idx, capacity, &m);
    if (rc) return rc;
  }
  if (rest)  // SelectByIndex(inliers, invert = true)
    rc = compact_kept_t<P4>(h, in, n, nflags, pos, "segment_plane", *rest, nullptr, 0, &m);
  return rc;
}
}  // namespace

extern "C" {

int o3ds_segment_plane(o3ds_handle h, o3ds_cloud cloud, double distance_threshold, int ransac_n, int64_t num_iterations, uint64_t seed,
                       o3ds_plane_result* out, uint32_t* inlier_idx, size_t capacity, o3ds_cloud* inliers_out, o3ds_cloud* rest_out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: out is required");
  *out = o3ds_plane_result{};
  out->best_t = -1;
  if (ransac_n < 3) return fail(h, O3DS_ERR_INVALID_ARG, "ransac_n should be set to higher than or equal to 3.");  // [O3D]
  if (ransac_n > kRansacMaxN) return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: ransac_n > 8 unsupported");
  if (num_iterations < 0 || num_iterations > kPlaneMaxIterations)
    return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: num_iterations is negative or above 16777216");
  if (!inlier_idx && capacity > 0) return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: inlier_idx is NULL with capacity > 0");
  CloudRec* c = find_cloud(h, cloud);  // (with its exact size; a persistent map as its array)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: unknown cloud id");
  if (c->n < (size_t)ransac_n) return fail(h, O3DS_ERR_INVALID_ARG, "There must be at least 'ransac_n' points.");  // [O3D]
  if (c->n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_INVALID_ARG, "segment_plane: clouds of 2^31 points and more are unsupported (the scan's positions are 32-bit)");
  return new_cloud(h, rest_out, [&](CloudRec& rest) {  // (the inner cloud gets its id first)
    return new_cloud(h, inliers_out, [&](CloudRec& inl) {
      return DISPATCH(c->precision, segment_plane_t, h, *c, distance_threshold, ransac_n, num_iterations, seed, out, inlier_idx, capacity,
                      inliers_out ? &inl : nullptr, rest_out ? &rest : nullptr);
    });
  });
}

}  // extern "C"

namespace {
// ---- [O3D] coloured ICP (colored_icp_kernels.hpp) ------------------------------------------------------------------------------------
constexpr int kSpanColorGradient = 15, kSpanColoredStep = 16;
constexpr int kColoredGradMaxNN = 30;  // [O3D] RegistrationColoredICP initialises its target with KDTreeSearchParamHybrid(2 r, 30)

bool cgrad_valid(const CloudRec& c) { return c.has_cgrad && c.cgrad && c.cgrad_n == c.n && !c.pm; }

// InitializePointCloudForColoredICP: the Hybrid lists of the cloud in itself stay in device arrays, one thread per point reads its own
template <typename P4>
int color_gradients_t(o3ds_handle h, CloudRec& c, double radius, int max_nn) {
  const size_t n = c.n;
  free_cgrad(h, c);
  if (n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_CAPACITY, "compute_color_gradients: clouds of 2^31 points and more are unsupported");
  const size_t grad_bytes = n * 3 * sizeof(double), list_bytes = n * (size_t)max_nn * sizeof(uint32_t);
  if (grad_bytes > pool_cap_bytes() || list_bytes > pool_cap_bytes())
    return fail(h, O3DS_ERR_CAPACITY, "compute_color_gradients: a buffer exceeds the pool cap (O3DS_POOL_CAP_MB)");
  uint32_t *d_idx = nullptr, *d_cnt = nullptr;
  bool empty = true;
  if (n) {
    TMP_ALLOC(d_idx, list_bytes);
    TMP_ALLOC(d_cnt, n * sizeof(uint32_t));
    const int rc = neighbor_launch_t<P4>(h, c, c, nullptr, nullptr, n, max_nn, radius, d_idx, nullptr, d_cnt, nullptr, nullptr, &empty);
    if (rc) return rc;
  }
  double* out = nullptr;
  HIP_TRY(dev_alloc(h, (void**)&out, std::max<size_t>(grad_bytes, 8)));
  c.cgrad = out;
  if (n && empty) {  // no point with three finite coordinates: every list is empty
    HIP_TRY(hipMemsetAsync(out, 0, grad_bytes, h->stream));
  } else if (n) {
    span_mark(h, kSpanColorGradient);
    color_gradient_kernel<P4><<<(unsigned int)((n + kBlock - 1) / kBlock), kBlock, 0, h->stream>>>((const P4*)c.pts, (const P4*)c.nrm, (const P4*)c.col, n, d_idx,
                                                                                                  d_cnt, max_nn, out);
    span_mark(h, kSpanColorGradient);
    HIP_TRY(hipGetLastError());
  }
  c.has_cgrad = true;
  c.cgrad_n = n;
  c.cgrad_radius = radius;
  c.cgrad_max_nn = max_nn;
  return O3DS_OK;
}

// what the passes of one call share: the search's arrays, the block sums, the record, and what the target needed once
struct ColoredPass {
  unsigned int* d_fin = nullptr;
  bool empty = true;  // no query or no finite target point: the record is zero
  uint32_t *d_idx = nullptr, *d_cnt = nullptr;
  double *d_d2 = nullptr, *d_partial = nullptr, *d_record = nullptr;
  size_t nblocks = 0;
};
template <typename P4>
int colored_prepare_t(o3ds_handle h, const CloudRec& s, CloudRec& t, double r, ColoredPass& cp) {
  cp.nblocks = (s.n + kColStepBlock - 1) / kColStepBlock;
  TMP_ALLOC(cp.d_record, sizeof(double) * kRec);
  if (s.n == 0) return O3DS_OK;
  TMP_ALLOC(cp.d_idx, sizeof(uint32_t) * s.n);
  TMP_ALLOC(cp.d_cnt, sizeof(uint32_t) * s.n);
  TMP_ALLOC(cp.d_d2, sizeof(double) * s.n);
  TMP_ALLOC(cp.d_partial, sizeof(double) * kRec * cp.nblocks);
  return neighbor_prepare_t<P4>(h, t, s.n, 1, r, &cp.d_fin, &cp.empty);
}
// one correspondence pass under T and its reduction into cp.d_record; nothing waits
template <typename P4>
int colored_pass_t(o3ds_handle h, const CloudRec& s, const CloudRec& t, const double T[16], double r, double sg, double sp, const ColoredPass& cp) {
  if (cp.empty) {
    HIP_TRY(hipMemsetAsync(cp.d_record, 0, sizeof(double) * kRec, h->stream));
    return O3DS_OK;
  }
  const int rc = neighbor_run_t<P4>(h, s, t, T, nullptr, s.n, 1, r, cp.d_fin, cp.d_idx, cp.d_d2, cp.d_cnt, nullptr, nullptr);
  if (rc) return rc;
  span_mark(h, kSpanColoredStep);
  colored_step_kernel<P4><<<(unsigned int)cp.nblocks, kColStepBlock, 0, h->stream>>>((const P4*)s.pts, (const P4*)s.col, s.n, mat34(T), (const P4*)t.pts,
                                                                                     (const P4*)t.nrm, (const P4*)t.col, t.cgrad, t.n, cp.d_idx, cp.d_cnt,
                                                                                     cp.d_d2, sg, sp, cp.d_partial);
  colored_finish_kernel<<<1, 64, 0, h->stream>>>(cp.d_partial, cp.nblocks, cp.d_record);
  span_mark(h, kSpanColoredStep);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

template <typename P4>
int colored_step_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double T[16], double r, double lambda, double record[32]) {
  ColoredPass cp;
  int rc = colored_prepare_t<P4>(h, s, t, r, cp);
  if (rc) return rc;
  rc = colored_pass_t<P4>(h, s, t, T, r, std::sqrt(lambda), std::sqrt(1.0 - lambda), cp);
  if (rc) return rc;
  return read_back(h, {{record, cp.d_record, sizeof(double) * kRec}});
}

// [O3D] RegistrationICP's loop around the joint step: the record of every pass goes to the tail the sharded path runs (icp_update_kernel:
// convergence test, 6x6 LDL^T, T <- U T), and the host reads the state it publishes -- the next pose and whether the loop has ended
// `pass(T, cp)` enqueues one correspondence pass under T and leaves its record in cp.d_record (colored_pass_t, robust_pass_t)
// `tail(cp)` enqueues the one-workgroup kernel that turns the record into the next state (icp_update_kernel, or the degeneracy-aware one)
// `cp` arrives prepared (colored_prepare_t for the passes that search, ndt_prepare for the one that does not): the loop itself knows
// nothing of how a pass finds its pairs
template <typename Pass, typename Tail>
int step_loop_run(o3ds_handle h, size_t n_src, const double init[16], const o3ds_icp_params& p, o3ds_icp_result* out, const ColoredPass& cp, Pass pass,
                  Tail tail) {
  int rc = O3DS_OK;
  h->session = false;  // (the handle's one state is taken: a step-wise session that was open is over)
  IcpStateDev st{};
  memcpy(st.T, init, sizeof(double) * 16);
  *h->h_state = st;
  if (n_src == 0) {  // [O3D]: no correspondence, fitness 0, the initial pose
    copy_result(h, out);
    return O3DS_OK;
  }
  HIP_TRY(hipMemcpyAsync(h->d_state, h->h_state, sizeof(IcpStateDev), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (h_state is read back into below)
  for (int j = 0; j <= p.max_iteration; ++j) {
    double T[16];
    memcpy(T, h->h_state->T, sizeof(T));
    rc = pass(T, cp);
    if (rc) return rc;
    tail(cp);
    HIP_TRY(hipGetLastError());
    rc = read_state(h, out);
    if (rc) return rc;
    if (h->h_state->done) break;
  }
  return O3DS_OK;
}
// the loop of the passes that search: the search is prepared here, once per call
template <typename P4, typename Pass, typename Tail>
int step_loop_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double init[16], const o3ds_icp_params& p, o3ds_icp_result* out, Pass pass, Tail tail) {
  ColoredPass cp;
  const int rc = colored_prepare_t<P4>(h, s, t, p.max_correspondence_distance, cp);  // the finite count's read-back and the index check: once, not per pass
  if (rc) return rc;
  return step_loop_run(h, s.n, init, p, out, cp, pass, tail);
}
// the ordinary tail: the solve and update every step loop runs, with the point-to-plane treatment of an empty set
void update_tail(o3ds_handle h, const ColoredPass& cp, size_t n_src, const o3ds_icp_params& p) {
  icp_update_kernel<<<1, 128, 0, h->stream>>>(cp.d_record, h->d_state, (unsigned long long)n_src, p.max_iteration, p.relative_fitness, p.relative_rmse,
                                             O3DS_ICP_POINT_TO_PLANE, nullptr, 0);
}
template <typename P4, typename Pass>
int step_loop_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double init[16], const o3ds_icp_params& p, o3ds_icp_result* out, Pass pass) {
  return step_loop_t<P4>(h, s, t, init, p, out, pass, [&](const ColoredPass& cp) { update_tail(h, cp, s.n, p); });
}

// the target's gradients of (2 r, 30), as [O3D] RegistrationColoredICP initialises it: made if absent or of other parameters, and left
template <typename P4>
int ensure_registration_gradients_t(o3ds_handle h, CloudRec& t, double r) {
  if (cgrad_valid(t) && t.cgrad_radius == 2.0 * r && t.cgrad_max_nn == kColoredGradMaxNN) return O3DS_OK;
  return color_gradients_t<P4>(h, t, 2.0 * r, kColoredGradMaxNN);
}

template <typename P4>
int colored_register_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double init[16], const o3ds_icp_params& p, double lambda, o3ds_icp_result* out) {
  const double r = p.max_correspondence_distance;
  const int rc = ensure_registration_gradients_t<P4>(h, t, r);
  if (rc) return rc;
  const double sg = std::sqrt(lambda), sp = std::sqrt(1.0 - lambda);
  return step_loop_t<P4>(h, s, t, init, p, out, [&](const double* T, const ColoredPass& cp) { return colored_pass_t<P4>(h, s, t, T, r, sg, sp, cp); });
}

// ---- [O3D] robust loss kernels on the point-to-plane and the coloured estimator (robust_icp_kernels.hpp) ------------------------------
constexpr int kSpanRobustStep = 17;

struct RobustSpec {
  bool colored = false;
  double sg = 1.0, sp = 0.0;  // sqrt(lambda), sqrt(1 - lambda); COLORED only
  RobustLossDev loss{O3DS_LOSS_L2, 0.0};
};

// one correspondence pass under T and its weighted reduction into cp.d_record; nothing waits
template <typename P4>
int robust_pass_t(o3ds_handle h, const CloudRec& s, const CloudRec& t, const double T[16], double r, const RobustSpec& spec, const ColoredPass& cp) {
  if (cp.empty) {
    HIP_TRY(hipMemsetAsync(cp.d_record, 0, sizeof(double) * kRec, h->stream));
    return O3DS_OK;
  }
  const int rc = neighbor_run_t<P4>(h, s, t, T, nullptr, s.n, 1, r, cp.d_fin, cp.d_idx, cp.d_d2, cp.d_cnt, nullptr, nullptr);
  if (rc) return rc;
  const unsigned int grid = (unsigned int)cp.nblocks;
  span_mark(h, kSpanRobustStep);
  if (spec.colored)
    robust_step_kernel<P4, true><<<grid, kColStepBlock, 0, h->stream>>>((const P4*)s.pts, (const P4*)s.col, s.n, mat34(T), (const P4*)t.pts, (const P4*)t.nrm,
                                                                       (const P4*)t.col, t.cgrad, t.n, cp.d_idx, cp.d_cnt, cp.d_d2, spec.sg, spec.sp, spec.loss,
                                                                       cp.d_partial);
  else
    robust_step_kernel<P4, false><<<grid, kColStepBlock, 0, h->stream>>>((const P4*)s.pts, nullptr, s.n, mat34(T), (const P4*)t.pts, (const P4*)t.nrm, nullptr,
                                                                        nullptr, t.n, cp.d_idx, cp.d_cnt, cp.d_d2, 1.0, 0.0, spec.loss, cp.d_partial);
  colored_finish_kernel<<<1, 64, 0, h->stream>>>(cp.d_partial, cp.nblocks, cp.d_record);
  span_mark(h, kSpanRobustStep);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

template <typename P4>
int robust_step_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double T[16], double r, const RobustSpec& spec, double record[32]) {
  ColoredPass cp;
  int rc = colored_prepare_t<P4>(h, s, t, r, cp);
  if (rc) return rc;
  rc = robust_pass_t<P4>(h, s, t, T, r, spec, cp);
  if (rc) return rc;
  return read_back(h, {{record, cp.d_record, sizeof(double) * kRec}});
}

template <typename P4>
int robust_register_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double init[16], const o3ds_icp_params& p, const RobustSpec& spec,
                      o3ds_icp_result* out) {
  const double r = p.max_correspondence_distance;
  if (spec.colored) {
    const int rc = ensure_registration_gradients_t<P4>(h, t, r);
    if (rc) return rc;
  }
  return step_loop_t<P4>(h, s, t, init, p, out, [&](const double* T, const ColoredPass& cp) { return robust_pass_t<P4>(h, s, t, T, r, spec, cp); });
}

// the checks the step and the registration share; *src / *tgt with their exact sizes, a persistent map folded into its array
int validate_colored(o3ds_handle h, const char* what, o3ds_cloud source, o3ds_cloud target, double r, double lambda, CloudRec** src, CloudRec** tgt) {
  CloudRec* s = find_cloud(h, source);
  CloudRec* t = s ? find_cloud(h, target) : nullptr;
  if (!s || !t) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown cloud id");
  if (!(r > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");  // [O3D] RegistrationICP
  if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": lambda_geometric must be in [0, 1]");
  if (t->n == 0) return fail(h, O3DS_ERR_EMPTY, std::string(what) + ": empty target");
  if (s->precision != t->precision) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": source/target precision mismatch");
  if (!t->nrm) return fail(h, O3DS_ERR_NO_NORMALS, "ColoredICP requires target pointcloud to have normals.");  // [O3D]
  if (!t->col) return fail(h, O3DS_ERR_INVALID_ARG, "ColoredICP requires target pointcloud to have colors.");  // [O3D]
  if (s->n > 0 && !s->col) return fail(h, O3DS_ERR_INVALID_ARG, "ColoredICP requires source pointcloud to have colors.");  // [O3D]
  *src = s;
  *tgt = t;
  return O3DS_OK;
}

// a caller's loss in the form the kernels take
int validate_loss(o3ds_handle h, const char* what, const o3ds_robust_loss* loss, RobustLossDev* out) {
  if (!loss) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": null loss");
  if (loss->kind < O3DS_LOSS_L2 || loss->kind > O3DS_LOSS_TUKEY) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown loss kind");
  if (loss->reserved != 0) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": o3ds_robust_loss.reserved must be 0");
  const bool uses_k = loss->kind != O3DS_LOSS_L2 && loss->kind != O3DS_LOSS_L1;
  if (uses_k && !(std::isfinite(loss->k) && loss->k > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": the loss's k must be finite and > 0");
  *out = RobustLossDev{loss->kind, uses_k ? loss->k : 1.0};
  return O3DS_OK;
}

// the loss and the estimator, then the clouds: COLORED is held to validate_colored, POINT_TO_PLANE to its checks without the colours
int validate_robust(o3ds_handle h, const char* what, o3ds_cloud source, o3ds_cloud target, double r, int estimator, double lambda,
                    const o3ds_robust_loss* loss, RobustSpec* spec, CloudRec** src, CloudRec** tgt) {
  const int rl = validate_loss(h, what, loss, &spec->loss);
  if (rl) return rl;
  if (estimator != O3DS_ROBUST_POINT_TO_PLANE && estimator != O3DS_ROBUST_COLORED)
    return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown estimator");
  spec->colored = estimator == O3DS_ROBUST_COLORED;
  if (spec->colored) {
    spec->sg = std::sqrt(lambda);
    spec->sp = std::sqrt(1.0 - lambda);
    return validate_colored(h, what, source, target, r, lambda, src, tgt);
  }
  CloudRec* s = find_cloud(h, source);
  CloudRec* t = s ? find_cloud(h, target) : nullptr;
  if (!s || !t) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown cloud id");
  if (!(r > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "Invalid max_correspondence_distance.");  // [O3D] RegistrationICP
  if (t->n == 0) return fail(h, O3DS_ERR_EMPTY, std::string(what) + ": empty target");
  if (s->precision != t->precision) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": source/target precision mismatch");
  if (!t->nrm) return fail(h, O3DS_ERR_NO_NORMALS, "TransformationEstimationPointToPlane requires pre-computed normal vectors for target PointCloud.");  // [O3D]
  *src = s;
  *tgt = t;
  return O3DS_OK;
}

// ---- degeneracy-aware ICP (degeneracy_kernels.hpp): the analysis of a pass's 6x6 system and the update constrained to what it observes ----
struct DegeneracyRun {
  DegeneracyDev* d_dg = nullptr;
  double* d_c0 = nullptr;
};

// the device struct next to the state, zeroed, and c0 = the source's centre as o3ds_cloud_center forms it: once per call, nothing waits
template <typename P4>
int degeneracy_prepare_t(o3ds_handle h, const CloudRec& s, DegeneracyRun& run) {
  TMP_ALLOC(run.d_dg, sizeof(DegeneracyDev));
  TMP_ALLOC(run.d_c0, sizeof(double) * 3);
  HIP_TRY(hipMemsetAsync(run.d_dg, 0, sizeof(DegeneracyDev), h->stream));
  HIP_TRY(hipMemsetAsync(run.d_c0, 0, sizeof(double) * 3, h->stream));
  if (s.n == 0) return O3DS_OK;
  double* partial = nullptr;
  TMP_ALLOC(partial, sizeof(double) * 3 * kCenterChunks);
  const CountRef cnt = count_ref(h, s);
  center_partial_kernel<P4><<<kCenterChunks, kBlock, 0, h->stream>>>((const P4*)s.pts, cnt, partial);
  center_finish_kernel<<<1, kBlock, 0, h->stream>>>(partial, cnt, run.d_c0);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

void degeneracy_tail(o3ds_handle h, const ColoredPass& cp, const DegeneracyRun& run, const o3ds_degeneracy_params& dp, size_t n_src, int max_iter,
                     double rel_fitness, double rel_rmse) {
  icp_degeneracy_update_kernel<<<1, 128, 0, h->stream>>>(cp.d_record, h->d_state, run.d_dg, run.d_c0, dp.min_eigenvalue_rotation,
                                                         dp.min_eigenvalue_translation, (unsigned long long)n_src, max_iter, rel_fitness, rel_rmse);
}

template <typename P4>
int degeneracy_register_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double init[16], const o3ds_icp_params& p, const RobustSpec& spec,
                          const o3ds_degeneracy_params& dp, o3ds_icp_result* out, o3ds_degeneracy_report* report) {
  const double r = p.max_correspondence_distance;
  if (report) memset(report, 0, sizeof(*report));
  if (spec.colored) {
    const int rc = ensure_registration_gradients_t<P4>(h, t, r);
    if (rc) return rc;
  }
  DegeneracyRun run;
  int rc = degeneracy_prepare_t<P4>(h, s, run);
  if (rc) return rc;
  rc = step_loop_t<P4>(
      h, s, t, init, p, out, [&](const double* T, const ColoredPass& cp) { return robust_pass_t<P4>(h, s, t, T, r, spec, cp); },
      [&](const ColoredPass& cp) { degeneracy_tail(h, cp, run, dp, s.n, p.max_iteration, p.relative_fitness, p.relative_rmse); });
  if (rc || !report || s.n == 0) return rc;
  DegeneracyDev dg;
  rc = read_back(h, {{&dg, run.d_dg, sizeof(dg)}});
  if (rc) return rc;
  memcpy(report->centre, dg.centre, sizeof(dg.centre));
  memcpy(report->eigenvalues, dg.eigenvalues, sizeof(dg.eigenvalues));
  memcpy(report->eigenvectors, dg.eigenvectors, sizeof(dg.eigenvectors));
  for (int k = 0; k < 6; ++k) {
    report->degenerate[k] = dg.degenerate[k];
    report->ever_degenerate[k] = dg.ever_degenerate[k];
  }
  report->n_degenerate = dg.n_degenerate;
  report->n_passes_constrained = dg.n_passes_constrained;
  return O3DS_OK;
}

// one pass under T and the tail on a fresh state that may apply one update: the record, the analysis and the x of that pass
template <typename P4>
int localizability_t(o3ds_handle h, const CloudRec& s, CloudRec& t, const double T[16], double r, const RobustSpec& spec, const o3ds_degeneracy_params& dp,
                     o3ds_localizability* out) {
  memset(out, 0, sizeof(*out));
  ColoredPass cp;
  int rc = colored_prepare_t<P4>(h, s, t, r, cp);
  if (rc) return rc;
  DegeneracyRun run;
  rc = degeneracy_prepare_t<P4>(h, s, run);
  if (rc) return rc;
  h->session = false;  // (the handle's one state is taken, as by a registration)
  IcpStateDev st{};
  memcpy(st.T, T, sizeof(double) * 16);
  *h->h_state = st;
  HIP_TRY(hipMemcpyAsync(h->d_state, h->h_state, sizeof(IcpStateDev), hipMemcpyHostToDevice, h->stream));
  rc = robust_pass_t<P4>(h, s, t, T, r, spec, cp);
  if (rc) return rc;
  degeneracy_tail(h, cp, run, dp, std::max<size_t>(s.n, 1), 1, 0.0, 0.0);
  HIP_TRY(hipGetLastError());
  DegeneracyDev dg;
  rc = read_back(h, {{out->record, cp.d_record, sizeof(double) * kRec}, {&dg, run.d_dg, sizeof(dg)}});
  if (rc) return rc;
  memcpy(out->centre, dg.centre, sizeof(dg.centre));
  memcpy(out->eigenvalues, dg.eigenvalues, sizeof(dg.eigenvalues));
  memcpy(out->eigenvectors, dg.eigenvectors, sizeof(dg.eigenvectors));
  for (int k = 0; k < 6; ++k) out->degenerate[k] = dg.degenerate[k];
  out->n_degenerate = dg.n_degenerate;
  memcpy(out->x, dg.x, sizeof(dg.x));
  return O3DS_OK;
}

int validate_degeneracy(o3ds_handle h, const char* what, const o3ds_degeneracy_params* dp) {
  if (!dp) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": null degeneracy params");
  for (const double v : {dp->min_eigenvalue_rotation, dp->min_eigenvalue_translation})
    if (!(std::isfinite(v) && v >= 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": a minimum eigenvalue must be finite and >= 0");
  return O3DS_OK;
}

// ---- search-free registration against voxel Gaussians (ndt_kernels.hpp) ---------------------------------------------------------------
constexpr int kSpanNdtBuild = 18, kSpanNdtStep = 19;

// keys, the stable sort, segment heads, one statistics kernel; two read-backs (the sizes, then the counters)
template <typename P4>
int voxel_gaussians_build_t(o3ds_handle h, const CloudRec& c, const o3ds_voxel_gaussian_params& vp, NdtRec& g) {
  const size_t n = c.n;
  g.voxel = vp.voxel_size;
  if (n >= ((size_t)1 << 31)) return fail(h, O3DS_ERR_CAPACITY, "voxel_gaussians_create: clouds of 2^31 points and more are unsupported");
  if (n * sizeof(NdtVoxel) > pool_cap_bytes())  // (the largest array of the object, had every point a voxel of its own)
    return fail(h, O3DS_ERR_CAPACITY, "voxel_gaussians_create: a buffer exceeds the pool cap (O3DS_POOL_CAP_MB)");
  if (n == 0) return O3DS_OK;
  unsigned long long *k0 = nullptr, *k1 = nullptr, *d_inside = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  int *head = nullptr, *seg_id = nullptr, *seg_start = nullptr;
  unsigned int* d_counters = nullptr;
  TMP_ALLOC(k0, sizeof(unsigned long long) * n);
  TMP_ALLOC(k1, sizeof(unsigned long long) * n);
  TMP_ALLOC(v0, sizeof(uint32_t) * n);
  TMP_ALLOC(v1, sizeof(uint32_t) * n);
  TMP_ALLOC(head, sizeof(int) * (n + 1));
  TMP_ALLOC(seg_id, sizeof(int) * (n + 1));
  TMP_ALLOC(d_inside, sizeof(unsigned long long));
  TMP_ALLOC(d_counters, sizeof(unsigned int) * 2);
  span_mark(h, kSpanNdtBuild);
  ndt_key_kernel<P4><<<grid_for(n), kBlock, 0, h->stream>>>((const P4*)c.pts, n, vp.voxel_size, k0, v0);
  int rc = sort_pairs(h, k0, k1, v0, v1, n);
  if (!rc) {
    ndt_inside_kernel<<<1, 64, 0, h->stream>>>(k1, n, d_inside);
    rc = key_segments(h, k1, n, head, seg_id, nullptr);
  }
  int n_seg = 0;
  unsigned long long n_inside = 0;
  if (!rc) rc = read_back(h, {{&n_seg, seg_id + n, sizeof(int)}, {&n_inside, d_inside, sizeof(n_inside)}});
  if (rc) {
    span_mark(h, kSpanNdtBuild);
    return rc;
  }
  const size_t n_vox = (size_t)n_seg - (n_inside < n ? 1 : 0);  // the points without a voxel share the last key
  g.info.n_skipped_points = n - n_inside;
  if (n_vox == 0) {
    span_mark(h, kSpanNdtBuild);
    return O3DS_OK;
  }
  TMP_ALLOC(seg_start, sizeof(int) * ((size_t)n_seg + 1));
  segment_start_kernel<<<grid_for(n), kBlock, 0, h->stream>>>(head, seg_id, n, seg_start);
  DevGuard guard(h);
  for (void** q : {(void**)&g.keys, (void**)&g.counts, (void**)&g.mean, (void**)&g.cov, (void**)&g.information, (void**)&g.valid, (void**)&g.rec}) guard.add(q);
  HIP_TRY(dev_alloc(h, (void**)&g.keys, sizeof(unsigned long long) * n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.counts, sizeof(uint32_t) * n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.mean, sizeof(double) * 3 * n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.cov, sizeof(double) * 6 * n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.information, sizeof(double) * 6 * n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.valid, n_vox));
  HIP_TRY(dev_alloc(h, (void**)&g.rec, sizeof(NdtVoxel) * n_vox));
  HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(unsigned int) * 2, h->stream));
  ndt_stats_kernel<P4><<<(unsigned int)((n_vox + kBlock - 1) / kBlock), kBlock, 0, h->stream>>>((const P4*)c.pts, k1, v1, seg_start, n_vox, (size_t)n_inside,
                                                                                               vp.min_points, vp.min_eigenvalue_ratio, g.keys, g.counts, g.mean,
                                                                                               g.cov, g.information, g.valid, g.rec, d_counters);
  span_mark(h, kSpanNdtBuild);
  HIP_TRY(hipGetLastError());
  unsigned int counters[2] = {0, 0};
  rc = read_back(h, {{counters, d_counters, sizeof(counters)}});
  if (rc) return rc;
  guard.release();
  g.n_vox = n_vox;
  g.info.n_voxels = n_vox;
  g.info.n_valid = counters[0];
  g.info.n_flat = counters[1];
  return O3DS_OK;
}

// what the passes of one call share; no search is prepared.  A target without a valid voxel gives the zero record
int ndt_prepare(o3ds_handle h, const CloudRec& s, const NdtRec& g, ColoredPass& cp) {
  cp.nblocks = (s.n + kColStepBlock - 1) / kColStepBlock;
  TMP_ALLOC(cp.d_record, sizeof(double) * kRec);
  if (s.n == 0) return O3DS_OK;
  TMP_ALLOC(cp.d_partial, sizeof(double) * kRec * cp.nblocks);
  cp.empty = g.info.n_valid == 0;
  return O3DS_OK;
}
// one pass under T and its reduction into cp.d_record; nothing waits
template <typename P4>
int ndt_pass_t(o3ds_handle h, const CloudRec& s, const NdtRec& g, const double T[16], int neighbourhood, RobustLossDev loss, const ColoredPass& cp) {
  if (cp.empty) {
    HIP_TRY(hipMemsetAsync(cp.d_record, 0, sizeof(double) * kRec, h->stream));
    return O3DS_OK;
  }
  span_mark(h, kSpanNdtStep);
  ndt_step_kernel<P4><<<(unsigned int)cp.nblocks, kColStepBlock, 0, h->stream>>>((const P4*)s.pts, s.n, mat34(T), g.voxel, g.keys, g.rec, g.n_vox, neighbourhood, loss,
                                                                                 cp.d_partial);
  colored_finish_kernel<<<1, 64, 0, h->stream>>>(cp.d_partial, cp.nblocks, cp.d_record);
  span_mark(h, kSpanNdtStep);
  HIP_TRY(hipGetLastError());
  return O3DS_OK;
}

template <typename P4>
int ndt_step_t(o3ds_handle h, const CloudRec& s, const NdtRec& g, const double T[16], int neighbourhood, RobustLossDev loss, double record[32]) {
  ColoredPass cp;
  int rc = ndt_prepare(h, s, g, cp);
  if (rc) return rc;
  rc = ndt_pass_t<P4>(h, s, g, T, neighbourhood, loss, cp);
  if (rc) return rc;
  return read_back(h, {{record, cp.d_record, sizeof(double) * kRec}});
}

template <typename P4>
int ndt_register_t(o3ds_handle h, const CloudRec& s, const NdtRec& g, const double init[16], const o3ds_icp_params& p, int neighbourhood, RobustLossDev loss,
                   o3ds_icp_result* out) {
  ColoredPass cp;
  const int rc = ndt_prepare(h, s, g, cp);
  if (rc) return rc;
  return step_loop_run(
      h, s.n, init, p, out, cp, [&](const double* T, const ColoredPass& c) { return ndt_pass_t<P4>(h, s, g, T, neighbourhood, loss, c); },
      [&](const ColoredPass& c) { update_tail(h, c, s.n, p); });
}

// the checks the step and the registration share
int validate_ndt(o3ds_handle h, const char* what, o3ds_cloud source, o3ds_voxel_gaussians target, int neighbourhood, const o3ds_robust_loss* loss,
                 RobustLossDev* ld, CloudRec** src, NdtRec** tgt) {
  const int rc = validate_loss(h, what, loss, ld);
  if (rc) return rc;
  if (neighbourhood != 1 && neighbourhood != 7) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": neighbourhood must be 1 or 7");
  CloudRec* s = find_cloud(h, source);
  if (!s) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown cloud id");
  auto it = h->voxel_gaussians.find(target);
  if (it == h->voxel_gaussians.end()) return fail(h, O3DS_ERR_INVALID_ARG, std::string(what) + ": unknown voxel Gaussians id");
  *src = s;
  *tgt = &it->second;
  return O3DS_OK;
}
}  // namespace

extern "C" {

int o3ds_compute_color_gradients(o3ds_handle h, o3ds_cloud cloud, double radius, int max_nn) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  CloudRec* c = find_cloud(h, cloud);  // (with its exact size; a persistent map as its array)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "compute_color_gradients: unknown cloud id");
  if (!(radius > 0.0)) return fail(h, O3DS_ERR_INVALID_ARG, "compute_color_gradients: radius must be > 0");
  if (max_nn < 1 || max_nn > 128) return fail(h, O3DS_ERR_INVALID_ARG, "compute_color_gradients: max_nn outside 1..128");
  if (c->n > 0 && !c->nrm) return fail(h, O3DS_ERR_NO_NORMALS, "compute_color_gradients: the cloud has no normals");
  if (c->n > 0 && !c->col) return fail(h, O3DS_ERR_INVALID_ARG, "compute_color_gradients: the cloud has no colours");
  return DISPATCH(c->precision, color_gradients_t, h, *c, radius, max_nn);
}

int o3ds_cloud_has_color_gradients(o3ds_handle h, o3ds_cloud cloud, int* has_gradients) {
  CHECK_HANDLE(h);
  if (!has_gradients) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_has_color_gradients: null argument");
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_has_color_gradients: unknown cloud id");
  *has_gradients = cgrad_valid(*c) ? 1 : 0;
  return O3DS_OK;
}

int o3ds_cloud_download_color_gradients(o3ds_handle h, o3ds_cloud cloud, double* out, size_t capacity) {
  CHECK_HANDLE(h);
  CloudRec* c = find_cloud(h, cloud);
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_color_gradients: unknown cloud id");
  if (!cgrad_valid(*c)) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_color_gradients: the cloud has no colour gradients");
  if (capacity < c->n) return fail(h, O3DS_ERR_CAPACITY, "cloud_download_color_gradients: buffer too small");
  if (c->n == 0) return O3DS_OK;
  if (!out) return fail(h, O3DS_ERR_INVALID_ARG, "cloud_download_color_gradients: null buffer");
  return d2h_copy(h, out, c->cgrad, c->n * 3 * sizeof(double));
}

int o3ds_colored_icp_step(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance,
                          double lambda_geometric, double record[32]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !record) return fail(h, O3DS_ERR_INVALID_ARG, "colored_icp_step: null argument");
  CloudRec *s = nullptr, *t = nullptr;
  const int rc = validate_colored(h, "colored_icp_step", source, target, max_correspondence_distance, lambda_geometric, &s, &t);
  if (rc) return rc;
  if (!cgrad_valid(*t)) return fail(h, O3DS_ERR_INVALID_ARG, "colored_icp_step: the target has no colour gradients (o3ds_compute_color_gradients)");
  return DISPATCH(t->precision, colored_step_t, h, *s, *t, T, max_correspondence_distance, lambda_geometric, record);
}

int o3ds_icp_colored_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* params,
                         double lambda_geometric, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init || !params || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_colored: null argument");
  if (params->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp_colored: negative max_iteration");
  CloudRec *s = nullptr, *t = nullptr;
  const int rc = validate_colored(h, "icp_colored", source, target, params->max_correspondence_distance, lambda_geometric, &s, &t);
  if (rc) return rc;
  return DISPATCH(t->precision, colored_register_t, h, *s, *t, init, *params, lambda_geometric, out);
}

int o3ds_robust_icp_step(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance, int estimator,
                         double lambda_geometric, const o3ds_robust_loss* loss, double record[32]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !record) return fail(h, O3DS_ERR_INVALID_ARG, "robust_icp_step: null argument");
  CloudRec *s = nullptr, *t = nullptr;
  RobustSpec spec;
  const int rc = validate_robust(h, "robust_icp_step", source, target, max_correspondence_distance, estimator, lambda_geometric, loss, &spec, &s, &t);
  if (rc) return rc;
  if (spec.colored && !cgrad_valid(*t))
    return fail(h, O3DS_ERR_INVALID_ARG, "robust_icp_step: the target has no colour gradients (o3ds_compute_color_gradients)");
  return DISPATCH(t->precision, robust_step_t, h, *s, *t, T, max_correspondence_distance, spec, record);
}

int o3ds_icp_robust_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* params, int estimator,
                        double lambda_geometric, const o3ds_robust_loss* loss, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init || !params || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_robust: null argument");
  if (params->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp_robust: negative max_iteration");
  CloudRec *s = nullptr, *t = nullptr;
  RobustSpec spec;
  const int rc = validate_robust(h, "icp_robust", source, target, params->max_correspondence_distance, estimator, lambda_geometric, loss, &spec, &s, &t);
  if (rc) return rc;
  return DISPATCH(t->precision, robust_register_t, h, *s, *t, init, *params, spec, out);
}

int o3ds_icp_localizability(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance, int estimator,
                            double lambda_geometric, const o3ds_robust_loss* loss, const o3ds_degeneracy_params* params, o3ds_localizability* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_localizability: null argument");
  int rc = validate_degeneracy(h, "icp_localizability", params);
  if (rc) return rc;
  CloudRec *s = nullptr, *t = nullptr;
  RobustSpec spec;
  rc = validate_robust(h, "icp_localizability", source, target, max_correspondence_distance, estimator, lambda_geometric, loss, &spec, &s, &t);
  if (rc) return rc;
  if (spec.colored && !cgrad_valid(*t))
    return fail(h, O3DS_ERR_INVALID_ARG, "icp_localizability: the target has no colour gradients (o3ds_compute_color_gradients)");
  return DISPATCH(t->precision, localizability_t, h, *s, *t, T, max_correspondence_distance, spec, *params, out);
}

int o3ds_icp_degeneracy_aware_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* icp_params,
                                  int estimator, double lambda_geometric, const o3ds_robust_loss* loss, const o3ds_degeneracy_params* params,
                                  o3ds_icp_result* out, o3ds_degeneracy_report* report) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init || !icp_params || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_degeneracy_aware: null argument");
  if (icp_params->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp_degeneracy_aware: negative max_iteration");
  int rc = validate_degeneracy(h, "icp_degeneracy_aware", params);
  if (rc) return rc;
  CloudRec *s = nullptr, *t = nullptr;
  RobustSpec spec;
  rc = validate_robust(h, "icp_degeneracy_aware", source, target, icp_params->max_correspondence_distance, estimator, lambda_geometric, loss, &spec, &s,
                       &t);
  if (rc) return rc;
  return DISPATCH(t->precision, degeneracy_register_t, h, *s, *t, init, *icp_params, spec, *params, out, report);
}

int o3ds_voxel_gaussians_create(o3ds_handle h, o3ds_cloud cloud, const o3ds_voxel_gaussian_params* params, o3ds_voxel_gaussians* out,
                                o3ds_voxel_gaussians_info* info) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!params || !out) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: null argument");
  if (!(std::isfinite(params->voxel_size) && params->voxel_size > 0.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: voxel_size must be finite and > 0");
  if (params->min_points < 2) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: min_points must be at least 2");
  if (!(params->min_eigenvalue_ratio > 0.0 && params->min_eigenvalue_ratio <= 1.0))
    return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: min_eigenvalue_ratio must be in (0, 1]");
  if (params->reserved != 0) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: o3ds_voxel_gaussian_params.reserved must be 0");
  CloudRec* c = find_cloud(h, cloud);  // (with its exact size; a persistent map as its array)
  if (!c) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_create: unknown cloud id");
  NdtRec g;
  const int rc = DISPATCH(c->precision, voxel_gaussians_build_t, h, *c, *params, g);
  if (rc) return rc;
  const uint64_t id = h->next_id++;
  h->voxel_gaussians.emplace(id, g);
  *out = id;
  if (info) *info = g.info;
  return O3DS_OK;
}

int o3ds_voxel_gaussians_free(o3ds_handle h, o3ds_voxel_gaussians id) {
  CHECK_HANDLE(h);
  auto it = h->voxel_gaussians.find(id);
  if (it == h->voxel_gaussians.end()) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_free: unknown id");
  ndt_release(h, it->second);  // (whatever still reads the arrays was enqueued earlier on the handle's one stream)
  h->voxel_gaussians.erase(it);
  return O3DS_OK;
}

int o3ds_voxel_gaussians_info_get(o3ds_handle h, o3ds_voxel_gaussians id, o3ds_voxel_gaussians_info* info, double* voxel_size) {
  CHECK_HANDLE(h);
  auto it = h->voxel_gaussians.find(id);
  if (it == h->voxel_gaussians.end() || !info) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_info_get: bad argument");
  *info = it->second.info;
  if (voxel_size) *voxel_size = it->second.voxel;
  return O3DS_OK;
}

int o3ds_voxel_gaussians_download(o3ds_handle h, o3ds_voxel_gaussians id, int32_t* keys, uint32_t* counts, double* mean, double* cov, double* information,
                                  uint8_t* valid, size_t capacity) {
  CHECK_HANDLE(h);
  auto it = h->voxel_gaussians.find(id);
  if (it == h->voxel_gaussians.end()) return fail(h, O3DS_ERR_INVALID_ARG, "voxel_gaussians_download: unknown id");
  const NdtRec& g = it->second;
  const size_t n = g.n_vox;
  if (capacity < n) return fail(h, O3DS_ERR_CAPACITY, "voxel_gaussians_download: buffer too small");
  if (n == 0) return O3DS_OK;
  int rc = O3DS_OK;
  if (keys) {
    std::vector<unsigned long long> packed(n);
    rc = d2h_copy(h, packed.data(), g.keys, n * sizeof(unsigned long long));
    for (size_t v = 0; v < n && !rc; ++v)
      for (int a = 0; a < 3; ++a) keys[3 * v + a] = (int32_t)((long long)((packed[v] >> (21 * a)) & 0x1FFFFFull) - (1ll << 20));
  }
  if (!rc && counts) rc = d2h_copy(h, counts, g.counts, n * sizeof(uint32_t));
  if (!rc && mean) rc = d2h_copy(h, mean, g.mean, n * 3 * sizeof(double));
  if (!rc && cov) rc = d2h_copy(h, cov, g.cov, n * 6 * sizeof(double));
  if (!rc && information) rc = d2h_copy(h, information, g.information, n * 6 * sizeof(double));
  if (!rc && valid) rc = d2h_copy(h, valid, g.valid, n);
  return rc;
}

int o3ds_ndt_step(o3ds_handle h, o3ds_cloud source, o3ds_voxel_gaussians target, const double T[16], int neighbourhood, const o3ds_robust_loss* loss,
                  double record[32]) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!T || !record) return fail(h, O3DS_ERR_INVALID_ARG, "ndt_step: null argument");
  CloudRec* s = nullptr;
  NdtRec* g = nullptr;
  RobustLossDev ld{O3DS_LOSS_L2, 0.0};
  const int rc = validate_ndt(h, "ndt_step", source, target, neighbourhood, loss, &ld, &s, &g);
  if (rc) return rc;
  return DISPATCH(s->precision, ndt_step_t, h, *s, *g, T, neighbourhood, ld, record);
}

int o3ds_icp_ndt_dev(o3ds_handle h, o3ds_cloud source, o3ds_voxel_gaussians target, const double init[16], const o3ds_icp_params* params, int neighbourhood,
                     const o3ds_robust_loss* loss, o3ds_icp_result* out) {
  CHECK_HANDLE(h);
  ArenaScope arena_scope(h);
  if (!init || !params || !out) return fail(h, O3DS_ERR_INVALID_ARG, "icp_ndt: null argument");
  if (params->max_iteration < 0) return fail(h, O3DS_ERR_INVALID_ARG, "icp_ndt: negative max_iteration");
  CloudRec* s = nullptr;
  NdtRec* g = nullptr;
  RobustLossDev ld{O3DS_LOSS_L2, 0.0};
  const int rc = validate_ndt(h, "icp_ndt", source, target, neighbourhood, loss, &ld, &s, &g);
  if (rc) return rc;
  if (g->n_vox == 0) return fail(h, O3DS_ERR_EMPTY, "icp_ndt: the target has no voxel");
  return DISPATCH(s->precision, ndt_register_t, h, *s, *g, init, *params, neighbourhood, ld, out);
}

}  // extern "C"
