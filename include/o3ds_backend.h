/*
 * o3ds_backend.h -- C-ABI of the MI355X (gfx950) scan-matching / map-fusion backend
 * for open3d_slam.  Plain pointers and sizes only; no C++/torch/Eigen types.
 *
 * Every entry point names the reference interface it replaces; paths are relative to
 * /root/reference/open3d_slam/open3d_slam/.  "[O3D]" = Open3D v0.15.1 routine the
 * reference calls at that line (third-party, pinned by open3d_catkin/CMakeLists.txt:116-118).
 *
 * Conventions
 *   clouds : const double* xyz, 3*n contiguous == std::vector<Eigen::Vector3d>::data()->data()
 *            (open3d::geometry::PointCloud::points_ / normals_, typedefs.hpp:24)
 *   poses  : const double[16] COLUMN-MAJOR == Eigen::Matrix4d::data() / Transform::matrix().data()
 *            (Transform = Eigen::Isometry3d, Transform.hpp:15)
 *   errors : every call returns O3DS_OK (0) or a negative o3ds_status; text via o3ds_last_error().
 *            Nothing throws across the ABI; the C++ adapter (open3d_slam_amd/host/) re-throws
 *            std::runtime_error to keep the reference's behaviour (assert.hpp:13-64).
 *   threads: a handle owns one HIP stream and its scratch; it is NOT re-entrant -- create one
 *            handle per calling thread (odometryWorker / mappingWorker / loopClosureWorker,
 *            SlamWrapper.cpp:258-347,406-448).  Device clouds/maps belong to the handle that made them.
 *   device : all work is enqueued on the handle's stream; calls that return host data synchronise it.
 */
#ifndef O3DS_BACKEND_H
#define O3DS_BACKEND_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3ds_context* o3ds_handle;
typedef uint64_t o3ds_cloud;  /* device-resident cloud (+ optional normals, + optional NN index) */

typedef enum {
  O3DS_OK = 0,
  O3DS_ERR_INVALID_ARG = -1,   /* e.g. max_correspondence_distance <= 0  ([O3D] RegistrationICP LogError) */
  O3DS_ERR_NO_NORMALS = -2,    /* point-to-plane needs target normals    ([O3D] RegistrationICP LogError) */
  O3DS_ERR_OOM = -3,
  O3DS_ERR_HIP = -4,
  O3DS_ERR_BAD_HANDLE = -5,
  O3DS_ERR_EMPTY = -6,         /* assert_gt(size,0): ScanToMapRegistration.cpp:51-52,60 */
  O3DS_ERR_CAPACITY = -7       /* caller-provided output buffer too small */
} o3ds_status;

/* numeric storage of device clouds: f32 xyz (default; accumulation is always f64) or f64 xyz */
typedef enum { O3DS_PRECISION_F32 = 0, O3DS_PRECISION_F64 = 1 } o3ds_precision;

/* croppers.hpp:26-47, croppers.cpp:121-165 (+ setIsInvertVolume croppers.cpp:57-59) */
typedef enum {
  O3DS_CROP_NONE = 0,
  O3DS_CROP_MAX_RADIUS = 1,
  O3DS_CROP_MIN_RADIUS = 2,
  O3DS_CROP_MIN_MAX_RADIUS = 3,
  O3DS_CROP_CYLINDER = 4
} o3ds_crop_kind;

typedef struct {
  int32_t kind;      /* o3ds_crop_kind */
  int32_t invert;    /* isInvertVolume_ */
  double center[3];  /* pose_.translation() -- only the translation is used (croppers.cpp:121-165) */
  double rmin, rmax; /* ScanCroppingParameters::croppingMinRadius_/MaxRadius_ (Parameters.hpp:52-58) */
  double zmin, zmax; /* croppingMinZ_/MaxZ_ (cylinder) */
} o3ds_crop;

/* open3d::pipelines::registration::RegistrationResult as consumed by open3d_slam
 * (Odometry.cpp:51-72, Mapper.cpp:151-159): transformation_, fitness_, inlier_rmse_.
 * correspondence_set_ is never read for ICP results and is not materialised. */
typedef struct {
  double transformation[16]; /* column-major */
  double fitness;
  double inlier_rmse;
  int32_t iterations; /* Gauss-Newton updates applied */
  int32_t converged;  /* ICPConvergenceCriteria test fired */
  uint64_t n_corr;
} o3ds_icp_result;

/* CloudRegistrationType (Parameters.hpp:37-42) as far as the HIP backend implements it */
typedef enum { O3DS_ICP_POINT_TO_PLANE = 0, O3DS_ICP_GENERALIZED = 1, O3DS_ICP_POINT_TO_POINT = 2 } o3ds_icp_method;

/* IcpParameters (Parameters.hpp:66-71) + [O3D] ICPConvergenceCriteria */
typedef struct {
  double max_correspondence_distance; /* IcpParameters::maxCorrespondenceDistance_ */
  int32_t max_iteration;              /* IcpParameters::maxNumIter_ -> criteria.max_iteration_ (CloudRegistration.cpp:63) */
  int32_t method;                     /* o3ds_icp_method; read by o3ds_icp_register_dev / o3ds_icp_begin only */
  double relative_fitness;            /* [O3D] default 1e-6, never overridden by the reference */
  double relative_rmse;               /* [O3D] default 1e-6 */
} o3ds_icp_params;

/* ---- lifecycle --------------------------------------------------------------------------- */
int o3ds_create(int device_id, o3ds_handle* out);
int o3ds_destroy(o3ds_handle h);
const char* o3ds_last_error(o3ds_handle h); /* h may be NULL: last error of the calling thread */
int o3ds_set_precision(o3ds_handle h, int precision /* o3ds_precision */);
int o3ds_synchronize(o3ds_handle h);
/* the hipStream_t all work of this handle is enqueued on (for event timing / interop) */
void* o3ds_stream(o3ds_handle h);
/* Enqueue this handle's work on the caller's hipStream_t instead (e.g. torch's current stream, so that a
 * torch.distributed all-reduce of the step-wise record is stream-ordered with the kernels); NULL restores the
 * handle's own stream.  The caller keeps the stream alive. */
int o3ds_set_stream(o3ds_handle h, void* hip_stream);
/* Kernel timing for bench.py's roofline line: when enabled, every ICP correspondence/reduction pass
 * (icp_accumulate_kernel launch) is bracketed by hipEvents on the launch stream.  profile_read synchronises,
 * returns the number of bracketed launches and their summed duration (ms), and resets the counters.
 * on = 2 enables the tagged spans below WITHOUT the per-launch brackets: a span around a whole registration then
 * measures its kernels back to back (bench.py's roofline.avg_launch_us = that span / passes). */
int o3ds_profile_enable(o3ds_handle h, int on);
int o3ds_profile_read(o3ds_handle h, uint64_t* n_launches, double* total_ms);
/* Tagged spans for bench.py's per-call table: while profiling is enabled, o3ds_profile_span(h, tag, 0) / (h, tag, 1) record a pair
 * of hipEvents on the handle's stream around whatever the caller enqueues in between (tags 0..7).  Tags 8 (the two kernels of
 * normal estimation), 9 (the kernels of an index build) and 10 (the kernel of o3ds_neighbor_search and of the outlier filters' search)
 * and 11 to 13 (the steps of o3ds_cluster_dbscan, see there) and 14 (the evaluation kernel of o3ds_segment_plane, once per batch of
 * hypotheses) and 15 (the kernel of o3ds_compute_color_gradients) and 16 (the two kernels of one coloured-ICP step: the block sums and
 * their fold) and 17 (the same two of one robust-loss step, o3ds_robust_icp_step) and 18 (the kernels of o3ds_voxel_gaussians_create) and 19
 * (the two kernels of one o3ds_ndt_step) are marked inside the library.  span_read synchronises, returns the
 * number of complete spans of a tag and their summed duration (ms) and resets that tag. */
int o3ds_profile_span(o3ds_handle h, int tag, int end);
int o3ds_profile_span_read(o3ds_handle h, int tag, uint64_t* n_spans, double* total_ms);
/* library / kernel identification string (arch, build flags) */
const char* o3ds_version(void);

/* ---- device clouds ----------------------------------------------------------------------- */
/* Upload a host cloud (PointCloud::points_, normals_ may be NULL). */
int o3ds_cloud_upload(o3ds_handle h, const double* xyz, const double* normals, size_t n, o3ds_cloud* out);
/* The same from a sensor_msgs/PointCloud2-style buffer, without the float -> double -> float detour of
 * open3d_conversions::rosToOpen3d (open3d_utils/open3d_conversions/src/open3d_conversions.cpp:59-68, which reads the float32
 * fields x, y, z of every record and widens them): n records of point_step bytes, float32 x / y / z at byte offsets off_x /
 * off_y / off_z.  The raw buffer is copied to the device as it is and unpacked there; the values stored are exactly those the
 * double route would store.  Other fields (intensity, ring, t, rgb) are ignored, as on the scan-matching path. */
int o3ds_cloud_upload_f32(o3ds_handle h, const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y, size_t off_z,
                          o3ds_cloud* out);
/* The ingest is ASYNCHRONOUS: copy, unpack and (for the volume this handle last passed to o3ds_crop_voxel_down_sample) the bounding box
 * of the points inside the cropping volume run on the handle's copy stream, so that scan k + 1 crosses PCIe while frame k is still being
 * registered and merged; the first operation that uses the cloud queues a wait for it on the handle's stream (no host wait).  A buffer
 * of ordinary (pageable) memory has been consumed when the call returns (it goes through the handle's pinned ring).  A buffer from
 * o3ds_pinned_alloc (or any memory registered with the HIP runtime) is read by DMA after the call has returned: keep its contents until
 * o3ds_cloud_wait_ingest(cloud) has returned or any call that returns data derived from the cloud (a registration result, a size, a
 * download) has. */
int o3ds_pinned_alloc(o3ds_handle h, size_t bytes, void** out);  /* page-locked host memory for sensor / message buffers (ROS 2 allocators, drivers) */
int o3ds_pinned_free(o3ds_handle h, void* p);
int o3ds_cloud_wait_ingest(o3ds_handle h, o3ds_cloud c);
int o3ds_cloud_free(o3ds_handle h, o3ds_cloud c);
/* The number of points of a cloud and whether it has normals.  The clouds of the per-scan chain -- o3ds_voxel_down_sample /
 * o3ds_crop_voxel_down_sample and what o3ds_estimate_normals, the registrations and o3ds_map_insert_scan make of their results -- are
 * sized ON THE DEVICE: the kernel that counts the voxels publishes the number where the kernels that consume the cloud read it, the
 * frame's launches are queued from an upper bound, and nothing waits for a size to come back.  Asking for n is what waits (once; the
 * number usually arrived with the next registration result and then costs nothing); n == NULL asks for has_normals only and never
 * waits.  Every call that sizes a host buffer or another cloud by the number (download, crop, select, transform, append ...) asks. */
int o3ds_cloud_size(o3ds_handle h, o3ds_cloud c, size_t* n, int* has_normals);
/* Elements of the neighbourhood-major replica of the cloud's nearest-neighbour index (9 per point), 0 if it has none.  The replica is
 * built by the registration that is the fourth against the same index (an index a stream rebuilds every frame never gets one); it
 * changes no result, only how fast the search runs. */
int o3ds_cloud_index_replica(o3ds_handle h, o3ds_cloud c, size_t* elements);
/* Whether the cloud is a map in its PERSISTENT form right now (o3ds_map_insert_scan): persistent = 1 or 0.  Never waits,
 * never folds, changes nothing -- the only way to tell which form a map is in; the form changes no result, only what an insertion costs.
 * O3DS_ERR_INVALID_ARG for an unknown id. */
int o3ds_cloud_is_persistent_map(o3ds_handle h, o3ds_cloud c, int* persistent);
/* What is known of the size without waiting: lower <= n <= upper (equal once the number has arrived).  The reference's emptiness checks
 * (assert_gt(cloud.size(), 0), ScanToMapRegistration.cpp:51-52; preProcessedScan.IsEmpty(), Submap.cpp:41) are decided by the bounds:
 * a VoxelDownSample result whose input had a point inside the volume has lower = 1. */
int o3ds_cloud_size_bound(o3ds_handle h, o3ds_cloud c, size_t* lower, size_t* upper);
/* Download into caller buffers of capacity >= n points (normals may be NULL). */
int o3ds_cloud_download(o3ds_handle h, o3ds_cloud c, double* xyz, double* normals, size_t capacity);
/* The way out, again without a double detour: write the cloud as n records of point_step bytes with float32 x / y / z at byte
 * offsets off_x / off_y / off_z; unless off_normal == O3DS_NO_FIELD, the normal as three float32 at off_normal, +4, +8; unless
 * off_rgb == O3DS_NO_FIELD, the colour as the packed `rgb` field (bytes b, g, r, 0 at off_rgb, +1, +2, +3); every other byte of the
 * records is zero.  point_step 16, offsets 0 / 4 / 8 is the sensor_msgs/PointCloud2 layout that open3d_conversions::open3dToRos
 * produces for a cloud without colours, point_step 32 with rgb at 16 the one for a coloured cloud
 * (open3d_utils/open3d_conversions/src/open3d_conversions.cpp:19-53: `*ros_pc2_x = point(0)`, a double -> float narrowing, and
 * `*ros_pc2_r = (int)(255 * color(0))` = rgb_rounding 0); point_step 24, offsets 0 / 4 / 8 / 12 is the row of a binary PCD with FIELDS
 * x y z normal_x normal_y normal_z as [O3D] io::WritePointCloudToPCD writes it for saveToFile
 * (open3d_slam/open3d_slam/src/output.cpp:39-47), whose rgb field uses [O3D] utility::ColorToUint8 (clamp, scale, round = rgb_rounding
 * 1).  data must hold capacity >= n records. */
#define O3DS_NO_FIELD ((size_t)-1)
int o3ds_cloud_download_f32(o3ds_handle h, o3ds_cloud c, void* data, size_t capacity, size_t point_step, size_t off_x, size_t off_y,
                            size_t off_z, size_t off_normal, size_t off_rgb, int rgb_rounding);
/* Colours of an ingested cloud, read from the same PointCloud2 records as rosToOpen3d does when skip_colors is false -- which is how
 * every caller in the reference invokes it (OnlineRangeDataProcessorRos.cpp:40, RosbagRangeDataProcessorRos.cpp:129,
 * SlamMapInitializer.cpp:124): O3DS_COLOR_FIELD_RGB = a fourth field named "rgb" at byte offset off_field (r, g, b = bytes +2, +1, +0,
 * each / 255.0; open3d_conversions.cpp:71-80); O3DS_COLOR_FIELD_INTENSITY = a fourth field named "intensity", which the reference reads
 * through a uint8 iterator: the FIRST byte of the field, unscaled, for all three channels (open3d_conversions.cpp:81-86).  The cloud
 * must have been made from the same n records (o3ds_cloud_upload_f32). */
enum { O3DS_COLOR_FIELD_RGB = 0, O3DS_COLOR_FIELD_INTENSITY = 1 };
int o3ds_cloud_set_colors_from_records(o3ds_handle h, o3ds_cloud c, const void* data, size_t point_step, size_t off_field, int kind);
/* PointCloud::colors_ (3n doubles in [0, 1]) of a device cloud.  The three geometric registrations never read them (coloured ICP,
 * o3ds_icp_colored_dev at the end of this header, is the one algorithm that does); the cloud operations carry them
 * the way the reference does: crop / select / carve keep the colours of the kept points, transform copies them, append follows
 * [O3D] PointCloud::operator+= (kept only if the map is empty or coloured AND the added cloud is coloured), o3ds_voxel_down_sample
 * averages them ([O3D] VoxelDownSample), and the map merge o3ds_voxelize_within_volume / o3ds_map_insert_scan gives a voxel the
 * colour of its LAST point in cloud order (AccumulatedPoint::AddPoint assigns, helpers.cpp:40-42,61-63; isValidColor,
 * helpers.cpp:83-85, holds for every value).  rgb == NULL clears.  get_colors returns O3DS_ERR_EMPTY for an uncoloured cloud. */
int o3ds_cloud_set_colors(o3ds_handle h, o3ds_cloud c, const double* rgb);
/* PointCloud::covariances_ is NOT carried: a device cloud has points, normals and colours.  The reference's own flow never holds any --
 * the one call that would fill them, EstimateCovariances, is commented out (CloudRegistration.cpp:29), generalized ICP builds its
 * covariances from the normals inside the registration (Open3D does the same when a cloud has none), and nothing else writes the field --
 * so the copies croppers.cpp:86-101 and helpers.cpp:48-50,64-67,297-302 make of it move empty vectors.  A caller that fills
 * covariances_ itself keeps them on its host PointCloud; they do not cross the seams (integration/o3ds_open3d_slam.hpp clears the field
 * of every cloud it hands back, as an Open3D call that recomputes a cloud would). */
int o3ds_cloud_has_colors(o3ds_handle h, o3ds_cloud c, int* has_colors);
int o3ds_cloud_get_colors(o3ds_handle h, o3ds_cloud c, double* rgb, size_t capacity);
/* Build the nearest-neighbour index of a cloud (replaces [O3D] KDTreeFlann::SetGeometry(target), which
 * RegistrationICP does on every call).  cell_size <= 0 selects max_corr_hint/4.  Idempotent per cell size. */
int o3ds_cloud_build_index(o3ds_handle h, o3ds_cloud c, double max_corr_hint, double cell_size);

/* ---- Seam 1: CloudRegistration::registerClouds (CloudRegistration.hpp:25) ----------------- */
/* RegistrationIcpPointToPlane::registerClouds (CloudRegistration.cpp:44-48) = [O3D] RegistrationICP with
 * TransformationEstimationPointToPlane.  Host-buffer form: uploads both clouds, builds the target index
 * (as the reference rebuilds its KD-tree per call), runs ICP, frees the device copies. */
int o3ds_icp_point_to_plane(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, const double* tgt_normals,
                            size_t n_tgt, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);
/* Device-resident form.  target must have normals and an index.  target_crop (may be NULL) restricts the
 * target to the points inside the volume -- ScanToMapIcp::scanToMapRegistration's
 * scanMatcherCropper_->crop(activeSubmapPointCloud) (ScanToMapRegistration.cpp:58-59) fused into the search. */
int o3ds_icp_point_to_plane_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop,
                                const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);

/* Same loop with params->method selecting the estimator (point-to-plane, generalized or point-to-point). */
int o3ds_icp_register_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                          const o3ds_icp_params* params, o3ds_icp_result* out);
/* Work for the time the host would wait for a registration.  The callback is handed to the NEXT device-resident registration on the
 * handle (o3ds_icp_register_dev and the per-estimator entry points above) and is called at most once, on the calling thread, after the
 * registration's launches have been queued and before the host waits for their result: whatever it queues on the handle runs behind them,
 * in the time the host spends waiting and -- afterwards -- deciding what to do with the pose.  In open3d_slam that is the odometry
 * worker's pre-processing of the NEXT raw scan (SlamWrapper.cpp:228-229 runs it on its own thread; a single-threaded caller gets the
 * same overlap this way).  The callback may call any o3ds_* function on this handle except a registration, a session call or anything
 * that frees or changes the two clouds being registered; calls that read a size back (o3ds_cloud_size, downloads) wait for the
 * registration first and so defeat the purpose.  Not called when the registration fails before it queues anything or takes the
 * two-launch form (sources beyond 262 144 points): *the caller checks* (the callback can count).  fn == NULL withdraws it. */
typedef void (*o3ds_overlap_fn)(void* arg);
int o3ds_icp_overlap_next(o3ds_handle h, o3ds_overlap_fn fn, void* arg);
/* RegistrationIcpGeneralized::registerClouds (CloudRegistration.cpp:16-21) = [O3D] RegistrationGeneralizedICP with a
 * default TransformationEstimationForGeneralizedICP (epsilon 1e-3): per-point covariances C = Rx diag(eps,1,1) Rx^T built from
 * the clouds' (unit) normals, residual (Ct + R Cs R^T)^-1/2 (p - q), same loop / solve / convergence test as point-to-plane.
 * The device evaluates the closed form C = I - k n n^T (k = 1 - eps), with n := e1 where the stored normal has x < -0.99
 * ([O3D] GetRotationFromE1ToX's special case) or is the zero vector (for which the same function returns the identity: the
 * voxel merges of the pipeline store one where the merged normals cancel); both are decided on the stored normal, the
 * source's before it is rotated by the pose.  Out of scope: NaN normals, and non-unit normals other than zero -- the model is
 * stated for unit normals, and no producer in the pipeline makes others (both voxel merges renormalise, the estimator
 * normalises).
 * open3d_slam always calls estimateNormalsOrCovariancesIfNeeded first (CloudRegistration.cpp:22-30); a cloud that still has no
 * normals (null pointer / device cloud without normals) gets [O3D] InitializePointCloudForGeneralizedICP's treatment:
 * EstimateNormals(KDTreeSearchParamKNN(20)) on a copy, the caller's cloud is left as it was. */
int o3ds_icp_generalized(o3ds_handle h, const double* src_xyz, const double* src_normals, size_t n_src, const double* tgt_xyz,
                         const double* tgt_normals, size_t n_tgt, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);
int o3ds_icp_generalized_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                             const o3ds_icp_params* params, o3ds_icp_result* out);
/* RegistrationIcpPointToPoint::registerClouds (CloudRegistration.cpp:69-74) = [O3D] RegistrationICP with
 * TransformationEstimationPointToPoint: the update of every iteration is the closed-form Eigen::umeyama (no scaling) of the
 * matched pairs; same loop and convergence test.  No normals are needed on either cloud.
 * Step-wise record in this method: [0..8] sum q'_a p'_b (row-major, q = matched target point, p = transformed source point),
 * [9..11] sum p', [12..14] sum q', [28] #corr, [29] sum d^2 (of p - q), the rest 0, where p' = p - c and q' = q - c are taken relative to
 * the session's pivot c: per axis the multiple of 1024 m nearest (rint) to T s_0, the pose of the pass applied to point 0 of the source
 * CLOUD (not of the range a call covers), and 0 on an axis where that is not finite or beyond 2^30 m.  o3ds_icp_accumulate forms the record about c and
 * o3ds_icp_update derives the same c from the same pose and point, so records of ranks that hold the same source cloud and pose add up;
 * a caller that writes a record itself forms it about that c.  Within 512 m of the origin c = 0 and the record is the sums of the
 * coordinates themselves.  (Sigma = E[q p^T] - E[q] E[p]^T does not depend on c; about a far origin its subtraction cancels.) */
int o3ds_icp_point_to_point(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, size_t n_tgt,
                            const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);
int o3ds_icp_point_to_point_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                                const o3ds_icp_params* params, o3ds_icp_result* out);
/* [O3D] GetInformationMatrixFromPointClouds(source, target, max_correspondence_distance, transformation) (call sites
 * constraint_builders.cpp:70-73, PlaceRecognition.cpp:148-149): one correspondence pass under T (same exact 1-NN search as the
 * ICP passes), Lambda = sum over the matched TARGET points q of G^T G, G = [-[q]x | I].  information: 36 doubles; a symmetric
 * matrix, so row- and column-major coincide (Eigen::Matrix6d::data() can be passed). */
int o3ds_information_matrix(o3ds_handle h, const double* src_xyz, size_t n_src, const double* tgt_xyz, size_t n_tgt, const double T[16],
                            double max_correspondence_distance, double information[36]);
int o3ds_information_matrix_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double T[16],
                                double max_correspondence_distance, double information[36]);
/* epsilon of the plane-to-plane covariance model (default 1e-3, Open3D's default) */
int o3ds_set_gicp_epsilon(o3ds_handle h, double epsilon);

/* Step-wise form of the same loop, for sharded (multi-GPU) registration: the caller all-reduces the 32-double
 * normal-equation record between accumulate and update.  Record layout (doubles):
 *   [0..20] upper triangle of JtJ row-major, [21..26] Jtr, [27] sum r^2, [28] #corr, [29] sum d^2, [30..31] 0.
 * begin      : T <- init, resets iteration state.
 * accumulate : one correspondence + reduction pass ([O3D] GetRegistrationResultAndCorrespondences +
 *              ComputeJTJandJTr) of source points [first, first+count) under the current T; writes the record to
 *              d_record (DEVICE pointer to 32 doubles, e.g. a torch tensor's data_ptr).
 * update     : consumes a (possibly all-reduced) record on the device: convergence test against the previous pass,
 *              6x6 LDLT, T <- U*T ([O3D] SolveJacobianSystemAndObtainExtrinsicMatrix).  n_src_total = |source| over
 *              all shards (fitness denominator).
 * finish     : synchronises and returns the result (state after the last evaluated pass). */
int o3ds_icp_begin(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop, const double init[16],
                   const o3ds_icp_params* params);
int o3ds_icp_accumulate(o3ds_handle h, size_t first, size_t count, double* d_record);
int o3ds_icp_update(o3ds_handle h, const double* d_record, uint64_t n_src_total);
int o3ds_icp_finish(o3ds_handle h, o3ds_icp_result* out);
/* Target-sharded registration against ONE map whose points are split over up to 16 GPUs (SURVEY.md 8e
 * Partitioning B) -- the sharding that reproduces the reference's registration against a single cloud (Mapper.cpp:141,
 * ScanToMapRegistration.cpp:57-61).  Per iteration, inside an o3ds_icp_begin session on this rank's shard:
 *   o3ds_icp_nn_keys(h, 0, n, rank, d_keys)      every query's best match in THIS shard as a key: float bits of d2 << 32 | rank << 28 |
 *                                                position in the shard's index; INT64_MAX when nothing lies within the radius (keys order as signed or unsigned)
 *   ncclAllReduce(d_keys, n, uint64, min)        non-negative float bit patterns order like the floats: the minimum is the match in
 *                                                the union of the shards (equal distances: lower rank, then lower position)
 *   o3ds_icp_accumulate_keys(h, 0, n, rank, d_keys, d_record)   the queries whose winning key names this rank contribute their rows
 *   ncclAllReduce(d_record, 32, double, sum)  ->  o3ds_icp_update(h, d_record, n)
 * and o3ds_icp_finish as usual.  d2 enters the key as a float: distances that differ only beyond float precision tie. */
int o3ds_icp_nn_keys(o3ds_handle h, size_t first, size_t count, int rank, unsigned long long* d_keys);
int o3ds_icp_accumulate_keys(o3ds_handle h, size_t first, size_t count, int rank, const unsigned long long* d_keys, double* d_record);
/* 1 when the device-side loop has terminated (converged or max_iteration reached); synchronises. */
/* Fused step-wise form -- ONE kernel per iteration plus the caller's collective (the accumulate / reduce / update triple above is
 * three).  o3ds_icp_pass enqueues launch j of the fused loop over the source range [first, first + count): its prologue folds
 * d_sums_in (the ALL-REDUCED sums of the previous pass; ignored by the first call of a session) and applies the update, its body
 * adds this rank's part of pass j to d_sums_out, and it clears d_sums_next.  The three buffers are O3DS_ICP_SUMS_DOUBLES doubles
 * each, on the device, owned and rotated by the caller (out -> in -> next -> out ...), all zero before the first call.  Between
 * two calls the caller sums d_sums_out element-wise over the ranks (ncclAllReduce, in place, on o3ds_stream(h)).  The addends are
 * split so that these sums are exact: the result does not depend on the number of ranks or the reduction order.
 * o3ds_icp_pass_finish folds the last pass (one-workgroup launch) and returns the result; max_iteration + 1 passes make a full
 * registration, passes issued after the loop has terminated on the device are no-ops. */
#define O3DS_ICP_SUMS_DOUBLES 512
/* o3ds_icp_pass serves at most this many source points per call (one workgroup per 128 queries -- 64 until the end of round 6 --; the exact sums hold for 4096 workgroup records per pass);
 * a larger range returns O3DS_ERR_CAPACITY -- shards beyond it use the o3ds_icp_accumulate / o3ds_icp_update triple, which loops
 * (open3d_slam_amd/sharded.py falls back by itself).  o3ds_icp_register_dev has no such limit (it switches form internally). */
#define O3DS_ICP_PASS_MAX_QUERIES 262144
int o3ds_icp_pass(o3ds_handle h, size_t first, size_t count, size_t n_src_total, const double* d_sums_in, double* d_sums_out,
                  double* d_sums_next);
int o3ds_icp_pass_finish(o3ds_handle h, size_t n_src_total, const double* d_sums_in, double* d_sums_scratch, o3ds_icp_result* out);
int o3ds_icp_done(o3ds_handle h, int* done);

/* ---- the same registrations, sharded over the GPUs of a node, entirely inside the library: kernels and RCCL collectives queued on
 *      o3ds_stream(h) for ALL max_iteration + 1 passes, no host code between them (the reference registers against one cloud,
 *      Mapper.cpp:141 -> ScanToMapRegistration.cpp:55-62 -> CloudRegistration.cpp:44-48; the partitionings are SURVEY.md 8e's).
 * One process per GPU, one handle per process.  RCCL (librccl.so) is loaded with dlopen at the first call of this group -- a
 * single-GPU user of the library does not need it installed -- and the communicator is created by THAT copy of the library:
 *   o3ds_comm_unique_id   on ONE rank: a 128-byte ncclUniqueId, to be handed to every rank by whatever the processes share
 *                         (torch.distributed's broadcast, MPI, a file);
 *   o3ds_comm_init        on EVERY rank (collective: ncclCommInitRank): the handle keeps the communicator;
 *   o3ds_comm_attach      instead of init: an ncclComm_t the caller made with the same librccl.so the process has loaded;
 *   o3ds_comm_destroy     (also done by o3ds_destroy).
 * o3ds_icp_register_sharded: `partitioning`
 *   O3DS_SHARD_SOURCE  every rank holds the same target; rank r contributes the source points [r n / W, (r + 1) n / W): per pass ONE
 *                      icp_fused_kernel + ONE ncclAllReduce(sum) of the 512-double exact hi / lo record (4 KB) -- equal to the one-GPU
 *                      registration bit for bit, whatever W (the sums are exact);
 *   O3DS_SHARD_SUBMAP  every rank holds ITS OWN submap and the whole source: the same kernel and collective, the summed record is the
 *                      joint problem over the W submaps (BASELINE.json configs[3]; fitness = mean over the submaps);
 *   O3DS_SHARD_UNION   ONE map split over the ranks, every rank holds the whole source: per pass search kernel -> ncclAllReduce(min) of
 *                      n 64-bit keys -> accumulate kernel -> ncclAllReduce(sum) of 32 doubles -> update kernel; equal to the
 *                      registration against the whole map (W <= 16).
 * Point-to-plane, generalized and point-to-point estimators (params->method) as o3ds_icp_register_dev.  With a communicator of one
 * rank every collective is the identity and SOURCE / SUBMAP reproduce o3ds_icp_register_dev bit for bit. */
#define O3DS_SHARD_SOURCE 0
#define O3DS_SHARD_SUBMAP 1
#define O3DS_SHARD_UNION 2
int o3ds_comm_unique_id(o3ds_handle h, unsigned char id[128]);
int o3ds_comm_init(o3ds_handle h, const unsigned char id[128], int rank, int world);
int o3ds_comm_attach(o3ds_handle h, void* nccl_comm, int rank, int world);
int o3ds_comm_destroy(o3ds_handle h);
int o3ds_icp_register_sharded(o3ds_handle h, int partitioning, o3ds_cloud source, o3ds_cloud target, const o3ds_crop* target_crop,
                              const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);

/* ---- one registration against SEVERAL resident targets of one handle (a SubmapCollection's submaps), in one process and without a
 *      copy: BASELINE.json configs[3] on one GPU.  A capability beyond the reference, which registers against the active submap only
 *      (Mapper.cpp:141).  All targets are clouds of `h` in one common frame, each in the state o3ds_icp_register_dev accepts a target
 *      in, WITH its index (o3ds_cloud_build_index, or a persistent-form map) and, for the estimators that need them, its normals.
 *      `target_crop` is a predicate inside every target's search, as in the one-target call; params->method, the loop, the solve, the
 *      convergence test and the result fields are that call's.  One launch walks the whole list per query and pass.
 *   O3DS_MULTI_UNION  the correspondence of a query is its nearest point over the union of the targets' (cropped) points within
 *                     max_correspondence_distance.  The d2 compared across targets is the d2 the one-target search compares (storage
 *                     precision, never rounded further); equal d2 go to the LOWER slot of `targets`, inside a slot to the one-target
 *                     search's choice (the smaller original index).  The result is the registration o3ds_icp_register_dev gives against
 *                     the cloud obtained by appending the targets in slot order (o3ds_cloud_append) and indexing it.
 *   O3DS_MULTI_JOINT  every target contributes its own correspondence per query and the normal-equation records are summed over the
 *                     targets: fitness = correspondences / (n_targets * n_src), the mean over the targets; inlier_rmse over all
 *                     correspondences.  O3DS_SHARD_SUBMAP in one process.  The sums are exact: K copies of one cloud give the
 *                     one-target pose bit for bit when K is a power of two.
 * n_targets == 1 returns the bits of o3ds_icp_register_dev in either form.  An empty target in the list is legal and contributes
 * nothing (JOINT still counts it in the denominator); a list of empty targets only returns O3DS_ERR_EMPTY as the one-target call does.
 * O3DS_ERR_INVALID_ARG: n_targets == 0 or > O3DS_MULTI_MAX_TARGETS, a null list, an unknown form, an id that is not a cloud of `h`
 * (a cloud of another handle), a non-empty target without an index, without the normals the estimator needs or of another precision
 * than the source.  O3DS_ERR_CAPACITY (nothing is looped): with n_targets > 1 the source may have at most O3DS_ICP_PASS_MAX_QUERIES
 * points, and in JOINT form n_targets * ceil(n_src / 128) may be at most 4096, the number of workgroup records the exact sums hold per
 * pass (8 targets x 65 536 points, 16 x 32 768).  Candidate sets are not carried between the passes of this call: every pass searches,
 * from the previous pass's match as its bound.  A function armed with o3ds_icp_overlap_next is NOT consumed by this call: it stays
 * armed for the next one-target registration. */
#define O3DS_MULTI_MAX_TARGETS 16 /* as the sharded forms: W <= 16 */
#define O3DS_MULTI_UNION 0
#define O3DS_MULTI_JOINT 1
int o3ds_icp_register_multi(o3ds_handle h, int form, o3ds_cloud source, const o3ds_cloud* targets, size_t n_targets,
                            const o3ds_crop* target_crop, const double init[16], const o3ds_icp_params* params, o3ds_icp_result* out);

/* ---- SEVERAL INDEPENDENT registrations of one handle in one call: loop-closure refinements of a scan's candidates, the odometry
 *      constraints between adjacent submaps, several initial guesses for one pair.  A capability beyond the reference, which runs them
 *      one after another (PlaceRecognition.cpp:71-111, its `omp parallel for` is commented out).  The other axis of
 *      o3ds_icp_register_multi: that is one problem with many targets, this is many problems, each with its own pose, state and
 *      convergence.  One launch per pass serves every entry that is still running.
 * Entry k IS the registration o3ds_icp_register_dev(h, entries[k].source, entries[k].target, entries[k].target_crop, entries[k].init,
 * params, &out[k]): out[k] holds that call's values in every field (transformation, fitness, inlier_rmse, iterations, converged,
 * n_corr), bit for bit, in both storage precisions and for the three estimators.  Grounds: the target index and the quanta of the exact
 * sums are per entry and are the one-pair call's; the queries of an entry are dealt out in the same batches of 128 in the same order;
 * the sums over the batches are exact and hence order-free; and searching every pass instead of keeping candidate sets does not change
 * a bit of the matches.  `params` (method, radius, max_iteration, thresholds) is shared by the batch.  All clouds belong to `h` and have
 * its precision.  Entries may repeat a source or a target (the same pair with different `init` is the multi-hypothesis case); some may
 * carry a crop and others not.  A target without an index is indexed as the one-pair call would index it.  A cloud in persistent-map
 * form that is the SOURCE of an entry is folded into array form before the batch starts (the one-pair call folds it when its turn comes).
 * n_entries == 1 delegates to o3ds_icp_register_dev.  A function armed with o3ds_icp_overlap_next is NOT consumed by this call, whatever
 * n_entries: it stays armed for the next one-pair registration.
 * Whole-call errors, returned before anything is touched (the handle stays usable, out / status are not written):
 *   O3DS_ERR_INVALID_ARG  a null pointer (entries, params, out, status); n_entries == 0 or > O3DS_BATCH_MAX_ENTRIES; an id that is not a
 *                         cloud of `h`; a non-empty target without the normals the estimator needs; a source / target precision
 *                         mismatch; max_correspondence_distance <= 0, an unknown method, a negative max_iteration.
 *   O3DS_ERR_CAPACITY     (nothing is looped) a source of more than O3DS_ICP_PASS_MAX_QUERIES points; a total of more than
 *                         O3DS_BATCH_MAX_WORKGROUPS workgroups per pass, sum over the entries of max(ceil(n_src_k / 128), 1).
 * Per-entry outcomes go to status[k]: O3DS_OK; O3DS_ERR_EMPTY for an entry whose target is empty (as the one-pair call); otherwise the
 * code the one-pair call returns for that entry (a generalized-ICP source without normals: O3DS_ERR_NO_NORMALS).  Such an entry is
 * skipped, its out[k] is zeroed and the others run.  The function returns O3DS_OK when the batch ran, whatever the entries reported.
 * Candidate sets and the fused loop are not used by this call: every pass is two launches and searches from the previous pass's match
 * as its bound.  A batch of small sources fills the device where one of them cannot; a batch of large ones is better served by the
 * one-pair call in a loop (DESIGN.md 7.5 has the measurements). */
#define O3DS_BATCH_MAX_ENTRIES 64
#define O3DS_BATCH_MAX_WORKGROUPS 65536
typedef struct {
  o3ds_cloud source, target;
  const o3ds_crop* target_crop; /* may be NULL */
  double init[16];              /* column-major, as everywhere */
} o3ds_icp_batch_entry;
int o3ds_icp_register_batch(o3ds_handle h, const o3ds_icp_batch_entry* entries, size_t n_entries, const o3ds_icp_params* params,
                            o3ds_icp_result* out /* [n_entries] */, int* status /* [n_entries] */);

/* ---- scan pre-processing: ScanToMapIcp::preprocess (ScanToMapRegistration.cpp:35-40),
 *      LidarOdometry::preprocess (Odometry.cpp:25-30) ------------------------------------------ */
/* CroppingVolume::crop (croppers.cpp:76-106): stable compaction of points (+normals) inside the volume. */
int o3ds_crop_cloud(o3ds_handle h, o3ds_cloud in, const o3ds_crop* crop, o3ds_cloud* out);
/* o3d_slam::voxelize (helpers.cpp:107-113) -> [O3D] PointCloud::VoxelDownSample: data-anchored grid,
 * per-voxel mean of points (and normals), each sum taken in cloud order.  Output order: voxels in order of their first point in the
 * cloud (the reference's order is unordered_map iteration order, i.e. unspecified).  voxel <= 0 returns a copy. */
int o3ds_voxel_down_sample(o3ds_handle h, o3ds_cloud in, double voxel_size, o3ds_cloud* out);
/* The first two steps of ScanToMapIcp::preprocess (ScanToMapRegistration.cpp:36-37) and LidarOdometry::preprocess (Odometry.cpp:26-27),
 * `cropped = cropper->crop(in); voxelize(voxelSize, cropped)`, as one call: the same cloud o3ds_crop_cloud followed by
 * o3ds_voxel_down_sample returns, bit for bit (grid anchored at the bounding box of the points INSIDE the volume, voxel means summed
 * in the same order), without materialising the cropped cloud.  voxel_size <= 0 is o3ds_crop_cloud. */
int o3ds_crop_voxel_down_sample(o3ds_handle h, o3ds_cloud in, const o3ds_crop* crop, double voxel_size, o3ds_cloud* out);
/* RegistrationIcpPointToPlane::estimateNormalsOrCovariancesIfNeeded (CloudRegistration.cpp:49-56):
 * [O3D] EstimateNormals(KDTreeSearchParamHybrid(radius,max_nn)) + NormalizeNormals +
 * OrientNormalsTowardsCameraLocation(0,0,0).  In place (adds/overwrites the cloud's normals). */
int o3ds_estimate_normals(o3ds_handle h, o3ds_cloud c, double radius, int max_nn);
/* [O3D] RandomDownSample is seeded from std::random_device (non-reproducible); the ABI takes the
 * kept indices explicitly: SelectByIndex(keep_idx[0..m)). */
int o3ds_select_by_index(o3ds_handle h, o3ds_cloud in, const uint32_t* keep_idx, size_t m, o3ds_cloud* out);
/* [O3D] PointCloud::RandomDownSample(sampling_ratio) as open3d_slam calls it (Odometry.cpp:29, ScanToMapRegistration.cpp:39), drawn on the
 * device: keeps k = (int)(ratio * n) points, a uniformly drawn k-subset, in cloud order (the order [O3D] SelectByIndex's mask walk emits).
 * The reference draws from an mt19937 seeded by std::random_device -- there is no sequence to reproduce --; here index i gets the 64-bit key
 * mix(seed + (i + 1) * 0x9E3779B97F4A7C15) (splitmix64's finaliser: distinct keys) and the k smallest keys are kept, so the subset is a
 * function of (seed, n, ratio) alone, restated in numpy for the checker (oracle/pipeline.py draw_keep).  Neither n nor k passes through the
 * host: a cloud whose size is still in flight (o3ds_crop_voxel_down_sample's result) is drawn from as it is, and the result's size is in
 * flight in turn.  ratio outside [0, 1]: O3DS_ERR_INVALID_ARG with Open3D's message; the input is left as it is. */
int o3ds_random_down_sample(o3ds_handle h, o3ds_cloud in, double ratio, uint64_t seed, o3ds_cloud* out);

/* ---- map fusion: Submap::insertScan (Submap.cpp:39-75) ------------------------------------- */
/* o3d_slam::transform (helpers.cpp:273-305): p' = (T p).xyz/w, n' = R n.  Returns a new cloud.
 * (The reference's duplicate-on-identity quirk, SURVEY B4, is intentionally not reproduced.)  FPFH features of the input
 * (o3ds_compute_fpfh) are carried over unchanged, as [O3D] PointCloud::Transform leaves a Feature alone. */
int o3ds_transform_cloud(o3ds_handle h, o3ds_cloud in, const double T[16], o3ds_cloud* out);
/* The mean of the points, [O3D] PointCloud::GetCenter as Submap::computeSubmapCenter (Submap.cpp:255-259) uses it: summed in f64
 * whatever the storage precision, in one fixed order that depends on the number of points only (not on the device, the handle or whether
 * the host knew the size), so repeated calls give the same bits; non-finite points propagate into the mean; an empty cloud gives
 * (0, 0, 0).  A submap in its persistent form is first turned into its array (as a download would).  Waits for the result. */
int o3ds_cloud_center(o3ds_handle h, o3ds_cloud c, double center[3]);

/* ---- neighbour queries between device clouds: [O3D] KDTreeFlann::SearchKNN / SearchRadius / SearchHybrid ------------------------------
 * The neighbours in `target` of n_queries points of `queries` (the points query_idx[0..n_queries), repeats allowed; NULL: all its points,
 * in order, and n_queries is its size).  Both ids may name the same cloud; a query that is a point of the target finds itself.
 * The result of one query is defined without reference to a search structure:
 *   - target coordinates are the stored ones; the query is the stored point, or with a pose storage(T s), T s = ((T00 x + T01 y) + T02 z)
 *     + T03 per row in f64 (T column-major, rigid: the fourth row is not read);
 *   - d2 = (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own;
 *   - a candidate is accepted iff d2 is finite and (radius <= 0, or d2 < storage(radius * radius) strictly, the product formed in f64);
 *   - row i of idx / d2 holds the first max_nn accepted candidates in the order (d2, original target index), count[i] of them; entries
 *     past count[i] are zero; d2 is the storage-type value widened;
 *   - total[i] is the number of accepted candidates whatever max_nn is (truncation shows as total[i] > count[i]);
 *   - a query with a non-finite coordinate has an empty list and total 0; target points with a NaN coordinate are never accepted.
 * Modes:  KNN     radius <= 0, max_nn 1..128   (SearchKNN)
 *         Hybrid  radius >  0, max_nn 1..128   (SearchHybrid)
 *         Radius  radius >  0, max_nn 0..128   (SearchRadius; max_nn == 0 counts only: idx and d2 are NULL)
 * Without `total` a Hybrid search ends at its max_nn-th neighbour; with it, it visits everything within the radius.
 * The target's grid index is used if it has one (o3ds_cloud_build_index, o3ds_estimate_normals, an earlier search) and built and left
 * with the cloud otherwise; a target in the persistent map form is first folded into its array.  An empty target is not an error: every
 * list is empty.  O3DS_ERR_INVALID_ARG: max_nn < 0 or > 128, max_nn == 0 without a radius, idx NULL with max_nn > 0 (or the reverse),
 * an unknown id, a query_idx entry beyond the query cloud, clouds of two storage types, a target with an infinite coordinate.
 * Waits for the result. */
int o3ds_neighbor_search(o3ds_handle h, o3ds_cloud queries, o3ds_cloud target, const double T[16] /* NULL: queries as stored */,
                         const uint32_t* query_idx /* NULL: all points of `queries`, in order */, size_t n_queries, int max_nn, double radius,
                         uint32_t* idx /* n_queries * max_nn, row i = list of query i; NULL iff max_nn == 0 */,
                         double* d2 /* same shape; may be NULL */, uint32_t* count /* n_queries: entries of row i that are valid */,
                         uint32_t* total /* n_queries; may be NULL */);
/* [O3D] PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio), wholly on the device: the KNN search above with the cloud as its
 * own target (self included, so one term is 0), a_i = (sum of sqrt(d2)) / count over point i's list, square root and sum in f64 in list
 * order; a point is valid iff a_i > 0; mean = sum a_i / n_valid and std = sqrt(sum (a_i - mean)^2 / (n_valid - 1)) over the valid points,
 * both sums in f64 in the fixed order of o3ds_cloud_center; point i is kept iff a_i > 0 && a_i < mean + std_ratio * std.  With
 * n_valid < 2 the threshold is NaN (0 / 0) and nothing is kept.  `out` receives the kept points with their normals and colours, in cloud
 * order, as o3ds_crop_cloud carries them (FPFH features are not carried); kept_idx (may be NULL) their indices in `in`, at most
 * `capacity` of them -- more kept points than that: O3DS_ERR_CAPACITY, *n_kept holds their number and no cloud is made.
 * O3DS_ERR_INVALID_ARG with Open3D's message for nb_neighbors < 1 or std_ratio <= 0; nb_neighbors > 128 is unsupported. */
int o3ds_remove_statistical_outliers(o3ds_handle h, o3ds_cloud in, int nb_neighbors, double std_ratio, o3ds_cloud* out,
                                     uint32_t* kept_idx /* may be NULL */, size_t capacity, size_t* n_kept);
/* [O3D] PointCloud::RemoveRadiusOutliers(nb_points, radius): point i is kept iff total_i > nb_points, total_i the Radius-mode count of
 * the search above with the cloud as its own target, self included.  Output and errors as for the statistical filter (Open3D's message
 * for nb_points < 1 or radius <= 0). */
int o3ds_remove_radius_outliers(o3ds_handle h, o3ds_cloud in, int nb_points, double radius, o3ds_cloud* out, uint32_t* kept_idx /* may be NULL */,
                                size_t capacity, size_t* n_kept);
/* ---- [O3D] PointCloud::ClusterDBSCAN(eps, min_points) on a device cloud, and the filter that drops the noise and the small clusters ----
 * The labels are defined without reference to a search structure, with the arithmetic of the neighbour search above:
 *   - coordinates are the stored ones; d2(i, j) = (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own;
 *   - j is a neighbour of i iff d2 is finite and d2 < storage(eps * eps), strictly, the product formed in f64;
 *   - N_i is the neighbour set of point i in its own cloud, self included; a point with a non-finite coordinate has an empty N_i;
 *   - i is a core point iff |N_i| >= min_points;
 *   - the clusters are the connected components of the graph on the core points with an edge i - j iff j is in N_i (the relation is
 *     symmetric bit for bit); cluster ids are 0 .. n_clusters - 1, in the order of each component's smallest core index;
 *   - a point that is not core gets the smallest cluster id among the core points in N_i, or -1 if there is none.  (The smallest id is
 *     not the cluster of its lowest-index core neighbour.)
 * This closed form equals Open3D v0.15.1's sequential procedure -- seeds in index order, a breadth-first walk, a point first marked
 * noise relabelled by the first cluster that reaches it.  |N_i| has no upper limit.
 * labels receives one entry per point; cluster_sizes (may be NULL) the number of points labelled c, core and border, for c in
 * 0 .. n_clusters - 1.  An empty cloud gives *n_clusters = 0 and is not an error.  The cloud's grid index is used if it has one and built
 * and left with the cloud otherwise (no result depends on its cell size); a cloud in the persistent map form is first folded into its
 * array.  O3DS_ERR_INVALID_ARG: eps not greater than 0 or not finite, min_points < 1, an unknown id, labels NULL for a non-empty cloud,
 * an infinite coordinate (reported by the index build), 2^31 points or more.  O3DS_ERR_CAPACITY: capacity smaller than the cloud, or
 * size_capacity < n_clusters when cluster_sizes is given; *n_clusters is set all the same and neither array is written.
 * O3DS_ERR_HIP if a loop of the device's union-find exceeded its bound (never expected): nothing is published.  Waits for the result.
 * While profiling is enabled (o3ds_profile_enable) the library marks spans 11 (the hooking kernel), 12 (flatten and the rank scan) and
 * 13 (the border walk, labels and sizes); the count of |N_i| is span 10. */
int o3ds_cluster_dbscan(o3ds_handle h, o3ds_cloud cloud, double eps, int min_points, int32_t* labels /* n */, size_t capacity, size_t* n_clusters,
                        uint32_t* cluster_sizes /* may be NULL; n_clusters entries, at most size_capacity */, size_t size_capacity);
/* Point i is kept iff label_i >= 0 and cluster_sizes[label_i] >= min_cluster_size (>= 1; 1 drops the noise only), labels and sizes those
 * of o3ds_cluster_dbscan(eps, min_points), which never leave the device.  out, kept_idx, capacity, n_kept and O3DS_ERR_CAPACITY exactly as
 * for o3ds_remove_radius_outliers: points, normals and colours of the kept points in cloud order, FPFH features not carried. */
int o3ds_remove_small_clusters(o3ds_handle h, o3ds_cloud in, double eps, int min_points, int min_cluster_size, o3ds_cloud* out,
                               uint32_t* kept_idx /* may be NULL */, size_t capacity, size_t* n_kept);
/* ---- [O3D] PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations) on a device cloud, and the split by its plane ---------
 * The procedure of Open3D v0.15.1 (PointCloudSegmentation.cpp), restated from the upstream sources; like every [O3D] row it is not pinned
 * against a build of Open3D.  The result is defined here without reference to an implementation (tests/plane_restatement.py is the same
 * text in numpy):
 *   - COORDINATES are the stored ones widened to f64; all arithmetic is f64 whatever the storage, every operation rounded on its own (no
 *     fused multiply-add).  n is the number of points.
 *   - SUM ORDER.  Every sum over points below -- each hypothesis's error, the centroid, the six moments, the sums over a sample -- is taken
 *     in ONE order that depends on the number m of terms alone: len = max(1, ceil(m / 256)); chunk c (c = 0 .. 255) is the terms
 *     [c len, min(m, (c + 1) len)) added one after the other in index order onto +0.0 (an empty chunk is +0.0); then a halving tree over the
 *     256 chunk sums, v[t] = v[t] + v[t + s] for t < s, with s = 128, 64, ..., 1; the sum is v[0].  A term of a point that is no inlier is +0.0.
 *   - SAMPLE t (t = 0 .. num_iterations - 1) is the points mix(seed + (ransac_n t + j + 1) 0x9E3779B97F4A7C15) mod n for j = 0 ..
 *     ransac_n - 1, mix the splitmix64 finaliser and the arithmetic modulo 2^64 (the draw of o3ds_ransac_feature_matching).  It draws with
 *     replacement.  DEPARTURE: Open3D draws distinct indices from a generator seeded by std::random_device, so it has no sequence to
 *     reproduce; a repeated index among three gives the zero plane and is skipped like any collinear sample.
 *   - HYPOTHESIS PLANE.  ransac_n == 3 (ComputeTrianglePlane): (a, b, c) = (p1 - p0) x (p2 - p0), each component one product minus the
 *     other; norm = sqrt((a a + b b) + c c); norm == 0 gives the zero plane; else a, b, c are each divided by norm and
 *     d = -((a x0 + b y0) + c z0).  ransac_n > 3: the fit below over the sample's ransac_n points in sample order (m = ransac_n terms).
 *     A hypothesis is skipped, and counted in n_degenerate, iff all four coefficients are exactly 0; a plane with a NaN is evaluated and
 *     finds no inliers.
 *   - EVALUATION.  dist_i = |((a x + b y) + c z) + d|; point i is an inlier iff dist_i < distance_threshold, strictly (never for a NaN or an
 *     infinite dist_i); count = the number of inliers; error = sum of dist_i over the inliers (the distance, not its square: Open3D's rule);
 *     fitness = count / n; inlier_rmse = error / sqrt(count), 0 when count is 0.
 *   - WINNER.  The hypotheses that are not skipped are read in index order, starting from fitness 0 and inlier_rmse 0; hypothesis t replaces
 *     the best iff its fitness is greater, or its fitness is equal and its inlier_rmse strictly smaller.  All num_iterations hypotheses run
 *     (v0.15.1 has no early stop).  best_plane, fitness, inlier_rmse and best_t are the winner's.
 *   - INLIERS.  The points that pass the same test against best_plane, in cloud order; n_inliers of them.
 *   - FIT (GetPlaneFromPoints) of k points: centroid = (sum x / k, sum y / k, sum z / k); r = p - centroid; xx = sum r.x r.x, and xy, xz, yy,
 *     yz, zz alike; det_x = yy zz - yz yz, det_y = xx zz - xz xz, det_z = xx yy - xy xy; the largest picks the axis, x if det_x >= det_y and
 *     det_x >= det_z, else y if det_y >= det_z, else z; the normal is
 *         x: (det_x, xz yz - xy zz, xy yz - xz yy)    y: (xz yz - xy zz, det_y, xy xz - yz xx)    z: (xy yz - xz yy, xy xz - yz xx, det_z)
 *     norm = sqrt((a a + b b) + c c); norm == 0 gives the zero plane (a NaN goes through); else a, b, c are each divided by norm and
 *     d = -((a cx + b cy) + c cz).  `plane` is this fit of the inliers (m = n terms, non-inliers +0.0, k = n_inliers).
 *   - NO WINNER (num_iterations == 0, distance_threshold <= 0 or NaN, every sample degenerate, no hypothesis with an inlier): plane and
 *     best_plane are zeros, fitness and inlier_rmse 0, best_t -1, n_inliers 0, the inlier cloud is empty and the rest is a copy of the cloud.
 *     DEPARTURE: Open3D returns a plane of NaNs here.
 * inlier_idx (may be NULL) receives the inliers' indices, ascending, at most `capacity` of them; inliers_out (may be NULL) is
 * SelectByIndex(inliers) and rest_out (may be NULL) SelectByIndex(inliers, invert = true): points, normals and colours in cloud order, as
 * o3ds_remove_radius_outliers carries them; FPFH features are not carried.  More inliers than `capacity` with inlier_idx given:
 * O3DS_ERR_CAPACITY, *out is complete (n_inliers holds their number) and no cloud is made.  A cloud in the persistent map form is first
 * folded into its array; no grid index is built or needed, and an infinite coordinate is no error (such a point is never an inlier).
 * O3DS_ERR_INVALID_ARG: ransac_n < 3 and n < ransac_n (an empty cloud included) with Open3D's messages, ransac_n > 8, num_iterations < 0 or
 * > 16 777 216, an unknown id, out NULL, inlier_idx NULL with capacity > 0, 2^31 points or more.  Waits for the result.  While profiling
 * is enabled the library marks span 14 around every launch of the kernel that evaluates a batch of hypotheses against all points. */
typedef struct {
  double plane[4];        /* a x + b y + c z + d = 0, refitted on the inliers; zeros when there is no winner */
  double best_plane[4];   /* the winning hypothesis before the refit */
  double fitness, inlier_rmse; /* of the winning hypothesis */
  uint64_t n_inliers;
  int64_t best_t;         /* winning hypothesis, -1: none */
  int64_t n_degenerate;   /* hypotheses skipped because their plane was zero */
} o3ds_plane_result;
int o3ds_segment_plane(o3ds_handle h, o3ds_cloud cloud, double distance_threshold, int ransac_n, int64_t num_iterations, uint64_t seed,
                       o3ds_plane_result* out, uint32_t* inlier_idx /* may be NULL */, size_t capacity,
                       o3ds_cloud* inliers_out /* may be NULL */, o3ds_cloud* rest_out /* may be NULL */);
/* mapCloud_ += cloud (Submap.cpp:70; [O3D] PointCloud::operator+=). Appends `add` to `map` in place. */
int o3ds_cloud_append(o3ds_handle h, o3ds_cloud map, o3ds_cloud add);
/* A copy of a cloud of handle `src` as a cloud of handle `dst` (same device, same storage precision), device to device: points,
 * normals, colours and the known bounding box; the search index is not copied.  This is how a scan that one worker pre-processed
 * (ScanToMapIcp::processForScanMatchingAndMerging on the mapping thread's handle, ScanToMapRegistration.cpp:42-54) reaches the
 * handle that owns the submap (Submap::insertScan, Submap.cpp:39-75; ScanToMapIcp::scanToMapRegistration, :55-62) without a second
 * trip through host memory -- the reference passes the same host PointCloud to both.  `dst`'s stream waits for what `src` queued;
 * neither handle may be in use by another thread during the call; returns when the copy is complete. */
int o3ds_cloud_copy_across(o3ds_handle dst, o3ds_handle src, o3ds_cloud src_cloud, o3ds_cloud* out);
/* The same hand-over WITHOUT the source handle: open3d_slam's odometry and mapping workers run on two threads (SlamWrapper.cpp:227-236),
 * each with its own handle, and the mapper wants the scan the odometry worker pre-processed while that worker is busy registering -- a
 * call that needs both handles idle (o3ds_cloud_copy_across) either waits for the other worker or falls back to the host arrays.
 * o3ds_cloud_export_view, called by the OWNER right after it made the cloud, freezes what a copy needs -- the device arrays, the size,
 * the box, and an event behind everything the owner has queued for the cloud -- in a plain struct the caller keeps with the cloud;
 * o3ds_cloud_import_view makes a copy on `dst` from the struct alone (dst's stream waits for the event; device-to-device copies;
 * complete on return) and may run while the owner's handle is in use by its own thread.  The owner keeps the cloud alive and does not
 * change it while views of it are in use (a pre-processed scan is never changed), and releases the view (its event) before or after
 * freeing the cloud.  Same device, same storage precision. */
typedef struct o3ds_cloud_view {
  void* pts;
  void* nrm;
  void* col;
  size_t n;
  int precision;
  int device;
  int has_box;
  int reserved;
  double box_min[3], box_max[3];
  void* event;
} o3ds_cloud_view;
int o3ds_cloud_export_view(o3ds_handle h, o3ds_cloud c, o3ds_cloud_view* out);
int o3ds_cloud_import_view(o3ds_handle dst, const o3ds_cloud_view* view, o3ds_cloud* out);
int o3ds_cloud_view_release(o3ds_cloud_view* view);
/* voxelizeWithinCroppingVolume (helpers.cpp:115-183) via Submap::voxelizeInsideCroppingVolume (Submap.cpp:138-144):
 * points outside the volume pass through (original order, first); points inside are replaced by per-voxel means on
 * the WORLD-anchored grid key = floor(p * (1/voxel)) (VoxelHashMap.hpp:47-50), normals averaged (NaN skipped) and
 * re-normalised (helpers.cpp:172).  Voxel means are emitted in ascending key order.  In place. */
int o3ds_voxelize_within_volume(o3ds_handle h, o3ds_cloud map, double voxel_size, const o3ds_crop* crop);
/* (Submap::insertScan's core in one call: o3ds_map_insert_scan, declared with its description at the end of this header.) */
/* ConstantVelocityMotionCompensation::undistortInputPointCloud (src/MotionCompensation.cpp:64-139), in place on a device cloud in
 * the sensor frame: every point is moved by the motion accumulated over phase * scan_duration at the given constant velocity
 * (phase = azimuth / 2 pi, or 1 - that for spinning_clockwise; angular velocity as roll / pitch / yaw rates, R = Rz Ry Rx).  The
 * velocities are estimated from the pose buffer by the caller (estimateLinearAndAngularVelocity, :33-58).  Normals and the NN index
 * of the cloud, if any, are dropped (the reference de-skews raw scans). */
int o3ds_cloud_undistort(o3ds_handle h, o3ds_cloud cloud, const double linear_velocity[3], const double angular_velocity_rpy[3],
                         double scan_duration, int spinning_clockwise);
/* Dense voxel map = VoxelizedPointCloud (include/open3d_slam/Voxel.hpp:38-76, src/Voxel.cpp:18-114), the "TSDF-style" fusion of
 * BASELINE configs[4]: a persistent map voxel (key floor(p / voxel_size)) -> {count, sum of positions, sum of normals}.
 *   insert    : VoxelizedPointCloud::insert of o3d_slam::transform(T, cloud) (Submap::insertScanDenseMap, Submap.cpp:77-92); T may be
 *               NULL (identity).  The cropping steps of insertScanDenseMap are o3ds_crop_cloud calls of the caller.
 *   to_cloud  : toPointCloud -- sum / count per voxel (the mean normal is NOT re-normalised, Voxel.cpp:21-23), voxels in ascending key
 *               order (the reference's order is its hash map's).
 *   transform : VoxelizedPointCloud::transform (Voxel.cpp:49-64) as written: keys unchanged, the Isometry applied to the sums as
 *               if they were points (its translation enters the position sum once, and the normal sum too).
 * Sums are kept in fixed point on the device (2^-30 m / 2^-40), so a map does not depend on the order of concurrent insertions.
 *   carve     : Submap::carve for the dense map (Submap.cpp:126-136): the scan (placed by scan_pose, NULL = identity -- NB the
 *               reference passes the RAW scan, i.e. sensor-frame points, together with the map-frame sensor position, Submap.cpp:88)
 *               is reduced to the first point of every voxel (removeDuplicatePointsWithinSameVoxels, Voxel.cpp:162-191); every kept
 *               point casts a ray from sensor_position sampled every 2 * neighborhood_radius while
 *               distance < max(2 * radius, min(length - truncation, max_length)); at every sample the voxels of
 *               getVoxelsWithinPointNeighborhood (VoxelHashMap.cpp:13-44) are removed (helpers.cpp:347-377).
 *               neighborhood_radius must be > 0: with 0 the reference's own ray loop (step 2 * radius) never terminates. */
typedef uint64_t o3ds_dense_map;
int o3ds_dense_map_create(o3ds_handle h, double voxel_size, o3ds_dense_map* out);
int o3ds_dense_map_free(o3ds_handle h, o3ds_dense_map id);
int o3ds_dense_map_insert(o3ds_handle h, o3ds_dense_map id, o3ds_cloud cloud, const double T[16]);
int o3ds_dense_map_size(o3ds_handle h, o3ds_dense_map id, size_t* n_voxels);
int o3ds_dense_map_to_cloud(o3ds_handle h, o3ds_dense_map id, o3ds_cloud* out);
int o3ds_dense_map_transform(o3ds_handle h, o3ds_dense_map id, const double T[16]);
int o3ds_dense_map_carve(o3ds_handle h, o3ds_dense_map id, o3ds_cloud scan, const double scan_pose[16], const double sensor_position[3],
                         double neighborhood_radius, double max_raytracing_length, double truncation_distance, size_t* n_removed);
/* Number of points of `cloud` (placed by T; NULL = identity) that fall into an occupied voxel of the map:
 * VoxelHashMap::hasVoxelContainingPoint per point, the count behind SubmapCollection::isSwitchingSubmapsConsistant
 * (src/SubmapCollection.cpp:352-364: fitness = hits / scan size, compared with adjacencyBasedRevisitingMinFitness_). */
/* ONE dense voxel map over several GPUs (BASELINE.json configs[4]; SURVEY.md 8e "map fusion across GPUs"): a voxel lives on the rank
 * hash(voxel) mod world, with the reference's own hash (VoxelHashMap.hpp:25-35).  export places the cloud by T (NULL: as it is), rounds
 * to the storage type, drops non-finite points and writes the rows [x y z nx ny nz] (doubles; zeros when the cloud has no normals)
 * grouped by owner into d_rows (device memory, capacity cloud size x 6) and the group sizes into d_counts (device memory, world
 * entries) -- the send buffer and split sizes of one all-to-all.  import turns received rows into a cloud of this handle, ready for
 * o3ds_dense_map_insert.  No host copy on either side of the collective. */
int o3ds_cloud_export_rows_by_owner(o3ds_handle h, o3ds_cloud cloud, const double T[16], double voxel_size, int world, double* d_rows,
                                    long long* d_counts);
int o3ds_cloud_import_rows(o3ds_handle h, const double* d_rows, size_t n, int has_normals, o3ds_cloud* out);
int o3ds_dense_map_count_occupied(o3ds_handle h, o3ds_dense_map id, o3ds_cloud cloud, const double T[16], size_t* n_hits);
/* computeIndicesOfOverlappingPoints (src/helpers.cpp:307-332; call sites src/PlaceRecognition.cpp:103,
 * src/constraint_builders.cpp:54): both clouds are binned with the voxel key floor(p / voxel_size) -- the source after being
 * placed by source_to_target --, and every voxel that holds at least min_points_per_voxel points of EACH cloud contributes all its
 * source and all its target indices.  idx_source / idx_target: caller buffers with room for every point of the respective cloud;
 * filled in ascending order (the reference's order is its hash map's iteration order, i.e. unspecified). */
int o3ds_overlap_indices(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double source_to_target[16], double voxel_size,
                         size_t min_points_per_voxel, uint64_t* idx_source, size_t* n_idx_source, uint64_t* idx_target, size_t* n_idx_target);
/* Submap::carve for the sparse map (Submap.cpp:109-125 -> getIdxsOfCarvedPoints, helpers.cpp:235-271; SpaceCarvingParameters,
 * Parameters.hpp:85-92): the raw scan (sensor frame) is placed with map_to_range_sensor; every ray from the sensor position is
 * sampled every voxel_size metres while distance < max(voxel_size, min(length - truncation_distance, max_raytracing_length));
 * map points inside map_builder_crop that share a sampled voxel (key floor(p / voxel_size)) are removed when the map has no
 * normals or |ray direction . unit normal| > min_dot_product_with_normal.  The surviving points keep their order.  The caller
 * decides WHEN to carve (nScansInsertedMap_ % carveSpaceEveryNscans_ == 1, Submap.cpp:111). */
typedef struct {
  double voxel_size;                  /* 0.1  */
  double max_raytracing_length;       /* 20.0 */
  double truncation_distance;         /* 0.1  */
  double min_dot_product_with_normal; /* 0.5  */
} o3ds_carving_params;
int o3ds_map_carve(o3ds_handle h, o3ds_cloud map, o3ds_cloud raw_scan, const double map_to_range_sensor[16],
                   const o3ds_crop* map_builder_crop, const o3ds_carving_params* params, size_t* n_removed);
/* The same, and the carved points come back as a cloud of their own (map order; empty when nothing was carved): what Submap::carve keeps in
 * its toRemove_ member for the visualisation (Submap.cpp:119, `toRemove_ = *map->SelectByIndex(idxsToRemove)`).  removed_out may be NULL. */
int o3ds_map_carve_removed(o3ds_handle h, o3ds_cloud map, o3ds_cloud raw_scan, const double map_to_range_sensor[16],
                           const o3ds_crop* map_builder_crop, const o3ds_carving_params* params, size_t* n_removed, o3ds_cloud* removed_out);
/* Submap::insertScan's tail (Submap.cpp:66-75): map += T * scan, voxelizeWithinCroppingVolume(map_voxel_size, map_builder_crop)
 * (helpers.cpp:115-183), and -- max_corr_hint > 0 -- the map's search index for the next registration.  The RESULT is the reference's: the
 * array [points outside the volume in their previous order | one mean per voxel inside it, in voxel-key order], bit for bit in f64
 * storage.  HOW it is kept is the backend's: from its second insertion on a map with an index stays in a PERSISTENT form (slot arrays +
 * voxel hash + row-paged index; o3ds_cloud_is_persistent_map tells) that an insertion updates only where the scan falls --
 * the call queues eight kernels over the scan and returns, nothing is proportional to the map's size and nothing comes back to the host.
 * Colours follow [O3D] PointCloud::operator+= in that form as in the array: (1) coloured map, coloured scan: persistent, every slot
 * carries its colour (a voxel's: that of its last member in cloud order, see o3ds_cloud_set_colors); (2) uncoloured non-empty map,
 * coloured scan: persistent, the scan's colours are ignored as += drops them; (3) coloured map, uncoloured scan: the map is folded and
 * this insertion takes the array form, which drops the map's colours as += does -- later insertions re-enter the persistent form,
 * uncoloured.  o3ds_cloud_has_colors answers without folding.  The persistent form turns into
 * the array above when somebody asks for it: o3ds_cloud_download*, o3ds_map_carve with another voxel size, o3ds_overlap_indices,
 * o3ds_estimate_normals ON the map, a registration with the map as its SOURCE, any call that reads or rewrites the map as an array
 * (that fold sorts the live points once, O(N log N)).  o3ds_cloud_size answers from the device's counters (live = slots - dead) and
 * leaves the map persistent.
 * Registrations against the map (target = map) and o3ds_map_carve with params->voxel_size ==
 * map_voxel_size and n_removed == NULL or not -- the shipped configuration: 0.1 m both -- work on the persistent form directly.  The map's
 * o3ds_cloud_size_bound is an upper bound while it is in that form.  An error inside the queued kernels (an internal capacity) is
 * reported by the next call on the map. */
int o3ds_map_insert_scan(o3ds_handle h, o3ds_cloud map, o3ds_cloud scan, const double T[16], double map_voxel_size,
                         const o3ds_crop* map_builder_crop, double max_corr_hint);

/* ---- place recognition: PlaceRecognition::buildLoopClosureConstraints' front half (src/PlaceRecognition.cpp:71-90) ---------------
 * [O3D] ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) as Submap::computeFeatures calls it (src/Submap.cpp:228-248):
 * the neighbourhood of point i is the max_nn smallest (d2, index) among the points with d2 < radius^2, i itself included (the set
 * o3ds_estimate_normals keeps); 33 bins per point, f64 arithmetic whatever the storage precision.  The cloud must have normals
 * (O3DS_ERR_INVALID_ARG otherwise), 1 <= max_nn <= 128.  The n x 33 doubles are kept on the cloud like its normals and dropped by every
 * call that changes the cloud's points or normals in place; a buffer beyond the handle's pool cap (O3DS_POOL_CAP_MB) is
 * O3DS_ERR_CAPACITY.  download_fpfh: n x 33 row-major doubles, capacity in points. */
int o3ds_compute_fpfh(o3ds_handle h, o3ds_cloud cloud, double radius, int max_nn);
int o3ds_cloud_has_fpfh(o3ds_handle h, o3ds_cloud cloud, int* has_fpfh);
int o3ds_cloud_download_fpfh(o3ds_handle h, o3ds_cloud cloud, double* out, size_t capacity);
/* The correspondences of [O3D] RegistrationRANSACBasedOnFeatureMatching: for every source point i, j = the target point whose feature
 * is nearest (sum over the 33 bins of the squared difference, f64, ties to the lower index).  mutual_filter: keep (i, j) only where
 * the nearest source feature of j is i, in source order; fewer than 3 ransac_n such pairs falls back to the one-way set
 * (*fell_back = 1).  pairs: [n][2] (source, target) with room for capacity pairs; *n_pairs is set even when the buffer is too small
 * (O3DS_ERR_CAPACITY).  Both clouds need features. */
int o3ds_feature_correspondences(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, int mutual_filter, int ransac_n, uint32_t* pairs,
                                 size_t capacity, size_t* n_pairs, int* fell_back);
/* [O3D] RegistrationRANSACBasedOnFeatureMatching(source, target, features, mutual_filter, max_correspondence_distance,
 * TransformationEstimationPointToPoint(false), ransac_n, {CorrespondenceCheckerBasedOnEdgeLength(edge_length),
 * CorrespondenceCheckerBasedOnDistance(distance)}, RANSACConvergenceCriteria(max_iteration, confidence)).
 *   sampling   hypothesis t draws correspondence indices mix(seed + (ransac_n t + j + 1) 0x9E3779B97F4A7C15) mod m, j < ransac_n (with
 *              replacement; mix = splitmix64's finaliser, as o3ds_random_down_sample).  Open3D seeds from std::random_device -- there
 *              is no sequence to reproduce --; here the result is a function of (clouds, features, parameters, seed) alone.
 *   estimate   Umeyama without scaling over the sample; the checkers run where their threshold is > 0.
 *   validate   every source point placed by T, its nearest target point with d2 < max_correspondence_distance^2; fitness = pairs /
 *              n_src, rmse = sqrt(sum d2 / pairs).  Better = more pairs, then lower rmse, then lower t.
 *   stopping   Open3D's loop read in index order: est_k = max_iteration; t runs iff t < est_k; when t improves the best,
 *              est_k = ceil(log(1 - confidence) / log(1 - fitness^ransac_n)) if that is below est_k (confidence clamped to [0, 1]).
 *              The device evaluates hypotheses in batches and folds each batch in index order: the cut and the winner are the serial
 *              rule's for any batch size.
 * ransac_n < 3, fewer correspondences than ransac_n or max_correspondence_distance <= 0: Open3D's empty RegistrationResult (identity,
 * zeros, best_t = -1).  ransac_n > 8: O3DS_ERR_INVALID_ARG.  trace (may be NULL): entry t < trace_cap describes hypothesis t; entries of
 * hypotheses that did not run have checks = -1. */
typedef struct {
  int32_t mutual_filter;
  int32_t ransac_n;                   /* ransacModelSize_ */
  double max_correspondence_distance; /* ransacMaxCorrespondenceDistance_ */
  double edge_length;                 /* correspondenceCheckerEdgeLength_ (similarity), <= 0: no checker */
  double distance;                    /* correspondenceCheckerDistance_, <= 0: no checker */
  int64_t max_iteration;              /* ransacNumIter_ */
  double confidence;                  /* ransacProbability_ */
} o3ds_ransac_params;
typedef struct {
  double transformation[16]; /* column-major */
  double fitness;
  double inlier_rmse;
  uint64_t n_corr;           /* correspondence_set_.size() of the result */
  uint64_t n_feature_corr;   /* feature correspondences RANSAC drew from */
  int64_t iterations_run;    /* hypotheses the serial rule runs */
  int64_t validations;       /* of which passed both checkers and were validated */
  int64_t best_t;            /* the winner, -1 = none */
  int32_t fell_back;         /* the mutual set was too small */
  int32_t reserved;
} o3ds_ransac_result;
typedef struct {
  uint32_t sample[8];        /* correspondence indices drawn (ransac_n of them) */
  int32_t checks;            /* bit 0: edge length passed (or off), bit 1: distance passed (or off); -1: not run */
  int32_t pairs;             /* validated: correspondences found; -1: not validated */
  double error_sum;          /* validated: sum of d2 */
  double transformation[16]; /* the estimate, column-major */
} o3ds_ransac_trace;
int o3ds_ransac_feature_matching(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const o3ds_ransac_params* params, uint64_t seed,
                                 o3ds_ransac_result* out, o3ds_ransac_trace* trace, size_t trace_cap);

/* ---- pose-graph optimisation: OptimizationProblem::solve (src/OptimizationProblem.cpp:26-44) -----------------------------------------
 * [O3D] GlobalOptimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option) of Open3D v0.15.1, restated:
 *   1. ValidatePoseGraph: a graph that is not connected (over all edges), or a certain edge whose confidence is not 1, is Open3D's
 *      "warn and return unchanged": O3DS_OK, out->valid = 0, poses and edges untouched.
 *   2. an LM pass over every edge (the line-process weight preference * d^2 * mean(information(5,5)), the confidences of the uncertain
 *      edges (mu / (mu + e^T Info e))^2, lambda0 = 1e-5 max diag(H), Open3D's stop checks);
 *   3. CreatePoseGraphWithoutInvalidEdges: uncertain edges with confidence <= edge_prune_threshold are dropped (edge_kept[k] = 0);
 *   4. a second LM pass on the pruned graph with its own line-process weight;
 *   5. CompensateReferencePoseGraphNode: 0 <= reference_node < n_nodes keeps that node's input pose (every pose is premultiplied).
 * Everything runs on the handle's stream in f64 whatever its storage precision: per-edge residuals and Jacobians, H (6N x 6N, dense)
 * and b summed per block in edge order (no atomics), the solve of (H + lambda I) delta = b by Cholesky (one workgroup in LDS for
 * 6N <= 128, blocked with an f64-MFMA trailing update above), the pose update and the step's sums in a fixed order.  The LM control
 * flow runs on the host on those numbers, so a run is bit-reproducible.  A non-positive pivot is O3DS_ERR_INVALID_ARG.
 * node_poses: n_nodes x 16 column-major, replaced by the optimised poses.  edges[k].confidence: in, Open3D's 1.0 by default for a new
 * edge; out, its value after the last pass that held the edge.  Node ids out of range or a non-finite input: O3DS_ERR_INVALID_ARG.
 * 0 or 1 nodes: valid = 1, nothing changes.  More than 4096 nodes (H and its factor are (6N)^2 doubles each, 4.8 GB at the cap) or
 * 2^20 edges: O3DS_ERR_CAPACITY.  stop_reason: 0 none ran, 1 right term (max(b) < min_right_term), 2 relative increment, 3 relative
 * residual increment, 4 residual, 5 max iteration, 6 max LM iteration (the first check that stopped the pass). */
typedef struct {
  int32_t source_node_id, target_node_id;
  int32_t uncertain;          /* loop closures: 1, odometry: 0 */
  int32_t pad;
  double transformation[16];  /* column-major */
  double information[36];     /* row-major 6x6 */
  double confidence;          /* in: 1.0 (Open3D's default); out: final */
} o3ds_pose_graph_edge;
typedef struct {
  double max_correspondence_distance; /* GlobalOptimizationParameters::maxCorrespondenceDistance_ */
  double edge_prune_threshold;        /* edgePruneThreshold_ */
  double preference_loop_closure;     /* loopClosurePreference_ */
  int32_t reference_node;             /* referenceNode_, -1: none */
  int32_t pad;
} o3ds_global_optimization_option;
typedef struct {
  int32_t max_iteration, max_iteration_lm; /* Open3D's defaults: 100, 20 */
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual; /* 1e-6 each */
  double upper_scale_factor, lower_scale_factor;                                               /* 2/3, 1/3 */
} o3ds_global_optimization_criteria;
typedef struct {
  int32_t valid, n_edges_kept;
  int32_t iterations[2], lm_steps[2], stop_reason[2]; /* per pass: outer iterations, linear solves, why it stopped */
  double residual[2], line_process_weight[2];
} o3ds_pose_graph_result;
int o3ds_global_optimization(o3ds_handle h, double* node_poses, size_t n_nodes, o3ds_pose_graph_edge* edges, size_t n_edges,
                             const o3ds_global_optimization_option* opt, const o3ds_global_optimization_criteria* crit, uint8_t* edge_kept,
                             o3ds_pose_graph_result* out);

/* ---- coloured ICP: [O3D] pipelines::registration::RegistrationColoredICP (Park, Zhou, Koltun 2017), the fourth RegistrationICP estimator --
 * Open3D v0.15.1's procedure (ColoredICP.cpp), restated from the upstream sources; like every [O3D] row it is not pinned against a build of
 * Open3D.  The reference ships no caller of it (there is no CloudRegistrationType for it): the entry points are OFFERED and are not
 * switched on in the frame loop.  Everything is defined here without reference to an implementation (tests/colored_icp_restatement.py is
 * the same text in numpy):
 *   - ARITHMETIC is f64 on the stored values widened (points, normals and colours are held in the storage type), every operation rounded
 *     on its own (no fused multiply-add).  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 *     a.x b.y - a.y b.x); the intensity of a colour is I = ((r + g) + b) / 3.0.
 *
 * 1. COLOUR GRADIENTS of a cloud, [O3D] InitializePointCloudForColoredICP with KDTreeSearchParamHybrid(radius, max_nn), 1 <= max_nn <= 128.
 *    For point k with point p, normal n, intensity I: L is the Hybrid list of o3ds_neighbor_search of point k in its own cloud at (radius,
 *    max_nn), in that search's order (d2, original index).  Fewer than 4 entries: the gradient is (0, 0, 0).  Otherwise the FIRST entry of L
 *    is skipped, whichever point it is (Open3D assumes it is the point itself; among exact duplicates it need not be -- the definition
 *    follows Open3D), and every other entry j, in list order, gives a row
 *        e = dot(q_j - p, n);   a = (q_j - e n) - p, per component;   b = I_j - I
 *    followed by a last row a = (|L| - 1) n, b = 0.  M = sum a a^T and v = sum a b, every entry summed in that row order onto +0.0
 *    (M[r][c] += a[r] a[c], v[r] += a[r] b).  M x = v is solved by an UNPIVOTED LDL^T in this order:
 *        d0 = M00;  l10 = M10 / d0;  l20 = M20 / d0;  d1 = M11 - l10 M10;  w = M21 - l20 M10;  l21 = w / d1;
 *        d2 = (M22 - l20 M20) - l21 w;  y0 = v0;  y1 = v1 - l10 y0;  y2 = (v2 - l20 y0) - l21 y1;
 *        x2 = y2 / d2;  x1 = y1 / d1 - l21 x2;  x0 = (y0 / d0 - l10 x1) - l20 x2.
 *    DEPARTURE: a pivot d0, d1 or d2 that is not finite or not greater than 0 gives the gradient (0, 0, 0) -- a NaN normal, a non-finite
 *    neighbourhood, and a zero normal or a collinear neighbourhood wherever the cancellation is exact; Open3D takes whatever Eigen's pivoted
 *    ldlt() returns.  A point with a non-finite coordinate has an empty list, hence a zero gradient.
 *    The n x 3 doubles stay on the cloud, remembered with the (radius, max_nn) that made them.  They are DROPPED by every call that changes
 *    the cloud's points, normals or colours in place (o3ds_cloud_set_colors*, o3ds_estimate_normals, o3ds_cloud_append, the map merges,
 *    carving, de-skew) and are NOT CARRIED into any cloud another call makes (crop, select, filter, copy; o3ds_transform_cloud would have to
 *    rotate them and does not).  O3DS_ERR_NO_NORMALS / O3DS_ERR_INVALID_ARG for a non-empty cloud without normals / without colours;
 *    O3DS_ERR_INVALID_ARG for radius <= 0, max_nn outside 1..128, an unknown id, an infinite coordinate (the index build reports it);
 *    O3DS_ERR_CAPACITY for 2^31 points or a buffer beyond the pool cap.  A persistent-form map is folded into its array first.
 *    While profiling is enabled the library marks span 15 around the gradient kernel (its search is span 10).
 *    download: n x 3 row-major doubles, capacity in points. */
int o3ds_compute_color_gradients(o3ds_handle h, o3ds_cloud cloud, double radius, int max_nn);
int o3ds_cloud_has_color_gradients(o3ds_handle h, o3ds_cloud cloud, int* has_gradients);
int o3ds_cloud_download_color_gradients(o3ds_handle h, o3ds_cloud cloud, double* out, size_t capacity);
/* 2. ONE COLOURED STEP: [O3D] TransformationEstimationForColoredICP::ComputeTransformation up to its solve, with the L2 loss (weights 1;
 *    the robust losses are o3ds_robust_icp_step's, below).  One correspondence pass and one reduction; waits for the record.  The testable unit, as
 *    o3ds_icp_accumulate is for the other estimators.  The target must have normals, colours and gradients (of any parameters), the
 *    source colours.
 *    CORRESPONDENCES are the neighbour search's own: o3ds_neighbor_search(source, target, T, Hybrid, max_nn = 1, radius =
 *    max_correspondence_distance) -- the query is storage(T s), d2 is taken in the storage type and accepted iff strictly below
 *    storage(r r), ties go to the lower original target index.
 *    PER ACCEPTED PAIR, with p the query widened, q, n, g the target's point, normal and gradient, I_s and I_t the two intensities,
 *    sg = sqrt(lambda_geometric), sp = sqrt(1 - lambda_geometric):
 *        dn = dot(p - q, n);                      J_G = (sg cross(p, n) ; sg n), per component;   r_G = sg dn;
 *        p' = p - dn n, per component;            I_0 = dot(g, p' - q) + I_t;      gn = dot(g, n);
 *        g_M = gn n - g, per component;           J_I = (sp cross(p, g_M) ; sp g_M);              r_I = sp (I_s - I_0).
 *    RECORD TERMS of the pair (the layout of o3ds_icp_accumulate): [0..20] the upper triangle, row-major, of J_G[r] J_G[c] + J_I[r] J_I[c];
 *    [21..26] J_G[r] r_G + J_I[r] r_I; [27] r_G r_G + r_I r_I; [28] 1; [29] the search's d2 widened.  [30..31] of the record are 0.
 *    SUM ORDER, a function of the number of source points alone (never of launch geometry, handle or timing; no floating-point atomics):
 *    the term of a query without a correspondence is +0.0; the queries are cut into blocks of 256 in index order, the missing queries of
 *    the last block being +0.0; inside a block a halving tree, v[t] = v[t] + v[t + s] for t < s, s = 128, 64, ..., 1, the block's sum is
 *    v[0]; the block sums are added in ascending block order onto +0.0.  An empty source, or a target without a finite point, gives the
 *    zero record.
 *    While profiling is enabled the library marks span 16 around the two kernels of the step (the search is span 10). */
int o3ds_colored_icp_step(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance,
                          double lambda_geometric, double record[32]);
/* 3. THE REGISTRATION: [O3D] RegistrationColoredICP(source, target, max_correspondence_distance, init,
 *    TransformationEstimationForColoredICP(lambda_geometric), criteria).  params is o3ds_icp_params with `method` ignored; Open3D's default
 *    lambda_geometric is 0.968.  The loop is [O3D] RegistrationICP's: pass j evaluates the step above under the current pose; fitness =
 *    [28] / |source| and inlier_rmse = sqrt([29] / [28]) (0 without correspondences); from the second pass on the loop ends as converged
 *    when |fitness - previous| < relative_fitness and |inlier_rmse - previous| < relative_rmse; otherwise, while fewer than max_iteration
 *    updates have been applied, the 6x6 system [0..20] x = -[21..26] is solved (LDL^T, the solve of o3ds_icp_update, with the point-to-plane
 *    estimator's treatment of an empty correspondence set: the identity) and T <- (Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5) T.  max_iteration
 *    solves take max_iteration + 1 passes; fitness, inlier_rmse and n_corr are those of the pass after the last update.  The record of
 *    every pass is consumed on the device by the kernel behind o3ds_icp_update; the host reads the state it publishes once per pass.
 *    The result is a function of (clouds, params, lambda_geometric, init) alone: two calls give the same bytes.
 *    GRADIENTS of the target are those of (2 max_correspondence_distance, 30), as RegistrationColoredICP initialises it: computed if the
 *    cloud has none or has them from other parameters, and then LEFT on the cloud -- a map registered against repeatedly pays once, where
 *    Open3D pays per call.  The target's grid index is used if it has one and built and left with the cloud otherwise.
 *    There is no target_crop: a caller crops the map patch with o3ds_crop_cloud, which keeps colours, as the reference does.  A cloud in
 *    the persistent map form is folded into its array first.  An o3ds_icp_begin session open on the handle is ended.
 *    O3DS_ERR_NO_NORMALS: target without normals.  O3DS_ERR_EMPTY: empty target.  O3DS_ERR_INVALID_ARG: source or target without colours
 *    (Open3D's messages), lambda_geometric outside [0, 1] or NaN, max_correspondence_distance <= 0, clouds of two storage types, an
 *    unknown id, a negative max_iteration, a null pointer.  An empty source gives fitness 0 and the initial pose. */
int o3ds_icp_colored_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* params,
                         double lambda_geometric, o3ds_icp_result* out);

/* ---- robust loss kernels: [O3D] pipelines::registration::RobustKernel (Open3D v0.15.1, RobustKernel.cpp) on two estimators of the coloured
 * section above -- TransformationEstimationPointToPlane(kernel) and TransformationEstimationForColoredICP(lambda_geometric, kernel).  A
 * registration whose correspondences all weigh 1 is pulled by everything inside max_correspondence_distance that is not in the map (a moved
 * object, a person, the rim of a partial overlap); a robust loss weighs each residual by how plausible it is.  OFFERED like the coloured
 * section and switched on nowhere; the tuned geometric passes (o3ds_icp_register_dev and its kin) take no loss, and GICP is not covered.
 * ARITHMETIC, CORRESPONDENCES, SUM ORDER and the LOOP are those of the coloured section: f64 on stored values widened, every operation
 * rounded on its own (no fused multiply-add); the neighbour search's pairs under the query storage(T s); blocks of 256 queries in index order,
 * the halving tree inside a block, the block sums in ascending order onto +0.0.  tests/robust_icp_restatement.py is this text in numpy.
 *
 * WEIGHT of a residual r under a loss, with e = |r| ([O3D] <Loss>::Weight; the comparisons are as written, so a NaN residual takes
 * whatever they give):
 *     L2      1
 *     L1      1 / e                                      DEPARTURE: r == 0 gives 1 (Open3D gives inf, and NaN from inf * 0 in the sums)
 *     HUBER   e > k ? k / e : 1
 *     CAUCHY  1 / (1 + (r / k) (r / k))
 *     GM      k / ((k + r r) (k + r r))
 *     TUKEY   u = (e / k < 1) ? e / k : 1;   v = 1 - u u;   w = v v
 * k must be finite and > 0 for HUBER, CAUCHY, GM and TUKEY and is ignored for L2 and L1.  `reserved` must be 0. */
typedef enum { O3DS_LOSS_L2 = 0, O3DS_LOSS_L1 = 1, O3DS_LOSS_HUBER = 2, O3DS_LOSS_CAUCHY = 3, O3DS_LOSS_GM = 4, O3DS_LOSS_TUKEY = 5 } o3ds_loss_kind;
typedef struct {
  int32_t kind; /* o3ds_loss_kind */
  int32_t reserved;
  double k;
} o3ds_robust_loss; /* 16 bytes */
typedef enum { O3DS_ROBUST_POINT_TO_PLANE = 0, O3DS_ROBUST_COLORED = 1 } o3ds_robust_estimator;
/* 1. ONE ROBUST STEP.  Correspondences, the query p, and q, n, g, J_G, r_G, J_I, r_I of an accepted pair are exactly those of
 *    o3ds_colored_icp_step.  RECORD TERMS of the pair:
 *    COLORED, with w_G = Weight(r_G) and w_I = Weight(r_I) (Open3D's weighted form: each residual is weighted after its multiplication by
 *    sqrt(lambda) or sqrt(1 - lambda)): [0..20] the upper triangle, row-major, of w_G (J_G[r] J_G[c]) + w_I (J_I[r] J_I[c]); [21..26]
 *    w_G (J_G[r] r_G) + w_I (J_I[r] r_I); [27] r_G r_G + r_I r_I, UNWEIGHTED as in [O3D] ComputeJTJandJTr; [28] 1; [29] the search's d2
 *    widened; [30..31] of the record are 0.  The target must have normals, colours and gradients, the source colours, as for
 *    o3ds_colored_icp_step.  With the L2 loss the record is that of o3ds_colored_icp_step, bit for bit.
 *    POINT_TO_PLANE: J = (cross(p, n) ; n), r = dot(p - q, n), w = Weight(r): [0..20] w (J[r] J[c]); [21..26] w (J[r] r); [27] r r; the rest
 *    as above.  lambda_geometric is ignored (any value, NaN included).  The target needs normals only; colours and gradients are read on
 *    neither cloud.
 *    Empty cases and error codes are the coloured step's (an empty source, a target without a finite point, or no accepted pair: the zero
 *    record; O3DS_ERR_EMPTY for an empty target; O3DS_ERR_NO_NORMALS); in addition O3DS_ERR_INVALID_ARG for a null loss, an unknown kind, a
 *    non-zero `reserved`, a k that is not finite or not > 0 where the loss uses it, and an unknown estimator.
 *    While profiling is enabled the library marks span 17 around the two kernels of the step (the search is span 10). */
int o3ds_robust_icp_step(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance,
                         int estimator, double lambda_geometric, const o3ds_robust_loss* loss, double record[32]);
/* 2. THE REGISTRATION: [O3D] RegistrationICP(source, target, max_correspondence_distance, init, estimation(kernel), criteria): the loop of
 *    o3ds_icp_colored_dev around the step above -- the same convergence rule, the same solve and update.  fitness and inlier_rmse come
 *    from [28] and [29], which carry no weight: as in Open3D they do not depend on the loss.  A system whose weights are all zero
 *    ([0..26] all zero with [28] > 0: every pair at or beyond Tukey's k) gives the IDENTITY update: the solve follows Eigen's LDLT, which
 *    zeroes the components of pivots not above the smallest normal double.  For COLORED the target's gradients of
 *    (2 max_correspondence_distance, 30) are computed if absent and left on the target; POINT_TO_PLANE neither needs nor makes them.
 *    The result is a function of (clouds, params, estimator, lambda_geometric, loss, init) alone: two calls give the same bytes; with
 *    COLORED and the L2 loss they are the bytes of o3ds_icp_colored_dev.  Errors: those of o3ds_icp_colored_dev (for POINT_TO_PLANE
 *    without the colour requirements) and of the step above. */
int o3ds_icp_robust_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* params,
                        int estimator, double lambda_geometric, const o3ds_robust_loss* loss, o3ds_icp_result* out);

/* ---- degeneracy-aware ICP: which directions the normal equations of a pass leave unconstrained, and the update solved in the others only
 * (Zhang, Kaess, Singh, "On degeneracy of optimization-based state estimation", ICRA 2016: solution remapping; Tuna et al., X-ICP, 2022:
 * rotation and translation analysed apart, so that radians and metres are never compared).  In a corridor, on an open floor or facing one
 * wall the 6x6 system of the geometric estimators is near-singular: the solve makes something of a pivot that is noise, the pose slides
 * along the unobservable direction, and fitness and inlier_rmse stay excellent.  OFFERED like the two sections above and switched on nowhere;
 * with both thresholds 0 the registration below is o3ds_icp_robust_dev to the byte.  tests/degeneracy_restatement.py is this text in numpy.
 *
 * INPUT of the analysis: the 32-double record of a pass under the pose T (o3ds_robust_icp_step's: H = the symmetric matrix of [0..20],
 * g = -[21..26], n_corr = [28]) and c0, the centre of the source as stored, as o3ds_cloud_center forms it, taken once per call.
 * ARITHMETIC: f64, every operation rounded on its own (no fused multiply-add).  Every product of 6x6 matrices and of a matrix and a vector
 * is the dense one: entry (i, j) = P[i][0] Q[0][j], then + P[i][k] Q[k][j] for k = 1 .. 5, zeros included.
 *  1. RE-CENTRE.  c[i] = ((T[i][0] c0.x + T[i][1] c0.y) + T[i][2] c0.z) + T[i][3].  With x = (omega, t) the parameters of the update about
 *     the map origin and x_c those of the same motion as a rotation about c, x = M x_c, M = [[I, 0], [[c]x, I]], [c]x = ((0, -c.z, c.y),
 *     (c.z, 0, -c.x), (-c.y, c.x, 0)).  W = H M;  H_c = M^T W;  g_c = M^T g.  Of H_c the UPPER triangle is what is read below.  Without this the
 *     rotation block of a scan far from the origin is dominated by |p|^2 and says nothing about the scan.
 *  2. EIGEN-DECOMPOSE H_rr = H_c[0:3, 0:3] and, apart from it, H_tt = H_c[3:6, 3:6]: cyclic Jacobi, EIGHT sweeps over the pairs (0,1),
 *     (0,2), (1,2), from V = I.  One rotation on (p, q), r the third index: nothing if a_pq == 0; else theta = (a_qq - a_pp) / (2 a_pq);
 *     t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1));  c = 1 / sqrt(t t + 1);  s = t c;  h = t a_pq;  a_pp = a_pp - h;
 *     a_qq = a_qq + h;  a_pq = 0;  (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq);  for each row k of V: (V_kp, V_kq) = (c V_kp - s V_kq,
 *     s V_kp + c V_kq).  The values are the diagonal, the vectors the columns of V.  ORDER: ascending, by exchanging the pairs (0,1), (1,2),
 *     (0,1) in turn where the first value is > the second.  SIGN: a vector is negated if its component of largest magnitude (the first of
 *     equals) is < 0.
 *  3. NORMALISE: lambda^ = lambda / n_corr, the mean information per correspondence (point-to-plane: the three translation values sum to 1;
 *     the rotation values are in m^2).  There is no other form and no threshold on raw eigenvalues.
 *  4. DEGENERATE: rotation direction i iff lambda^_i < min_eigenvalue_rotation, translation direction iff lambda^ < min_eigenvalue_translation,
 *     the comparison as written.  n_corr == 0 (not > 0): all six are degenerate and every lambda^ is +0.0.
 *  5. THE SOLVE.  No direction degenerate: the ordinary solve of the ORIGINAL record, the very tail o3ds_icp_robust_dev runs (the LDL^T with
 *     symmetric pivoting of every step loop here), bit for bit.  Otherwise, with V = blockdiag(V_r, V_t): W = H_c V (H_c symmetric from its upper
 *     triangle), A = V^T W, b = V^T g_c; for every degenerate index i row and column i of A become those of the unit matrix and b_i = +0.0;
 *     y = the same LDL^T solve of (upper triangle of A, b);  x_c = V y;  x = M x_c;  x = x + 0.0.  That x minimises the pass's quadratic among
 *     the updates without motion along the dropped directions.
 *  6. APPLY: T <- (Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5) T, convergence rule and loop exactly those of o3ds_icp_robust_dev.
 * Thresholds: both finite and >= 0; (0, 0) switches the feature off (no lambda^ of a pass with correspondences is < 0 -- unless it is NaN or
 * rounding made a vanishing value negative, which 0 then rightly drops).  No default is offered: DESIGN.md 7.11 quotes the values measured on
 * the test scenes. */
typedef struct {
  double min_eigenvalue_rotation, min_eigenvalue_translation;
} o3ds_degeneracy_params; /* 16 bytes */
typedef struct {
  double record[32];       /* the pass's record */
  double centre[3];        /* c = T c0 */
  double eigenvalues[6];   /* normalised; [0..2] rotation ascending, [3..5] translation ascending */
  double eigenvectors[36]; /* V, row-major, in the re-centred parameters: column i belongs to eigenvalues[i] */
  int32_t degenerate[6];
  int32_t n_degenerate;
  int32_t reserved;
  double x[6]; /* the update this pass would apply */
} o3ds_localizability; /* 696 bytes */
typedef struct {
  double centre[3], eigenvalues[6], eigenvectors[36]; /* of the last pass evaluated, whether or not its update was applied */
  int32_t degenerate[6];
  int32_t n_degenerate;
  int32_t ever_degenerate[6];   /* OR of `degenerate` over the passes whose update was applied */
  int32_t n_passes_constrained; /* how many of those dropped at least one direction */
} o3ds_degeneracy_report; /* 416 bytes */
/* 1. ONE STEP AND ITS ANALYSIS, the testable unit: the record of o3ds_robust_icp_step(source, target, T, ...), steps 1 to 5 on it, and x.
 *    estimator, lambda_geometric and loss are o3ds_robust_icp_step's (the L2 loss gives the plain estimator).  Errors: those of
 *    o3ds_robust_icp_step; O3DS_ERR_INVALID_ARG for a null params or out and for a threshold that is negative, NaN or infinite.  An empty
 *    source or a pass without a pair gives the zero record, hence n_corr == 0: six degenerate directions, V = I, x = 0. */
int o3ds_icp_localizability(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double T[16], double max_correspondence_distance,
                            int estimator, double lambda_geometric, const o3ds_robust_loss* loss, const o3ds_degeneracy_params* params,
                            o3ds_localizability* out);
/* 2. THE REGISTRATION: o3ds_icp_robust_dev with step 5 in the place of its solve.  `report` may be NULL.  Errors: those of
 *    o3ds_icp_robust_dev and of the step above.  An empty source: fitness 0, the initial pose, an all-zero report.  The result and the
 *    report are functions of the arguments alone: two calls give the same bytes. */
int o3ds_icp_degeneracy_aware_dev(o3ds_handle h, o3ds_cloud source, o3ds_cloud target, const double init[16], const o3ds_icp_params* icp_params,
                                  int estimator, double lambda_geometric, const o3ds_robust_loss* loss, const o3ds_degeneracy_params* params,
                                  o3ds_icp_result* out, o3ds_degeneracy_report* report);

/* ---- search-free registration against voxel Gaussians: the normal-distributions transform (Biber and Strasser 2003; Magnusson 2009) in the
 * voxelised form of Koide et al. (VGICP, 2021).  Every registration above pays for an exact nearest-neighbour search per pass; here the
 * target is summarised ONCE as one Gaussian per voxel of a world-anchored grid, and a pass costs per source point a voxel key, a lookup and
 * one or seven 3x3 quadratic forms.  OFFERED like the three sections above and switched on nowhere; there is no Open3D 0.15.1 counterpart,
 * so this text and tests/ndt_restatement.py (the same text in numpy) are the definition.
 * ARITHMETIC: f64 on the stored values widened, every operation rounded on its own (no fused multiply-add).
 * dot3(a, b) = (a0 b0 + a1 b1) + a2 b2.
 *
 * 1. THE VOXEL GAUSSIANS OF A CLOUD: a snapshot -- the cloud may be changed or freed afterwards; a map in its persistent form is folded first.
 *    KEY: inv = 1.0 / voxel_size; k_a = floor(x_a * inv) per axis (the map merge's rounding).  A point with a non-finite coordinate, or with
 *    some |k_a| >= 2^20, belongs to no voxel and is counted in n_skipped_points.
 *    MEMBERS of a voxel: its points in ascending original index, n_v of them.  The voxels are stored and downloaded in ascending packed-key
 *    order: kz major, then ky, then kx.
 *    MEAN: per axis the members' coordinates added one after the other in index order onto +0.0, then divided by n_v.
 *    COVARIANCE: r = p - mean per component; the six sums r_a r_b (a <= b) taken in the same order onto +0.0; C = S / (n_v - 1).  n_v == 1:
 *    C = S (six times +0.0; nothing is divided).
 *    VALID iff n_v >= min_points and, with (lambda, V) the eigen-decomposition of C by step 2 of the degeneracy section (eight cyclic Jacobi
 *    sweeps, ascending order, the sign rule), lambda_2 is finite and lambda_2 > 0.  A voxel with n_v >= min_points that fails on lambda_2
 *    is counted in n_flat (coincident points).  The decomposition of a voxel with fewer members is not taken.
 *    INFORMATION of a valid voxel: f = min_eigenvalue_ratio * lambda_2; l_i = lambda_i < f ? f : lambda_i;
 *    B[a][b] = ((V[a][0] V[b][0]) / l_0 + (V[a][1] V[b][1]) / l_1) + (V[a][2] V[b][2]) / l_2 for a <= b, mirrored.  An invalid voxel downloads
 *    zeros for `information` and valid = 0.
 *    Errors: O3DS_ERR_INVALID_ARG for null params or out, a voxel_size that is not finite or not > 0, min_points < 2, a
 *    min_eigenvalue_ratio outside (0, 1] or NaN, reserved != 0, an unknown id; O3DS_ERR_CAPACITY for 2^31 points or more, a buffer beyond
 *    the pool cap, a download capacity below n_voxels.  An empty cloud, or one whose points are all skipped, gives an object with 0 voxels.
 *    Any output pointer of the download may be NULL: that array is not wanted.  PCL's defaults are min_points 6 and ratio 0.01.
 *    While profiling is enabled the library marks span 18 around the kernels of the build. */
typedef uint64_t o3ds_voxel_gaussians;
typedef struct {
  double voxel_size;
  int32_t min_points;
  int32_t reserved; /* must be 0 */
  double min_eigenvalue_ratio;
} o3ds_voxel_gaussian_params; /* 24 bytes */
typedef struct {
  uint64_t n_voxels, n_valid, n_skipped_points, n_flat;
} o3ds_voxel_gaussians_info; /* 32 bytes */
int o3ds_voxel_gaussians_create(o3ds_handle h, o3ds_cloud cloud, const o3ds_voxel_gaussian_params* params, o3ds_voxel_gaussians* out,
                                o3ds_voxel_gaussians_info* info /* may be NULL */);
int o3ds_voxel_gaussians_free(o3ds_handle h, o3ds_voxel_gaussians g);
int o3ds_voxel_gaussians_info_get(o3ds_handle h, o3ds_voxel_gaussians g, o3ds_voxel_gaussians_info* info, double* voxel_size /* may be NULL */);
int o3ds_voxel_gaussians_download(o3ds_handle h, o3ds_voxel_gaussians g, int32_t* keys /* n x 3 */, uint32_t* counts, double* mean /* n x 3 */,
                                  double* cov /* n x 6 upper, row-major */, double* information /* n x 6 */, uint8_t* valid, size_t capacity);
/* 2. ONE STEP.  QUERY: p_a = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3] in f64, NOT rounded to storage: no search has to agree with
 *    it.  Its key is formed as above; a query the build rule would skip matches nothing.
 *    NEIGHBOURHOOD: the voxels at the offsets (0,0,0), (+1,0,0), (-1,0,0), (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1) of the query's, in this
 *    order; `neighbourhood` = 1 takes the first only, 7 all of them.
 *    PER VALID VOXEL found, with its mean mu and information B: e = p - mu; u_a = (B[a][0] e_0 + B[a][1] e_1) + B[a][2] e_2; m = dot3(e, u);
 *    r = m > 0 ? sqrt(m) : 0; w = Weight(r) of the robust section (the same six losses, the same validation of `loss`).  J is 3x6, the
 *    update being applied on the left as everywhere here: its columns are e_0 x p = (0, -p_z, p_y), (p_z, 0, -p_x), (-p_y, p_x, 0), e_0, e_1,
 *    e_2.  G[a][c] = (B[a][0] J[0][c] + B[a][1] J[1][c]) + B[a][2] J[2][c], zeros included.  The voxel's terms:
 *    h[r][c] = w * ((J[0][r] G[0][c] + J[1][r] G[1][c]) + J[2][r] G[2][c]) for r <= c; g[r] = w * ((J[0][r] u_0 + J[1][r] u_1) + J[2][r] u_2);
 *    m; ee = dot3(e, e).
 *    TERM OF A QUERY: [0..20] and [21..26] the h and g of its voxels added in neighbourhood order onto +0.0; [27] the same sum of m,
 *    unweighted; [28] 1 if at least one valid voxel was found, else the whole term is +0.0; [29] the smallest ee among them, the first of
 *    equals; [30..31] 0.
 *    SUM ORDER over the queries: the coloured section's -- blocks of 256 in index order, the halving tree, the block sums ascending onto +0.0.
 *    The zero record for an empty source, a target without a valid voxel, and no matched query.  With J as above J^T n = cross(p, n): sign
 *    and parameter conventions are the point-to-plane record's, and [0..20] x = -[21..26] is the Gauss-Newton / IRLS step of
 *    sum w e^T B e.  The Gaussian weight of textbook NDT, exp(-d2 m / 2), is deliberately not offered: a device exp is not correctly
 *    rounded, so the record could not be held bit for bit; Cauchy and GM on r = sqrt(m) have the same bell shape.
 *    No result depends on how a voxel is looked up.  Errors: O3DS_ERR_INVALID_ARG for a neighbourhood other than 1 or 7, null pointers,
 *    unknown ids and an invalid loss.  While profiling is enabled the library marks span 19 around the two kernels of the step. */
int o3ds_ndt_step(o3ds_handle h, o3ds_cloud source, o3ds_voxel_gaussians target, const double T[16], int neighbourhood /* 1 or 7 */,
                  const o3ds_robust_loss* loss, double record[32]);
/* 3. THE REGISTRATION: the loop of o3ds_icp_robust_dev around the step above.  fitness = [28] / |source|, inlier_rmse = sqrt([29] / [28]);
 *    the convergence rule, the solve and the update are unchanged (the point-to-plane treatment of an empty set).  params->method and
 *    params->max_correspondence_distance are IGNORED: the neighbourhood is the radius.  Errors: O3DS_ERR_EMPTY for a target with 0 voxels;
 *    O3DS_ERR_INVALID_ARG for a negative max_iteration, null pointers, unknown ids, and the step's.  An empty source gives fitness 0 and the
 *    initial pose.  Two calls, or two handles, give the same bytes. */
int o3ds_icp_ndt_dev(o3ds_handle h, o3ds_cloud source, o3ds_voxel_gaussians target, const double init[16], const o3ds_icp_params* params,
                     int neighbourhood, const o3ds_robust_loss* loss, o3ds_icp_result* out);

#ifdef __cplusplus
}
#endif
#endif /* O3DS_BACKEND_H */
