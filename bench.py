#!/usr/bin/env python
"""bench.py -- BASELINE.json's metric on MI355X: ICP iterations/s (64k scan vs 1M-pt map) + scans/s, in ONE JSON line on rank 0.

M1 (`value`): one STEP = one registerClouds-equivalent (CloudRegistration.cpp:44-48): point-to-plane ICP of a 65 536-pt VLP-16-like
scan against a 1 000 000-pt submap with normals (BASELINE.json configs[1]), FIXED 10 iterations (relative_fitness = relative_rmse =
0 so the convergence test never fires), initial guess identity, truth (0.30,-0.20,0.05) m / rpy (0.5,-0.5,2.0) deg.
Clouds and the target index are resident in HBM before the timed region (index build reported as index_build_ms).  Measured with
f32 point storage (`value`) and with f64 storage (`m1_f64`), each with the roofline of the dominant kernel from hipEvent brackets
around every launch.

M2 (`scans_per_sec`): BASELINE.json configs[2] -- the full per-scan stack, LidarOdometry::addRangeScan + Mapper::addRangeMeasurement
(Mapper.cpp:101-181 -> ScanToMapRegistration.cpp:35-62 -> Submap.cpp:39-75) on a 200-frame OS-128-like stream (131 072 points per
scan, float32 records as a lidar driver delivers them) through the reference-named host classes, the submap growing to ~1 M points;
`cpu_baseline` beside it = the same loop on the CPU oracle for the first frames; `calls` = per-call table (hipEvent spans on the
handle's stream) of algorithmic bytes (SURVEY.md 8d formulas) / time / 8 TB/s.

N GPUs (one process per GPU, torch.distributed.run): rank r holds ITS OWN 1M-pt submap (seed 1235+r) and the whole scan; every ICP
iteration is ONE fused kernel plus one 4-KB RCCL all-reduce of the exact hi/lo sums of the normal equations ("submap" partitioning,
open3d_slam_amd/sharded.py).  Weak scaling: per-GPU work is fixed.  `value` = the units all ranks processed per second, the unit being
BASELINE.json's -- one ICP iteration of the 64k scan against one 1M-point submap -- i.e. N per iteration of the joint registration;
`joint_registration_iterations_per_sec` (= value / N: the registration over N submaps is ONE registration, not N) and
`point_queries_per_sec` (source points searched per second over all ranks) stand beside it.

A plain run (`--steps K --warmup W`) sets up, warms up, times the K steps of M1 with f32 storage and prints the line: nothing else runs.
`--full` adds everything above that takes runs of its own -- the roofline re-runs, the f64 / 8 M-point map / in-library / GeneralizedIcp /
concurrent legs, the copy bandwidth, M2 and its tables, the CPU baselines and, at N > 1, configs 3u and 4.  `--dump-outputs DIR` writes the
result of the last timed step as DIR/<field>.npy (float64).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the CPU baseline's OpenMP threads stay on their cores (read by libgomp when it is first loaded, i.e. before torch is imported);
# without it the best thread count of the sweep was 16 of 256 hardware threads and the rate halved by 64
os.environ.setdefault("OMP_PROC_BIND", "close")
os.environ.setdefault("OMP_PLACES", "cores")

ICP_ITERS = 10
N_SRC, N_MAP = 65536, 1_000_000
MAX_CORR = 1.0
ALGO_BYTES_PER_POINT = 228  # 12 src + 16*12 NN candidates + 12 matched point + 12 matched normal
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8 TB/s spec
TAG_NORMALS, TAG_INSERT, TAG_VOXEL, TAG_ICP, TAG_UPLOAD = 1, 2, 3, 4, 5  # caller span tags; 8 / 9 are the library's own (normals kernels, index build)


# ------------------------------------------------------------------------------------------------ synthetic inputs
def _scan_job(k):
    from open3d_slam_amd import synthetic as syn

    scene = syn.make_scene()
    poses = syn.figure_eight_poses(200, 0.1)
    return syn.os128_scan(scene, poses[k], frame=k).astype(np.float32)


def make_stream(frames):
    """OS-128-like scans of the C3 trajectory, ray-cast on the host cores in parallel; called BEFORE any GPU runtime
    is initialised in this process (fork)."""
    import multiprocessing as mp

    # no more workers than the CPU allowance (cgroup cpu.max): beyond it the pool is throttled, not faster
    q = cpu_quota()
    procs = max(1, min(32, (os.cpu_count() or 2) // 2, int(q) - 2 if q else 32, frames))
    if procs == 1:
        return [_scan_job(k) for k in range(frames)]
    with mp.get_context("fork").Pool(procs) as pool:
        return pool.map(_scan_job, range(frames), chunksize=max(1, frames // (4 * procs)))


def stream_parameters(max_iter=50, shipped=False):
    """shipped: the registration type and the random down-sampling as the shipped Lua has them
    (ros/open3d_slam_ros/param/default/parameter_structure_definitions.lua:62,76,109: GeneralizedIcp, downsampling_ratio 0.3)"""
    from open3d_slam_amd import parameters as P

    mp = P.lua_default_mapper_parameters()
    mp.scanMatcher_.icp_.maxNumIter_ = max_iter
    op = P.OdometryParameters()
    op.scanMatcher_.icp_ = P.IcpParameters(maxNumIter_=max_iter, maxCorrespondenceDistance_=1.0, knn_=20, maxDistanceKnn_=3.0)
    op.scanProcessing_.voxelSize_ = 0.1
    op.scanProcessing_.cropper_ = P.ScanCroppingParameters(croppingMinRadius_=2.0, croppingMaxRadius_=30.0, cropperName_="MinMaxRadius")
    if shipped:
        mp.scanMatcher_.scanToMapRegType_ = P.ScanToMapRegistrationType.GeneralizedIcp
        op.scanMatcher_.regType_ = P.CloudRegistrationType.GeneralizedIcp
        mp.scanProcessing_.downSamplingRatio_ = 0.3
        op.scanProcessing_.downSamplingRatio_ = 0.3
    return mp, op


# ------------------------------------------------------------------------------------------------ CPU baselines (oracle = checker)
def cpu_quota():
    """CPUs this container may use at once (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited: the GPU boxes expose all 256
    hardware threads of the host but allow 16 CPUs' worth of time, which is why the OpenMP sweep peaks at 16 threads there"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def host_cpu():
    """logical CPU the calling thread runs on right now (-1 when the C library has no sched_getcpu)"""
    try:
        import ctypes

        return int(ctypes.CDLL(None).sched_getcpu())
    except Exception:
        return -1


def cpu_baseline_m1(src, tgt, nrm, budget_s=16.0):
    """CPU restatement of Open3D v0.15.1 (the oracle, 'port'), timed on this box's host cores.  The thread count is the
    best of a short sweep: on the 2x64-core EPYC host of the MI355X boxes the OpenMP loops peak at 16-32 threads
    and collapse beyond the physical cores, so 'all cores' would flatter the GPU."""
    from oracle import pyoracle as po

    ncpu = os.cpu_count() or 1
    t0 = time.perf_counter()
    tree = po.KDTree(tgt)
    build_s = time.perf_counter() - t0

    def one():
        return po.icp_point_to_plane(src, tgt, nrm, MAX_CORR, max_iter=ICP_ITERS, rel_fitness=0.0, rel_rmse=0.0, tree=tree)

    def sustained(seconds):
        reps, spent, res = 0, 0.0, None
        while reps < 2 or spent < seconds:
            t0 = time.perf_counter()
            res = one()
            spent += time.perf_counter() - t0
            reps += 1
            if reps >= 5000:
                break
        return reps, spent, res

    quota = cpu_quota()
    limit = min(ncpu, int(2 * quota)) if quota else ncpu  # threads far beyond the container's CPU allowance are throttled, not faster
    cands = [t for t in (8, 16, 32, 64, 128) if t <= limit] or [min(ncpu, 8)]
    sweep, best_t, best_rate = {}, cands[0], 0.0
    for th in cands:
        po.lib().orc_set_num_threads(th)
        one()  # warm the thread pool
        r, sp, _ = sustained(budget_s / (2.0 * len(cands)))
        sweep[th] = round(ICP_ITERS * r / sp, 1)
        if sweep[th] > best_rate:
            best_t, best_rate = th, sweep[th]
    po.lib().orc_set_num_threads(best_t)
    one()
    reps, spent, res = sustained(budget_s / 2.0)
    per_reg = spent / reps
    return dict(value=ICP_ITERS / per_reg, unit="icp_iterations/s", cores=best_t, kind="port", cpu_quota=quota,
                sample=f"{reps} x (64k scan vs 1M map, {ICP_ITERS} iters, KD-tree prebuilt) = {spent:.1f}s at the best thread count of the sweep "
                       f"{sweep} it/s (host has {ncpu} hardware threads, this container's CPU allowance (cgroup cpu.max) is "
                       f"{quota if quota else 'unlimited'}); KD-tree build {build_s*1e3:.0f} ms -> "
                       f"{ICP_ITERS/(per_reg+build_s):.2f} it/s when rebuilt per call as the reference does; "
                       f"CPU restatement of Open3D v0.15.1, {best_t} OpenMP threads"), res, best_t


def cpu_baseline_m2_reference_loop(scans32, frames, threads):
    """The CPU leg of the scans/s metric on the REFERENCE'S OWN frame loop: open3d_slam's Odometry.cpp / Mapper.cpp / ScanToMapRegistration.cpp /
    Submap.cpp / SubmapCollection.cpp compiled unchanged (oracle/ref_build -> oracle/_ref/libo3dslam_ref.so), the Open3D algorithms they call
    served by the oracle's C restatement.  Returns None when that library is neither built nor buildable (then the Python loop is used)."""
    from oracle import pyoracle as po
    from oracle import ref

    try:
        if not ref.available():
            return None
        mp, op = stream_parameters()
        po.lib().orc_set_num_threads(threads)  # the same shared library the reference build is linked to
        R = ref.ReferenceSlam(mp, op, carve_every_n_scans=mp.mapBuilder_.carving_.carveSpaceEveryNscans_, patched=False)
        ok, M, O, ms, n_map = R.run_stream(scans32[:frames])
        workers = dict(R.ms_workers)
        R.close()
    except Exception as e:  # noqa: BLE001 -- a reported baseline must not take the line down
        sys.stderr.write(f"reference-loop CPU leg unavailable ({e!r}); falling back to the Python loop\n")
        return None
    if ok != frames:
        return None
    m = frames - 1
    busy = (workers["odometry"] + workers["mapping"]) * 1e-3

    class Loop:  # what the caller reads of a loop object
        poses_per_frame = [(M[k], None) for k in range(frames)]

    return dict(value=m / busy, unit="scans/s", cores=int(po.lib().orc_num_threads()), kind="port",
                glue="reference: open3d_slam's own Odometry / Mapper / Submap sources compiled unchanged (oracle/_ref); only the Open3D algorithms are the port",
                mapping_only_scans_per_sec=m / (workers["mapping"] * 1e-3), ms_per_scan={k: v / m for k, v in workers.items()}, map_points=int(n_map),
                sample=f"frames 1..{frames - 1} of the same {len(scans32)}-frame stream through open3d_slam's OWN LidarOdometry::addRangeScan + "
                       f"Mapper::addRangeMeasurement (reference sources compiled unchanged, oracle/ref_build; the map holds {n_map} points at the end), "
                       "the Open3D algorithms underneath = CPU restatement of Open3D v0.15.1 (the port), KD-tree of the map patch rebuilt per "
                       "registration as the reference does, carving every 10th insertion"), Loop


def cpu_baseline_m2(scans32, frames, threads):
    """The same odometry + mapping loop on the CPU: the reference's own compiled frame loop when oracle/_ref is there, else the oracle's Python
    loop (oracle/pipeline.py; the two agree to 1e-10, tests/test_oracle_vs_reference.py); first `frames` frames of the stream."""
    from oracle import pyoracle as po
    from oracle.pipeline import OracleLoop

    got = cpu_baseline_m2_reference_loop(scans32, frames, threads)
    if got is not None:
        return got
    mp, op = stream_parameters()
    po.lib().orc_set_num_threads(threads)
    ref = OracleLoop(po, mp, op)
    cpu = {"odometry": 0.0, "mapping": 0.0}
    ref.poses_per_frame = []
    for k in range(frames):
        raw = scans32[k].astype(np.float64)
        t0 = time.perf_counter()
        ref.odometry(raw, 0.1 * k)
        t1 = time.perf_counter()
        ref.mapping(raw, 0.1 * k)
        t2 = time.perf_counter()
        ref.poses_per_frame.append((ref.T.copy(), len(ref.map_p)))
        if k > 0:
            cpu["odometry"] += t1 - t0
            cpu["mapping"] += t2 - t1
    m = frames - 1
    return dict(value=m / (cpu["odometry"] + cpu["mapping"]), unit="scans/s", cores=int(po.lib().orc_num_threads()), kind="port",
                mapping_only_scans_per_sec=m / cpu["mapping"], ms_per_scan={k: 1e3 * v / m for k, v in cpu.items()},
                map_points=int(len(ref.map_p)),
                sample=f"frames 1..{frames - 1} of the same {len(scans32)}-frame stream (the map holds {len(ref.map_p)} points at the end"
                       + ("" if frames == len(scans32) else "; the GPU leg runs all frames, its map grows further and its later frames cost more")
                       + "), CPU restatement of Open3D v0.15.1, KD-tree of the map patch rebuilt per registration as the reference does"), ref


# ------------------------------------------------------------------------------------------------ M2: the config-2 stream
def _wrap_spans(backend):
    """hipEvent spans around the ABI calls a frame is made of, with the sizes the byte formulas need (restored by the caller)."""
    B = backend.Backend
    saved, sizes = {}, {"normals": [], "insert": [], "voxel": [], "icp": [], "upload": []}

    def wrap(name, tag, note, spacer=None):
        fn = getattr(B, name)
        saved[name] = fn

        def w(self, *a, **k):
            pre = note(self, a, None)
            if spacer is not None:
                spacer(self, a)
            with self.span(tag):
                r = fn(self, *a, **k)
            note(self, a, (pre, r))
            return r

        setattr(B, name, w)

    def n_of(be, cid):
        return be.size(cid)[0]

    def note_normals(be, a, done):
        if done is not None:
            sizes["normals"].append((n_of(be, a[0]), a[2]))

    def note_insert(be, a, done):
        if done is None:
            return (n_of(be, a[0]), n_of(be, a[1]))
        sizes["insert"].append(done[0] + (n_of(be, a[0]),))

    def note_voxel(be, a, done):
        if done is None:
            return n_of(be, a[0])
        sizes["voxel"].append((done[0], n_of(be, done[1])))

    def note_icp(be, a, done):
        if done is not None:
            sizes["icp"].append((n_of(be, a[0]), done[1]["iterations"]))

    def note_upload(be, a, done):
        if done is not None:
            sizes["upload"].append(n_of(be, done[1]))

    wrap("estimate_normals", TAG_NORMALS, note_normals)
    # (asking for the sizes above drains the stream: without something for the device to do while the call queues its eight launches the span
    # would be the host's time, not the kernels' -- a normal estimation of the scan being inserted: same scan, same normals, ~100 us of work)
    wrap("map_insert_scan", TAG_INSERT, note_insert, spacer=lambda be, a: saved["estimate_normals"](be, a[1], 3.0, 20))
    wrap("crop_voxel_down_sample", TAG_VOXEL, note_voxel)
    wrap("icp_point_to_plane_dev", TAG_ICP, note_icp)
    wrap("upload_f32", TAG_UPLOAD, note_upload)
    return saved, sizes


def stage_scans(be, scans32, pinned=True):
    """the raw scans as sensor_msgs/PointCloud2-style records (16-byte float32 x y z + padding), in page-locked message buffers of the
    handle (Backend.pinned_records: what a driver or a ROS 2 allocator would hand the sensor data over in) or in ordinary numpy arrays"""
    out = []
    for s in scans32:
        n = len(s)
        rec = be.pinned_records(n, 16).view(np.float32).reshape(n, 4) if pinned else np.zeros((n, 4), dtype=np.float32)
        rec[:, :3] = s
        rec[:, 3] = 0.0
        out.append(rec)
    return out


def run_stream(be, scans32, profile=False, stage_sync=True, pinned=True, prefetch=True, shipped=False, ahead=True):
    """frames through the reference-named host classes; returns rates, per-stage wall times and (profile) the per-call table.
    ahead (with prefetch, not while profiling): the odometry's pre-processing of scan k + 1 is queued behind the launches of frame k's
    scan-to-scan registration, before the host waits for its result (o3ds_icp_overlap_next) -- the device works through it while the host
    waits, composes poses and sets the scan-to-map registration up; open3d_slam's odometry worker runs ahead of the mapper the same way, on
    its own thread (SlamWrapper.cpp:228-229).  The drains of a staged run (stage_sync) wait for it too: it shows in the free-running rate.
    Same kernels on the same inputs, only earlier: the poses are those of the loop without it, bit for bit (checked in main).
    pinned / prefetch: the scans wait in page-locked buffers and scan k + 1 is handed to the backend (o3ds_cloud_upload_f32: asynchronous, on
    the handle's copy stream) while frame k is being processed -- what the ROS callback thread does in open3d_slam; without
    them the scan is copied from pageable memory and ingested at the start of its own frame, as rounds 1-4 measured it.
    stage_sync: drain the stream after the odometry and after the mapping of every frame, so that the per-stage times are exact; without
    it the loop runs as a consumer would run it (the registrations hand their result back, nothing else waits) and only the total counts"""
    from open3d_slam_amd import backend, synthetic as syn
    from open3d_slam_amd.mapper import Mapper
    from open3d_slam_amd.odometry import LidarOdometry
    from open3d_slam_amd.pointcloud import PointCloud

    mp, op = stream_parameters(shipped=shipped)
    odo = LidarOdometry(be)
    odo.setParameters(op)
    mapper = Mapper(be, odo)
    mapper.setParameters(mp)
    if shipped:  # [O3D] RandomDownSample draws from std::random_device: the kept-index lists are pinned by seeds here
        odo.setDownSampleSeed(1001)
        mapper.scan2MapReg_.setDownSampleSeed(1002)
    saved, sizes = ({}, None)
    if profile:
        saved, sizes = _wrap_spans(backend)
        be.profile_enable(True)
    stage = {"upload": 0.0, "odometry": 0.0, "mapping": 0.0}
    frames = len(scans32)
    per_frame = []
    import gc

    records = stage_scans(be, scans32, pinned)
    ingest_s = []
    gc.collect()
    try:
        nxt = None
        for k, raw in enumerate(records):
            t0 = time.perf_counter()
            if prefetch:
                cloud = nxt if nxt is not None else PointCloud.from_pointcloud2(be, raw)
                nxt = PointCloud.from_pointcloud2(be, records[k + 1]) if k + 1 < frames else None
            else:
                cloud = PointCloud.from_pointcloud2(be, raw)
            if profile:  # how long an ingest takes from call to "on the device, unpacked, box reduced" (not on the frame's critical path)
                tw = time.perf_counter()
                be.wait_ingest((nxt or cloud).id)
                ingest_s.append(time.perf_counter() - tw + (tw - t0))
            t1 = time.perf_counter()
            if ahead and prefetch and not profile and nxt is not None:
                be.overlap_next = (lambda c=nxt: odo.preprocessAhead(c))
            ok1 = odo.addRangeScan(cloud, 0.1 * k)
            if be.overlap_next is not None:  # no registration took it (the first scan): nothing to overlap with
                be.overlap_next = None
            if stage_sync:
                be.synchronize()
            t2 = time.perf_counter()
            ok2 = mapper.addRangeMeasurement(cloud, 0.1 * k)
            if stage_sync:
                be.synchronize()
            t3 = time.perf_counter()
            if k == 0:
                be.synchronize()
                t_first = time.perf_counter()
            cloud.release()
            assert ok1 and ok2, (k, ok1, ok2)
            per_frame.append(mapper.getMapToRangeSensor().copy())
            if k > 0:  # frame 0 only initialises
                stage["upload"] += t1 - t0
                stage["odometry"] += t2 - t1
                stage["mapping"] += t3 - t2
    finally:
        for name, fn in saved.items():
            setattr(backend.Backend, name, fn)
    be.synchronize()
    t_end = time.perf_counter()
    n = frames - 1
    poses = syn.figure_eight_poses(200, 0.1)
    dt, dr = syn.se3_error(mapper.getMapToRangeSensor(), np.linalg.inv(poses[0]) @ poses[frames - 1])
    out = {"scans_per_sec": n / (stage["odometry"] + stage["mapping"] + stage["upload"]) if stage_sync else n / (t_end - t_first),
           "mapping_only_scans_per_sec": n / stage["mapping"], "ms_per_scan": {k: 1e3 * v / n for k, v in stage.items()},
           "frames": frames, "map_points": len(mapper.getActiveSubmap().getMapPointCloud()),
           "final_pose_error_vs_truth": {"dt_m": dt, "dr_rad": dr}, "pose": mapper.getMapToRangeSensor().copy(), "poses_per_frame": per_frame}
    if profile:
        def row(tag, nbytes, what):
            cnt, ms = be.span_read(tag)
            if cnt == 0:
                return None
            gbs = nbytes / (ms * 1e-3) / 1e9
            return {"calls": cnt, "avg_us": 1e3 * ms / cnt, "algorithmic_bytes_per_call": nbytes / cnt, "achieved_gbs": gbs,
                    "frac_of_hbm_peak": gbs / HBM_PEAK_GBS, "bytes": what}

        knn = 20
        n_nrm = sum(m for m, _ in sizes["normals"])
        calls = {
            "estimate_normals (index build + search kernel + eigen kernel)": row(TAG_NORMALS, n_nrm * (12 + knn * 12 + 12), "m x (12 + knn x 12) read + m x 12 written"),
            "normals kernels alone": row(8, n_nrm * (12 + knn * 12 + 12), "same bytes, the two kernels only"),
            "map_insert_scan (transform + append + voxelizeWithinCroppingVolume + index rebuild)": row(
                TAG_INSERT, sum(m * 36 + m * 72 + 2 * max(N2 - N, 0) * 24 for N, m, N2 in sizes["insert"]),
                "persistent submap (DESIGN.md 4.7): m x (12 read + 24 placed) + g x (16 hash entry + 32 slot record + 24 point and normal), g <= m voxels "
                "of the scan taken as m, + the index rows that open: 2 x new slots x 24; independent of the map's size N"),
            "crop + VoxelDownSample": row(TAG_VOXEL, sum(nr * (12 + 16) + m * 12 for nr, m in sizes["voxel"]), "n_raw x 12 read + keys n_raw x 16 + m x 12 written"),
            "registerClouds (device clouds, index kept by the submap)": row(TAG_ICP, sum(n_ * ALGO_BYTES_PER_POINT * (it + 1) for n_, it in sizes["icp"]),
                                                                             "n x 228 per correspondence pass, iterations + 1 passes"),
            "PointCloud2 float32 ingest (copy stream, beside the previous frame)": {
                "calls": len(ingest_s), "avg_us": 1e6 * float(np.mean(ingest_s)) if ingest_s else 0.0,
                "what": "host wall time from o3ds_cloud_upload_f32 to the scan being on the device, unpacked and its box reduced; it runs on the "
                        "handle's copy stream while the frame before it is registered and merged"},
            "index build kernels (every build of the stream)": row(9, 0, "see map_insert_scan / estimate_normals"),
        }
        icp_launches, icp_ms = be.profile_read()
        if icp_launches:
            calls["icp_fused_kernel launches of the stream"] = {"calls": icp_launches, "avg_us": 1e3 * icp_ms / icp_launches}
        be.profile_enable(False)
        out["calls"] = {k: v for k, v in calls.items() if v}
    return out


def run_stream_pipelined(device, scans32, depth=4, share=False, drain=True, shipped=False):
    """the same frames with odometry and mapping on two host threads, as the reference runs them (SlamWrapper.cpp:228-229 odometryWorker /
    mappingWorker, a bounded buffer between them): LidarOdometry on one backend handle (its own stream), Mapper on another, each ingesting
    the raw scan into its own handle (handles do not share clouds).  The mapper only reads the odometry pose of a frame that is already
    through, so the poses are those of the serial loop, bit for bit (checked by the caller).
    share: the mapper's handle takes the raw scan and its pre-processed version from VIEWS the odometry worker exports (o3ds_cloud_export_view /
    _import_view: device-to-device copies behind an event, nothing of the other handle is touched) instead of ingesting and pre-processing the
    scan a second time -- what integration/o3ds_open3d_slam.hpp does between the reference's two workers.
    drain=False: no stream drain at the end of a worker's frame (the registrations hand their results back, nothing else waits)."""
    import queue
    import threading

    from open3d_slam_amd import backend, synthetic as syn
    from open3d_slam_amd.mapper import Mapper
    from open3d_slam_amd.odometry import LidarOdometry
    from open3d_slam_amd.pointcloud import PointCloud

    mp, op = stream_parameters(shipped=shipped)
    be_o, be_m = backend.Backend(device), backend.Backend(device)
    odo = LidarOdometry(be_o)
    odo.setParameters(op)
    mapper = Mapper(be_m, odo)
    mapper.setParameters(mp)
    if shipped:  # (the seeds of run_stream's shipped leg: the same draws, the same poses)
        odo.setDownSampleSeed(1001)
        mapper.scan2MapReg_.setDownSampleSeed(1002)
    q = queue.Queue(maxsize=depth)
    err = []

    done = queue.Queue()  # share: (cloud on the odometry handle, its views) the mapper has finished copying from

    def drain_done(block=False):
        while True:
            try:
                cloud, views = done.get(block) if block else done.get_nowait()
            except queue.Empty:
                return
            for v in views:
                be_o.release_view(v)
            cloud.release()
            block = False

    # (share: the odometry worker takes its scans as run_stream does -- page-locked records, the next scan ingested and pre-processed
    # behind the registration of this one, o3ds_icp_overlap_next)
    records = stage_scans(be_o, scans32, True) if share else scans32

    def odometry_worker():
        try:
            nxt = None
            for k, raw in enumerate(records):
                if share:
                    cloud = nxt if nxt is not None else PointCloud.from_pointcloud2(be_o, raw)
                    nxt = PointCloud.from_pointcloud2(be_o, records[k + 1]) if k + 1 < len(records) else None
                    if nxt is not None:
                        be_o.overlap_next = (lambda c=nxt: odo.preprocessAhead(c))
                else:
                    cloud = PointCloud.from_pointcloud2(be_o, raw)
                ok = odo.addRangeScan(cloud, 0.1 * k)
                if be_o.overlap_next is not None:  # no registration took it (the first scan)
                    be_o.overlap_next = None
                if drain:
                    be_o.synchronize()
                assert ok, k
                if share:  # views of the raw scan and of what the pre-processing made of it; the clouds live until the mapper has copied
                    memo = dict(cloud._pre_memo or {})
                    views = {key: be_o.export_view(v.id) for key, v in memo.items()}
                    raw_view = be_o.export_view(cloud.id)
                    q.put((k, raw_view, views, cloud))
                    drain_done()
                else:
                    cloud.release()
                    q.put(k)
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            err.append(e)
            q.put(-1)

    th = threading.Thread(target=odometry_worker, daemon=True)
    t_start = None
    per_frame = []
    th.start()
    frames = len(scans32)
    for _ in range(frames):
        item = q.get()
        if item == -1:
            raise err[0]
        if share:
            k, raw_view, views, theirs = item
            cloud = PointCloud(be_m, be_m.import_view(raw_view))
            cloud._pre_memo = {key: PointCloud(be_m, be_m.import_view(v)) for key, v in views.items()}
        else:
            k = item
            cloud = PointCloud.from_pointcloud2(be_m, scans32[k])
        ok = mapper.addRangeMeasurement(cloud, 0.1 * k)
        if drain:
            be_m.synchronize()
        cloud.release()
        if share:  # (the copies are done -- they were queued in front of a registration whose result is here: the odometry worker may free what they were made from)
            done.put((theirs, [raw_view] + list(views.values())))
        assert ok, k
        per_frame.append(mapper.getMapToRangeSensor().copy())
        if k == 0:  # frame 0 only initialises (as in run_stream)
            t_start = time.perf_counter()
    be_m.synchronize()
    elapsed = time.perf_counter() - t_start
    th.join()
    drain_done()
    out = {"scans_per_sec": (frames - 1) / elapsed, "pose": mapper.getMapToRangeSensor().copy(), "poses_per_frame": per_frame,
           "odometry_poses_per_frame": [T.copy() for _, T in odo.odomToRangeSensorBuffer_],
           "map_points": len(mapper.getActiveSubmap().getMapPointCloud())}
    be_o.close()
    be_m.close()
    return out


def run_m1_gicp(device, src, tgt, nrm, steps, warmup, with_oracle=True):
    """configs[1] under the registration the shipped Lua selects: RegistrationIcpGeneralized (CloudRegistration.cpp:16-39), fixed 10
    iterations, device clouds, index prebuilt; the source's normals estimated on the device as estimateNormalsOrCovariancesIfNeeded does.
    Algorithmic bytes per source point and pass: the point-to-plane figure + the source normal (12 B)."""
    from open3d_slam_amd import backend, synthetic as syn

    be = backend.Backend(device)
    s_id = be.upload(src)
    be.estimate_normals(s_id, 3.0, 20)
    src_n = be.download(s_id)[1]
    t_id = be.upload(tgt, nrm)
    be.build_index(t_id, MAX_CORR, 0.0)
    kw = dict(max_iter=ICP_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    for _ in range(warmup):
        res = be.icp_generalized_dev(s_id, t_id, MAX_CORR, **kw)
    be.synchronize()
    be.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        res = be.icp_generalized_dev(s_id, t_id, MAX_CORR, **kw)
    be.synchronize()
    elapsed = time.perf_counter() - t0
    n_launch, kern_ms = be.profile_read()
    be.profile_enable(False)
    be.close()
    bytes_per_launch = N_SRC * (ALGO_BYTES_PER_POINT + 12)
    avg = kern_ms * 1e-3 / max(n_launch, 1)
    out = {"value": ICP_ITERS * steps / elapsed, "unit": "icp_iterations/s", "steps": steps, "ms_per_step": elapsed / steps * 1e3, "dtype": "f32 points, f64 accumulate",
           "workload": "configs[1] under GeneralizedIcp (the shipped scan_to_map_refinement_type): 65536-pt scan with device-estimated normals vs 1,000,000-pt submap",
           "roofline": {"bound": "hbm", "achieved": bytes_per_launch / avg / 1e9 if avg else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": bytes_per_launch / avg / 1e9 / HBM_PEAK_GBS if avg else None, "traffic": None,
                        "kernel": "icp_fused_kernel<P4f, ..., kGicp>", "launches": n_launch, "avg_launch_us_event_brackets": avg * 1e6,
                        "algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_bytes_per_point": ALGO_BYTES_PER_POINT + 12},
           "result": {"fitness": res["fitness"], "inlier_rmse": res["inlier_rmse"], "iterations": res["iterations"]}}
    if with_oracle:  # the checker beside it, same inputs, same fixed iterations
        from oracle import pyoracle as po

        ref = po.icp_generalized(src, src_n, tgt, nrm, MAX_CORR, **kw)
        dt, dr = syn.se3_error(res["transformation"], ref["transformation"])
        out["parity_vs_oracle"] = {"dt_m": dt, "dr_rad": dr, "fitness_gpu": res["fitness"], "fitness_oracle": ref["fitness"],
                                   "what": "oracle/o3d_oracle.c orc_icp_generalized on the same clouds and normals (restated from Open3D v0.15.1, unpinned)"}
    return out


def run_insert_sweep(device, scans32, marks=(100_000, 300_000, 1_000_000)):
    """Submap::insertScan (o3ds_map_insert_scan) as the map grows: the stream's pre-processed scans inserted at their true poses, one after
    the other, into one map -- the way the mapper fills a submap, without the registrations --, every insertion under a hipEvent span; the
    rows are the insertions whose map size lies within 20 % of a mark.  (A map seeded with random surface samples is not a submap: its
    points outside the volume were never merged, tens of thousands of voxels hold several of them, and the insertion walks that list.)"""
    from open3d_slam_amd import backend, synthetic as syn

    poses = syn.figure_eight_poses(200, 0.1)
    be = backend.Backend(device)
    m = be.upload(np.zeros((0, 3)))
    crop_scan = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=2.0, rmax=30.0)
    be.profile_enable(True)
    rec = []
    for k in range(len(scans32)):
        raw = be.upload_f32(np.ascontiguousarray(np.hstack([scans32[k], np.zeros((len(scans32[k]), 1), np.float32)])))
        v = be.crop_voxel_down_sample(raw, crop_scan, 0.1)
        be.estimate_normals(v, 3.0, 20)
        be.free(raw)
        n_scan = be.size(v)[0]  # (its size has arrived, as it has in the stream by the time a scan is inserted: two registrations lie in between)
        T = np.linalg.inv(poses[0]) @ poses[k]
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=2.0, rmax=30.0)
        n_before = be.size(m)[0]
        # the device is busy while the call queues its launches -- a normal estimation of the same scan, same result -- so that the span is
        # the kernels' time and not the host's (in the stream the host runs ahead of the device)
        be.estimate_normals(v, 3.0, 20)
        with be.span(0):
            be.map_insert_scan(m, v, T, 0.1, crop, max_corr_hint=1.0)
        cnt, ms = be.span_read(0)
        rec.append((n_before, 1e3 * ms, n_scan))
        be.free(v)
    be.profile_enable(False)
    be.close()
    rows = []
    for mark in marks:
        sel = [r for r in rec[2:] if 0.8 * mark <= r[0] <= 1.2 * mark]  # (the first two insertions found the map and bring it into its persistent form)
        if sel:
            rows.append({"map_points_mark": int(mark), "map_points": [int(sel[0][0]), int(sel[-1][0])], "insertions": len(sel),
                         "avg_us": float(np.mean([r[1] for r in sel])), "median_us": float(np.median([r[1] for r in sel])),
                         "max_us": float(np.max([r[1] for r in sel])),
                         "scan_points": int(np.mean([r[2] for r in sel]))})
    return rows



# ------------------------------------------------------------------------------------------------ the line the driver parses
LINE_LIMIT = 8192  # bytes: round 5's 21 KB line could not be parsed by the driver (BENCH_r05.json parsed = null)


def _num(v, digits=6):
    """numbers only, strict JSON: floats to `digits` significant digits, NaN / inf -> null, numpy scalars -> Python"""
    if isinstance(v, (bool, type(None), str)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")):
            return None
        return float(f"{v:.{digits}g}")
    return v


def _pick(d, *keys):
    """the named numeric leaves of a (possibly missing) dict; a key 'a.b' reaches into d['a']['b'] and is stored as 'a_b'"""
    out = {}
    for k in keys:
        cur = d
        for part in k.split("."):
            cur = cur.get(part) if isinstance(cur, dict) else None
        if cur is not None and not isinstance(cur, (dict, list)):
            out[k.replace(".", "_")] = _num(cur)
    return out


def compact_line(out, detail_path=None):
    """The ONE line rank 0 prints: the contract's keys, `roofline` and `cpu_baseline`, and the other legs as bare numbers -- everything else
    (`calls`, per-kernel traffic, the prose that says what each leg is) lives in the detail file.  <= LINE_LIMIT bytes of strict JSON."""
    roof_keys = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "launches", "avg_launch_us", "algorithmic_bytes_per_launch",
                 "bracket_avg_launch_us", "measured_copy_gbs")
    line = {k: _num(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                          "vs_baseline", "dtype", "data")}
    cfg = out.get("config", {})
    line["config"] = {k: _num(cfg[k]) if not isinstance(cfg[k], str) else cfg[k][:260] for k in ("workload", "n_src", "n_map_per_gpu", "icp_iterations_per_step", "parallelism", "nn_cell_m") if k in cfg}
    line["roofline"] = {k: _num(out.get("roofline", {}).get(k)) for k in roof_keys if k in out.get("roofline", {})}
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {**_pick(cb, "value", "unit", "cores", "kind"), "sample": str(cb.get("sample", ""))[:160]}
    if "parity_vs_cpu" in out:
        line["parity_vs_cpu"] = _pick(out["parity_vs_cpu"], "dt_m", "dr_rad", "fitness_gpu", "fitness_cpu")
    if "speedup_vs_cpu_baseline" in out:
        line["speedup_vs_cpu_baseline"] = _num(out["speedup_vs_cpu_baseline"])
    line.update(_pick(out, "index_build_ms", "joint_registration_iterations_per_sec", "point_queries_per_sec"))
    line["pose_error_vs_truth"] = _pick(out.get("pose_error_vs_truth", {}), "dt_m", "dr_rad", "fitness", "inlier_rmse")
    for leg in ("m1_f64", "m1_large_map", "m1_gicp", "m1_in_library_sharded_one_rank"):
        if isinstance(out.get(leg), dict):
            line[leg] = _pick(out[leg], "value", "ms_per_step", "roofline.frac", "roofline.avg_launch_us", "roofline.traffic", "n_map", "error")
            if "error" in out[leg]:
                line[leg]["error"] = str(out[leg]["error"])[:120]
    if isinstance(out.get("concurrent"), dict):
        line["concurrent"] = _pick(out["concurrent"], "streams", "value")
    m2 = out.get("scans_per_sec")
    if isinstance(m2, dict):
        line["scans_per_sec"] = {
            **({"error": str(m2["error"])[:120]} if "error" in m2 else {}),
            **_pick(m2, "scans_per_sec", "mapping_only_scans_per_sec", "frames", "map_points", "final_pose_error_vs_truth.dt_m", "final_pose_error_vs_truth.dr_rad",
                    "pose_repeats_bitwise_between_the_two_runs", "speedup_vs_cpu_baseline"),
            "free_running": _num((m2.get("free_running") or {}).get("scans_per_sec")),
            "host_seam": _num((m2.get("host_seam") or {}).get("scans_per_sec")),
            "host_seam_two_threads": _num((m2.get("host_seam") or {}).get("two_threads_scans_per_sec")),
            "patched_reference": _num(((m2.get("patched_reference") or {}).get("serial") or {}).get("scans_per_sec")),
            "patched_reference_two_threads": _num(((m2.get("patched_reference") or {}).get("two_threads") or {}).get("scans_per_sec")),
            "shipped_configuration": _num((m2.get("shipped_configuration") or {}).get("scans_per_sec")),
            "pipelined": _num((m2.get("pipelined") or {}).get("scans_per_sec")),
            "two_workers": _num((m2.get("two_workers") or {}).get("scans_per_sec")),
            "shipped_configuration_two_workers": _num((m2.get("shipped_configuration") or {}).get("two_workers_scans_per_sec")),
            "pageable_ingest": _num((m2.get("pageable_ingest_at_frame_start") or {}).get("scans_per_sec")),
            "cpu_baseline": _pick(m2.get("cpu_baseline") or {}, "value", "unit", "cores", "kind"),
            "parity_vs_cpu": _pick(m2.get("parity_vs_cpu") or {}, "frames_compared", "worst_dt_m", "worst_dr_rad", "within_stated_tolerance"),
        }
        calls = m2.get("calls") or {}
        short = {"estimate_normals": "estimate_normals (", "normals_kernels": "normals kernels alone", "map_insert_scan": "map_insert_scan (", "crop_voxel_down_sample": "crop + VoxelDownSample",
                 "register_clouds": "registerClouds"}
        line["scans_per_sec"]["call_us"] = {a: _num(v.get("avg_us"), 4) for a, b in short.items() for k, v in calls.items() if k.startswith(b) and isinstance(v, dict)}
    also = out.get("also")
    if isinstance(also, dict):
        line["also"] = {k: (_pick(v, "metric", "value", "unit", "ms_per_step", "error") if isinstance(v, dict) else None) for k, v in also.items()}
    if detail_path:
        line["detail"] = detail_path
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(text) > LINE_LIMIT:  # never print an unparseable line: fall back to the contract's keys alone
        for k in ("scans_per_sec", "also", "concurrent", "m1_f64", "m1_large_map", "m1_gicp", "pose_error_vs_truth"):
            line.pop(k, None)
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    assert len(text) <= LINE_LIMIT, len(text)
    return text


_LINE_FD = None  # the process's real stdout, set aside by claim_stdout()


def claim_stdout():
    """Nothing but the ONE line may reach stdout: libraries write there on their own (RCCL prints a version banner from ncclCommInitRank
    through C stdio, which a redirected stdout only flushes at exit -- BEHIND the line; round 6's first evidence run had five such lines
    after the JSON).  File descriptor 1 is pointed at stderr for the rest of the run -- Python's prints, C stdio, child processes -- and
    the line is written to the descriptor set aside here."""
    global _LINE_FD
    if _LINE_FD is None:
        sys.stdout.flush()
        _LINE_FD = os.dup(1)
        os.dup2(2, 1)


def emit(out):
    """detail -> gpurun_out/bench_detail.json (O3DS_BENCH_DETAIL overrides the path), the compact line -> stdout, last"""
    path = os.environ.get("O3DS_BENCH_DETAIL", os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    rel = None
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, default=lambda o: o.tolist() if hasattr(o, "tolist") else repr(o))
        rel = os.path.relpath(path, ROOT)
    except OSError as e:
        sys.stderr.write(f"bench detail not written: {e!r}\n")
    line = compact_line(out, rel)
    sys.stdout.flush()
    try:
        import ctypes

        ctypes.CDLL(None).fflush(None)  # whatever C stdio still holds goes where fd 1 points now (stderr), not behind the line
    except Exception:
        pass
    if _LINE_FD is not None:
        os.write(_LINE_FD, (line + "\n").encode())
    else:
        print(line, flush=True)


def dump_outputs(out_dir, res):
    """--dump-outputs: the registration result the last timed step returned, one float64 array per numeric field (transformation,
    fitness, inlier_rmse, iterations, ...), so that two builds run on the same seeded inputs can be compared output for output"""
    os.makedirs(out_dir, exist_ok=True)
    for k, v in res.items():
        a = np.asarray(v)
        if a.dtype.kind in "biuf":
            np.save(os.path.join(out_dir, k + ".npy"), a.astype(np.float64))


# ------------------------------------------------------------------------------------------------ M1
def run_m1(be, world, s_id, t_id, steps, warmup, barrier, drv, profile):
    if drv is not None:
        def step():
            return drv.register(s_id, t_id, N_SRC, MAX_CORR, max_iter=ICP_ITERS, rel_fitness=0.0, rel_rmse=0.0, check_every=ICP_ITERS + 2)
    else:
        def step():
            return be.icp_point_to_plane_dev(s_id, t_id, MAX_CORR, max_iter=ICP_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    import gc

    gc_log = []
    def on_gc(phase, info):
        gc_log.append((phase, info.get("generation"), time.perf_counter()))
    gc.collect()  # cheap once main() has frozen the interpreter's long-lived objects; BEFORE the warm-up, so that the device does not sit
    # idle for milliseconds between the last warm-up step and the first timed one (the first timed step was 15-25 us slower than the rest)
    marks = [0.0] * (steps + 1)
    res = None
    for _ in range(warmup):
        res = step()
    barrier()
    gc.callbacks.append(on_gc)
    t0 = marks[0] = time.perf_counter()
    for k in range(steps):
        res = step()
        marks[k + 1] = time.perf_counter()  # every registration ends with its result on the host, so these are step boundaries
    barrier()
    elapsed = time.perf_counter() - t0
    assert res["iterations"] == ICP_ITERS
    gc.callbacks.remove(on_gc)
    step_us = np.diff(np.array(marks)) * 1e6
    collections = [(g, round((b - a) * 1e3, 2), round((a - t0) * 1e3, 2)) for (p0, g, a), (p1, _, b) in zip(gc_log[::2], gc_log[1::2])]
    if not profile:
        return res, elapsed, None, None, step_us, collections, None
    # roofline of the dominant kernel (icp_fused_kernel: one ICP pass + the previous pass's solve/update in its prologue): the same
    # steps re-run with hipEvent brackets around every launch on the launch stream (outside the timed region above)
    be.profile_enable(True)
    for _ in range(min(steps, 100)):
        step()
    n_launch, kern_ms = be.profile_read()
    be.profile_enable(False)
    # ... and once more with ONE pair of events around every whole registration and none inside it: the launches of a registration
    # run back to back on the stream, so span / passes is the per-pass kernel time that `rocprofv3 --kernel-trace --stats` reproduces
    # (plus the gaps between launches and the one-workgroup fold launch: an upper bound of it)
    be.profile_enable(2)
    for _ in range(min(steps, 100)):
        with be.span(1):
            step()
    n_span, span_ms = be.span_read(1)
    be.profile_enable(False)
    return res, elapsed, n_launch, kern_ms, step_us, collections, (n_span, span_ms)


def run_config4(args, world, rank, local_rank, barrier, emit=True):
    """BASELINE.json configs[4]: ONE dense voxel map (VoxelizedPointCloud, Voxel.cpp:18-114) over the GPUs of the node.  A STEP = every
    rank contributes a 2 M-point placed scan (16 OS-128 frames fused; voxel 0.02 m): rows grouped by voxel owner on the
    device, one all-to-all between the GPUs, fusion into the local table.  Weak scaling; value = points fused per second over all ranks."""
    import torch
    import torch.distributed as dist

    from open3d_slam_amd import backend, sharded, synthetic as syn

    scene = syn.make_scene()
    poses = syn.figure_eight_poses(200, 0.1)
    frames = [syn.os128_scan(scene, poses[(16 * rank + k) % 200], frame=16 * rank + k) @ poses[(16 * rank + k) % 200][:3, :3].T
              + poses[(16 * rank + k) % 200][:3, 3] for k in range(16)]
    scan = np.vstack(frames)  # 2 097 152 points in the map frame
    be = backend.Backend(local_rank)
    dm = sharded.ShardedDenseMap(be, 0.02, has_normals=False)
    cid = be.upload(scan)
    steps, warmup = min(args.steps, 50), min(args.warmup, 5)
    for _ in range(warmup):
        dm.insert(cid)
    import gc

    gc.collect()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        dm.insert(cid)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=f"cuda:{local_rank}")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    voxels = dm.size()
    if rank == 0:
        n = len(scan)
        algo = n * (12 + 40)  # SURVEY.md 8d C5 (no normals): 12 B xyz read + 40 B voxel record read-modify-write per point
        gbs = world * steps * algo / elapsed / 1e9
        line = {
            "metric": "dense_fusion_points_per_sec", "value": world * steps * n / elapsed, "unit": "points/s", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 points, int64 fixed-point sums", "data": "synthetic",
            "config": {"workload": f"configs[4]: one dense voxel map over {world} GPU(s), {n} placed points per GPU per step (16 OS-128 frames), voxel 0.02 m, "
                                   "rows grouped by voxel owner on the device + one all-to-all + hash fusion", "points_per_gpu_per_step": n,
                       "voxel_m": 0.02, "parallelism": "1 GPU" if world == 1 else f"voxel-owner sharding over {world} GPUs, one all_to_all_single per step"},
            "global_voxels": voxels,
            "roofline": {"bound": "hbm", "achieved": gbs / world, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / world / HBM_PEAK_GBS, "traffic": None,
                         "kernel": "whole step per GPU (owner count + scatter, all-to-all, import, dense_insert_kernel)",
                         "algorithmic_bytes_per_point": 52}}
        if emit:
            sys.stdout.flush()
            if _LINE_FD is not None:
                os.write(_LINE_FD, (json.dumps(line, separators=(",", ":")) + "\n").encode())
            else:
                print(json.dumps(line), flush=True)
    be.free(cid)
    dm.close()
    be.close()
    return line if rank == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cell", type=float, default=0.0, help="NN grid cell size (0 = max_corr/4)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=16.0)
    ap.add_argument("--m2-frames", type=int, default=200, help="frames of the configs[2] stream (0: skip M2)")
    ap.add_argument("--m2-cpu-frames", type=int, default=200, help="frames of the stream the CPU oracle loop plays (all of them by default: like for like)")
    ap.add_argument("--no-host-seam", action="store_true", help="skip the configs[2] run through the integration header with host clouds at the seams")
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--no-gicp", action="store_true", help="skip the m1_gicp line (configs[1] under GeneralizedIcp)")
    ap.add_argument("--large-map", type=int, default=8_000_000, help="points of the larger-than-Infinity-Cache map of the m1_large_map line (0: skip)")
    ap.add_argument("--concurrent", type=int, default=4, help="registrations in flight at once for the `concurrent` line (0 / 1: skip)")
    ap.add_argument("--config", default="auto", choices=["auto", "1", "3", "3u", "4"],
                    help="BASELINE.json configs: 1 = scan vs 1M map on one GPU (+ M2); 3 = joint registration over one submap per GPU (sum of the "
                         "per-submap normal equations); 3u = ONE map split over the GPUs, union-equivalent (key MIN all-reduce + record sum); "
                         "4 = one dense voxel map over the GPUs, 2M-pt scan per GPU per step, voxel 0.02 (all-to-all of rows by voxel owner). "
                         "auto = 1 at N = 1, 3 at N > 1")
    ap.add_argument("--dry-line", metavar="DETAIL_JSON", default=None,
                    help="no GPU work: assemble and print the compact line from a detail file of an earlier run (tests/test_bench_line.py)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the roofline re-runs, the f64 / 8 M-point map / in-library / GeneralizedIcp / concurrent "
                         "legs, the copy bandwidth, M2 and its tables, the CPU baselines, and at N > 1 configs 3u and 4 beside configs[3]. "
                         "Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the result of the last timed registration (what icp_point_to_plane_dev returns) "
                         "as DIR/<field>.npy, float64; the inputs are seeded, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.dump_outputs and args.config == "4":
        ap.error("--dump-outputs: configs[1] / [3] only")
    if args.dry_line:
        print(compact_line(json.load(open(args.dry_line)), os.path.relpath(args.dry_line, ROOT)), flush=True)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    all_configs = args.full and args.config == "auto" and world > 1  # configs[3] is the line, 3u and 4 ride along in it
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            # started bare (`python bench.py --gpus N`): become the launcher -- one rank per GPU through torch.distributed.run, same
            # arguments, rank 0 prints the JSON line, the launcher passes its exit status on
            import socket
            import subprocess

            env = dict(os.environ)
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            rc = 1
            for _attempt in range(3):  # a port found free by bind-and-close can be taken before the rendezvous binds it: then try another
                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    port = sk.getsockname()[1]
                cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
                       "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
                p = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, text=True)
                sys.stderr.write(p.stderr)
                rc = p.returncode
                if rc == 0 or "address already in use" not in p.stderr.lower():
                    break
            raise SystemExit(rc)
        args.gpus = world
    if args.config == "auto":
        args.config = "1" if world == 1 else "3"
    claim_stdout()
    do_m2 = args.full and world == 1 and args.m2_frames > 1 and args.config == "1"
    scans32 = make_stream(args.m2_frames) if do_m2 else None  # before the GPU runtime exists in this process (fork)

    import torch
    import torch.distributed as dist

    from open3d_slam_amd import backend, sharded, synthetic as syn

    # one rank per GPU; O3DS_BENCH_BACKEND=gloo lets the N>1 path be smoke-tested on a box with fewer GPUs than ranks
    dist_backend = os.environ.get("O3DS_BENCH_BACKEND", "nccl")
    if dist_backend != "nccl":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(dist_backend, rank=rank, world_size=world)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # The interpreter's long-lived objects (about a million after `import torch`) leave the garbage collector's sight: a full collection
    # over them takes 30-40 ms, it falls wherever the allocation counters happen to trip -- step 14 of a 50-ms timed region, measured
    # (22.6 k instead of 40.2 k it/s on the line, the steps themselves untouched at 248 us median) -- and it has nothing to
    # do with the work being timed.  The collector stays ON; every timed region starts from a collected heap.
    import gc

    gc.collect()
    gc.freeze()

    if args.config == "4":
        run_config4(args, world, rank, local_rank, barrier)
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- M1 workload (seeded)
    scene = syn.make_scene()
    T_gt = syn.ground_truth_pose()
    src = syn.vlp16_scan(scene, T_gt)
    tgt, nrm = syn.sample_map(scene, N_MAP, seed=syn.SEED_MAP + rank)
    assert len(src) == N_SRC
    algo_bytes = N_SRC * ALGO_BYTES_PER_POINT

    def m1(prec, steps, warmup, target=None, mode=None, library=False):
        be = backend.Backend(local_rank, prec)
        s_id = be.upload(src)
        t_id = be.upload(*(target or (tgt, nrm)))
        t0 = time.perf_counter()
        be.build_index(t_id, MAX_CORR, args.cell)
        be.synchronize()
        index_build_ms = (time.perf_counter() - t0) * 1e3
        if mode is None:
            mode = "union" if args.config == "3u" else "submap"
        # library: o3ds_icp_register_sharded -- the loop, the kernels and the ncclAllReduce calls inside libo3ds_backend.so (its own RCCL
        # communicator); else open3d_slam_amd/sharded.py: the same kernels driven from Python with torch.distributed collectives in between
        drv = (sharded.LibraryShardedIcp(be, mode=mode) if library else sharded.ShardedIcp(be, mode=mode)) if (world > 1 or args.config == "3u" or library) else None
        res, elapsed, n_launch, kern_ms, su, collections, spans = run_m1(be, world, s_id, t_id, steps, warmup, barrier, drv, profile=args.full)
        if args.full:
            # what a hipEvent bracket costs by itself on this stream (two records back to back): the brackets around the pass launches include it
            be.profile_enable(True)
            for _ in range(200):
                with be.span(0):
                    pass
            n_br, br_ms = be.span_read(0)
            be.profile_enable(False)
            bracket_s = br_ms * 1e-3 / max(n_br, 1)
        if world > 1:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device=f"cuda:{local_rank}")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        be.close()
        spread = {"median": float(np.median(su)), "p10": float(np.percentile(su, 10)), "p90": float(np.percentile(su, 90)), "max": float(su.max()),
                  "host_cpu": host_cpu(), "argmax": int(np.argmax(su)), "gc": collections}
        if not args.full:
            return dict(res=res, elapsed=elapsed, index_build_ms=index_build_ms, step_us=spread)
        n_span, span_ms = spans
        avg_bracket_s = kern_ms * 1e-3 / max(n_launch, 1)
        bracket_kernel_s = max(avg_bracket_s - bracket_s, 1e-9)  # a bracket minus an empty one: over-subtracts; kept as a second figure
        passes = ICP_ITERS + 1
        avg_kernel_s = span_ms * 1e-3 / max(n_span, 1) / passes  # device span of a whole registration / its correspondence passes
        gbs = algo_bytes / avg_kernel_s / 1e9
        # (the pass launches of a step must fit inside the step they are part of: a roofline figure that does not invites distrust of the rest)
        # (the passes of a step must fit inside the step they are part of; the span is measured in a re-run of the steps, so a disturbed box --
        # or a profiler that serialises the kernels of one run differently from the other -- can break that by a few per cent: reported, not fatal)
        span_fits = world > 1 or passes * avg_kernel_s <= elapsed / steps * 1.05
        return dict(res=res, elapsed=elapsed, index_build_ms=index_build_ms, n_launch=n_span * passes, avg_kernel_s=avg_kernel_s, gbs=gbs, step_us=spread,
                    avg_bracket_s=avg_bracket_s, bracket_overhead_s=bracket_s, bracket_kernel_s=bracket_kernel_s, span_fits=bool(span_fits))

    r32 = m1(backend.PRECISION_F32, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, r32["res"])
    r64 = None
    if args.full and not args.no_f64:
        try:
            r64 = m1(backend.PRECISION_F64, max(args.steps // 2, 1), args.warmup)
        except Exception as e:  # noqa: BLE001 -- a secondary leg: reported, never fatal to the line
            sys.stderr.write(f"m1_f64 leg failed: {e!r}\n")
    # the same registration against a map that does NOT fit the 256 MiB Infinity Cache (8 M points: 256 MB of cell-sorted points + normals,
    # as much again in cloud order, 36 MB of grid): configs[1]'s own working set (32 MB + 9 MB) is cache resident, so its counter readings
    # and its rate say nothing about HBM -- this line does
    r_big = None
    if args.full and world == 1 and args.config == "1" and args.large_map > 0:
        try:
            big = syn.sample_map(scene, args.large_map, seed=syn.SEED_MAP + 17)
            r_big = m1(backend.PRECISION_F32, max(args.steps // 4, 5), 3, target=big)
            r_big["n_map"] = args.large_map
            del big
        except Exception as e:  # noqa: BLE001
            sys.stderr.write(f"m1_large_map leg failed: {e!r}\n")
            r_big = None

    r_lib = None
    if args.full and world == 1 and args.config == "1" and not args.no_f64:
        try:
            r_lib = m1(backend.PRECISION_F32, max(args.steps // 4, 5), 3, mode="source", library=True)
        except Exception as e:  # noqa: BLE001 -- an extra leg: it must not take the line down
            r_lib = {"error": repr(e)[:300]}
    # ---- the same registration from several host threads at once, one handle (= one HIP stream) each: how open3d_slam calls it
    # (odometry, mapping and loop-closure workers register concurrently, SlamWrapper.cpp:258-347).  One 64k-query grid is a single wave of
    # workgroups and a registration is a chain of dependent launches, so one stream leaves most of the chip idle most of the time.
    conc = None
    if args.full and world == 1 and args.config == "1" and args.concurrent > 1:
        import threading

        K = args.concurrent
        bes = [backend.Backend(local_rank) for _ in range(K)]
        ids = []
        for b in bes:
            s_id, t_id = b.upload(src), b.upload(tgt, nrm)
            b.build_index(t_id, MAX_CORR, args.cell)
            ids.append((s_id, t_id))
        steps_c = max(args.steps // 2, 1)

        def work(b, s_id, t_id, n):
            for _ in range(n):
                b.icp_point_to_plane_dev(s_id, t_id, MAX_CORR, max_iter=ICP_ITERS, rel_fitness=0.0, rel_rmse=0.0)

        for b, (s_id, t_id) in zip(bes, ids):
            work(b, s_id, t_id, 3)
        torch.cuda.synchronize()
        th = [threading.Thread(target=work, args=(b, s_id, t_id, steps_c)) for b, (s_id, t_id) in zip(bes, ids)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        conc = {"streams": K, "value": K * steps_c * ICP_ITERS / el, "unit": "icp_iterations/s (sum over the streams)", "steps_per_stream": steps_c,
                "ms_per_step_per_stream": el / steps_c * 1e3,
                "algorithmic_gbs": K * steps_c * (ICP_ITERS + 1) * algo_bytes / el / 1e9,
                "frac_of_hbm_peak_over_wall_time": K * steps_c * (ICP_ITERS + 1) * algo_bytes / el / 1e9 / HBM_PEAK_GBS}
        for b in bes:
            b.close()
    # measured device copy bandwidth on this box (report against the vendor peak AND a measured copy kernel)
    copy_gbs = None
    if args.full and rank == 0:
        nb = 1 << 30
        a_, b_ = torch.empty(nb, dtype=torch.uint8, device=f"cuda:{local_rank}"), torch.empty(nb, dtype=torch.uint8, device=f"cuda:{local_rank}")
        b_.copy_(a_)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            b_.copy_(a_)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 5 * 2 * nb / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del a_, b_

    # ---- M2: the configs[2] stream, once untouched for the rates and once with event spans for the per-call table
    m2 = None
    if do_m2:
        try:  # (the stream legs must not take the M1 line down with them)
            be2 = backend.Backend(local_rank)
            run_stream(be2, scans32[: min(12, len(scans32))])  # warm the allocator and the code paths
            be2.close()
            be2 = backend.Backend(local_rank)
            m2 = run_stream(be2, scans32)
            be2.close()
            be2 = backend.Backend(local_rank)
            free = run_stream(be2, scans32, stage_sync=False)
            m2["free_running"] = {"scans_per_sec": free["scans_per_sec"], "pose_equals_staged_run_bitwise": bool(np.array_equal(free["pose"], m2["pose"])),
                                  "what": "the same loop without the stream drains that make the per-stage times exact (after the odometry and after "
                                          "the mapping of every frame): what a consumer that only needs the poses sees; frames 1.. / wall time"}
            be2.close()
            be2 = backend.Backend(local_rank)
            pg = run_stream(be2, scans32, pinned=False, prefetch=False)
            m2["pageable_ingest_at_frame_start"] = {
                "scans_per_sec": pg["scans_per_sec"], "pose_equals_bitwise": bool(np.array_equal(pg["pose"], m2["pose"])),
                "what": "as rounds 1-4 measured it: the raw scan sits in pageable memory and is handed over at the start of its own frame (the copy "
                        "through the handle's pinned ring and the wait for it are on the frame's critical path); the headline keeps the scans in "
                        "page-locked message buffers and hands scan k + 1 over while frame k runs (o3ds_pinned_alloc, o3ds_cloud_upload_f32)"}
            be2.close()
            be2 = backend.Backend(local_rank)
            free_na = run_stream(be2, scans32, stage_sync=False, ahead=False)
            m2["free_running"]["scans_per_sec_without_preprocessing_ahead"] = free_na["scans_per_sec"]
            m2["free_running"]["pose_equals_bitwise_without_it"] = bool(np.array_equal(free_na["pose"], m2["pose"]))
            be2.close()
            be2 = backend.Backend(local_rank)
            na = run_stream(be2, scans32, ahead=False)
            m2["next_scan_preprocessed_behind_the_odometry_registration"] = {
                "scans_per_sec_without": na["scans_per_sec"], "pose_equals_bitwise": bool(np.array_equal(na["pose"], m2["pose"])),
                "what": "the odometry's pre-processing of scan k + 1 is queued behind frame k's scan-to-scan registration, before the host waits for the result "
                        "(o3ds_icp_overlap_next; open3d_slam's odometry worker runs ahead on its own thread); without: at the start of frame k + 1.  A staged "
                        "run drains the stream after every stage and so gains nothing from it; free-running loops do (free_running_without below)"}
            be2.close()
            # the same loop with the odometry's and the mapper's identical pre-processing of a raw scan computed twice, as the reference does
            # (open3d_slam_amd/pointcloud.py shared_preprocess: by default the second caller gets the first caller's cloud)
            from open3d_slam_amd import pointcloud as _pc
            be2 = backend.Backend(local_rank)
            _pc.SHARE_PREPROCESS = False
            try:
                twice = run_stream(be2, scans32)
            finally:
                _pc.SHARE_PREPROCESS = True
            m2["shared_preprocess"] = {"what": "LidarOdometry::preprocess and ScanToMapIcp::preprocess run the same crop -> voxelize -> normals on the same raw "
                                               "scan when configured alike (the shipped configuration); the host mirror computes it once per scan",
                                       "scans_per_sec_when_computed_twice": twice["scans_per_sec"],
                                       "pose_equals_bitwise": bool(np.array_equal(twice["pose"], m2["pose"]))}
            be2.close()
            be2 = backend.Backend(local_rank)
            prof = run_stream(be2, scans32, profile=True)
            be2.close()
            m2["calls"] = prof["calls"]
            m2["pose_repeats_bitwise_between_the_two_runs"] = bool(np.array_equal(m2["pose"], prof["pose"]))
            try:  # an extra line of the report: it must not take the measured lines above down with it
                run_stream_pipelined(local_rank, scans32[: min(12, len(scans32))])
                pl = run_stream_pipelined(local_rank, scans32)
                m2["pipelined"] = {"scans_per_sec": pl["scans_per_sec"], "map_points": pl["map_points"],
                                   "pose_equals_serial_bitwise": bool(np.array_equal(m2["pose"], pl["pose"])),
                                   "what": "odometry and mapping on two host threads and two backend handles (SlamWrapper.cpp:228-229), raw scan ingested by both"}
                # ... and with the hand-over the integration header has between the reference's two workers: the mapper's handle copies
                # the raw scan and its pre-processed version from views the odometry worker exported, the odometry worker takes its
                # scans as the one-handle loop does (page-locked records, the next scan pre-processed behind this one's registration)
                run_stream_pipelined(local_rank, scans32[: min(12, len(scans32))], share=True, drain=False)
                ps = run_stream_pipelined(local_rank, scans32, share=True, drain=False)
                same = len(ps["poses_per_frame"]) == len(m2["poses_per_frame"]) and all(
                    np.array_equal(a, b) for a, b in zip(ps["poses_per_frame"], m2["poses_per_frame"]))
                m2["two_workers"] = {"scans_per_sec": ps["scans_per_sec"], "map_points": ps["map_points"], "every_pose_equals_the_one_handle_run_bitwise": bool(same),
                                     "what": "odometry and mapping on two host threads and two backend handles; the mapper's handle takes the raw scan and "
                                             "its pre-processed version through o3ds_cloud_export_view / _import_view (device-to-device copies behind an "
                                             "event), nothing is ingested or pre-processed twice; no stream drains (each worker waits only for its own "
                                             "registrations' results)"}
            except Exception as e:  # noqa: BLE001
                m2["pipelined"] = {"error": repr(e)}
            try:  # the stream as the shipped Lua configures it: GeneralizedIcp in both workers, downsampling_ratio 0.3 (seeded index lists)
                be2 = backend.Backend(local_rank)
                run_stream(be2, scans32[: min(12, len(scans32))], shipped=True)
                be2.close()
                be2 = backend.Backend(local_rank)
                sh = run_stream(be2, scans32, shipped=True)
                be2.close()
                run_stream_pipelined(local_rank, scans32[: min(12, len(scans32))], share=True, drain=False, shipped=True)
                sh2 = run_stream_pipelined(local_rank, scans32, share=True, drain=False, shipped=True)
                same2 = len(sh2["poses_per_frame"]) == len(sh["poses_per_frame"]) and all(np.array_equal(a, b) for a, b in zip(sh2["poses_per_frame"], sh["poses_per_frame"]))
                m2["shipped_configuration"] = {
                    "two_workers_scans_per_sec": sh2["scans_per_sec"], "two_workers_every_pose_equals_the_one_handle_run_bitwise": bool(same2),
                    "scans_per_sec": sh["scans_per_sec"], "mapping_only_scans_per_sec": sh["mapping_only_scans_per_sec"], "ms_per_scan": sh["ms_per_scan"],
                    "map_points": sh["map_points"], "final_pose_error_vs_truth": sh["final_pose_error_vs_truth"],
                    "what": "the same 200 frames with cloud_registration_type / scan_to_map_refinement_type = GeneralizedIcp and downsampling_ratio = 0.3 "
                            "(parameter_structure_definitions.lua:62,76,109) in the odometry and the mapper; the crop -> voxelize -> normals chain is "
                            "shared up to the RandomDownSample, each worker draws its own (seeded) subset ON THE DEVICE (o3ds_random_down_sample: no shuffle on the host, no wait for the size)"}
            except Exception as e:  # noqa: BLE001
                m2["shipped_configuration"] = {"error": repr(e)[:400]}
            try:
                m2["map_insert_scan_by_map_size"] = {
                    "rows": run_insert_sweep(local_rank, scans32),
                    "what": "o3ds_map_insert_scan (Submap::insertScan: transform, +=, voxelizeWithinCroppingVolume, search index) of the stream's "
                            "pre-processed scans at their true poses into one growing map; hipEvent span per call; rows = the insertions whose map "
                            "size lies within 20 % of 100 k / 300 k / 1 M points"}
                for row_ in m2["map_insert_scan_by_map_size"]["rows"]:  # ... and as rows of the per-call table, beside the stream's average
                    m2["calls"]["map_insert_scan at ~%d k map points (growing map, sweep)" % (row_["map_points_mark"] // 1000)] = {
                        "calls": row_["insertions"], "avg_us": row_["avg_us"], "median_us": row_["median_us"], "max_us": row_["max_us"],
                        "map_points": row_["map_points"], "scan_points": row_["scan_points"],
                        "bytes": "independent of the map's size by construction (DESIGN.md 4.7): ~100 B per scan point and voxel touched"}
            except Exception as e:  # noqa: BLE001
                m2["map_insert_scan_by_map_size"] = {"error": repr(e)[:400]}
            try:  # open3d_slam's own LidarOdometry / Mapper sources with integration/open3d_slam_o3ds.patch applied, on this library
                from oracle import ref as _ref

                if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libo3dslam_ref_patched.so")) and not args.no_host_seam:
                    # (--no-host-seam, the profiler runs: under rocprofv3 the reference's worker threads abort the process -- round 5's evidence
                    # visit lost 35 GPU-minutes to that)
                    mp_, op_ = stream_parameters()
                    res_p = {}
                    for name, threads in (("serial", False), ("two_threads", True)):
                        R = _ref.ReferenceSlam(mp_, op_, patched=True)
                        R.run_stream(scans32[:8], threads=threads)
                        R.close()
                        R = _ref.ReferenceSlam(mp_, op_, patched=True)
                        ok, M_, O_, ms_, n_map_ = R.run_stream(scans32, threads=threads)
                        R.close()
                        res_p[name] = {"scans_per_sec": len(scans32) * 1e3 / ms_, "frames_ok": int(ok), "map_points": int(n_map_)}
                    res_p["what"] = ("the reference's own addRangeScan + addRangeMeasurement (sources compiled with the patch, stand-in Eigen / PointCloud "
                                     "container: oracle/ref_build) calling libo3ds_backend.so; raw scans are host PointClouds of doubles")
                    m2["patched_reference"] = res_p
            except Exception as e:  # noqa: BLE001
                m2["patched_reference"] = {"error": repr(e)[:400]}
            del m2["pose"]
            m2_poses = m2.pop("poses_per_frame")
            prof.pop("poses_per_frame", None)
            if not args.no_host_seam:
                # the same stream through integration/o3ds_open3d_slam.hpp -- the functions the open3d_slam patch calls -- with HOST clouds at
                # every seam: what a patched open3d_slam gets; never `value`
                try:
                    import importlib.util
                    import tempfile

                    spec = importlib.util.spec_from_file_location("stream_integration", os.path.join(ROOT, "scripts", "stream_integration.py"))
                    si = importlib.util.module_from_spec(spec)
                    spec.loader.exec_module(si)
                    with tempfile.TemporaryDirectory() as tmp:
                        path = os.path.join(tmp, "scans.bin")
                        si.write_scans(path, scans32, syn.figure_eight_poses(200, 0.1)[: len(scans32)])
                        exe = si.compile_program(tmp, werror=False)
                        hs = si.run(exe, path, "serial", os.path.join(tmp, "poses.bin"))
                        hp, _ = si.read_poses(os.path.join(tmp, "poses.bin"), len(scans32))
                        worst = max(max(syn.se3_error(a, b)) for a, b in zip(hp, m2_poses))
                        ht = si.run(exe, path, "threads")
                    m2["host_seam"] = {"scans_per_sec": hs["scans_per_sec"], "mapping_only_scans_per_sec": hs["scans_per_sec_mapping_only"],
                                       "ms_per_scan": hs["ms_per_scan"], "map_points": hs["map_points"],
                                       "two_threads_scans_per_sec": ht["scans_per_sec"],
                                       "worst_pose_difference_vs_device_resident_loop": worst,
                                       "what": "C++ through integration/o3ds_open3d_slam.hpp (tests/cpp/stream_integration.cpp): every raw scan arrives as a host "
                                               "PointCloud of doubles, every pre-processed cloud is downloaded for its readers; a scan the previous seam put on "
                                               "the device is not uploaded again (o3ds::ScanOnDevice)"}
                except Exception as e:  # noqa: BLE001
                    m2["host_seam"] = {"error": repr(e)[:600]}
        except Exception as e:  # noqa: BLE001
            import traceback

            traceback.print_exc()
            m2, m2_poses = {"error": repr(e)[:600]}, None

    if rank == 0:
        res, elapsed = r32["res"], r32["elapsed"]
        classic = world > 1 and os.environ.get("O3DS_SHARDED_FORM") == "classic"  # (the shipped library has no O3DS_ICP_MODE switch: always the fused form)
        pass_kernel = "icp_accumulate_kernel" if classic else "icp_fused_kernel"
        dt_gt, dr_gt = syn.se3_error(res["transformation"], T_gt)

        # counter-based traffic per launch: measured under rocprofv3 --pmc in separate passes (scripts/gpu_pmc_traffic.sh), calibrated against
        # known byte counts in this kernel's access pattern (scripts/pmc_calib.hip), committed as profiles/r05_pmc_traffic.json -- a profiler
        # cannot run inside this process, so the line quotes the committed measurement of the same command and names it
        # (quoted only while the kernel source is the one it was measured on: the file carries the hash of icp_kernels.hpp)
        import glob

        TRAFFIC_FILE = os.path.relpath(sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_traffic.json")))[-1], ROOT)
        try:
            import hashlib

            tdoc = json.load(open(os.path.join(ROOT, TRAFFIC_FILE)))
            now = hashlib.sha256(open(os.path.join(ROOT, "open3d_slam_amd", "csrc", "icp_kernels.hpp"), "rb").read()).hexdigest()[:16]
            traffic_db = tdoc["kernels"] if tdoc.get("kernel_source_sha16", {}).get("icp_kernels.hpp") == now else {}
            hs = hashlib.sha256()
            for name in ("cloud_kernels.hpp", "normals_kernel.hpp", "map_kernels.hpp"):
                hs.update(open(os.path.join(ROOT, "open3d_slam_amd", "csrc", name), "rb").read())
            stream_traffic = (tdoc.get("stream_kernels", {})
                              if tdoc.get("kernel_source_sha16", {}).get("stream (cloud_kernels.hpp + normals_kernel.hpp + map_kernels.hpp)") == hs.hexdigest()[:16] else {})
        except (OSError, ValueError, KeyError):
            traffic_db, stream_traffic = {}, {}

        def roof(r, which="icp_fused_kernel<P4f> configs[1] (1 M-point map)"):
            t = traffic_db.get(which) if pass_kernel == "icp_fused_kernel" and world == 1 else None
            return {"bound": "hbm", "achieved": r["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": r["gbs"] / HBM_PEAK_GBS,
                    "traffic": t["traffic_bytes_per_launch"] if t else None,
                    "traffic_detail": None if not t else {
                        "what": "bytes per launch between L2 and the fabric (Infinity Cache + HBM; the counters cannot separate them): TCC_EA0_RDREQ x 64 B + "
                                "TCC_EA0_WRREQ x 64 B, means over the pass launches; the upper figure takes every read request as a full 128-B line",
                        "upper": t["traffic_bytes_per_launch_if_every_read_is_a_full_line"], "over_algorithmic": t["traffic_over_algorithmic"],
                        "over_compulsory": t["traffic_over_compulsory"], "source": TRAFFIC_FILE + " (" + which + ")"},
                    "kernel": pass_kernel, "launches": r["n_launch"], "avg_launch_us": r["avg_kernel_s"] * 1e6,
                    "avg_launch_us_what": "hipEvent span of a whole registration on its stream (no events inside) / its 11 correspondence passes: kernels back "
                                          "to back incl. the gaps and the one-workgroup fold launch, i.e. an upper bound of the per-pass kernel time of "
                                          "rocprofv3 --kernel-trace --stats (profiles/); a bracket around every single launch reads "
                                          f"{r['avg_bracket_s'] * 1e6:.2f} us, an empty bracket {r['bracket_overhead_s'] * 1e6:.2f} us",
                    "bracket_avg_launch_us": r["avg_bracket_s"] * 1e6, "bracket_minus_empty_us": r["bracket_kernel_s"] * 1e6,
                    "passes_x_avg_launch_fit_the_step": r["span_fits"],
                    "algorithmic_bytes_per_launch": algo_bytes, "measured_copy_gbs": copy_gbs,
                    "frac_of_measured_copy": r["gbs"] / copy_gbs if copy_gbs else None}

        steps = args.steps
        out = {
            "metric": "icp_iterations_per_sec",
            "value": world * ICP_ITERS * steps / elapsed,  # N = 1: the registration's iterations/s; N > 1: summed over the N submaps (docstring)
            "unit": "icp_iterations/s",
            "n_gpus": world,
            "steps": steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32 points, f64 accumulate",
            "data": "synthetic",
            "config": {"workload": ("configs[1]" if world == 1 and args.config != "3u" else "configs[3]" + (" (union form)" if args.config == "3u" else "")) +
                                   ": point-to-plane ICP, 65536-pt VLP-16 scan vs " + ("a" if world == 1 else f"{world} x one") + " 1,000,000-pt submap" +
                                   ("" if world == 1 else " per GPU") + f", max_corr {MAX_CORR} m, {ICP_ITERS} fixed iterations/step (+1 evaluation pass), index prebuilt",
                       "n_src": N_SRC, "n_map_per_gpu": N_MAP, "icp_iterations_per_step": ICP_ITERS,
                       "parallelism": "1 GPU" if world == 1 and args.config != "3u" else (
                           f"configs[3], union-equivalent: ONE map of {world} x {N_MAP} points split over {world} GPUs; per iteration a search kernel, "
                           f"one MIN all-reduce of {N_SRC} 64-bit keys (512 KB), an accumulate kernel, one 256-B sum all-reduce, an update kernel"
                           if args.config == "3u" else
                           f"configs[3]: ONE joint registration over {world} submaps x 1 GPU: one fused kernel + one 4-KB RCCL "
                           "all-reduce per iteration (value = scan-vs-one-submap iterations per second summed over the GPUs; "
                           "joint_registration_iterations_per_sec counts the joint iterations once)"),
                       "nn_cell_m": args.cell if args.cell > 0 else MAX_CORR / 4},
            "index_build_ms": r32["index_build_ms"],
            "point_queries_per_sec": world * N_SRC * (ICP_ITERS + 1) * steps / elapsed,
            "joint_registration_iterations_per_sec": ICP_ITERS * steps / elapsed,
            "registrations_per_sec": steps / elapsed,
            "pose_error_vs_truth": {"dt_m": dt_gt, "dr_rad": dr_gt, "fitness": res["fitness"], "inlier_rmse": res["inlier_rmse"]},
            "step_us": r32["step_us"],  # spread of the timed steps on the host clock: a wide one means the enqueueing host thread was disturbed
        }
        if args.full:
            out["roofline"] = roof(r32)
        if r64 is not None:
            s64 = max(args.steps // 2, 1)
            d64 = syn.se3_error(r64["res"]["transformation"], res["transformation"])
            out["m1_f64"] = {"value": ICP_ITERS * s64 / r64["elapsed"], "unit": "icp_iterations/s", "steps": s64, "ms_per_step": r64["elapsed"] / s64 * 1e3,
                             "dtype": "f64", "index_build_ms": r64["index_build_ms"], "step_us": r64["step_us"], "roofline": roof(r64, "icp_fused_kernel<P4d> configs[1] (f64 storage)"),
                             "pose_vs_f32_storage": {"dt_m": d64[0], "dr_rad": d64[1]}}
        if r_big is not None:
            sb = max(args.steps // 4, 5)
            out["m1_large_map"] = {"value": ICP_ITERS * sb / r_big["elapsed"], "unit": "icp_iterations/s", "steps": sb, "ms_per_step": r_big["elapsed"] / sb * 1e3,
                                   "n_map": r_big["n_map"], "index_build_ms": r_big["index_build_ms"], "roofline": roof(r_big, "icp_fused_kernel<P4f> 8 M-point map"),
                                   "pose_error_vs_truth": dict(zip(("dt_m", "dr_rad"), syn.se3_error(r_big["res"]["transformation"], T_gt))),
                                   "what": "the configs[1] scan against a map whose index (256 MB cell-sorted + 36 MB grid) exceeds the Infinity Cache"}
        if args.full and world == 1 and args.config == "1" and not args.no_gicp:
            try:
                out["m1_gicp"] = run_m1_gicp(local_rank, src, tgt, nrm, max(args.steps // 2, 1), args.warmup, with_oracle=not args.no_cpu_baseline)
            except Exception as e:  # noqa: BLE001
                out["m1_gicp"] = {"error": repr(e)[:400]}
        if r_lib is not None:
            sl_ = max(args.steps // 4, 5)
            out["m1_in_library_sharded_one_rank"] = r_lib if "error" in r_lib else {
                "value": ICP_ITERS * sl_ / r_lib["elapsed"], "unit": "icp_iterations/s", "steps": sl_, "ms_per_step": r_lib["elapsed"] / sl_ * 1e3,
                "pose_equals_value_leg_bitwise": bool(np.array_equal(r_lib["res"]["transformation"], res["transformation"])),
                "what": "o3ds_icp_register_sharded(O3DS_SHARD_SOURCE) with an RCCL communicator of ONE rank: per pass one icp_fused_kernel + one "
                        "ncclAllReduce(512 doubles) on the handle's stream, queued by the library -- what the collective costs when it moves nothing"}
        if conc is not None:
            out["concurrent"] = conc
        if m2 is not None:
            out["scans_per_sec"] = {"workload": f"configs[2]: OS-128-like stream, {len(scans32[0])} raw float32 points/scan, {args.m2_frames} frames, "
                                                "LidarOdometry::addRangeScan + Mapper::addRangeMeasurement through the host classes (voxel 0.1, knn 20 / r 3, "
                                                "default ICP criteria, map voxel 0.1); upload included", **m2}
            if stream_traffic:
                # counter-based bytes per launch of the stream's kernels (same file, same calibration as roofline.traffic), and on the rows
                # of the per-call table that are one or two kernels
                kt = {k: {"traffic": v["traffic_bytes_per_launch"], "upper": v["traffic_bytes_per_launch_if_every_read_is_a_full_line"], "launches": v["launches"]}
                      for k, v in stream_traffic.items()}
                out["scans_per_sec"]["kernel_traffic"] = {"source": TRAFFIC_FILE + " (stream_kernels)", "bytes_per_launch": kt}
                calls_ = out["scans_per_sec"].get("calls") or {}

                def tsum(*pats):
                    vals = [v["traffic"] for k, v in kt.items() if any(p_ in k for p_ in pats)]
                    return sum(vals) if vals else None
                for row_name, pats in (("normals kernels alone", ("normals_kernel", "normals_finish_kernel")),
                                       ("crop + VoxelDownSample", ("vox_insert_kernel", "vox_order_kernel", "vox_mean_kernel")),
                                       ("map_insert_scan (transform + append + voxelizeWithinCroppingVolume + index rebuild)",
                                        ("pm_place_kernel", "vox_order_kernel", "pm_group_kernel", "pm_merge_kernel", "pm_misc_kernel", "pm_rows_kernel", "pm_place_new_kernel",
                                         "pm_turn_kernel")),
                                       ("index build kernels (every build of the stream)", ("cell_count_kernel", "scatter_kernel"))):
                    if row_name in calls_ and calls_[row_name]:
                        calls_[row_name]["traffic"] = tsum(*pats)
                        calls_[row_name]["traffic_what"] = "sum over one launch each of: " + ", ".join(pats) + " (scans excluded)"
        cres, best_t = None, min(32, os.cpu_count() or 1)
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb, cres, best_t = cpu_baseline_m1(src, tgt, nrm, args.cpu_budget)
            out["cpu_baseline"] = cb
            dt, dr = syn.se3_error(res["transformation"], cres["transformation"])
            out["parity_vs_cpu"] = {"dt_m": dt, "dr_rad": dr, "fitness_gpu": res["fitness"], "fitness_cpu": cres["fitness"]}
            out["speedup_vs_cpu_baseline"] = out["value"] / cb["value"]
            if m2 is not None and "error" not in m2 and args.m2_cpu_frames > 1:
                n_cpu = min(args.m2_cpu_frames, len(scans32))
                cb2, ref2 = cpu_baseline_m2(scans32, n_cpu, best_t)  # the thread count the M1 sweep found best
                out["scans_per_sec"]["cpu_baseline"] = cb2
                out["scans_per_sec"]["speedup_vs_cpu_baseline"] = out["scans_per_sec"]["scans_per_sec"] / cb2["value"]
                # parity of the two legs, frame by frame (f32 storage on the device: stated tolerance 1e-3 m / 1e-3 rad)
                errs = [syn.se3_error(m2_poses[k], ref2.poses_per_frame[k][0]) for k in range(n_cpu)]
                out["scans_per_sec"]["parity_vs_cpu"] = {"frames_compared": n_cpu, "worst_dt_m": max(e[0] for e in errs), "worst_dr_rad": max(e[1] for e in errs),
                                                         "map_points_gpu": out["scans_per_sec"]["map_points"], "map_points_cpu": cb2["map_points"],
                                                         "within_stated_tolerance": bool(max(max(e) for e in errs) <= 1e-3)}
    if all_configs:
        # configs[3] in its union-equivalent form and configs[4] in the same invocation, so that one scaling run covers them (VERDICT round 2,
        # next #4).  They must not cost the line above: a watchdog prints it and ends every rank if they do not come back.
        import threading

        def give_up():
            if rank == 0:
                out["also"] = {"error": "the additional configurations did not finish within 240 s; the line above is configs[3] alone"}
                emit(out)
            os._exit(0)

        dog = threading.Timer(240.0, give_up)
        dog.daemon = True
        dog.start()
        also = {}
        try:  # configs[3] once more with the registration sharded INSIDE the library (RCCL called by libo3ds_backend.so, no Python in the loop)
            if dist_backend != "nccl":
                raise RuntimeError("skipped: RCCL needs one GPU per rank (this run carries its collectives over " + dist_backend + ")")
            sl = max(args.steps // 2, 5)
            rl = m1(backend.PRECISION_F32, sl, 3, library=True)
            if rank == 0:
                also["config_3_in_library"] = {"metric": "icp_iterations_per_sec", "value": world * ICP_ITERS * sl / rl["elapsed"], "unit": "icp_iterations/s", "steps": sl,
                                               "ms_per_step": rl["elapsed"] / sl * 1e3, "joint_registration_iterations_per_sec": ICP_ITERS * sl / rl["elapsed"],
                                               "what": "o3ds_icp_register_sharded(O3DS_SHARD_SUBMAP): per pass one icp_fused_kernel + one ncclAllReduce of 512 doubles, "
                                                       "queued by the library on its own stream for all passes; same work as the line above",
                                               "pose_equals_the_line_above_bitwise": bool(np.array_equal(rl["res"]["transformation"], r32["res"]["transformation"]))}
        except Exception as e:  # noqa: BLE001
            also["config_3_in_library"] = {"error": repr(e)[:400]}
        try:
            s3u = max(args.steps // 4, 5)
            r3u = m1(backend.PRECISION_F32, s3u, 3, mode="union")
            if rank == 0:
                also["config_3u"] = {"metric": "icp_iterations_per_sec", "value": world * ICP_ITERS * s3u / r3u["elapsed"], "unit": "icp_iterations/s", "steps": s3u,
                                     "ms_per_step": r3u["elapsed"] / s3u * 1e3, "joint_registration_iterations_per_sec": ICP_ITERS * s3u / r3u["elapsed"],
                                     "what": f"ONE map of {world} x {N_MAP} points split over the GPUs, union-equivalent: per iteration a search kernel, one MIN "
                                             f"all-reduce of {N_SRC} 64-bit keys, an accumulate kernel, one 256-B sum all-reduce, an update kernel",
                                     "pose_error_vs_truth": dict(zip(("dt_m", "dr_rad"), syn.se3_error(r3u["res"]["transformation"], T_gt)))}
        except Exception as e:  # noqa: BLE001
            also["config_3u"] = {"error": repr(e)[:400]}
        try:
            line4 = run_config4(args, world, rank, local_rank, barrier, emit=False)
            if rank == 0:
                also["config_4"] = line4
        except Exception as e:  # noqa: BLE001
            also["config_4"] = {"error": repr(e)[:400]}
        dog.cancel()
        if rank == 0:
            out["also"] = also
    if rank == 0:
        emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
