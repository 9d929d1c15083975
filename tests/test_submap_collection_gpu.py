"""SubmapCollection on the device: o3ds_cloud_center, the collection at the shipped radius (nothing changes), parity with the reference's
own SubmapCollection (patched: on this device; unpatched: on the CPU) at a 2 m radius, maps that never leave the device, and the
loop-closure cycle of loop_closure.py end to end -- a constraint where the figure-eight comes back, injected drift removed, and two runs
on fresh handles giving the same bits."""
import math
import os

import numpy as np
import pytest

from open3d_slam_amd import backend
from open3d_slam_amd import synthetic as syn

pytestmark = pytest.mark.gpu

RADIUS = 2.0  # several switches over the 20 m figure-eight
PARITY_FRAMES = 70
STRICT_FRAMES = 24  # frames over which the mirror and the patched reference agree on every map size and within 1e-9 on the poses
LOOP_FRAMES = 200


@pytest.fixture(scope="module")
def stream():
    scene = syn.make_scene()
    poses = syn.figure_eight_poses(200, 0.1)
    scans = [np.asarray(syn.os128_scan(scene, poses[k % 200], frame=k), dtype=np.float32) for k in range(LOOP_FRAMES + 12)]
    return scans, [poses[k % 200] for k in range(LOOP_FRAMES + 12)]


def _params(radius, loop_closures):
    import bench

    mp, op = bench.stream_parameters()
    mp.submaps_.radius_ = radius
    mp.isBuildDenseMap_ = False  # as ref_slam_create sets them
    mp.isAttemptLoopClosures_ = loop_closures
    if loop_closures:
        mp.placeRecognition_.loopClosureSearchRadius_ = 2.0 * radius  # (the shipped 20 m against 2 m submaps would skip 10 neighbours)
    return mp, op


def _mapper(be, mp, op, collection):
    from open3d_slam_amd.mapper import Mapper
    from open3d_slam_amd.odometry import LidarOdometry
    from open3d_slam_amd.submap_collection import SubmapCollection

    odo = LidarOdometry(be)
    odo.setParameters(op)
    mapper = Mapper(be, odo, submaps=SubmapCollection(be) if collection else None)
    mapper.setParameters(mp)
    return odo, mapper


def _step(be, odo, mapper, raw, k):
    from open3d_slam_amd.pointcloud import PointCloud

    cloud = PointCloud.from_pointcloud2(be, raw)
    try:
        a = odo.addRangeScan(cloud, 0.1 * k)
        b = a and mapper.addRangeMeasurement(cloud, 0.1 * k)
    finally:
        cloud.release()
    return 1 if (a and b) else (0 if not a else -1)


@pytest.fixture
def no_map_downloads(monkeypatch):
    """Backend.download / download_f32 / fpfh raise while the fixture is active: no map (nor feature) comes to the host."""
    def refuse(*a, **k):
        raise AssertionError("a map or its features was downloaded to the host")

    for name in ("download", "download_f32", "fpfh"):
        monkeypatch.setattr(backend.Backend, name, refuse)
    return monkeypatch


# ------------------------------------------------------------------------------------------------------------ 1. o3ds_cloud_center
@pytest.mark.parametrize("precision", [backend.PRECISION_F32, backend.PRECISION_F64])
def test_cloud_center_is_the_fsum_mean_and_reproducible(precision):
    be, be2 = backend.Backend(0, precision=precision), backend.Backend(0, precision=precision)
    rng = np.random.default_rng(11)
    try:
        for n in (0, 1, 63, 64, 65, 1_000_003):
            P = rng.normal(size=(n, 3)) * [40.0, 25.0, 3.0] + [120.0, -35.0, 4.0]
            cid, cid2 = be.upload(P), be2.upload(P)
            c1, c1b, c2 = be.cloud_center(cid), be.cloud_center(cid), be2.cloud_center(cid2)
            assert c1.tobytes() == c1b.tobytes() == c2.tobytes(), n  # the same bits: repeated calls, two handles
            stored = be.download(cid)[0]  # the points as stored (f32: rounded)
            want = np.array([math.fsum(stored[:, j]) / n for j in range(3)]) if n else np.zeros(3)
            scale = float(np.abs(stored).max()) if n else 1.0
            assert np.abs(c1 - want).max() <= 1e-12 * scale, (n, c1 - want)
            if n == 0:
                assert np.array_equal(c1, np.zeros(3))
            be.free(cid)
            be2.free(cid2)
        # a size the host has not seen yet (VoxelDownSample publishes it on the device) gives the same bits as once it is known
        P = rng.uniform(-30.0, 30.0, size=(200_000, 3))
        src = be.upload(P)
        v1 = be.voxel_down_sample(src, 0.5)
        lazy = be.cloud_center(v1)
        v2 = be.voxel_down_sample(src, 0.5)
        be.size(v2)
        assert lazy.tobytes() == be.cloud_center(v2).tobytes()
        # non-finite points propagate into the mean, as in GetCenter
        Q = rng.normal(size=(1000, 3))
        Q[17, 1] = np.nan
        q = be.upload(Q)
        c = be.cloud_center(q)
        assert np.isfinite(c[0]) and np.isnan(c[1]) and np.isfinite(c[2])
        Q[17, 1] = np.inf
        q2 = be.upload(Q)
        assert be.cloud_center(q2)[1] == np.inf
    finally:
        be.close()
        be2.close()


# ------------------------------------------------------------------------------------------------------------ 2. shipped radius
def test_the_collection_at_the_shipped_radius_changes_nothing(stream):
    scans, _ = stream
    frames = 60
    mp, op = _params(20.0, False)
    out = {}
    for collection in (False, True):
        be = backend.Backend(0)
        odo, mapper = _mapper(be, mp, op, collection)
        poses = []
        for k in range(frames):
            assert _step(be, odo, mapper, scans[k], k) == 1
            poses.append(mapper.getMapToRangeSensor().copy())
        if collection:
            assert mapper.getSubmaps().getNumSubmaps() == 1
        out[collection] = (np.array(poses), be.download(mapper.getActiveSubmap().getMapPointCloud().id))
        be.close()
    assert np.array_equal(out[False][0], out[True][0])
    assert np.array_equal(out[False][1][0], out[True][1][0]) and np.array_equal(out[False][1][1], out[True][1][1])


# ------------------------------------------------------------------------------------------------------------ 3. + 4. parity, no downloads
def _ref_available():
    from oracle import ref

    return os.path.isfile(ref.LIB_PATCHED) or ref.sources_present()


@pytest.mark.skipif(not _ref_available(), reason="oracle/_ref/libo3dslam_ref_patched.so is neither built nor buildable here")
def test_switching_matches_the_references_own_collection(stream, no_map_downloads):
    from oracle import ref

    scans, _ = stream
    mp, op = _params(RADIUS, False)
    be = backend.Backend(0)
    odo, mapper = _mapper(be, mp, op, True)
    coll = mapper.getSubmaps()
    margins = []
    original = coll.updateActiveSubmap

    def recorded(T, scan):  # the distances the switching decision compares with the radius
        if not coll.isForceNewSubmapCreation_ and coll.numScansMergedInActiveSubmap_ >= mp.submaps_.minNumRangeData_:
            p = coll.mapToRangeSensor_[:3, 3]
            for s in (coll.submaps_[coll.findClosestSubmap(coll.mapToRangeSensor_)], coll.getActiveSubmap()):
                margins.append(abs(np.linalg.norm(p - s.getMapToSubmapCenter()) - RADIUS))
        return original(T, scan)

    coll.updateActiveSubmap = recorded
    R = ref.ReferenceSlam(mp, op, submap_radius=RADIUS, patched=True)
    rows, worst = [], []
    for k in range(PARITY_FRAMES):
        st = _step(be, odo, mapper, scans[k], k)
        rc, O, M, n_map, n_sub = R.add_scan(np.asarray(scans[k], dtype=np.float64), 0.1 * k)
        assert st == rc, k
        assert n_sub == coll.getNumSubmaps(), (k, n_sub, coll.getNumSubmaps())
        n_ours = len(mapper.getActiveSubmap().getMapPointCloud())
        if k < STRICT_FRAMES:
            assert n_map == n_ours, k
        else:
            assert abs(n_map - n_ours) <= 0.002 * n_map, (k, n_map, n_ours)
        if k == STRICT_FRAMES - 1:  # a device copy of the active map (submap 1 by now: the first switch and its drained ring are in it)
            assert coll.getNumSubmaps() >= 2
            strict_map = (R.map()[0], be.transform_cloud(mapper.getActiveSubmap().getMapPointCloud().id, np.eye(4)))
        if st == 1:
            worst.append(max(*syn.se3_error(M, mapper.getMapToRangeSensor())))
        rows.append((rc, M, coll.getNumSubmaps()))
    no_map_downloads.undo()
    got = be.download(strict_map[1])[0]
    assert len(got) == len(strict_map[0])
    differ = int(np.sum(np.any(strict_map[0] != got, axis=1)))
    print(f"active map after the first switch: {len(got)} points in both, {differ} rows differ, by at most "
          f"{float(np.abs(strict_map[0] - got).max()):.3e} m")
    ulp = np.spacing(np.abs(strict_map[0]).astype(np.float32)).astype(np.float64)
    print(f"  largest difference in f32 ulps of the coordinate: {float((np.abs(strict_map[0] - got) / ulp).max()):.1f}")
    assert np.all(np.abs(strict_map[0] - got) <= 8.0 * ulp), differ  # the same points to a few f32 ulps (measured: 4): the poses' 1e-10 differences
    print(f"patched reference vs the mirror: worst pose difference {max(worst):.3e} (frames 0-23: {max(worst[:STRICT_FRAMES]):.3e}), "
          f"first frame above 1e-9: {next((k for k, w in enumerate(worst) if w > 1e-9), None)}")
    assert max(worst[:STRICT_FRAMES]) <= 1e-9  # the bar of tests/test_patched_reference_gpu.py over its 24 frames
    # Beyond them the two harnesses part by ulps -- the reference looks its poses up in a TransformInterpolationBuffer, the mirror
    # exactly -- which the registrations carry on at the 1e-9 level (measured: 1.0e-9 at frame 42) and which, by frame 61, moved one
    # point of the active map across a voxel boundary (measured: 2.2e-6 worst over 70 frames).  So the rest of the stream is held to
    # equal decisions (status, number of submaps) and to tolerances well inside those of the unpatched comparison.
    assert max(worst) <= 1e-4, max(worst)
    assert coll.getNumSubmaps() >= 3, coll.getNumSubmaps()  # several switches happened
    ref_map, _ = R.map()
    R.close()
    got = be.download(mapper.getActiveSubmap().getMapPointCloud().id)[0]
    print(f"final active map: {len(got)} / {len(ref_map)} points")
    assert abs(len(got) - len(ref_map)) <= 0.002 * len(ref_map)
    be.close()
    # the reference BEFORE the patch (Open3D served by the CPU oracle): the same switches, poses within f32 storage error
    R0 = ref.ReferenceSlam(mp, op, submap_radius=RADIUS, patched=False)
    worst0 = 0.0
    for k in range(PARITY_FRAMES):
        rc, O, M, n_map, n_sub = R0.add_scan(np.asarray(scans[k], dtype=np.float64), 0.1 * k)
        assert rc == rows[k][0] and n_sub == rows[k][2], k
        dt, dr = syn.se3_error(M, rows[k][1])
        assert max(dt, dr) <= 1e-3, (k, dt, dr)
        worst0 = max(worst0, dt)
    R0.close()
    # no switching decision lay so close to the radius that the differences between the three runs could have flipped it: the
    # smallest margin (measured: 0.88 mm) is held against ten times the largest position difference seen (not against a fixed 1 mm)
    print(f"unpatched reference: worst position difference {worst0:.3e} m; smallest margin to the radius {min(margins):.3e} m")
    assert min(margins) > 10.0 * max(worst0, max(worst)), (min(margins), worst0, max(worst))
    print(f"collection parity over {PARITY_FRAMES} frames: {rows[-1][2]} submaps, smallest margin to the radius {min(margins):.3e} m")


# ------------------------------------------------------------------------------------------------------------ 5. - 7. loop closure
def _loop_closure_run(scans, truth, inject=None, extra=10):
    """The figure-eight with the loop-closure cycle after every frame (as SlamWrapper's mapping worker runs it) until the first cycle
    that closes a loop; then `extra` more frames.  inject = 4x4: applied to the last finished submap and every later one just before
    that cycle's constraints are built."""
    from open3d_slam_amd.loop_closure import LoopClosure
    from open3d_slam_amd.optimization_problem import buildConstraint

    mp, op = _params(RADIUS, True)
    be = backend.Backend(0)
    odo, mapper = _mapper(be, mp, op, True)
    coll = mapper.getSubmaps()
    lc = LoopClosure(be, mapper)
    base = np.linalg.inv(truth[0])
    drift_t = drift_r = 0.0
    res = {"closed_at": None}
    k = 0
    while k < len(scans):
        assert _step(be, odo, mapper, scans[k], k) == 1, k
        dt, dr = syn.se3_error(mapper.getMapToRangeSensor(), base @ truth[k])
        drift_t, drift_r = max(drift_t, dt), max(drift_r, dr)
        if res["closed_at"] is None:
            lc.computeFeaturesIfReady()
            lc.attemptLoopClosuresIfReady()
            pending = [t.submapId_ for t in lc.loopClosureCandidates_ if coll.getLoopClosureCandidatesIdxs(t.submapId_)]
            if pending and inject is not None and "inject" not in res:
                src = max(pending)
                for s in coll.submaps_[src:]:
                    s.transform(inject)
                res["inject"] = src
            adjacent_before = {(a, b) for a in range(coll.getNumSubmaps()) for b in range(coll.getNumSubmaps())
                               if coll.adjacencyMatrix_.isAdjacent(a, b)}
            pose_before = mapper.getMapToRangeSensor().copy()
            cs = lc.loopClosureWorker()
            if cs:
                if inject is not None:  # the misalignment of the loop, re-registered from identity, before the update
                    c = cs[0]
                    res["before"] = buildConstraint(be, c.sourceSubmapIdx_, c.targetSubmapIdx_, coll.submaps_, mp, True, 1.0, 2.0, False, False)
                lc.updateSubmapsAndTrajectory()
                res.update(closed_at=k, constraints=cs, adjacent_before=adjacent_before, pose_before=pose_before,
                           pose_after=mapper.getMapToRangeSensor().copy(), dT=lc.lastIncrement, drift=(drift_t, drift_r),
                           buffer_after=len(coll.overlapScansBuffer_), op_constraints=list(lc.optimizationProblem_.getLoopClosureConstraints()),
                           poses=[np.array(n.pose_) for n in lc.optimizationProblem_.poseGraphOptimized_.nodes_],
                           adjacency=coll.adjacencyMatrix_)
                if inject is not None:
                    c = cs[0]
                    res["after"] = buildConstraint(be, c.sourceSubmapIdx_, c.targetSubmapIdx_, coll.submaps_, mp, True, 1.0, 2.0, False, False)
                    break
                last = min(len(scans), k + 1 + extra)
                for j in range(k + 1, last):
                    res.setdefault("continued", []).append(_step(be, odo, mapper, scans[j], j))
                break
        k += 1
    res["maps"] = lambda: [be.download(s.getMapPointCloud().id)[0] for s in coll.submaps_]
    res["be"] = be
    return res


@pytest.fixture(scope="module")
def closed_loop(stream):
    scans, truth = stream
    mp = pytest.MonkeyPatch()
    for name in ("download", "download_f32", "fpfh"):
        mp.setattr(backend.Backend, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("a map was downloaded")))
    try:
        res = _loop_closure_run(scans, truth)
    finally:
        mp.undo()
    res["map_arrays"] = res["maps"]()
    yield res
    res["be"].close()


def test_a_loop_is_closed_where_the_figure_eight_comes_back(closed_loop):
    r = closed_loop
    assert r["closed_at"] is not None, "no loop-closure constraint over the whole figure-eight"
    cs = r["constraints"]
    far = [c for c in cs if (c.sourceSubmapIdx_, c.targetSubmapIdx_) not in r["adjacent_before"] and c.sourceSubmapIdx_ > c.targetSubmapIdx_ + 1]
    assert far, [(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in cs]
    drift_t, drift_r = r["drift"]
    for c in far:
        dt, dr = syn.se3_error(c.sourceToTarget_, np.eye(4))
        assert dt <= drift_t + 0.05 and dr <= drift_r + 0.01, (dt, dr, drift_t, drift_r)
        assert r["adjacency"].isAdjacent(c.sourceSubmapIdx_, c.targetSubmapIdx_)
        assert r["adjacency"].isLoopClosureSubmap_[c.sourceSubmapIdx_] and r["adjacency"].isLoopClosureSubmap_[c.targetSubmapIdx_]
    assert r["buffer_after"] == 0
    assert all(np.array_equal(c.sourceToTarget_, np.eye(4)) for c in r["op_constraints"])
    assert np.allclose(r["pose_after"], r["dT"] @ r["pose_before"], atol=1e-12)
    assert r.get("continued") and all(s == 1 for s in r["continued"]), r.get("continued")
    print(f"loop closed at frame {r['closed_at']}: {[(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in cs]}, drift {r['drift']}")


def test_injected_drift_is_removed(stream):
    scans, truth = stream
    inject = syn.make_pose([0.3, 0.0, 0.0], [0.0, 0.0, 2.0])  # (degrees)
    r = _loop_closure_run(scans, truth, inject=inject)
    try:
        assert r["closed_at"] is not None and "inject" in r
        before = syn.se3_error(r["before"].sourceToTarget_, np.eye(4))
        after = syn.se3_error(r["after"].sourceToTarget_, np.eye(4))
        print(f"misalignment at the loop: before {before}, after {after}")
        assert before[0] >= 0.15  # the offset is there before the cycle
        assert after[0] <= 0.5 * 0.3 and after[1] <= 0.5 * 2.0 * math.pi / 180.0, (before, after)
    finally:
        r["be"].close()


def test_two_runs_give_the_same_bits(stream, closed_loop):
    scans, truth = stream
    r = _loop_closure_run(scans, truth)
    try:
        a, b = closed_loop, r
        assert a["closed_at"] == b["closed_at"]
        assert len(a["constraints"]) == len(b["constraints"])
        for c1, c2 in zip(a["constraints"], b["constraints"]):
            assert (c1.sourceSubmapIdx_, c1.targetSubmapIdx_) == (c2.sourceSubmapIdx_, c2.targetSubmapIdx_)
            assert np.array_equal(c1.sourceToTarget_, c2.sourceToTarget_) and np.array_equal(c1.informationMatrix_, c2.informationMatrix_)
        assert len(a["poses"]) == len(b["poses"]) and all(np.array_equal(p, q) for p, q in zip(a["poses"], b["poses"]))
        maps = b["maps"]()
        assert len(maps) == len(a["map_arrays"]) and all(np.array_equal(p, q) for p, q in zip(a["map_arrays"], maps))
    finally:
        r["be"].close()
