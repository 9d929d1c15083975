"""o3ds_icp_register_batch on the device: every entry of a batch is its one-pair registration (o3ds_icp_register_dev) bit for bit --
one entry, ragged batches with shared sources / targets and mixed crops, any order, an entry without correspondences, several initial
guesses for one pair --, the oracle's registrations within DESIGN.md section 2's tolerances (f64 storage 1e-6 m / rad, f32 1e-3,
fitness +-4/n, rmse rel 1e-3), the error conventions, and the loop-closure wiring (the constraints of the sequential form, byte for
byte).  Shapes are small on purpose: a workgroup takes 128 queries, so the edges are at 1, 127, 128 and 129 queries and at the
boundaries between entries."""
import ctypes as C
import struct

import numpy as np
import pytest

from open3d_slam_amd import backend
from open3d_slam_amd import synthetic as syn

pytestmark = pytest.mark.gpu

B = backend.Backend
R = 1.0
METHODS = (backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED, backend.ICP_POINT_TO_POINT)
PRECISIONS = (backend.PRECISION_F32, backend.PRECISION_F64)


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def inputs():
    """scans taken at the ground-truth pose (sensor frame) and three sampled maps with analytic normals"""
    scene = syn.make_scene()
    gt = syn.ground_truth_pose()
    scans = {n_az: syn.vlp16_scan(scene, gt, n_az=n_az) for n_az in (64, 192, 512)}
    clean = syn.vlp16_scan(scene, gt, n_az=512, noise_sigma=0.0)
    maps = [syn.sample_map(scene, n, seed=syn.SEED_MAP + k) for k, n in enumerate((40_000, 20_000, 5_000))]
    dense = syn.sample_map(scene, 200_000, seed=syn.SEED_MAP + 7)  # test_several_initial_guesses_for_one_pair says why
    return dict(scans=scans, clean=clean, maps=maps, dense=dense, gt=gt)


def _params(max_iter=30, method=backend.ICP_POINT_TO_PLANE, rel=1e-6):
    return B._params(R, max_iter, rel, rel, method)


def _bits(r):
    """every field of a result as bytes (NaN compares equal to itself this way)"""
    return (np.ascontiguousarray(r["transformation"]).tobytes(), struct.pack("<dd", r["fitness"], r["inlier_rmse"]), int(r["iterations"]),
            bool(r["converged"]), int(r["n_corr"]))


def _one_pair(be, e, max_iter=30, method=backend.ICP_POINT_TO_PLANE, rel=1e-6):
    s, t, crop, init = e
    return be.icp_register_dev(s, t, R, init=init, max_iter=max_iter, rel_fitness=rel, rel_rmse=rel, target_crop=crop, method=method)


def _source(be, pts):
    cid = be.upload(pts)
    if len(pts):
        be.estimate_normals(cid, 2.0, 10)  # generalized ICP builds its covariances from them
    return cid


CROP = backend.make_crop(backend.CROP_MAX_RADIUS, center=(0.3, -0.2, 0.0), rmax=12.0)
CROP2 = backend.make_crop(backend.CROP_CYLINDER, center=(0.0, 0.0, 0.0), rmax=20.0, zmin=-1.0, zmax=6.0)


def _ragged(be, inputs):
    """Sources of 3072, 127, 128, 129 and 1 points in six entries: entries 2 and 4 share the 128-point source, entries 0 and 3 share a
    target, as do 1 and 4 and 2 and 5; entries 1 and 4 carry a crop; every entry has its own initial guess."""
    gt, scans, maps = inputs["gt"], inputs["scans"], inputs["maps"]
    big = scans[192]  # 16 x 192 = 3072 points
    perm = np.random.default_rng(5).permutation(len(scans[512]))
    spread = scans[512][perm]  # a random subset is spread over the whole scan
    s1, s127, s128, s129, s3k = (_source(be, spread[:1]), _source(be, spread[:127]), _source(be, spread[:128]), _source(be, spread[:129]),
                                 _source(be, big))
    t = [be.upload(*m) for m in maps]  # no index: the batch indexes a target as the one-pair call does
    near = syn.make_pose([0.02, -0.01, 0.0], [0.0, 0.0, 0.2]) @ gt
    far = syn.make_pose([0.35, 0.25, -0.05], [1.0, -1.0, 4.0]) @ gt
    mid = syn.make_pose([-0.15, 0.1, 0.02], [0.0, 0.5, -1.5]) @ gt
    return [
        (s3k, t[0], None, near),
        (s127, t[1], CROP, mid),
        (s128, t[2], None, far),
        (s129, t[0], None, np.eye(4)),
        (s128, t[1], CROP2, gt),
        (s1, t[2], None, gt),
    ]


# ------------------------------------------------------------------------------------------------- 1. one entry = the existing call
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_entry_is_the_existing_call_and_leaves_an_armed_overlap_function_armed(inputs, precision):
    be = B(0, precision=precision)
    try:
        s = _source(be, inputs["scans"][192])
        t = be.upload(*inputs["maps"][0])
        for method in METHODS:
            for crop in (None, CROP):
                e = (s, t, crop, inputs["gt"])
                ref = _one_pair(be, e, 10, method)
                got, status = be.icp_register_batch([e], _params(10, method))
                assert status == [0] and _bits(got[0]) == _bits(ref), (method, crop is not None)
        calls = []
        cb = backend.OVERLAP_FN(lambda _arg: calls.append(1))
        assert be.lib.o3ds_icp_overlap_next(be.h, cb, None) == 0
        be.icp_register_batch([(s, t, None, None)], _params(10))
        be.icp_register_batch([(s, t, None, None), (s, t, CROP, None)], _params(10))
        assert calls == []  # not consumed by the batch, whatever its size ...
        be.icp_register_dev(s, t, R, max_iter=10)
        assert calls == [1]  # ... and still armed for the next one-pair registration
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 2. + 3. every entry, any order
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("method", METHODS)
def test_every_entry_is_its_one_pair_call_bit_for_bit_in_any_order(inputs, precision, method):
    be = B(0, precision=precision)
    try:
        entries = _ragged(be, inputs)
        refs = [_one_pair(be, e, 30, method) for e in entries]
        its = [r["iterations"] for r in refs]
        print(f"precision {precision} method {method}: one-pair iterations {its}, fitness {[round(r['fitness'], 4) for r in refs]}")
        # per-entry termination and the host's look-in cadence (after 12 passes, then every 8) are exercised
        assert min(its) < 10 and max(its) > 20 and len(set(its)) > 1, its
        got, status = be.icp_register_batch(entries, _params(30, method))
        assert status == [0] * len(entries)
        for k, (g, r) in enumerate(zip(got, refs)):
            assert _bits(g) == _bits(r), (k, g, r)
        rev, status = be.icp_register_batch(entries[::-1], _params(30, method))
        assert status == [0] * len(entries)
        assert [_bits(g) for g in rev[::-1]] == [_bits(r) for r in refs]
        again, _ = be.icp_register_batch(entries, _params(30, method))
        assert [_bits(g) for g in again] == [_bits(g) for g in got]
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 4. an entry without correspondences
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_entry_without_correspondences_is_the_one_pair_result_and_disturbs_nobody(inputs, precision):
    be = B(0, precision=precision)
    try:
        entries = _ragged(be, inputs)[:4]
        away = syn.make_pose([50.0, 0.0, 40.0], [0.0, 0.0, 0.0]) @ inputs["gt"]
        entries.insert(2, (entries[0][0], entries[0][1], None, away))
        refs = [_one_pair(be, e) for e in entries]
        assert refs[2]["fitness"] == 0.0 and refs[2]["n_corr"] == 0
        got, status = be.icp_register_batch(entries, _params())
        assert status == [0] * 5
        assert [_bits(g) for g in got] == [_bits(r) for r in refs]
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 4b. every query goes to stage 3
def far_grid_inputs():
    """A flat 64 x 64 grid (spacing 0.05 m, z = 0, normals +z) and 129 points 0.8 m above its interior: one full workgroup of 128
    queries and one with a single live query."""
    g = 0.05 * np.arange(64)
    tgt = np.stack([np.repeat(g, 64), np.tile(g, 64), np.zeros(64 * 64)], axis=1)  # x-major: rows [:2048] are the half x < 1.6
    up = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    rng = np.random.default_rng(23)
    src = np.column_stack([rng.uniform(0.8, 2.35, 129), rng.uniform(0.8, 2.35, 129), np.full(129, 0.8)])
    return tgt, up, src


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("method", (backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED))
def test_a_batch_whose_every_query_goes_to_stage_3_is_its_one_pair_calls(precision, method):
    """Pass 0 of every entry runs the workgroup-pooled stage-3 search for every query.  The index cell is r / 4 = 0.25 m for the
    correspondence distance r = 1 m, and stages 1 and 2 prove a match only within 2.5 cells = 0.625 r of the query (the stage
    description above nn_search_group in icp_kernels.hpp).  The queries start 0.8 m above the target plane and at least 0.8 m inside its
    border, and an initial guess moves no point by more than 0.09 m (rotations of at most 1 degree in total, 0.0175 rad x 3.42 m from
    the origin, and at most 0.03 m of translation), so every nearest target point is between 0.71 r and 0.9 r away: unresolved after
    stage 2, with a match inside the radius for stage 3 to find."""
    tgt, up, src = far_grid_inputs()
    be = B(0, precision=precision)
    try:
        s = be.upload(src, np.tile([0.0, 0.0, 1.0], (len(src), 1)))  # (generalized ICP builds its covariances from the normals)
        t = be.upload(tgt, up)
        inits = [syn.make_pose([0.02, -0.01, 0.01], [0.0, 0.0, 0.5]), syn.make_pose([-0.01, 0.02, -0.02], [0.5, -0.5, 0.0]),
                 syn.make_pose([0.0, 0.0, 0.02], [-0.4, 0.2, 0.4])]
        entries = [(s, t, None, T) for T in inits]
        refs = [_one_pair(be, e, 3, method, rel=0.0) for e in entries]
        assert all(r["n_corr"] > 0 and r["iterations"] == 3 for r in refs), refs
        got, status = be.icp_register_batch(entries, _params(3, method, rel=0.0))
        assert status == [0, 0, 0]
        for k, (g, r) in enumerate(zip(got, refs)):
            assert _bits(g) == _bits(r), (k, g, r)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 5. several guesses for one pair
def test_several_initial_guesses_for_one_pair(inputs):
    """Every entry is its one-pair call; the ones that reach the optimum end within 1e-3 m / rad of the ground truth (f32 storage).
    The bound needs a map whose sampling lets ANY registration get that close: the one-pair call from the ground truth itself ends
    4.3e-3 m away against a 40 000-point map (mean distance to the nearest sample 0.28 m, normals of curved surfaces taken a sample
    away), 5.0e-4 m against 200 000 points, 8.8e-5 m against 1 000 000 (measured on one MI355X, with and without range noise).  Hence
    the 200 000-point map here, and a noise-free scan (this map: 7.0e-4 m / 7.2e-5 rad for all eight guesses)."""
    be = B(0, precision=backend.PRECISION_F32)
    try:
        gt = inputs["gt"]
        s = _source(be, inputs["clean"])
        t = be.upload(*inputs["dense"])
        rng = np.random.default_rng(17)
        inits = []
        for k in range(8):  # 0 ... 0.5 m, 0 ... 5 degrees
            d = rng.normal(size=3)
            a = rng.normal(size=3)
            inits.append(syn.make_pose(0.5 * k / 7 * d / np.linalg.norm(d), 5.0 * k / 7 * a / np.linalg.norm(a)) @ gt)
        entries = [(s, t, None, T) for T in inits]
        refs = [_one_pair(be, e) for e in entries]
        got, status = be.icp_register_batch(entries, _params())
        assert status == [0] * 8
        assert [_bits(g) for g in got] == [_bits(r) for r in refs]
        n = len(inputs["clean"])
        ok = 0
        for k, g in enumerate(got):
            dt, dr = syn.se3_error(g["transformation"], gt)
            print(f"guess {k}: iterations {g['iterations']} converged {g['converged']} fitness {g['fitness']:.4f} |dt| {dt:.3e} m angle {dr:.3e} rad")
            # "converged": reached the optimum of the unperturbed guess (the same correspondences up to the fitness tolerance)
            if abs(g["fitness"] - got[0]["fitness"]) <= 4.0 / n:
                ok += 1
                assert dt <= 1e-3 and dr <= 1e-3, (k, dt, dr)
        assert ok >= 4, ok  # the unperturbed guess and the small perturbations at least
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 6. against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_batch_against_the_oracles_registrations(inputs, oracle, precision):
    tol = 1e-6 if precision == backend.PRECISION_F64 else 1e-3
    gt, scans, maps = inputs["gt"], inputs["scans"], inputs["maps"]
    pairs = [(scans[192], maps[0], syn.make_pose([0.05, 0.0, 0.0], [0.0, 0.0, 0.5]) @ gt), (scans[64], maps[1], gt),
             (scans[192][:129], maps[0], np.eye(4))]
    be = B(0, precision=precision)
    try:
        entries = [(be.upload(src), be.upload(*m), None, T) for src, m, T in pairs]
        for method in (backend.ICP_POINT_TO_PLANE, backend.ICP_POINT_TO_POINT):
            got, status = be.icp_register_batch(entries, _params(10, method, rel=0.0))
            assert status == [0, 0, 0]
            for (src, (tp, tn), T), g in zip(pairs, got):
                if method == backend.ICP_POINT_TO_PLANE:
                    ref = oracle.icp_point_to_plane(src, tp, tn, R, init=T, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
                else:
                    ref = oracle.icp_point_to_point(src, tp, R, init=T, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
                dt, dr = syn.se3_error(g["transformation"], ref["transformation"])
                print(f"method {method} n_src {len(src)}: |dt| {dt:.3e} angle {dr:.3e} fitness {g['fitness']:.5f}/{ref['fitness']:.5f} "
                      f"rmse {g['inlier_rmse']:.6f}/{ref['inlier_rmse']:.6f}")
                assert g["iterations"] == 10
                assert dt <= tol and dr <= tol, (dt, dr)
                assert abs(g["fitness"] - ref["fitness"]) <= 4.0 / len(src)
                assert abs(g["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-12)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 7. errors
def test_error_conventions(inputs):
    be = B(0)
    other = B(0)
    try:
        gt = inputs["gt"]
        s = _source(be, inputs["scans"][64])
        t = be.upload(*inputs["maps"][2])
        bare = be.upload(inputs["maps"][2][0])  # no normals
        empty = be.upload(np.zeros((0, 3)))
        foreign = other.upload(inputs["scans"][64])
        for _ in range(8):  # ids of `other` beyond the ones `be` has handed out
            foreign = other.upload(inputs["scans"][64][:4])
        assert be.lib.o3ds_set_precision(be.h, backend.PRECISION_F64) == 0
        s64 = be.upload(inputs["scans"][64])
        assert be.lib.o3ds_set_precision(be.h, backend.PRECISION_F32) == 0
        huge = be.upload(np.zeros((262_145, 3)))
        wide = be.upload(np.zeros((140_000, 3)))  # 64 x ceil(140 000 / 128) = 70 016 workgroups > 65 536
        ok = (s, t, None, gt)
        ref = _bits(_one_pair(be, ok))

        def refused(entries, code, params=None):
            with pytest.raises(backend.BackendError) as e:
                be.icp_register_batch(entries, params if params is not None else _params())
            assert e.value.code == code, (code, e.value)
            assert be.lib.o3ds_last_error(be.h)
            got, status = be.icp_register_batch([ok, ok], _params())  # the handle still registers correctly
            assert status == [0, 0] and _bits(got[0]) == ref and _bits(got[1]) == ref

        refused([], backend.ERR_INVALID_ARG)
        refused([ok] * 65, backend.ERR_INVALID_ARG)
        refused([ok, (foreign, t, None, gt)], backend.ERR_INVALID_ARG)
        refused([ok, (s, foreign, None, gt)], backend.ERR_INVALID_ARG)
        refused([ok, (10**12, t, None, gt)], backend.ERR_INVALID_ARG)
        refused([ok, (s, bare, None, gt)], backend.ERR_INVALID_ARG)                # point-to-plane needs the target's normals
        refused([ok, (s64, t, None, gt)], backend.ERR_INVALID_ARG)                # precision mismatch
        refused([ok, ok], backend.ERR_INVALID_ARG, B._params(0.0, 30, 1e-6, 1e-6))  # max_correspondence_distance <= 0
        refused([ok, (huge, t, None, gt)], backend.ERR_CAPACITY)
        refused([(wide, t, None, gt)] * 64, backend.ERR_CAPACITY)
        # null pointers, through the raw entry point
        p = _params()
        arr = (backend.IcpBatchEntry * 2)()
        out = (backend.IcpResult * 2)()
        st = (C.c_int * 2)()
        for args in ((None, 2, C.byref(p), out, st), (arr, 2, None, out, st), (arr, 2, C.byref(p), None, st), (arr, 2, C.byref(p), out, None)):
            assert be.lib.o3ds_icp_register_batch(be.h, *args) == backend.ERR_INVALID_ARG
            assert be.lib.o3ds_last_error(be.h)
        # the bare target is fine for point-to-point
        got, status = be.icp_register_batch([ok, (s, bare, None, gt)], _params(method=backend.ICP_POINT_TO_POINT))
        assert status == [0, 0]
        # an empty target in entry 1 of 3: skipped, zeroed, the others run
        e2 = (s, t, CROP, np.eye(4))
        got, status = be.icp_register_batch([ok, (s, empty, None, gt), e2], _params())
        assert status == [0, backend.ERR_EMPTY, 0]
        assert _bits(got[0]) == ref and _bits(got[2]) == _bits(_one_pair(be, e2))
        assert got[1]["n_corr"] == 0 and got[1]["iterations"] == 0 and not got[1]["transformation"].any()
        with pytest.raises(backend.BackendError) as e:
            _one_pair(be, (s, empty, None, gt))
        assert e.value.code == backend.ERR_EMPTY
        # 64 tiny entries run
        tiny = [(be.upload(inputs["scans"][64][k:k + 1 + k % 3]), t, None, gt) for k in range(64)]
        got, status = be.icp_register_batch(tiny, _params(5))
        assert status == [0] * 64
        for k in (0, 1, 31, 63):
            assert _bits(got[k]) == _bits(_one_pair(be, tiny[k], 5)), k
        refused(tiny + [ok], backend.ERR_INVALID_ARG)
    finally:
        be.close()
        other.close()


# ------------------------------------------------------------------------------------------------- 8. loop-closure wiring
RADIUS = 2.0
FRAMES = 125  # the figure-eight passes its start again near frame 109


class _Recorder:
    """a thin wrapper around a Backend: counts the calls by name"""

    def __init__(self, be):
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "calls", {})

    def __getattr__(self, name):
        v = getattr(self._be, name)
        if not callable(v) or name.startswith("_"):
            return v

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return v(*a, **k)

        return counted

    def __setattr__(self, name, value):
        setattr(self._be, name, value)


@pytest.fixture(scope="module")
def stream():
    scene = syn.make_scene()
    poses = syn.figure_eight_poses(200, 0.1)
    return [np.asarray(syn.os128_scan(scene, poses[k], frame=k, n_az=512), dtype=np.float32) for k in range(FRAMES)]


def _cycle(scans, batch, refine_odometry, record=False):
    """the figure-eight with the loop-closure cycle after every frame until the first cycle that closes a loop"""
    import bench
    from open3d_slam_amd.loop_closure import LoopClosure
    from open3d_slam_amd.mapper import Mapper
    from open3d_slam_amd.odometry import LidarOdometry
    from open3d_slam_amd.pointcloud import PointCloud
    from open3d_slam_amd.submap_collection import SubmapCollection, computeOdometryConstraints

    mp, op = bench.stream_parameters()
    mp.submaps_.radius_ = RADIUS
    mp.isBuildDenseMap_ = False
    mp.isAttemptLoopClosures_ = True
    mp.isRefineOdometryConstraintsBetweenSubmaps_ = refine_odometry
    mp.placeRecognition_.loopClosureSearchRadius_ = 2.0 * RADIUS
    raw = backend.Backend(0)
    be = _Recorder(raw) if record else raw
    odo = LidarOdometry(be)
    odo.setParameters(op)
    mapper = Mapper(be, odo, submaps=SubmapCollection(be))
    mapper.setParameters(mp)
    lc = LoopClosure(be, mapper, batchRegistrations=True) if batch else LoopClosure(be, mapper)
    out = dict(be=raw, constraints=[], closed_at=None, calls=getattr(be, "calls", {}))
    for k, scan in enumerate(scans):
        cloud = PointCloud.from_pointcloud2(be, scan)
        try:
            assert odo.addRangeScan(cloud, 0.1 * k) and mapper.addRangeMeasurement(cloud, 0.1 * k), k
        finally:
            cloud.release()
        cs = lc.run()
        if cs:
            out.update(constraints=cs, closed_at=k)
            break
    coll = mapper.getSubmaps()
    out["odometry"] = list(coll.getOdometryConstraints())
    every = []
    computeOdometryConstraints(be, coll, every, **({"batch": True} if batch else {}))
    out["every_pair"] = every
    out["coll"] = coll
    return out


def _same_constraints(a, b):
    assert [(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in a] == [(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in b]
    for c1, c2 in zip(a, b):
        assert np.asarray(c1.sourceToTarget_).tobytes() == np.asarray(c2.sourceToTarget_).tobytes()
        assert np.asarray(c1.informationMatrix_).tobytes() == np.asarray(c2.informationMatrix_).tobytes()
        assert c1.isOdometryConstraint_ == c2.isOdometryConstraint_ and c1.isInformationMatrixValid_ == c2.isInformationMatrixValid_


def test_loop_closure_wiring_gives_the_sequential_constraints(stream):
    seq = _cycle(stream, False, True, record=True)
    bat = _cycle(stream, True, True, record=True)
    try:
        assert seq["closed_at"] is not None and seq["closed_at"] == bat["closed_at"]
        print(f"loop closed at frame {seq['closed_at']}: {[(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in seq['constraints']]}; "
              f"{len(seq['odometry'])} + {len(seq['every_pair'])} odometry constraints")
        _same_constraints(seq["constraints"], bat["constraints"])
        assert len(seq["odometry"]) >= 2 and len(seq["every_pair"]) >= 2
        _same_constraints(seq["odometry"], bat["odometry"])
        _same_constraints(seq["every_pair"], bat["every_pair"])  # computeOdometryConstraints(batch=True), refinement on
        # flag off: the calls of today -- one ICP per constraint, never the batch; flag on: the ICPs of the constraints went through it
        assert "icp_register_batch" not in seq["calls"]
        assert bat["calls"].get("icp_register_batch", 0) >= 2
        n_icp = lambda c: c.get("icp_point_to_plane_dev", 0) + c.get("icp_generalized_dev", 0) + c.get("icp_point_to_point_dev", 0)
        assert n_icp(seq["calls"]) > n_icp(bat["calls"])
        for name in ("overlap_indices", "information_matrix_dev", "ransac_feature_matching", "select_by_index"):
            assert seq["calls"].get(name, 0) == bat["calls"].get(name, 0) > 0, name
        # several candidates at once: the finished submaps with features against the latest one, both forms on the same collection
        coll = seq["coll"]
        pr = coll.placeRecognition_
        finished = [i for i, sm in enumerate(coll.submaps_) if i != coll.activeSubmapIdx_ and sm.sparseMapCloud_ is not None]
        assert len(finished) >= 3, finished
        src, cands = finished[-1], finished[:-1]
        pr.batchRefinement = False
        one = pr.buildLoopClosureConstraints(coll.submaps_[src], [coll.submaps_[i] for i in cands], sourceSubmapIdx=src, candidateIdxs=cands)
        pr.batchRefinement = True
        two = pr.buildLoopClosureConstraints(coll.submaps_[src], [coll.submaps_[i] for i in cands], sourceSubmapIdx=src, candidateIdxs=cands)
        pr.batchRefinement = False
        print(f"source {src} against candidates {cands}: {[(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in one]}")
        _same_constraints(one, two)
    finally:
        seq["be"].close()
        bat["be"].close()
