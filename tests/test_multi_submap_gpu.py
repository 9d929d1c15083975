"""o3ds_icp_register_multi on the device: one target is the existing call bit for bit, UNION is the registration against the appended and
indexed copy, JOINT sums exact per-target records, configs[3] at its stated shape (8 x 1 M-point maps), the crop as a predicate,
determinism, the error conventions and the Mapper wiring.  Tolerances are DESIGN.md section 2's (f64 storage 1e-6 m / rad, f32 1e-3,
fitness +-4/n, rmse rel 1e-3)."""
import numpy as np
import pytest

from open3d_slam_amd import backend
from open3d_slam_amd import synthetic as syn

from multi_submap_restatement import register_multi

pytestmark = pytest.mark.gpu

B = backend.Backend
UNION, JOINT = B.MULTI_UNION, B.MULTI_JOINT
R = 1.0


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def scene_inputs():
    scene = syn.make_scene()
    src = syn.vlp16_scan(scene, syn.ground_truth_pose(), n_az=512)
    maps = [syn.sample_map(scene, n, seed=syn.SEED_MAP + k) for k, n in enumerate((60_000, 35_000, 50_000, 20_000, 45_000, 30_000, 25_000, 40_000))]
    return src, maps


def _params(max_iter=10, method=backend.ICP_POINT_TO_PLANE, fixed=True):
    return B._params(R, max_iter, 0.0 if fixed else 1e-6, 0.0 if fixed else 1e-6, method)


def _target(be, pts, nrm):
    cid = be.upload(pts, nrm)
    if len(pts):
        be.build_index(cid, R)
    return cid


def _appended(be, ids):
    """the targets appended in slot order into a fresh cloud, indexed: what UNION is defined against"""
    full = [cid for cid in ids if be.size(cid)[0] > 0]  # (an empty target contributes nothing to the copy either)
    cat = be.crop_cloud(full[0], backend.make_crop(backend.CROP_MAX_RADIUS, rmax=1e9))  # a copy of the first: everything is inside
    assert be.size(cat) == be.size(full[0])
    for cid in full[1:]:
        be.cloud_append(cat, cid)
    be.build_index(cat, R)
    return cat


def _bits(r):
    return (r["transformation"].tobytes(), r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"], r["n_corr"])


def _close(got, ref, n, tol):
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    print(f"  |dt| {dt:.3e} m  angle {dr:.3e} rad  fitness {got['fitness']:.6f}/{ref['fitness']:.6f}  rmse {got['inlier_rmse']:.6f}/{ref['inlier_rmse']:.6f}")
    assert dt <= tol and dr <= tol, (dt, dr)
    assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / n
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-12)


# ------------------------------------------------------------------------------------------------- 4. one target = the existing call
@pytest.mark.parametrize("precision", [backend.PRECISION_F32, backend.PRECISION_F64])
def test_one_target_is_the_existing_call_bit_for_bit(scene_inputs, precision):
    src, maps = scene_inputs
    be = B(0, precision=precision)
    try:
        s = be.upload(src)
        be.estimate_normals(s, 2.0, 10)
        t = _target(be, *maps[0])
        crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=(0.3, -0.2, 0.0), rmax=12.0)
        for method in (backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED, backend.ICP_POINT_TO_POINT):
            for c in (None, crop):
                ref = be.icp_register_dev(s, t, R, max_iter=10, rel_fitness=1e-6, rel_rmse=1e-6, target_crop=c, method=method)
                for form in (UNION, JOINT):
                    got = be.icp_register_multi(s, [t], form=form, crop=c, params=_params(10, method, fixed=False))
                    assert _bits(got) == _bits(ref), (method, c is not None, form)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 5. UNION = the concatenation
@pytest.mark.parametrize("precision", [backend.PRECISION_F64, backend.PRECISION_F32])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_union_is_the_registration_against_the_appended_copy(scene_inputs, oracle, precision, k):
    src, maps = scene_inputs
    maps = list(maps[:k])
    maps.insert(1, (np.zeros((0, 3)), np.zeros((0, 3))))       # an empty target
    maps.append((maps[0][0][:1] + 0.123, maps[0][1][:1]))      # a one-point target
    maps = maps[:backend.Backend.MULTI_MAX_TARGETS]
    be = B(0, precision=precision)
    try:
        s = be.upload(src)
        ids = [_target(be, *m) for m in maps]
        cat = _appended(be, ids)
        ref = be.icp_register_dev(s, cat, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        got = be.icp_register_multi(s, ids, form=UNION, params=_params())
        print(f"k={k} precision={precision}: n_corr {got['n_corr']}/{ref['n_corr']}  iterations {got['iterations']}/{ref['iterations']}")
        assert got["iterations"] == ref["iterations"] == 10
        assert got["n_corr"] == ref["n_corr"]
        if precision == backend.PRECISION_F64:
            assert _bits(got) == _bits(ref)  # exact, order-free sums over the same correspondences
        else:
            _close(got, ref, len(src), 1e-3)
        # the CPU restatement (tests/test_multi_submap_cpu.py checks it against the oracle's own registration)
        host = register_multi(oracle, "union", src, maps, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        assert got["iterations"] == host["iterations"]
        _close(got, host, len(src), 1e-6 if precision == backend.PRECISION_F64 else 1e-3)
        # slot order permuted: the same correspondences (no ties between continuous samples), the same pose within tolerance
        perm = be.icp_register_multi(s, ids[::-1], form=UNION, params=_params())
        assert perm["n_corr"] == got["n_corr"] and perm["iterations"] == got["iterations"]
        _close(perm, got, len(src), 1e-6 if precision == backend.PRECISION_F64 else 1e-3)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 6. JOINT
@pytest.mark.parametrize("precision", [backend.PRECISION_F64, backend.PRECISION_F32])
@pytest.mark.parametrize("method", [backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED, backend.ICP_POINT_TO_POINT])
def test_joint_over_copies_of_one_cloud_is_the_one_target_pose_bit_for_bit(scene_inputs, precision, method):
    src, maps = scene_inputs
    be = B(0, precision=precision)
    try:
        s = be.upload(src)
        be.estimate_normals(s, 2.0, 10)
        t = _target(be, *maps[0])
        ref = be.icp_register_dev(s, t, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0, method=method)
        for k in (2, 4, 8):
            got = be.icp_register_multi(s, [t] * k, form=JOINT, params=_params(10, method))
            assert got["transformation"].tobytes() == ref["transformation"].tobytes(), (k, method)
            assert (got["fitness"], got["inlier_rmse"], got["iterations"]) == (ref["fitness"], ref["inlier_rmse"], ref["iterations"]), k
            assert got["n_corr"] == k * ref["n_corr"]
    finally:
        be.close()


@pytest.mark.parametrize("precision", [backend.PRECISION_F64, backend.PRECISION_F32])
def test_joint_over_three_maps_is_the_host_restatement(scene_inputs, oracle, precision):
    src, maps = scene_inputs
    maps = maps[:3]
    be = B(0, precision=precision)
    try:
        s = be.upload(src)
        ids = [_target(be, *m) for m in maps]
        got = be.icp_register_multi(s, ids, form=JOINT, params=_params())
        host = register_multi(oracle, "joint", src, maps, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        assert got["iterations"] == host["iterations"] == 10
        _close(got, host, 3 * len(src), 1e-6 if precision == backend.PRECISION_F64 else 1e-3)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 7. configs[3] at its stated shape
def test_configs3_eight_maps_of_a_million_points():
    scene = syn.make_scene()
    src, tgt0, nrm0, T_gt = syn.config2_inputs(n_map=1_000_000, n_az=4096)
    assert len(src) == 65_536
    be = B(0)
    try:
        s = be.upload(src)
        ids = [_target(be, tgt0, nrm0)] + [_target(be, *syn.sample_map(scene, 1_000_000, seed=syn.SEED_MAP + k)) for k in range(1, 8)]
        joint = be.icp_register_multi(s, ids, form=JOINT, params=_params())
        dt, dr = syn.se3_error(joint["transformation"], T_gt)
        print(f"configs[3] JOINT: |dt| {dt:.3e} m angle {dr:.3e} rad fitness {joint['fitness']:.4f} rmse {joint['inlier_rmse']:.4f}")
        assert dt < 5e-3 and dr < 1e-3, (dt, dr)
        assert joint["iterations"] == 10
        union = be.icp_register_multi(s, ids, form=UNION, params=_params())
        cat = _appended(be, ids)
        assert be.size(cat)[0] == 8_000_000
        ref = be.icp_register_dev(s, cat, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        print(f"configs[3] UNION: n_corr {union['n_corr']}/{ref['n_corr']}")
        assert union["iterations"] == ref["iterations"] == 10 and union["n_corr"] == ref["n_corr"]
        _close(union, ref, len(src), 1e-3)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 8. the crop is a predicate
@pytest.mark.parametrize("precision", [backend.PRECISION_F64, backend.PRECISION_F32])
def test_union_under_a_crop_is_the_registration_against_the_cropped_targets(scene_inputs, precision):
    src, maps = scene_inputs
    # three targets: two halves of the scene that the ball cuts through, and a far corner it does not reach
    p0, n0 = maps[0]
    west, east = p0[:, 0] < 0.0, p0[:, 0] >= 0.0
    p2, n2 = maps[2]
    far = np.linalg.norm(p2[:, :2] - [0.3, -0.2], axis=1) > 14.0
    parts = [(p0[west], n0[west]), (p0[east], n0[east]), (p2[far], n2[far])]
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=(0.3, -0.2, 0.0), rmax=9.0)
    be = B(0, precision=precision)
    try:
        s = be.upload(src)
        ids = [_target(be, *m) for m in parts]
        cropped = [be.crop_cloud(cid, crop) for cid in ids]
        sizes = [be.size(c)[0] for c in cropped]
        assert 0 < sizes[0] < len(parts[0][0]) and 0 < sizes[1] < len(parts[1][0]) and sizes[2] == 0, sizes
        cat = _appended(be, cropped)
        ref = be.icp_register_dev(s, cat, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        got = be.icp_register_multi(s, ids, form=UNION, crop=crop, params=_params())
        assert got["iterations"] == ref["iterations"] == 10 and got["n_corr"] == ref["n_corr"]
        if precision == backend.PRECISION_F64:
            assert _bits(got) == _bits(ref)
        else:
            _close(got, ref, len(src), 1e-3)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 8b. every query goes to stage 3
def _far_grid_inputs():
    """A flat 64 x 64 grid (spacing 0.05 m, z = 0, normals +z) and 129 points 0.8 m above its interior: one full workgroup of 128
    queries and one with a single live query."""
    g = 0.05 * np.arange(64)
    tgt = np.stack([np.repeat(g, 64), np.tile(g, 64), np.zeros(64 * 64)], axis=1)  # x-major: rows [:2048] are the half x < 1.6
    up = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    rng = np.random.default_rng(23)
    src = np.column_stack([rng.uniform(0.8, 2.35, 129), rng.uniform(0.8, 2.35, 129), np.full(129, 0.8)])
    return tgt, up, src


@pytest.mark.parametrize("precision", [backend.PRECISION_F64, backend.PRECISION_F32])
@pytest.mark.parametrize("method", [backend.ICP_POINT_TO_PLANE, backend.ICP_GENERALIZED])
def test_both_forms_when_every_query_goes_to_stage_3(precision, method):
    """Pass 0 runs the workgroup-pooled stage-3 search for every query, in every slot.  The index cell is r / 4 = 0.25 m for the
    correspondence distance r = 1 m, and stages 1 and 2 prove a match only within 2.5 cells = 0.625 r of the query (the stage
    description above nn_search_group in icp_kernels.hpp).  The queries start 0.8 m above the target plane and at least 0.8 m inside its
    border, and the initial guess moves no point by more than 0.09 m (a rotation of 1 degree in total, 0.0175 rad x 3.42 m from the
    origin, and 0.03 m of translation at most), so every nearest target point is between 0.71 r and 0.9 r away: unresolved after
    stage 2, with a match inside the radius for stage 3 to find.  The same holds in each half of the grid for the queries above it; a
    query above the other half finds nothing or a farther point there, also in stage 3.
    JOINT over two copies of the grid is the one-target pose bit for bit; UNION over the two halves is the registration against the
    appended copy, compared as test_union_is_the_registration_against_the_appended_copy compares."""
    tgt, up, src = _far_grid_inputs()
    init = syn.make_pose([0.02, -0.01, 0.01], [0.5, -0.5, 0.0])
    be = B(0, precision=precision)
    try:
        s = be.upload(src, np.tile([0.0, 0.0, 1.0], (len(src), 1)))  # (generalized ICP builds its covariances from the normals)
        t = _target(be, tgt, up)
        ref = be.icp_register_dev(s, t, R, init=init, max_iter=3, rel_fitness=0.0, rel_rmse=0.0, method=method)
        assert ref["iterations"] == 3 and ref["n_corr"] > 0, ref
        got = be.icp_register_multi(s, [t, t], form=JOINT, init=init, params=_params(3, method))
        assert got["transformation"].tobytes() == ref["transformation"].tobytes()
        assert (got["fitness"], got["inlier_rmse"], got["iterations"]) == (ref["fitness"], ref["inlier_rmse"], ref["iterations"])
        assert got["n_corr"] == 2 * ref["n_corr"]
        halves = [_target(be, tgt[:2048], up[:2048]), _target(be, tgt[2048:], up[2048:])]
        cat = _appended(be, halves)
        ref = be.icp_register_dev(s, cat, R, init=init, max_iter=3, rel_fitness=0.0, rel_rmse=0.0, method=method)
        got = be.icp_register_multi(s, halves, form=UNION, init=init, params=_params(3, method))
        print(f"precision={precision} method={method}: n_corr {got['n_corr']}/{ref['n_corr']}  iterations {got['iterations']}/{ref['iterations']}")
        assert got["iterations"] == ref["iterations"] == 3
        assert got["n_corr"] == ref["n_corr"] > 0
        if precision == backend.PRECISION_F64:
            assert _bits(got) == _bits(ref)  # exact, order-free sums over the same correspondences
        else:
            _close(got, ref, len(src), 1e-3)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("form", [UNION, JOINT])
def test_the_same_call_gives_the_same_bits(scene_inputs, form):
    src, maps = scene_inputs
    be, be2 = B(0), B(0)
    try:
        everything = backend.make_crop(backend.CROP_MAX_RADIUS, center=(0.0, 0.0, 0.0), rmax=1e3)
        out = []
        for b in (be, be2):
            raw = b.upload(src)
            ids = [_target(b, *m) for m in maps[:3]]
            lazy = b.crop_voxel_down_sample(raw, everything, 0.05)  # its size is still in flight when the registration is queued
            first = b.icp_register_multi(lazy, ids, form=form, params=_params())
            known = b.crop_voxel_down_sample(raw, everything, 0.05)
            assert b.size(known)[0] > 1000
            out += [first, b.icp_register_multi(known, ids, form=form, params=_params()),
                    b.icp_register_multi(known, ids, form=form, params=_params())]
        assert len({_bits(r) for r in out}) == 1, [r["transformation"][:3, 3] for r in out]
    finally:
        be.close()
        be2.close()


# ------------------------------------------------------------------------------------------------- 10. errors
def test_errors_follow_the_conventions_and_leave_the_handle_usable(scene_inputs):
    import ctypes as C

    src, maps = scene_inputs
    be, other = B(0), B(0)
    try:
        s = be.upload(src)
        t = [_target(be, *m) for m in maps[:2]]
        usual = be.icp_register_dev(s, t[0], R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        no_index = be.upload(*maps[2])
        no_normals = be.upload(maps[2][0])
        be.build_index(no_normals, R)
        for _ in range(40):
            foreign = other.upload(maps[3][0][:10])  # an id this handle has never handed out
        big = be.upload(np.zeros((262_145, 3)))
        cases = [
            (dict(targets=[]), backend.ERR_INVALID_ARG),
            (dict(targets=[t[0]] * 17), backend.ERR_INVALID_ARG),
            (dict(targets=[t[0], no_index]), backend.ERR_INVALID_ARG),
            (dict(targets=[t[0], no_normals]), backend.ERR_INVALID_ARG),
            (dict(targets=[t[0], foreign]), backend.ERR_INVALID_ARG),
            (dict(targets=t, form=7), backend.ERR_INVALID_ARG),
            (dict(targets=t, source=big), backend.ERR_CAPACITY),
        ]
        for kw, code in cases:
            with pytest.raises(backend.BackendError) as e:
                be.icp_register_multi(kw.get("source", s), kw["targets"], form=kw.get("form", UNION), params=_params())
            assert e.value.code == code, (kw, e.value)
            assert _bits(be.icp_register_dev(s, t[0], R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)) == _bits(usual)
        # JOINT: n_targets * ceil(n_src / 128) <= 4096 workgroup records
        wide = be.upload(np.zeros((40_000, 3)))
        with pytest.raises(backend.BackendError) as e:
            be.icp_register_multi(wide, [t[0]] * 16, form=JOINT, params=_params())
        assert e.value.code == backend.ERR_CAPACITY
        # a null list
        out, p = backend.IcpResult(), _params()
        rc = be.lib.o3ds_icp_register_multi(be.h, UNION, s, None, 2, None, backend._IDENTITY16, C.byref(p), C.byref(out))
        assert rc == backend.ERR_INVALID_ARG
        # an empty target is legal; point-to-point needs no normals
        empty = be.upload(np.zeros((0, 3)))
        assert be.icp_register_multi(s, [t[0], empty, t[1]], form=UNION, params=_params())["n_corr"] > 0
        assert be.icp_register_multi(s, [t[0], no_normals], form=UNION, params=_params(10, backend.ICP_POINT_TO_POINT))["n_corr"] > 0
        assert _bits(be.icp_register_dev(s, t[0], R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)) == _bits(usual)
    finally:
        be.close()
        other.close()


# ------------------------------------------------------------------------------------------------- 11. the Mapper
def _run_mapper(scans, frames, num=None, probe=False):
    import bench
    from open3d_slam_amd.mapper import Mapper
    from open3d_slam_amd.odometry import LidarOdometry
    from open3d_slam_amd.pointcloud import PointCloud
    from open3d_slam_amd.submap_collection import SubmapCollection

    mp, op = bench.stream_parameters()
    mp.submaps_.radius_ = 2.0
    mp.isBuildDenseMap_ = False
    mp.isAttemptLoopClosures_ = False
    be = B(0)
    try:
        odo = LidarOdometry(be)
        odo.setParameters(op)
        coll = SubmapCollection(be)
        mapper = Mapper(be, odo, submaps=coll) if num is None else Mapper(be, odo, submaps=coll, numSubmapsForScanMatching=num)
        mapper.setParameters(mp)
        poses, probes, switched = [], [], False
        for k in range(frames):
            cloud = PointCloud.from_pointcloud2(be, scans[k])
            try:
                if probe and switched:  # the first frame after a switch: a zero-iteration evaluation under the current pose
                    T = mapper.getMapToRangeSensor()
                    proc = mapper.scan2MapReg_.processForScanMatchingAndMerging(cloud, T)
                    subs = coll.getSubmapsForScanMatching(3)
                    mapper.scan2MapReg_.scanToMultiMapRegistration(proc.match_, subs, T, T)  # (indexes the finished submaps' maps)
                    ids = [x.getMapPointCloud().id for x in subs]
                    p0 = B._params(mp.scanMatcher_.icp_.maxCorrespondenceDistance_, 0, 0.0, 0.0)
                    many = be.icp_register_multi(proc.match_.id, ids, form=UNION, init=T, params=p0)
                    one = be.icp_register_multi(proc.match_.id, ids[:1], form=UNION, init=T, params=p0)
                    probes.append((len(ids), many["n_corr"], one["n_corr"]))
                    Mapper._release(proc)
                before = coll.activeSubmapIdx_
                assert odo.addRangeScan(cloud, 0.1 * k) and mapper.addRangeMeasurement(cloud, 0.1 * k), k
                switched = coll.activeSubmapIdx_ != before
            finally:
                cloud.release()
            poses.append(mapper.getMapToRangeSensor().copy())
        return poses, probes, coll.getNumSubmaps()
    finally:
        be.close()


def test_the_mapper_with_one_submap_is_unchanged_and_three_submaps_never_lose_an_inlier():
    scene = syn.make_scene()
    truth = syn.figure_eight_poses(200, 0.1)
    frames = 70
    scans = [np.asarray(syn.os128_scan(scene, truth[k], frame=k), dtype=np.float32) for k in range(frames)]
    base, _, n_sub = _run_mapper(scans, frames)
    one, _, _ = _run_mapper(scans, frames, num=1)
    assert n_sub >= 3, n_sub
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base, one))
    three, probes, _ = _run_mapper(scans, frames, num=3, probe=True)
    assert len(three) == frames and probes, probes
    for n_ids, many, single in probes:
        print(f"first frame after a switch: {n_ids} submaps, correspondences {many} against {single} for the active submap alone")
        assert many >= single  # a superset of target points under the same pose cannot lose an inlier
    assert any(n_ids > 1 for n_ids, _, _ in probes)
    rel = [np.linalg.inv(truth[0]) @ t for t in truth]  # the map frame is the first scan's
    err1 = max(syn.se3_error(a, b)[0] for a, b in zip(base, rel))
    err3 = max(syn.se3_error(a, b)[0] for a, b in zip(three, rel))
    print(f"largest position error over {frames} frames: 1 submap {err1:.4f} m, 3 submaps {err3:.4f} m (recorded, not asserted)")
