"""Voxel Gaussians and the search-free (NDT) step and registration on the device against the numpy restatement
(tests/ndt_restatement.py): the Gaussians and the record of one step bit for bit, independence of the lookup, the registration at the
project's parity tolerance and within the pose bound, reproducibility, and every error code.  Both storages; needs an
MI355X.

The cases and what each is there for are in ndt_restatement; their premises are asserted without a device in
tests/test_ndt_restatement_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_restatement as nr  # noqa: E402
from ndt_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, synthetic as syn  # noqa: E402
from open3d_slam_amd import cloud_registration as creg  # noqa: E402
from open3d_slam_amd.parameters import CloudRegistrationParameters  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN_NDT_BUILD, SPAN_NDT_STEP = 18, 19
BUILD = (nr.VOXEL, nr.MIN_POINTS, nr.RATIO)
KERNELS = {nr.L2: lambda k: creg.L2Loss(), nr.CAUCHY: creg.CauchyLoss, nr.TUKEY: creg.TukeyLoss}


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


@pytest.fixture(scope="module")
def room(handles):
    """per storage: the Gaussians of the shifted noisy room, made from a cloud that is freed at once (they are a snapshot)"""
    ids = {}
    for storage, be in handles.items():
        c = be.upload(nr.target("room", True))
        ids[storage], _ = be.voxel_gaussians_create(c, *BUILD)
        be.free(c)
    yield ids
    for storage, be in handles.items():
        be.voxel_gaussians_free(ids[storage])


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint64).ravel() != want.view(np.uint64).ravel())
    assert len(bad) == 0, f"{what}: entries {bad.tolist()[:16]} differ: got {got.ravel()[bad][:16]}, restated {want.ravel()[bad][:16]}"


def _same_gaussians(be, gid, info, want: nr.Gaussians, what):
    assert info == want.info and be.voxel_gaussians_info(gid) == dict(want.info, voxel_size=want.voxel_size), (what, info, want.info)
    got = be.voxel_gaussians_download(gid)
    assert (got["keys"] == want.keys).all() and (got["counts"] == want.counts).all() and (got["valid"] == want.valid).all(), what
    for name in ("mean", "cov", "information"):
        _same_bits(got[name], getattr(want, name), (what, name))


# ---------------------------------------------------------------------------------------------------------------- 1. the Gaussians
@pytest.mark.parametrize("storage", nr.STORAGES)
def test_gaussians_are_the_restated_ones_bit_for_bit(handles, storage):
    be = handles[storage]
    for what, pts, want in (("room", nr.target("room", True), nr.reference_gaussians("room", True, storage)),
                            ("edge", nr.edge_cloud(), nr.voxel_gaussians(nr.edge_cloud(), *BUILD, storage))):
        c = be.upload(pts)
        be.profile_enable(2)
        try:
            gid, info = be.voxel_gaussians_create(c, *BUILD)
            assert be.span_read(SPAN_NDT_BUILD)[0] == 1
        finally:
            be.profile_enable(0)
        try:
            _same_gaussians(be, gid, info, want, (what, storage))
        finally:
            be.voxel_gaussians_free(gid)
            be.free(c)
    assert want.info["n_flat"] == 1 and want.info["n_skipped_points"] == 5  # (the edge cloud's, asserted in full without a device)


# ---------------------------------------------------------------------------------------------------------------- 2. the step
@pytest.mark.parametrize("storage", nr.STORAGES)
@pytest.mark.parametrize("n", nr.STEP_SIZES)
def test_step_record_is_the_restated_one_bit_for_bit(handles, room, n, storage):
    be = handles[storage]
    q = be.upload(nr.source("room", True, n))
    try:
        for nb in nr.NEIGHBOURHOODS:
            for kind, k in nr.STEP_LOSSES:
                got = be.ndt_step(q, room[storage], nb, (kind, k), T=nr.step_pose("room"))
                _same_bits(got, nr.reference_step("room", True, n, nb, kind, k, storage), (n, nb, nr.LOSS_NAMES[kind], storage))
                assert n < 255 or got[28] > 0.9 * n
    finally:
        be.free(q)


@pytest.mark.parametrize("storage", nr.STORAGES)
def test_step_with_a_point_outside_every_voxel_and_a_nan_point(handles, room, storage):
    be = handles[storage]
    src = np.array(nr.source("room", True, 257))
    src[3] = (100.0, 100.0, 100.0)
    src[200] = (np.nan, 1.0, 1.0)
    src[201] = (1.0, 1.0, 3e7)  # beyond 2^20 voxels
    q = be.upload(src)
    try:
        terms = nr.step_terms(src, nr.reference_gaussians("room", True, storage), nr.step_pose("room"), 7, nr.CAUCHY, 1.0, storage)
        assert (terms[[3, 200, 201]] == 0).all() and terms[:, 28].sum() > 200  # the three points match nothing
        for nb in nr.NEIGHBOURHOODS:
            for kind, k in nr.STEP_LOSSES:
                want = nr.step_record(src, nr.reference_gaussians("room", True, storage), nr.step_pose("room"), nb, kind, k, storage)
                got = be.ndt_step(q, room[storage], nb, (kind, k), T=nr.step_pose("room"))
                _same_bits(got, want, (nb, nr.LOSS_NAMES[kind], storage))
                assert np.isfinite(got).all()
    finally:
        be.free(q)


@pytest.mark.parametrize("storage", nr.STORAGES)
def test_step_on_the_room_moved_far_from_the_origin(handles, storage):
    be = handles[storage]
    t, q = be.upload(nr.target("room", True, far=True)), be.upload(nr.source("room", True, 2125))
    gid, info = be.voxel_gaussians_create(t, *BUILD)
    try:
        _same_gaussians(be, gid, info, nr.reference_gaussians("room", True, storage, True), ("far room", storage))
        for nb in nr.NEIGHBOURHOODS:
            for kind, k in nr.STEP_LOSSES:
                got = be.ndt_step(q, gid, nb, (kind, k), T=nr.step_pose("room", far=True))
                _same_bits(got, nr.reference_step("room", True, 2125, nb, kind, k, storage, True), ("far", nb, nr.LOSS_NAMES[kind], storage))
                assert got[28] > 1900
    finally:
        be.voxel_gaussians_free(gid)
        be.free(t)
        be.free(q)


@pytest.mark.parametrize("storage", nr.STORAGES)
def test_no_result_depends_on_the_lookup(handles, room, storage):
    """500 far-away points in 100 new voxels behind the target's last point: another table, the same record to the byte"""
    be = handles[storage]
    far = nr.far_voxels()
    t, q = be.upload(np.vstack([nr.target("room", True), far])), be.upload(nr.source("room", True, 2125))
    gid, info = be.voxel_gaussians_create(t, *BUILD)
    try:
        base = nr.reference_gaussians("room", True, storage).info
        assert info["n_voxels"] == base["n_voxels"] + nr.EDGE_FAR_VOXELS and info["n_valid"] == base["n_valid"]  # (five members: not valid)
        for nb in nr.NEIGHBOURHOODS:
            for kind, k in nr.STEP_LOSSES:
                got = be.ndt_step(q, gid, nb, (kind, k), T=nr.step_pose("room"))
                assert got.tobytes() == be.ndt_step(q, room[storage], nb, (kind, k), T=nr.step_pose("room")).tobytes()
                _same_bits(got, nr.reference_step("room", True, 2125, nb, kind, k, storage), ("lookup", nb, nr.LOSS_NAMES[kind], storage))
    finally:
        be.voxel_gaussians_free(gid)
        be.free(t)
        be.free(q)


# ---------------------------------------------------------------------------------------------------------------- 3. the registration
def _parity(got, ref, storage, n, what):
    """1e-3 m and 1e-3 rad in f32 storage, 1e-6 in f64; fitness within 4 / n; rmse relative 1e-3"""
    tol = 1e-3 if storage == F32 else 1e-6
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    print(f"parity {what} {storage}: |dt| {dt:.3e} m, angle {dr:.3e} rad, fitness {got['fitness']:.6f} / {ref['fitness']:.6f}, "
          f"rmse {got['inlier_rmse']:.6e} / {ref['inlier_rmse']:.6e}, iterations {got['iterations']} / {ref['iterations']}")
    assert dt <= tol and dr <= tol, (what, dt, dr)
    assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / n, what
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-12), what


@pytest.mark.parametrize("storage", nr.STORAGES)
@pytest.mark.parametrize("case", [(1, nr.L2, 0.0), (7, nr.CAUCHY, 1.0)], ids=["own_voxel_l2", "seven_cauchy"])
def test_registration_on_the_shifted_room(handles, case, storage):
    """from 0.20 m off the truth, through the seam's class: the restatement's loop at the parity tolerance, and the pose bound of the CPU
    test on the device's own result"""
    be = handles[storage]
    nb, kind, k = case
    src_pts = nr.source("room", True, nr.LOOP_N)
    src, tgt = PointCloud.from_numpy(be, src_pts), PointCloud.from_numpy(be, nr.target("room", True))
    other = PointCloud.from_numpy(be, nr.target("room", False))
    reg = creg.createNdt(CloudRegistrationParameters(), nr.VOXEL, nb, KERNELS[kind](k))
    assert isinstance(reg, creg.RegistrationNdt) and reg.minPoints_ == nr.MIN_POINTS and reg.minEigenvalueRatio_ == nr.RATIO
    reg.icpConvergenceCriteria_.max_iteration_ = nr.LOOP_ITER
    reg.icpConvergenceCriteria_.relative_fitness_ = reg.icpConvergenceCriteria_.relative_rmse_ = 0.0
    res = reg.registerClouds(src, tgt, nr.initial_pose())
    assert res.iterations_ == nr.LOOP_ITER and not res.converged_
    got = dict(transformation=res.transformation_, fitness=res.fitness_, inlier_rmse=res.inlier_rmse_, iterations=res.iterations_)
    _parity(got, nr.reference_registration("room", True, nb, kind, k, storage), storage, nr.LOOP_N, (nb, nr.LOSS_NAMES[kind]))
    dt, da = nr.pose_error(res.transformation_, "room", src_pts)
    print(f"device registration neighbourhood {nb} {nr.LOSS_NAMES[kind]} {storage}: {1e3 * dt:.2f} mm, {1e3 * da:.2f} mrad from the truth")
    assert dt <= nr.POSE_TOL[0] and da <= nr.POSE_TOL[1]
    # the class keeps the Gaussians of the last target it saw, and rebuilds for another cloud
    first, info = reg._gaussians, reg.lastInfo
    assert info == nr.reference_gaussians("room", True, storage).info
    again = reg.registerClouds(src, tgt, nr.initial_pose())
    assert reg._gaussians == first and (again.transformation_ == res.transformation_).all()
    reg.registerClouds(src, other, nr.initial_pose())
    assert reg._gaussians != first and reg.lastInfo == nr.reference_gaussians("room", False, storage).info
    reg.invalidate()


@pytest.mark.parametrize("storage", nr.STORAGES)
def test_two_calls_and_two_handles_give_the_same_bytes(handles, room, storage):
    be = handles[storage]
    other = backend.Backend(0, backend.PRECISION_F32 if storage == F32 else backend.PRECISION_F64)
    q = be.upload(nr.source("room", True, nr.LOOP_N))
    q2, t2 = other.upload(nr.source("room", True, nr.LOOP_N)), other.upload(nr.target("room", True))
    g2, _ = other.voxel_gaussians_create(t2, *BUILD)
    try:
        be.profile_enable(2)
        fixed = dict(init=nr.initial_pose(), max_iter=5, rel_fitness=0.0, rel_rmse=0.0, raw=True)  # five updates, six passes
        first = be.icp_ndt(q, room[storage], 7, (nr.CAUCHY, 1.0), **fixed)
        assert be.span_read(SPAN_NDT_STEP)[0] == 6 and be.span_read(10)[0] == 0  # (span 10: the neighbour search -- there is none)
        second = be.icp_ndt(q, room[storage], 7, (nr.CAUCHY, 1.0), **fixed)
        be.profile_enable(0)
        assert len(first) == 160 and first == second
        assert other.icp_ndt(q2, g2, 7, (nr.CAUCHY, 1.0), **fixed) == first
        assert be.icp_ndt(q, room[storage], 7, (nr.TUKEY, 3.0), **fixed) != first
        assert be.icp_ndt(q, room[storage], 1, (nr.CAUCHY, 1.0), **fixed) != first
    finally:
        be.profile_enable(0)
        be.free(q)
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 4. errors
@pytest.mark.parametrize("storage", nr.STORAGES)
def test_every_error_returns_its_code_and_leaves_the_handle_usable(handles, room, storage):
    be, g = handles[storage], room[storage]
    q = be.upload(nr.source("room", True, 257))
    t = be.upload(nr.target("room", True))
    empty = be.upload(np.zeros((0, 3)))
    skipped = be.upload(np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, 1e9]]))
    few = be.upload(nr.target("room", True)[:3])
    cauchy = (nr.CAUCHY, 1.0)
    ident = (C.c_double * 16)(*np.eye(4).ravel())
    made = []

    def fails(code, fn, *a, **k):
        with pytest.raises(backend.BackendError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        # the handle is usable: the step of a valid pair still gives the restated record
        _same_bits(be.ndt_step(q, g, 7, cauchy, T=nr.step_pose("room")), nr.reference_step("room", True, 257, 7, nr.CAUCHY, 1.0, storage),
                   ("after an error", storage))

    def raw_create(params, out):
        be._ck(be.lib.o3ds_voxel_gaussians_create(be.h, t, params, out, None))

    def raw_step(T, loss, rec):
        be._ck(be.lib.o3ds_ndt_step(be.h, q, g, T, 7, loss, rec))

    def raw_icp(init, params, loss, out):
        be._ck(be.lib.o3ds_icp_ndt_dev(be.h, q, g, init, params, 7, loss, out))

    try:
        # the build
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            fails(backend.ERR_INVALID_ARG, be.voxel_gaussians_create, t, bad)
        for bad in (1, 0, -3):
            fails(backend.ERR_INVALID_ARG, be.voxel_gaussians_create, t, nr.VOXEL, bad)
        for bad in (0.0, -0.01, 1.5, float("nan")):
            fails(backend.ERR_INVALID_ARG, be.voxel_gaussians_create, t, nr.VOXEL, nr.MIN_POINTS, bad)
        fails(backend.ERR_INVALID_ARG, be.voxel_gaussians_create, t, *BUILD, reserved=1)
        fails(backend.ERR_INVALID_ARG, be.voxel_gaussians_create, 987654321, *BUILD)
        vp, gid = backend.VoxelGaussianParams(*BUILD[:2], 0, BUILD[2]), C.c_uint64(0)
        fails(backend.ERR_INVALID_ARG, raw_create, None, C.byref(gid))
        fails(backend.ERR_INVALID_ARG, raw_create, C.byref(vp), None)
        made.append(be.voxel_gaussians_create(t, nr.VOXEL, 2, 1.0)[0])  # the smallest min_points and the largest ratio are accepted
        # the object
        for fn in (be.voxel_gaussians_free, be.voxel_gaussians_info, be.voxel_gaussians_download):
            fails(backend.ERR_INVALID_ARG, fn, 987654321)
        fails(backend.ERR_INVALID_ARG, lambda: be._ck(be.lib.o3ds_voxel_gaussians_info_get(be.h, g, None, None)))
        n_vox = be.voxel_gaussians_info(g)["n_voxels"]
        fails(backend.ERR_CAPACITY, be.voxel_gaussians_download, g, capacity=n_vox - 1)
        # the step and the registration
        for fn in (be.ndt_step, be.icp_ndt):
            for bad in (0, 3, 6, 8, 27, -1):
                fails(backend.ERR_INVALID_ARG, fn, q, g, bad, cauchy)
            fails(backend.ERR_INVALID_ARG, fn, 987654321, g, 7, cauchy)
            fails(backend.ERR_INVALID_ARG, fn, q, 987654321, 7, cauchy)
            fails(backend.ERR_INVALID_ARG, fn, q, t, 7, cauchy)  # (a cloud's id is not a Gaussians object's)
            for kind in (nr.HUBER, nr.CAUCHY, nr.GM, nr.TUKEY):
                for bad in (0.0, -1.0, float("nan"), float("inf")):
                    fails(backend.ERR_INVALID_ARG, fn, q, g, 7, (kind, bad))
            for kind in (-1, 6, 99):
                fails(backend.ERR_INVALID_ARG, fn, q, g, 7, (kind, 1.0))
            fails(backend.ERR_INVALID_ARG, fn, q, g, 7, backend.RobustLoss(nr.TUKEY, 1, 3.0))  # reserved
            for kind in (nr.L2, nr.L1):
                fn(q, g, 7, (kind, float("nan")))  # k is ignored where the loss has none
        rec, ls = (C.c_double * 32)(), backend.RobustLoss(nr.CAUCHY, 0, 1.0)
        p, out = be._params(0.0, 3, 0.0, 0.0), backend.IcpResult()
        fails(backend.ERR_INVALID_ARG, raw_step, ident, None, rec)
        fails(backend.ERR_INVALID_ARG, raw_step, None, C.byref(ls), rec)
        fails(backend.ERR_INVALID_ARG, raw_step, ident, C.byref(ls), None)
        fails(backend.ERR_INVALID_ARG, raw_icp, ident, C.byref(p), None, C.byref(out))
        fails(backend.ERR_INVALID_ARG, raw_icp, None, C.byref(p), C.byref(ls), C.byref(out))
        fails(backend.ERR_INVALID_ARG, raw_icp, ident, None, C.byref(ls), C.byref(out))
        fails(backend.ERR_INVALID_ARG, raw_icp, ident, C.byref(p), C.byref(ls), None)
        fails(backend.ERR_INVALID_ARG, be.icp_ndt, q, g, 7, cauchy, max_iter=-1)
        # params->method and max_correspondence_distance are ignored
        p2 = be._params(float("nan"), 3, 0.0, 0.0, method=99)
        out2 = backend.IcpResult()
        raw_icp(ident, C.byref(p), C.byref(ls), C.byref(out))
        raw_icp(ident, C.byref(p2), C.byref(ls), C.byref(out2))
        assert bytes(out) == bytes(out2)
        # targets without a voxel: no error to make, the zero record, O3DS_ERR_EMPTY from the registration
        for c, n_skipped in ((empty, 0), (skipped, 3)):
            gid0, info = be.voxel_gaussians_create(c, *BUILD)
            made.append(gid0)
            assert info == dict(n_voxels=0, n_valid=0, n_skipped_points=n_skipped, n_flat=0)
            assert all(len(v) == 0 for v in be.voxel_gaussians_download(gid0).values())
            assert (be.ndt_step(q, gid0, 7, cauchy) == 0).all()
            fails(backend.ERR_EMPTY, be.icp_ndt, q, gid0, 7, cauchy)
        # a target with voxels but no valid one: the zero record; the registration stays where it started
        gid1, info = be.voxel_gaussians_create(few, *BUILD)
        made.append(gid1)
        assert info["n_voxels"] > 0 and info["n_valid"] == 0
        assert (be.ndt_step(q, gid1, 7, cauchy) == 0).all()
        got = be.icp_ndt(q, gid1, 7, cauchy, init=nr.initial_pose())
        assert got["fitness"] == 0 and got["n_corr"] == 0 and (got["transformation"] == nr.initial_pose()).all()
        # no matched query: the zero record
        assert (be.ndt_step(q, g, 7, cauchy, T=nr.translation((50.0, 50.0, 50.0))) == 0).all()
        # an empty source is no error: fitness 0 and the initial pose; the zero record
        got = be.icp_ndt(empty, g, 7, cauchy, init=nr.initial_pose())
        assert got["fitness"] == 0 and got["iterations"] == 0 and (got["transformation"] == nr.initial_pose()).all()
        assert (be.ndt_step(empty, g, 7, cauchy) == 0).all()
    finally:
        for gid in made:
            be.voxel_gaussians_free(gid)
        for c in (q, t, empty, skipped, few):
            be.free(c)
