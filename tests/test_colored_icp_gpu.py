"""Coloured ICP on the device against the numpy restatement (tests/colored_icp_restatement.py): the colour gradients and the record of
one joint step bit for bit, the registration at the project's parity tolerance, the sliding case the feature exists for,
and every error code.  Both storages; needs an MI355X.

The cases and what each is there for are in colored_icp_restatement; their premises are asserted without a device in
tests/test_colored_icp_restatement_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_icp_restatement as cr  # noqa: E402
from colored_icp_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, synthetic as syn  # noqa: E402
from open3d_slam_amd.cloud_registration import RegistrationIcpColored, createColoredIcp  # noqa: E402
from open3d_slam_amd.parameters import CloudRegistrationParameters  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN_GRADIENT, SPAN_STEP = 15, 16


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


def _cloud(be, pts, nrm=None, col=None) -> int:
    cid = be.upload(pts, nrm)
    if col is not None:
        be.set_colors(cid, col)
    return cid


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).reshape(len(got), -1).any(axis=1) if got.ndim > 1
                         else got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[:8].tolist()}: got {got[bad[0]]}, restated {want[bad[0]]}"


@pytest.fixture(scope="module")
def scene_targets(handles):
    """the sliding scene's target on both handles, with the gradients the registration at STEP_R would make"""
    s = cr.sliding_scene()
    ids = {}
    for storage, be in handles.items():
        ids[storage] = _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
        be.compute_color_gradients(ids[storage], *cr.STEP_GRADIENT)
    yield ids
    for storage, be in handles.items():
        be.free(ids[storage])


# ---------------------------------------------------------------------------------------------------------------- 1. gradients
@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("case", cr.GRAD_CASES, ids=lambda c: c.name)
def test_gradients_are_the_restated_ones_bit_for_bit(handles, case, storage):
    be = handles[storage]
    pts, nrm, col = case.cloud()
    c = _cloud(be, pts, nrm, col)
    try:
        assert not be.has_color_gradients(c)
        with pytest.raises(backend.BackendError) as e:
            be.color_gradients(c)
        assert e.value.code == backend.ERR_INVALID_ARG
        be.compute_color_gradients(c, case.radius, case.max_nn)
        assert be.has_color_gradients(c)
        got = be.color_gradients(c)
        _same_bits(got, cr.reference_gradients(case.name, storage), (case.name, storage))
        if case.name == "uniform":
            assert (got == 0).all()
        be.compute_color_gradients(c, case.radius, case.max_nn)  # again: the same bits
        _same_bits(be.color_gradients(c), got, (case.name, storage, "again"))
    finally:
        be.free(c)


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_gradients_follow_the_cloud_they_were_made_for(handles, storage):
    """dropped by every in-place change of points, normals or colours; carried into no cloud another call makes"""
    be = handles[storage]
    pts, nrm, col = cr.edge_cloud()
    pts, nrm, col = pts[:70], nrm[:70], col[:70]
    c = _cloud(be, pts, nrm, col)
    add = _cloud(be, pts[:5] + [0.0, 50.0, 0.0], nrm[:5], col[:5])
    made = []
    try:
        def fresh():
            be.compute_color_gradients(c, cr.EDGE_RADIUS, 30)
            assert be.has_color_gradients(c)

        fresh()
        made.append(be.crop_cloud(c, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=1000.0)))
        made.append(be.transform_cloud(c, cr.NEAR_POSE))
        made.append(be.select_by_index(c, np.arange(10)))
        for m in made:
            assert not be.has_color_gradients(m) and be.has_colors(m)
        assert be.has_color_gradients(c)  # (making them took nothing from the cloud)
        be.set_colors(c, col[::-1])
        assert not be.has_color_gradients(c)
        fresh()
        be.estimate_normals(c, 0.5, 10)
        assert not be.has_color_gradients(c)
        fresh()
        be.cloud_append(c, add)
        assert not be.has_color_gradients(c) and be.size(c)[0] == 75
        fresh()
        assert be.color_gradients(c).shape == (75, 3)
    finally:
        for m in made + [c, add]:
            be.free(m)


# ---------------------------------------------------------------------------------------------------------------- 2. the step
@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("n", cr.STEP_SIZES)
def test_step_record_is_the_restated_one_bit_for_bit(handles, scene_targets, n, storage):
    be, t = handles[storage], scene_targets[storage]
    s = cr.sliding_scene()
    src, col = cr.step_source(n)
    q = _cloud(be, src, None, col)
    flat = _cloud(be, s.tgt, s.tgt_nrm, np.full(s.tgt.shape, 0.375))
    try:
        _same_bits(be.color_gradients(t), cr.reference_gradients("scene", storage), ("target gradients", storage))
        for pose, T in cr.STEP_POSES:
            for lam in cr.STEP_LAMBDAS:
                got = be.colored_icp_step(q, t, cr.STEP_R, lam, T=T)
                _same_bits(got, cr.reference_step(n, pose, lam, storage), (n, pose, lam, storage))
            # lambda = 1: the photometric half vanishes, rows [0..27] are the pure geometric restatement's
            _same_bits(be.colored_icp_step(q, t, cr.STEP_R, 1.0, T=T)[:28], cr.geometric_record(src, s.tgt, s.tgt_nrm, T, cr.STEP_R, storage)[:28],
                       (n, pose, "geometric", storage))
        assert (be.colored_icp_step(q, t, cr.STEP_R, cr.LAMBDA_DEFAULT, T=cr.FAR_POSE) == 0).all()  # no correspondence: a zero record
        be.compute_color_gradients(flat, *cr.STEP_GRADIENT)  # uniform colours: a target whose gradients are all zero
        assert (be.color_gradients(flat) == 0).all()
        for pose, T in cr.STEP_POSES:
            _same_bits(be.colored_icp_step(q, flat, cr.STEP_R, cr.LAMBDA_DEFAULT, T=T), cr.reference_step(n, pose, cr.LAMBDA_DEFAULT, storage, True),
                       (n, pose, "zero gradients", storage))
    finally:
        be.free(q)
        be.free(flat)


# ---------------------------------------------------------------------------------------------------------------- 3. the registration
def _parity(got, ref, storage, n):
    """1e-3 m and 1e-3 rad in f32 storage, 1e-6 in f64; fitness within 4 / n; rmse relative 1e-3"""
    tol = 1e-3 if storage == F32 else 1e-6
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    print(f"parity {storage}: |dt| {dt:.3e} m, angle {dr:.3e} rad, fitness {got['fitness']:.6f} / {ref['fitness']:.6f}, "
          f"rmse {got['inlier_rmse']:.6e} / {ref['inlier_rmse']:.6e}, iterations {got['iterations']} / {ref['iterations']}")
    assert dt <= tol and dr <= tol, (dt, dr)
    assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / n
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-12)


@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("r,lam", cr.SLIDING_PARAMS)
def test_the_sliding_case_on_the_device(handles, r, lam, storage):
    """the translation along the edge, which geometry does not see, is found from the colours -- through the seam's class"""
    be = handles[storage]
    s = cr.sliding_scene()
    src = PointCloud.from_numpy(be, s.src, None, s.src_col)
    tgt = PointCloud.from_numpy(be, s.tgt, s.tgt_nrm, s.tgt_col)
    reg = createColoredIcp(CloudRegistrationParameters())
    assert isinstance(reg, RegistrationIcpColored) and reg.lambdaGeometric_ == 0.968
    reg.maxCorrespondenceDistance_, reg.lambdaGeometric_ = r, lam
    reg.icpConvergenceCriteria_.max_iteration_ = 10
    reg.icpConvergenceCriteria_.relative_fitness_ = reg.icpConvergenceCriteria_.relative_rmse_ = 0.0
    res = reg.registerClouds(src, tgt, np.eye(4))
    err = cr.translation_error(res.transformation_)
    print(f"sliding case on the device r={r} lambda={lam} {storage}: translation error {err:.3e} m")
    assert err < cr.SLIDE / 10.0, err
    assert res.iterations_ == 10 and not res.converged_
    got = dict(transformation=res.transformation_, fitness=res.fitness_, inlier_rmse=res.inlier_rmse_, iterations=res.iterations_)
    _parity(got, cr.sliding_result(r, lam, storage), storage, len(s.src))
    assert be.has_color_gradients(tgt.id)  # left on the target, those of (2 r, 30)
    _same_bits(be.color_gradients(tgt.id), cr.gradients(s.tgt, s.tgt_nrm, s.tgt_col, 2.0 * r, 30, storage), ("gradients left", r, storage))


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_default_thresholds_converge_before_max_iteration(handles, storage):
    be = handles[storage]
    s = cr.sliding_scene()
    c = cr.CONVERGING
    q, t = _cloud(be, s.src, None, s.src_col), _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
    try:
        got = be.icp_colored_dev(q, t, c["r"], max_iter=c["max_iter"], lambda_geometric=c["lam"])
        print(f"converging case on the device {storage}: iterations {got['iterations']}")
        assert got["converged"] and 1 < got["iterations"] < c["max_iter"]
        assert cr.translation_error(got["transformation"]) < cr.SLIDE / 10.0
    finally:
        be.free(q)
        be.free(t)


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_two_calls_and_two_handles_give_the_same_bytes_and_the_gradients_are_made_once(handles, storage):
    be = handles[storage]
    other = backend.Backend(0, backend.PRECISION_F32 if storage == F32 else backend.PRECISION_F64)
    s = cr.sliding_scene()
    q, t = _cloud(be, s.src, None, s.src_col), _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
    q2, t2 = _cloud(other, s.src, None, s.src_col), _cloud(other, s.tgt, s.tgt_nrm, s.tgt_col)
    try:
        be.profile_enable(2)
        fixed = dict(init=cr.NEAR_POSE, max_iter=5, rel_fitness=0.0, rel_rmse=0.0, raw=True)  # five updates, six passes
        first = be.icp_colored_dev(q, t, 0.15, **fixed)
        assert be.span_read(SPAN_GRADIENT)[0] == 1 and be.span_read(SPAN_STEP)[0] == 6
        assert be.has_color_gradients(t)
        second = be.icp_colored_dev(q, t, 0.15, **fixed)
        assert be.span_read(SPAN_GRADIENT)[0] == 0 and be.span_read(SPAN_STEP)[0] == 6  # the gradients were reused
        be.icp_colored_dev(q, t, 0.3, init=cr.NEAR_POSE, max_iter=1)  # another radius: other gradients, made again
        assert be.span_read(SPAN_GRADIENT)[0] == 1
        be.profile_enable(0)
        assert len(first) == 160 and first == second
        assert other.icp_colored_dev(q2, t2, 0.15, **fixed) == first
    finally:
        be.profile_enable(0)
        be.free(q)
        be.free(t)
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 4. errors
@pytest.mark.parametrize("storage", cr.STORAGES)
def test_every_error_returns_its_code_and_leaves_the_handle_usable(handles, scene_targets, storage):
    be, t = handles[storage], scene_targets[storage]
    s = cr.sliding_scene()
    src, col = cr.step_source(100)
    q = _cloud(be, src, None, col)
    bare_src = _cloud(be, src)
    no_normals = _cloud(be, s.tgt[:200], None, s.tgt_col[:200])
    no_colors = _cloud(be, s.tgt[:200], s.tgt_nrm[:200])
    empty = be.upload(np.zeros((0, 3)))
    no_gradients = _cloud(be, s.tgt[:300], s.tgt_nrm[:300], s.tgt_col[:300])  # a complete target nobody computed gradients for
    be._ck(be.lib.o3ds_set_precision(be.h, backend.PRECISION_F64 if storage == F32 else backend.PRECISION_F32))
    other_type = _cloud(be, src, None, col)
    be._ck(be.lib.o3ds_set_precision(be.h, be.precision))

    def fails(code, fn, *a, **k):
        with pytest.raises(backend.BackendError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        # the handle is usable: the step of a valid pair still gives the restated record
        _same_bits(be.colored_icp_step(q, t, cr.STEP_R, cr.LAMBDA_DEFAULT, T=cr.NEAR_POSE), cr.reference_step(100, "near", cr.LAMBDA_DEFAULT, storage),
                   ("after an error", storage))

    try:
        for fn in (be.icp_colored_dev, be.colored_icp_step):
            lam = dict(lambda_geometric=0.968)
            fails(backend.ERR_NO_NORMALS, fn, q, no_normals, 0.15, **lam)
            fails(backend.ERR_INVALID_ARG, fn, q, no_colors, 0.15, **lam)
            fails(backend.ERR_INVALID_ARG, fn, bare_src, t, 0.15, **lam)
            for bad in (-0.1, 1.1, float("nan")):
                fails(backend.ERR_INVALID_ARG, fn, q, t, 0.15, lambda_geometric=bad)
            for bad in (0.0, -1.0, float("nan")):
                fails(backend.ERR_INVALID_ARG, fn, q, t, bad, **lam)
            fails(backend.ERR_INVALID_ARG, fn, other_type, t, 0.15, **lam)
            fails(backend.ERR_INVALID_ARG, fn, q, 987654321, 0.15, **lam)
            fails(backend.ERR_INVALID_ARG, fn, 987654321, t, 0.15, **lam)
            fails(backend.ERR_EMPTY, fn, q, empty, 0.15, **lam)
        fails(backend.ERR_INVALID_ARG, be.icp_colored_dev, q, t, 0.15, max_iter=-1)
        fails(backend.ERR_INVALID_ARG, be.colored_icp_step, q, no_gradients, 0.15)
        fails(backend.ERR_NO_NORMALS, be.compute_color_gradients, no_normals, 0.3, 30)
        fails(backend.ERR_INVALID_ARG, be.compute_color_gradients, no_colors, 0.3, 30)
        fails(backend.ERR_INVALID_ARG, be.compute_color_gradients, t, 0.0, 30)
        fails(backend.ERR_INVALID_ARG, be.compute_color_gradients, t, 0.3, 0)
        fails(backend.ERR_INVALID_ARG, be.compute_color_gradients, t, 0.3, 129)
        # an empty source is no error: fitness 0 and the initial pose
        got = be.icp_colored_dev(empty, t, 0.15, init=cr.NEAR_POSE)
        assert got["fitness"] == 0 and got["iterations"] == 0 and (got["transformation"] == cr.NEAR_POSE).all()
        assert (be.colored_icp_step(empty, t, 0.15) == 0).all()
    finally:
        for c in (q, bare_src, no_normals, no_colors, empty, no_gradients, other_type):
            be.free(c)
