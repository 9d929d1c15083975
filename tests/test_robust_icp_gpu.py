"""Robust loss kernels on the device against the numpy restatement (tests/robust_icp_restatement.py): the weighted record of one step bit
for bit, the L2 identity with the coloured step and registration, the outlier case the feature exists for at the project's parity
tolerance, reproducibility, and every error code.  Both storages; needs an MI355X.

The cases and what each is there for are in robust_icp_restatement; their premises are asserted without a device in
tests/test_robust_icp_restatement_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_icp_restatement as cr  # noqa: E402
import robust_icp_restatement as rr  # noqa: E402
from colored_icp_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, synthetic as syn  # noqa: E402
from open3d_slam_amd import cloud_registration as creg  # noqa: E402
from open3d_slam_amd.parameters import CloudRegistrationParameters  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN_COLORED_STEP, SPAN_ROBUST_STEP = 16, 17
EST = [e for e, _ in rr.ESTIMATORS]
EST_IDS = [name for _, name in rr.ESTIMATORS]
KERNELS = {rr.L2: lambda k: creg.L2Loss(), rr.L1: lambda k: creg.L1Loss(), rr.HUBER: creg.HuberLoss, rr.CAUCHY: creg.CauchyLoss,
           rr.GM: creg.GMLoss, rr.TUKEY: creg.TukeyLoss}


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
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{what}: terms {bad.tolist()} differ: got {got[bad]}, restated {want[bad]}"


@pytest.fixture(scope="module")
def scene_targets(handles):
    """per storage: the sliding scene's target with colours and the gradients the registration at STEP_R would make (COLORED), and the
    same points with normals alone (POINT_TO_PLANE reads nothing else)"""
    s = cr.sliding_scene()
    ids = {}
    for storage, be in handles.items():
        full = _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
        be.compute_color_gradients(full, *cr.STEP_GRADIENT)
        ids[storage] = {rr.COLORED: full, rr.POINT_TO_PLANE: _cloud(be, s.tgt, s.tgt_nrm)}
    yield ids
    for storage, be in handles.items():
        for c in ids[storage].values():
            be.free(c)


# ---------------------------------------------------------------------------------------------------------------- 1. the step
@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("estimator", EST, ids=EST_IDS)
@pytest.mark.parametrize("n", rr.STEP_SIZES)
def test_step_record_is_the_restated_one_bit_for_bit(handles, scene_targets, n, estimator, storage):
    be, t = handles[storage], scene_targets[storage][estimator]
    src, col = cr.step_source(n)
    q = _cloud(be, src, None, col if estimator == rr.COLORED else None)
    try:
        for kind, k in rr.STEP_LOSSES:
            got = be.robust_icp_step(q, t, rr.STEP_R, estimator, (kind, k), T=cr.NEAR_POSE)
            _same_bits(got, rr.reference_step(n, "near", estimator, kind, k, storage), (n, EST_IDS[estimator], rr.LOSS_NAMES[kind], storage))
        assert (be.robust_icp_step(q, t, rr.STEP_R, estimator, (rr.TUKEY, rr.STEP_K), T=cr.FAR_POSE) == 0).all()  # no correspondence
    finally:
        be.free(q)


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_edge_pairs(handles, storage):
    """residuals of exactly 0, k / 2, k and 2 k: L1's r == 0 rule, Huber at e == k, Tukey at and beyond k -- and a Tukey system without a
    single weight, from which the registration takes the identity update"""
    be = handles[storage]
    s = rr.edge_scene()
    t = _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
    q = _cloud(be, s.src, None, s.src_col)
    qb = _cloud(be, s.src[s.beyond], None, s.src_col[s.beyond])
    try:
        be.compute_color_gradients(t, *rr.EDGE_GRADIENT)
        _same_bits(be.color_gradients(t).ravel(), rr.edge_gradients(storage).ravel(), ("edge gradients", storage))
        for est in EST:
            for lam in rr.EDGE_LAMBDAS:
                for kind, k in rr.EDGE_LOSSES:
                    got = be.robust_icp_step(q, t, rr.EDGE_R, est, (kind, k), lambda_geometric=lam)
                    _same_bits(got, rr.reference_edge(est, kind, k, lam, storage), (EST_IDS[est], lam, rr.LOSS_NAMES[kind], storage))
                    assert got[28] == 16 and np.isfinite(got).all()
            got = be.robust_icp_step(qb, t, rr.EDGE_R, est, (rr.TUKEY, rr.EDGE_K), lambda_geometric=1.0)
            _same_bits(got, rr.reference_edge(est, rr.TUKEY, rr.EDGE_K, 1.0, storage, beyond_only=True), (EST_IDS[est], "beyond", storage))
            assert (got[:27] == 0).all() and got[27] > 0 and got[28] == 8 and got[29] > 0
            res = be.icp_robust_dev(qb, t, rr.EDGE_R, est, (rr.TUKEY, rr.EDGE_K), max_iter=2, rel_fitness=0.0, rel_rmse=0.0, lambda_geometric=1.0)
            assert (res["transformation"] == np.eye(4)).all() and res["iterations"] == 2 and res["fitness"] == 1.0 and res["n_corr"] == 8
    finally:
        for c in (t, q, qb):
            be.free(c)


# ---------------------------------------------------------------------------------------------------------------- 2. the L2 identity
@pytest.mark.parametrize("storage", cr.STORAGES)
def test_colored_with_l2_is_the_coloured_step_and_registration(handles, scene_targets, storage):
    be, t = handles[storage], scene_targets[storage][rr.COLORED]
    s = cr.sliding_scene()
    for n in rr.STEP_SIZES:
        src, col = cr.step_source(n)
        q = _cloud(be, src, None, col)
        try:
            for lam in cr.STEP_LAMBDAS:
                _same_bits(be.robust_icp_step(q, t, rr.STEP_R, rr.COLORED, (rr.L2, 0.0), lambda_geometric=lam, T=cr.NEAR_POSE),
                           be.colored_icp_step(q, t, rr.STEP_R, lam, T=cr.NEAR_POSE), (n, lam, storage))
        finally:
            be.free(q)
    q, t2 = _cloud(be, s.src, None, s.src_col), _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
    try:
        fixed = dict(max_iter=10, rel_fitness=0.0, rel_rmse=0.0, raw=True)
        want = be.icp_colored_dev(q, t2, 0.15, **fixed)
        got = be.icp_robust_dev(q, t2, 0.15, rr.COLORED, (rr.L2, 0.0), **fixed)
        assert len(got) == 160 and got == want
        assert be.icp_robust_dev(q, t2, 0.15, rr.COLORED, (rr.TUKEY, 0.05), **fixed) != want
    finally:
        be.free(q)
        be.free(t2)


# ---------------------------------------------------------------------------------------------------------------- 3. the outlier case
def _parity(got, ref, storage, n, what):
    """1e-3 m and 1e-3 rad in f32 storage, 1e-6 in f64; fitness within 4 / n; rmse relative 1e-3"""
    tol = 1e-3 if storage == F32 else 1e-6
    dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
    print(f"parity {what} {storage}: |dt| {dt:.3e} m, angle {dr:.3e} rad, fitness {got['fitness']:.6f} / {ref['fitness']:.6f}, "
          f"rmse {got['inlier_rmse']:.6e} / {ref['inlier_rmse']:.6e}, iterations {got['iterations']} / {ref['iterations']}")
    assert dt <= tol and dr <= tol, (what, dt, dr)
    assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / n, what
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-12), what


@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("estimator", EST, ids=EST_IDS)
def test_the_outlier_case_on_the_device(handles, estimator, storage):
    """300 raised floor points pull the L2 pose by centimetres; the robust losses take most of that away -- through the seam's class"""
    be = handles[storage]
    s = rr.outlier_scene()
    colored = estimator == rr.COLORED
    src = PointCloud.from_numpy(be, s.src, None, s.src_col if colored else None)
    tgt = PointCloud.from_numpy(be, s.tgt, s.tgt_nrm, s.tgt_col if colored else None)
    errors = {}
    for kind, k in rr.OUTLIER_LOSSES:
        reg = creg.createRobustIcp(CloudRegistrationParameters(), KERNELS[kind](k), EST_IDS[estimator])
        assert isinstance(reg, creg.RegistrationIcpRobust) and reg.lambdaGeometric_ == 0.968 and reg.estimator_ == EST_IDS[estimator]
        reg.maxCorrespondenceDistance_ = rr.OUTLIER["r"]
        reg.icpConvergenceCriteria_.max_iteration_ = rr.OUTLIER["max_iter"]
        reg.icpConvergenceCriteria_.relative_fitness_ = reg.icpConvergenceCriteria_.relative_rmse_ = 0.0
        res = reg.registerClouds(src, tgt, np.eye(4))
        errors[kind] = cr.translation_error(res.transformation_)
        assert res.iterations_ == rr.OUTLIER["max_iter"] and not res.converged_
        got = dict(transformation=res.transformation_, fitness=res.fitness_, inlier_rmse=res.inlier_rmse_, iterations=res.iterations_)
        _parity(got, rr.outlier_result(estimator, kind, k, storage), storage, len(s.src), rr.LOSS_NAMES[kind])
    print(f"outlier case on the device {EST_IDS[estimator]} {storage}: "
          + ", ".join(f"{rr.LOSS_NAMES[kd]} {1e3 * e:.3f} mm" for kd, e in errors.items()))
    rr.outlier_conditions(errors)
    assert be.has_color_gradients(tgt.id) == colored  # COLORED leaves those of (2 r, 30) on the target; POINT_TO_PLANE makes none


# ---------------------------------------------------------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("estimator", EST, ids=EST_IDS)
def test_two_calls_and_two_handles_give_the_same_bytes(handles, estimator, storage):
    be = handles[storage]
    other = backend.Backend(0, backend.PRECISION_F32 if storage == F32 else backend.PRECISION_F64)
    s = rr.outlier_scene()
    q, t = _cloud(be, s.src, None, s.src_col), _cloud(be, s.tgt, s.tgt_nrm, s.tgt_col)
    q2, t2 = _cloud(other, s.src, None, s.src_col), _cloud(other, s.tgt, s.tgt_nrm, s.tgt_col)
    try:
        be.profile_enable(2)
        fixed = dict(init=cr.NEAR_POSE, max_iter=5, rel_fitness=0.0, rel_rmse=0.0, raw=True)  # five updates, six passes
        first = be.icp_robust_dev(q, t, 0.15, estimator, (rr.CAUCHY, 0.02), **fixed)
        assert be.span_read(SPAN_ROBUST_STEP)[0] == 6 and be.span_read(SPAN_COLORED_STEP)[0] == 0
        second = be.icp_robust_dev(q, t, 0.15, estimator, (rr.CAUCHY, 0.02), **fixed)
        be.profile_enable(0)
        assert len(first) == 160 and first == second
        assert other.icp_robust_dev(q2, t2, 0.15, estimator, (rr.CAUCHY, 0.02), **fixed) == first
        assert be.icp_robust_dev(q, t, 0.15, estimator, (rr.HUBER, 0.02), **fixed) != first
    finally:
        be.profile_enable(0)
        be.free(q)
        be.free(t)
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("storage", cr.STORAGES)
def test_every_error_returns_its_code_and_leaves_the_handle_usable(handles, scene_targets, storage):
    be = handles[storage]
    t, tp = scene_targets[storage][rr.COLORED], scene_targets[storage][rr.POINT_TO_PLANE]
    s = cr.sliding_scene()
    src, col = cr.step_source(100)
    q = _cloud(be, src, None, col)
    bare_src = _cloud(be, src)
    no_normals = _cloud(be, s.tgt[:200], None, s.tgt_col[:200])
    no_colors = _cloud(be, s.tgt[:200], s.tgt_nrm[:200])
    empty = be.upload(np.zeros((0, 3)))
    no_gradients = _cloud(be, s.tgt[:300], s.tgt_nrm[:300], s.tgt_col[:300])
    be._ck(be.lib.o3ds_set_precision(be.h, backend.PRECISION_F64 if storage == F32 else backend.PRECISION_F32))
    other_type = _cloud(be, src, None, col)
    be._ck(be.lib.o3ds_set_precision(be.h, be.precision))
    tukey = (rr.TUKEY, 0.05)

    def fails(code, fn, *a, **k):
        with pytest.raises(backend.BackendError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        # the handle is usable: the step of a valid pair still gives the restated record
        _same_bits(be.robust_icp_step(q, t, rr.STEP_R, rr.COLORED, (rr.TUKEY, rr.STEP_K), T=cr.NEAR_POSE),
                   rr.reference_step(100, "near", rr.COLORED, rr.TUKEY, rr.STEP_K, storage), ("after an error", storage))

    def null_loss(step):
        ident = (C.c_double * 16)(*np.eye(4).ravel())
        if step:
            rec = (C.c_double * 32)()
            be._ck(be.lib.o3ds_robust_icp_step(be.h, q, t, ident, 0.15, rr.COLORED, 0.968, None, rec))
        else:
            p, out = be._params(0.15, 3, 0.0, 0.0), backend.IcpResult()
            be._ck(be.lib.o3ds_icp_robust_dev(be.h, q, t, ident, C.byref(p), rr.COLORED, 0.968, None, C.byref(out)))

    try:
        for step, fn in ((False, be.icp_robust_dev), (True, be.robust_icp_step)):
            for est, good in ((rr.COLORED, t), (rr.POINT_TO_PLANE, tp)):
                # the loss and the estimator
                for kind in (rr.HUBER, rr.CAUCHY, rr.GM, rr.TUKEY):
                    for bad in (0.0, -0.02, float("nan"), float("inf")):
                        fails(backend.ERR_INVALID_ARG, fn, q, good, 0.15, est, (kind, bad))
                for kind in (-1, 6, 99):
                    fails(backend.ERR_INVALID_ARG, fn, q, good, 0.15, est, (kind, 0.02))
                fails(backend.ERR_INVALID_ARG, fn, q, good, 0.15, est, backend.RobustLoss(rr.TUKEY, 1, 0.05))  # reserved
                # the clouds, as for the coloured step
                fails(backend.ERR_NO_NORMALS, fn, q, no_normals, 0.15, est, tukey)
                for bad in (0.0, -1.0, float("nan")):
                    fails(backend.ERR_INVALID_ARG, fn, q, good, bad, est, tukey)
                fails(backend.ERR_INVALID_ARG, fn, other_type, good, 0.15, est, tukey)
                fails(backend.ERR_INVALID_ARG, fn, q, 987654321, 0.15, est, tukey)
                fails(backend.ERR_INVALID_ARG, fn, 987654321, good, 0.15, est, tukey)
                fails(backend.ERR_EMPTY, fn, q, empty, 0.15, est, tukey)
            for est in (-1, 2):
                fails(backend.ERR_INVALID_ARG, fn, q, t, 0.15, est, tukey)
            fails(backend.ERR_INVALID_ARG, null_loss, step)
            # COLORED keeps its preconditions
            fails(backend.ERR_INVALID_ARG, fn, q, no_colors, 0.15, rr.COLORED, tukey)
            fails(backend.ERR_INVALID_ARG, fn, bare_src, t, 0.15, rr.COLORED, tukey)
            for bad in (-0.1, 1.1, float("nan")):
                fails(backend.ERR_INVALID_ARG, fn, q, t, 0.15, rr.COLORED, tukey, lambda_geometric=bad)
            # ... which POINT_TO_PLANE does not have: no colours anywhere, any lambda; k is ignored where the loss has none
            for lam in (0.968, -0.1, float("nan")):
                fn(bare_src, no_colors, 0.15, rr.POINT_TO_PLANE, tukey, lambda_geometric=lam)
            for kind in (rr.L2, rr.L1):
                fn(q, t, 0.15, rr.COLORED, (kind, float("nan")))
        fails(backend.ERR_INVALID_ARG, be.icp_robust_dev, q, t, 0.15, rr.COLORED, tukey, max_iter=-1)
        fails(backend.ERR_INVALID_ARG, be.robust_icp_step, q, no_gradients, 0.15, rr.COLORED, tukey)
        # an empty source is no error: fitness 0 and the initial pose; the zero record
        for est, good in ((rr.COLORED, t), (rr.POINT_TO_PLANE, tp)):
            got = be.icp_robust_dev(empty, good, 0.15, est, tukey, init=cr.NEAR_POSE)
            assert got["fitness"] == 0 and got["iterations"] == 0 and (got["transformation"] == cr.NEAR_POSE).all()
            assert (be.robust_icp_step(empty, good, 0.15, est, tukey) == 0).all()
    finally:
        for c in (q, bare_src, no_normals, no_colors, empty, no_gradients, other_type):
            be.free(c)
