"""Degeneracy-aware ICP on the device against the numpy restatement (tests/degeneracy_restatement.py): the analysis of one step bit for bit
in every field, the identity with o3ds_icp_robust_dev where nothing is dropped, the corridor the feature exists for -- verdict, the held
component, the remaining error and the whole result bit for bit against the restated loop -- the plane and the far corridor,
reproducibility, every error code and the Python seam.  Both storages; needs an MI355X.

The scenes, the thresholds (geometric means of what must be dropped and what must be kept) and the tolerances are recorded in
degeneracy_restatement and asserted without a device in tests/test_degeneracy_restatement_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_icp_restatement as cr  # noqa: E402
import degeneracy_restatement as dr  # noqa: E402
import robust_icp_restatement as rr  # noqa: E402
from degeneracy_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402
from open3d_slam_amd import cloud_registration as creg  # noqa: E402
from open3d_slam_amd.parameters import CloudRegistrationParameters  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu

THR = (dr.MIN_ROT, dr.MIN_TRANS)
FAR_AWAY = cr.rigid((0.0, 0.0, 0.0), (0.0, 0.0, 100.0))  # leaves no correspondence
FIXED = dict(max_iter=12, rel_fitness=0.0, rel_rmse=0.0)  # twelve updates, thirteen passes: reference_registration's


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


class Clouds:
    """uploads a scene's target and sources once per storage"""

    def __init__(self, handles):
        self.handles, self.ids = handles, {}

    def target(self, name, noisy, storage) -> int:
        key = ("t", name, noisy, storage)
        if key not in self.ids:
            s = dr.scene(name, noisy)
            self.ids[key] = (storage, self.handles[storage].upload(s.tgt, s.tgt_nrm))
        return self.ids[key][1]

    def source(self, name, noisy, n, storage) -> int:
        key = ("s", name, noisy, n, storage)
        if key not in self.ids:
            self.ids[key] = (storage, self.handles[storage].upload(dr.source(name, noisy, n)))
        return self.ids[key][1]

    def free(self):
        for storage, cid in self.ids.values():
            self.handles[storage].free(cid)


@pytest.fixture(scope="module")
def clouds(handles):
    c = Clouds(handles)
    yield c
    c.free()


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.ravel().view(np.uint64) != want.ravel().view(np.uint64))
    assert len(bad) == 0, f"{what}: entries {bad.tolist()} differ: got {got.ravel()[bad]}, restated {want.ravel()[bad]}"


def _same_analysis(got, an, what):
    for field in ("centre", "eigenvalues", "eigenvectors"):
        _same_bits(got[field], getattr(an, field), (what, field))
    assert got["degenerate"].tolist() == an.degenerate.tolist() and got["n_degenerate"] == an.n_degenerate, (what, got["degenerate"], an.degenerate)
    if "x" in got:
        _same_bits(got["x"], an.x, (what, "x"))


# ---------------------------------------------------------------------------------------------------------------- 1. the analysis
@pytest.mark.parametrize("storage", dr.STORAGES)
@pytest.mark.parametrize("name", dr.SCENES)
def test_localizability_is_the_restated_one_bit_for_bit(handles, clouds, name, storage):
    be = handles[storage]
    for noisy in dr.VARIANTS:
        t = clouds.target(name, noisy, storage)
        for n in dr.STEP_SIZES:
            q = clouds.source(name, noisy, n, storage)
            got = be.icp_localizability(q, t, dr.R, *THR)
            _same_bits(got["record"], dr.step_record(name, noisy, n, storage), (name, noisy, n, storage, "record"))
            _same_analysis(got, dr.reference_analysis(name, noisy, n, storage, *THR), (name, noisy, n, storage))
        # thresholds 0: the ordinary solve of the original record
        plain = be.icp_localizability(q, t, dr.R)
        _same_analysis(plain, dr.reference_analysis(name, noisy, n, storage, 0.0, 0.0), (name, noisy, n, storage, "thresholds 0"))
    # a source beyond max_correspondence_distance: n_corr == 0, six degenerate directions, V = I, x = 0; the centre is T c0
    got = be.icp_localizability(q, t, dr.R, *THR, T=FAR_AWAY)
    c0 = dr.cloud_center(dr.source(name, True, max(dr.STEP_SIZES)), storage)
    assert (got["record"] == 0).all()
    _same_analysis(got, dr.analyse(np.zeros(32), FAR_AWAY, c0, *THR), (name, storage, "no correspondence"))
    assert got["n_degenerate"] == 6 and (got["x"] == 0).all() and (got["eigenvectors"] == np.eye(6)).all()
    _same_bits(be.cloud_center(q), c0, (name, storage, "c0"))


@pytest.mark.parametrize("storage", dr.STORAGES)
def test_localizability_of_the_coloured_estimator(handles, storage):
    """the coloured tests' floor and wall: the record is the coloured step's, the analysis the restated one"""
    be = handles[storage]
    s = cr.sliding_scene()
    t = be.upload(s.tgt, s.tgt_nrm)
    be.set_colors(t, s.tgt_col)
    be.compute_color_gradients(t, *cr.STEP_GRADIENT)
    try:
        for n in rr.STEP_SIZES:
            src, col = cr.step_source(n)
            q = be.upload(src)
            be.set_colors(q, col)
            try:
                got = be.icp_localizability(q, t, rr.STEP_R, *THR, estimator=rr.COLORED, loss=(rr.TUKEY, rr.STEP_K), T=cr.NEAR_POSE)
                rec = rr.reference_step(n, "near", rr.COLORED, rr.TUKEY, rr.STEP_K, storage)
                _same_bits(got["record"], rec, (n, storage, "record"))
                _same_analysis(got, dr.analyse(rec, cr.NEAR_POSE, dr.cloud_center(src, storage), *THR), (n, storage, "coloured"))
            finally:
                be.free(q)
    finally:
        be.free(t)


# ---------------------------------------------------------------------------------------------------------------- 2. nothing dropped
@pytest.mark.parametrize("storage", dr.STORAGES)
@pytest.mark.parametrize("name", ("room", "corridor"))
def test_thresholds_zero_give_the_bytes_of_the_robust_registration(handles, clouds, name, storage):
    be = handles[storage]
    t, q = clouds.target(name, True, storage), clouds.source(name, True, dr.LOOP_N, storage)
    for loss in ((rr.L2, 0.0), (rr.TUKEY, 0.05)):
        want = be.icp_robust_dev(q, t, dr.R, rr.POINT_TO_PLANE, loss, raw=True, **FIXED)
        got, rep = be.icp_degeneracy_aware(q, t, dr.R, 0.0, 0.0, rr.POINT_TO_PLANE, loss, raw=True, **FIXED)
        assert len(got) == 160 and got == want, (name, storage, loss)
        res, report = be.icp_degeneracy_aware(q, t, dr.R, 0.0, 0.0, rr.POINT_TO_PLANE, loss, **FIXED)
        assert report["n_passes_constrained"] == 0 and not report["ever_degenerate"].any() and res["iterations"] == 12
    if name == "room":  # with the test thresholds nothing is dropped either: the same bytes again
        want = be.icp_robust_dev(q, t, dr.R, rr.POINT_TO_PLANE, (rr.L2, 0.0), raw=True, **FIXED)
        got, _ = be.icp_degeneracy_aware(q, t, dr.R, *THR, raw=True, **FIXED)
        assert got == want
        _, report = be.icp_degeneracy_aware(q, t, dr.R, *THR, **FIXED)
        assert report["n_passes_constrained"] == 0 and report["n_degenerate"] == 0 and not report["ever_degenerate"].any()
        assert (report["eigenvalues"][:3] >= 10 * dr.MIN_ROT).all() and (report["eigenvalues"][3:] >= 10 * dr.MIN_TRANS).all()
    else:  # ... and on the corridor they change the result
        assert be.icp_degeneracy_aware(q, t, dr.R, *THR, raw=True, **FIXED)[0] != want


# ---------------------------------------------------------------------------------------------------------------- 3. the corridor
@pytest.mark.parametrize("storage", dr.STORAGES)
def test_the_noisy_corridor(handles, clouds, storage):
    be = handles[storage]
    t, q = clouds.target("corridor", True, storage), clouds.source("corridor", True, dr.LOOP_N, storage)
    c0 = dr.cloud_center(dr.source("corridor", True, dr.LOOP_N), storage)
    plain = be.icp_robust_dev(q, t, dr.R, **FIXED)
    res, rep = be.icp_degeneracy_aware(q, t, dr.R, *THR, **FIXED)
    ref = dr.reference_registration("corridor", True, storage, *THR)
    slide = abs(float(dr.centre_motion(plain["transformation"], np.eye(4), c0) @ dr.AXIS))
    stay = abs(float(dr.centre_motion(res["transformation"], np.eye(4), c0) @ dr.AXIS))
    _, across, angle = dr.pose_error(res["transformation"], "corridor", c0)
    print(f"noisy corridor on the device {storage}: o3ds_icp_robust_dev moves the centre {1e3 * slide:.2f} mm along the axis (fitness "
          f"{plain['fitness']:.4f}), the constrained loop {1e3 * stay:.3f} mm; left across the axis {1e3 * across:.3f} mm, angle {angle:.3e} rad")
    assert slide > dr.SLIDE_MIN and plain["fitness"] == 1.0
    # the report names exactly the axis
    assert rep["degenerate"].tolist() == [0, 0, 0, 1, 0, 0] and rep["ever_degenerate"].tolist() == [0, 0, 0, 1, 0, 0]
    assert rep["n_degenerate"] == 1 and rep["n_passes_constrained"] == res["iterations"] == 12 and not res["converged"]
    assert abs(abs(float(rep["eigenvectors"][3:, 3] @ dr.AXIS)) - 1.0) <= 1e-3
    # the component along it stays where the initial guess put it; the rest is corrected
    assert stay <= dr.ALONG_TOL
    assert across <= dr.TRUTH_TOL and angle <= dr.TRUTH_TOL
    # the whole result is the restated loop's
    _same_bits(res["transformation"], ref["transformation"], (storage, "transformation"))
    _same_bits([res["fitness"], res["inlier_rmse"]], [ref["fitness"], ref["inlier_rmse"]], (storage, "fitness, rmse"))
    assert (res["iterations"], res["converged"], res["n_corr"]) == (ref["iterations"], ref["converged"], ref["n_corr"])
    for field in ("centre", "eigenvalues", "eigenvectors"):
        _same_bits(rep[field], ref[field], (storage, field))
    assert rep["ever_degenerate"].tolist() == ref["ever_degenerate"].tolist() and rep["n_passes_constrained"] == ref["n_passes_constrained"]


@pytest.mark.parametrize("storage", dr.STORAGES)
@pytest.mark.parametrize("name", ("plane", "far_corridor"))
def test_the_verdict_on_the_plane_and_on_the_far_corridor(handles, clouds, name, storage):
    be = handles[storage]
    for noisy in dr.VARIANTS:
        t, q = clouds.target(name, noisy, storage), clouds.source(name, noisy, dr.LOOP_N, storage)
        res, rep = be.icp_degeneracy_aware(q, t, dr.R, *THR, max_iter=3, rel_fitness=0.0, rel_rmse=0.0)
        assert tuple(np.flatnonzero(rep["degenerate"])) == dr.EXPECTED[name], (name, noisy, rep["eigenvalues"])
        assert tuple(np.flatnonzero(rep["ever_degenerate"])) == dr.EXPECTED[name] and rep["n_passes_constrained"] == res["iterations"] == 3
        assert rep["n_degenerate"] == len(dr.EXPECTED[name])
        if name == "far_corridor":  # the same verdict, and the same values, as the corridor at the origin
            _, near = be.icp_degeneracy_aware(clouds.source("corridor", noisy, dr.LOOP_N, storage), clouds.target("corridor", noisy, storage), dr.R, *THR,
                                              max_iter=0)
            _, far = be.icp_degeneracy_aware(q, t, dr.R, *THR, max_iter=0)
            assert far["degenerate"].tolist() == near["degenerate"].tolist()
            assert np.abs(far["eigenvalues"] - near["eigenvalues"]).max() <= dr.SHIFT_TOL[storage]


# ---------------------------------------------------------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("storage", dr.STORAGES)
def test_two_calls_and_two_handles_give_the_same_bytes(handles, clouds, storage):
    be = handles[storage]
    other = backend.Backend(0, backend.PRECISION_F32 if storage == F32 else backend.PRECISION_F64)
    s = dr.scene("corridor", True)
    t, q = clouds.target("corridor", True, storage), clouds.source("corridor", True, dr.LOOP_N, storage)
    t2, q2 = other.upload(s.tgt, s.tgt_nrm), other.upload(dr.source("corridor", True, dr.LOOP_N))
    try:
        fixed = dict(max_iter=5, rel_fitness=0.0, rel_rmse=0.0, raw=True)
        first = be.icp_degeneracy_aware(q, t, dr.R, *THR, loss=(rr.CAUCHY, 0.02), **fixed)
        assert len(first[0]) == 160 and len(first[1]) == 416
        assert be.icp_degeneracy_aware(q, t, dr.R, *THR, loss=(rr.CAUCHY, 0.02), **fixed) == first
        assert other.icp_degeneracy_aware(q2, t2, dr.R, *THR, loss=(rr.CAUCHY, 0.02), **fixed) == first
        assert be.icp_degeneracy_aware(q, t, dr.R, *THR, loss=(rr.HUBER, 0.02), **fixed) != first
        one = be.icp_localizability(q, t, dr.R, *THR, raw=True)
        assert len(one) == 696 and be.icp_localizability(q, t, dr.R, *THR, raw=True) == one
        assert other.icp_localizability(q2, t2, dr.R, *THR, raw=True) == one
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("storage", dr.STORAGES)
def test_every_error_returns_its_code_and_leaves_the_handle_usable(handles, clouds, storage):
    be = handles[storage]
    s = dr.scene("room", False)
    t, q = clouds.target("room", False, storage), clouds.source("room", False, 257, storage)
    no_normals = be.upload(s.tgt[:200])
    empty = be.upload(np.zeros((0, 3)))
    be._ck(be.lib.o3ds_set_precision(be.h, backend.PRECISION_F64 if storage == F32 else backend.PRECISION_F32))
    other_type = be.upload(dr.source("room", False, 100))
    be._ck(be.lib.o3ds_set_precision(be.h, be.precision))
    want = dr.reference_analysis("room", False, 257, storage, *THR)

    def fails(code, fn, *a, **k):
        with pytest.raises(backend.BackendError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        _same_analysis(be.icp_localizability(q, t, dr.R, *THR), want, ("after an error", storage))

    def null_params(step):
        ident = (C.c_double * 16)(*np.eye(4).ravel())
        ls = backend.RobustLoss(rr.L2, 0, 0.0)
        if step:
            out = backend.Localizability()
            be._ck(be.lib.o3ds_icp_localizability(be.h, q, t, ident, dr.R, rr.POINT_TO_PLANE, 0.968, C.byref(ls), None, C.byref(out)))
        else:
            p, out = be._params(dr.R, 3, 0.0, 0.0), backend.IcpResult()
            be._ck(be.lib.o3ds_icp_degeneracy_aware_dev(be.h, q, t, ident, C.byref(p), rr.POINT_TO_PLANE, 0.968, C.byref(ls), None, C.byref(out), None))

    try:
        for step, fn in ((False, be.icp_degeneracy_aware), (True, be.icp_localizability)):
            # the thresholds
            for bad in (-1e-9, -1.0, float("nan"), float("inf"), float("-inf")):
                fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, bad, 0.0)
                fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, 0.0, bad)
            fails(backend.ERR_INVALID_ARG, null_params, step)
            # the loss, the estimator and the clouds, as for o3ds_icp_robust_dev
            for kind in (rr.HUBER, rr.TUKEY):
                for bad in (0.0, -0.02, float("nan"), float("inf")):
                    fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, *THR, loss=(kind, bad))
            for kind in (-1, 6):
                fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, *THR, loss=(kind, 0.02))
            fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, *THR, loss=backend.RobustLoss(rr.TUKEY, 1, 0.05))
            for est in (-1, 2):
                fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, *THR, estimator=est)
            fails(backend.ERR_INVALID_ARG, fn, q, t, dr.R, *THR, estimator=rr.COLORED)  # no colours on these clouds
            fails(backend.ERR_NO_NORMALS, fn, q, no_normals, dr.R, *THR)
            for bad in (0.0, -1.0, float("nan")):
                fails(backend.ERR_INVALID_ARG, fn, q, t, bad, *THR)
            fails(backend.ERR_INVALID_ARG, fn, other_type, t, dr.R, *THR)
            fails(backend.ERR_INVALID_ARG, fn, q, 987654321, dr.R, *THR)
            fails(backend.ERR_INVALID_ARG, fn, 987654321, t, dr.R, *THR)
            fails(backend.ERR_EMPTY, fn, q, empty, dr.R, *THR)
        fails(backend.ERR_INVALID_ARG, be.icp_degeneracy_aware, q, t, dr.R, *THR, max_iter=-1)
        # an empty source is no error: fitness 0, the initial pose, an all-zero report
        res, rep = be.icp_degeneracy_aware(empty, t, dr.R, *THR, init=cr.NEAR_POSE)
        assert res["fitness"] == 0 and res["iterations"] == 0 and (res["transformation"] == cr.NEAR_POSE).all()
        assert be.icp_degeneracy_aware(empty, t, dr.R, *THR, init=cr.NEAR_POSE, raw=True)[1] == bytes(416)
        one = be.icp_localizability(empty, t, dr.R, *THR)
        assert (one["record"] == 0).all() and one["n_degenerate"] == 6 and (one["x"] == 0).all()
        # a NULL report is allowed
        p, out = be._params(dr.R, 2, 0.0, 0.0), backend.IcpResult()
        ls, dp = backend.RobustLoss(rr.L2, 0, 0.0), backend.DegeneracyParams(*THR)
        ident = (C.c_double * 16)(*np.eye(4).ravel())
        be._ck(be.lib.o3ds_icp_degeneracy_aware_dev(be.h, q, t, ident, C.byref(p), rr.POINT_TO_PLANE, 0.968, C.byref(ls), C.byref(dp), C.byref(out), None))
        assert out.iterations == 2
    finally:
        for c in (no_normals, empty, other_type):
            be.free(c)


# ---------------------------------------------------------------------------------------------------------------- 6. the seam
@pytest.mark.parametrize("storage", dr.STORAGES)
def test_registration_class_fills_last_report(handles, storage):
    be = handles[storage]
    s = dr.scene("corridor", True)
    src = PointCloud.from_numpy(be, dr.source("corridor", True, dr.LOOP_N))
    tgt = PointCloud.from_numpy(be, s.tgt, s.tgt_nrm)
    off = creg.createDegeneracyAwareIcp(CloudRegistrationParameters(), "point_to_plane", creg.L2Loss())
    assert isinstance(off, creg.RegistrationIcpDegeneracyAware) and isinstance(off, creg.RegistrationIcpRobust) and off.lastReport is None
    assert off.minEigenvalueRotation_ == 0.0 and off.minEigenvalueTranslation_ == 0.0  # no default but 0
    reg = creg.createDegeneracyAwareIcp(CloudRegistrationParameters(), "point_to_plane", creg.L2Loss(), dr.MIN_ROT, dr.MIN_TRANS)
    for r in (off, reg):
        r.maxCorrespondenceDistance_ = dr.R
        r.icpConvergenceCriteria_.max_iteration_ = 12
        r.icpConvergenceCriteria_.relative_fitness_ = r.icpConvergenceCriteria_.relative_rmse_ = 0.0
    res = reg.registerClouds(src, tgt, np.eye(4))
    ref = dr.reference_registration("corridor", True, storage, *THR)
    _same_bits(res.transformation_, ref["transformation"], (storage, "the seam's transformation"))
    assert res.iterations_ == 12 and reg.lastReport["ever_degenerate"].tolist() == [0, 0, 0, 1, 0, 0] and reg.lastReport["n_passes_constrained"] == 12
    assert reg.lastReport["eigenvectors"].shape == (6, 6) and reg.lastReport["eigenvalues"][3] < dr.MIN_TRANS
    plain = off.registerClouds(src, tgt, np.eye(4))
    assert off.lastReport["n_passes_constrained"] == 0 and (plain.transformation_ != res.transformation_).any()
