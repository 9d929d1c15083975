"""The premises of the degeneracy-aware ICP tests, held on the restatement alone (tests/degeneracy_restatement.py; no device): the accuracy
of its eigen-decomposition, the gap between what must be dropped and what must be kept (the thresholds of every test are its geometric
mean), the invariance under a shift of the scene that re-centring buys, the failure the feature exists for, the optimisation property
of the constrained update, and the edge cases of the rule."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colored_icp_restatement as cr  # noqa: E402
import degeneracy_restatement as dr  # noqa: E402
from degeneracy_restatement import F32, F64  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
CASES = [(name, noisy, st) for name in dr.SCENES for noisy in dr.VARIANTS for st in dr.STORAGES]


def _analysis(name, noisy, st, thresholds=(0.0, 0.0)):
    return dr.reference_analysis(name, noisy, dr.LOOP_N, st, *thresholds)


def test_the_pieces_against_numpy():
    """the dense product, the LDL^T with its fma and the centre against numpy's own forms, to rounding"""
    rng = np.random.default_rng(5)
    P, Q = rng.normal(size=(6, 6)), rng.normal(size=(6, 6))
    assert np.abs(dr.dense(P, Q) - P @ Q).max() <= 16 * EPS * np.abs(P).sum(axis=1).max() * np.abs(Q).max()
    for _ in range(20):
        J = rng.normal(size=(12, 6))
        A, b = J.T @ J, rng.normal(size=6)
        x = dr.solve6(A, b)
        assert np.abs(x - np.linalg.solve(A, b)).max() <= 64 * EPS * np.linalg.cond(A) * np.abs(x).max()
    assert (dr.solve6(np.eye(6), b) == b).all()  # the unit system hands its right-hand side through
    assert dr.fma(1.0 + EPS, 1.0 - EPS, -1.0) == -EPS * EPS and (1.0 + EPS) * (1.0 - EPS) - 1.0 == 0.0
    for n in (1, 255, 256, 257, 4200, 70000):
        pts = rng.normal(size=(n, 3)) + (3.0, -2.0, 1.0)
        for st in dr.STORAGES:
            want = dr.to_storage(pts, st).mean(axis=0)
            assert np.abs(dr.cloud_center(pts, st) - want).max() <= 1e-12 * 4.0


def test_eigen_decomposition_is_as_accurate_as_eigh():
    worst = 0.0
    for name, noisy, st in CASES:
        an = _analysis(name, noisy, st)
        for o in (0, 3):
            A = dr.upper_symmetric(an.Hc)[o:o + 3, o:o + 3]
            lam, V = an.raw[o:o + 3], an.eigenvectors[o:o + 3, o:o + 3]
            scale = EPS * np.linalg.norm(A)
            k_val = np.abs(lam - np.linalg.eigh(A)[0]).max() / scale
            k_res = np.linalg.norm(A @ V - V * lam) / scale
            worst = max(worst, k_val, k_res)
            assert k_val <= dr.EIGEN_K and k_res <= dr.EIGEN_K, (name, noisy, st, o, k_val, k_res)
            assert np.linalg.norm(V.T @ V - np.eye(3)) <= 32 * EPS and (lam[:-1] <= lam[1:]).all()
            assert all(V[np.argmax(np.abs(V[:, j])), j] > 0 for j in range(3))  # the sign rule
    print(f"eigen-decomposition: worst k {worst:.3f} (recorded {dr.EIGEN_K_MEASURED}, bound {dr.EIGEN_K})")
    assert dr.EIGEN_K == 4 * dr.EIGEN_K_MEASURED


def test_the_gap_between_dropped_and_kept_directions():
    drop, keep = {"rot": 0.0, "trans": 0.0}, {"rot": math.inf, "trans": math.inf}
    for name, noisy, st in CASES:
        lam = _analysis(name, noisy, st).eigenvalues
        assert lam[3:].sum() == pytest.approx(1.0, abs=1e-6)  # point-to-plane: the trace of the mean n n^T, unit normals as f32 stores them
        for i in range(6):
            kind = "rot" if i < 3 else "trans"
            if i in dr.EXPECTED[name]:
                drop[kind] = max(drop[kind], lam[i])
            else:
                keep[kind] = min(keep[kind], lam[i])
        if not noisy:  # analytic normals: an unobservable direction carries exactly nothing
            assert all(lam[i] == 0.0 for i in dr.EXPECTED[name]), (name, st, lam)
    print(f"normalised eigenvalues: rotation dropped <= {drop['rot']:.4e}, kept >= {keep['rot']:.5f} m^2; "
          f"translation dropped <= {drop['trans']:.4e}, kept >= {keep['trans']:.5f}; thresholds {dr.MIN_ROT:.3e}, {dr.MIN_TRANS:.3e}")
    assert 0.0 < drop["rot"] <= dr.DROP_ROT <= 1.01 * drop["rot"] and 0.99 * keep["rot"] <= dr.KEEP_ROT <= keep["rot"]
    assert 0.0 < drop["trans"] <= dr.DROP_TRANS <= 1.01 * drop["trans"] and 0.99 * keep["trans"] <= dr.KEEP_TRANS <= keep["trans"]
    assert dr.MIN_ROT == math.sqrt(dr.DROP_ROT * dr.KEEP_ROT) and dr.MIN_TRANS == math.sqrt(dr.DROP_TRANS * dr.KEEP_TRANS)
    assert dr.MIN_ROT >= 10 * dr.DROP_ROT and dr.KEEP_ROT >= 10 * dr.MIN_ROT
    assert dr.MIN_TRANS >= 10 * dr.DROP_TRANS and dr.KEEP_TRANS >= 10 * dr.MIN_TRANS
    for name, noisy, st in CASES:  # hence the verdicts
        an = _analysis(name, noisy, st, (dr.MIN_ROT, dr.MIN_TRANS))
        assert tuple(np.flatnonzero(an.degenerate)) == dr.EXPECTED[name], (name, noisy, st)


@pytest.mark.parametrize("storage", dr.STORAGES)
def test_recentring_makes_the_analysis_independent_of_where_the_scene_lies(storage):
    for noisy in dr.VARIANTS:
        near, far = _analysis("corridor", noisy, storage), _analysis("far_corridor", noisy, storage)
        d = np.abs(near.eigenvalues - far.eigenvalues).max()
        print(f"corridor against far corridor, {storage}, noisy {noisy}: largest difference of a normalised eigenvalue {d:.3e}")
        assert d <= dr.SHIFT_TOL[storage]
        # without it the rotation block of the far scene is |p|^2: two of its values are five orders above the scene's own
        c0 = dr.cloud_center(dr.source("far_corridor", noisy, dr.LOOP_N), storage)
        raw = dr.analyse(dr.step_record("far_corridor", noisy, dr.LOOP_N, storage), np.eye(4), c0, 0.0, 0.0, recentre=False)
        assert (raw.eigenvalues[1:3] > 100 * far.eigenvalues[1:3]).all(), (raw.eigenvalues, far.eigenvalues)


@pytest.mark.parametrize("storage", dr.STORAGES)
def test_the_ordinary_loop_slides_along_the_corridor_and_the_constrained_one_does_not(storage):
    c0 = dr.cloud_center(dr.source("corridor", True, dr.LOOP_N), storage)
    plain = dr.reference_registration("corridor", True, storage, 0.0, 0.0)
    held = dr.reference_registration("corridor", True, storage, dr.MIN_ROT, dr.MIN_TRANS)
    slide = abs(float(dr.centre_motion(plain["transformation"], np.eye(4), c0) @ dr.AXIS))
    stay = abs(float(dr.centre_motion(held["transformation"], np.eye(4), c0) @ dr.AXIS))
    _, across, angle = dr.pose_error(held["transformation"], "corridor", c0)
    print(f"noisy corridor {storage}: the ordinary loop moves the centre {1e3 * slide:.2f} mm along the axis, the constrained one "
          f"{1e3 * stay:.3f} mm; left across the axis {1e3 * across:.3f} mm, angle {angle:.3e} rad; fitness {plain['fitness']:.4f} / "
          f"{held['fitness']:.4f}, rmse {plain['inlier_rmse']:.5f} / {held['inlier_rmse']:.5f}")
    assert plain["n_passes_constrained"] == 0 and not plain["ever_degenerate"].any()
    assert slide > dr.SLIDE_MIN
    assert plain["fitness"] == 1.0  # ... and nothing the Mapper gates on has noticed
    assert held["n_passes_constrained"] == held["iterations"] == 12 and tuple(np.flatnonzero(held["ever_degenerate"])) == (3,)
    assert stay <= dr.ALONG_TOL
    assert across <= dr.TRUTH_TOL and angle <= dr.TRUTH_TOL


def test_the_constrained_update_minimises_the_quadratic_in_the_kept_directions():
    """x = B z with B the kept columns of M V; z the least-squares solution of |S^T B z - S^+ g| with H = S S^T (numpy.linalg.lstsq)"""
    for name, noisy, st in CASES:
        if not dr.EXPECTED[name]:
            continue
        an = _analysis(name, noisy, st, (dr.MIN_ROT, dr.MIN_TRANS))
        rec = dr.step_record(name, noisy, dr.LOOP_N, st)
        H, g = cr.jtj_from_record(rec), -rec[21:27]
        kept = np.flatnonzero(an.degenerate == 0)
        B = (an.M @ an.eigenvectors)[:, kept]
        w, Q = np.linalg.eigh(H)
        on = w > 1e-12 * w.max()
        St = np.sqrt(w[on])[:, None] * Q[:, on].T
        rhs = (Q[:, on].T @ g) / np.sqrt(w[on])
        z = np.linalg.lstsq(St @ B, rhs, rcond=None)[0]
        want = B @ z
        # the restatement solves a system of condition cond(B^T H B) in f64; the reference factors H itself, in the parameters about the
        # map origin, whose condition (far corridor: 1e6) is the larger of the two
        tol = 256 * EPS * max(np.linalg.cond(B.T @ H @ B), w[on].max() / w[on].min()) * np.abs(want).max()
        assert np.abs(an.x - want).max() <= tol, (name, noisy, st, an.x, want)
        # no component along a dropped direction, in the re-centred parameters
        y = an.eigenvectors.T @ np.linalg.solve(an.M, an.x)
        assert np.abs(y[an.degenerate == 1]).max() <= 64 * EPS * np.abs(y).max()


def test_edge_cases_of_the_rule():
    rec = dr.step_record("corridor", True, dr.LOOP_N, F64)
    c0 = dr.cloud_center(dr.source("corridor", True, dr.LOOP_N), F64)
    none = dr.analyse(rec, np.eye(4), c0, 0.0, 0.0)
    assert none.n_degenerate == 0 and (none.x == dr.ordinary_x(rec)).all()  # thresholds 0: the ordinary solve of the original record
    lam = none.eigenvalues
    at = dr.analyse(rec, np.eye(4), c0, float(lam[0]), float(lam[3]))  # `<` as written: a value AT its threshold is kept
    assert at.n_degenerate == 0
    above = dr.analyse(rec, np.eye(4), c0, float(np.nextafter(lam[0], np.inf)), float(np.nextafter(lam[3], np.inf)))
    assert tuple(np.flatnonzero(above.degenerate)) == (0, 3)
    everything = dr.analyse(rec, np.eye(4), c0, 1e300, 1e300)
    assert everything.n_degenerate == 6 and (everything.x == 0.0).all() and not np.signbit(everything.x).any()
    empty = dr.analyse(np.zeros(32), np.eye(4), c0, 0.0, 0.0)  # n_corr == 0: all six, every value +0.0, V = I
    assert empty.n_degenerate == 6 and (empty.eigenvalues == 0.0).all() and not np.signbit(empty.eigenvalues).any()
    assert (empty.eigenvectors == np.eye(6)).all() and (empty.x == 0.0).all()
    assert dr.register(np.zeros((0, 3)), dr.scene("room", False).tgt, dr.scene("room", False).tgt_nrm, dr.R, F32, 0.0, 0.0)["iterations"] == 0
    assert set(dr.STEP_SIZES) >= {1, 255, 256, 257} and max(dr.STEP_SIZES) > 4 * 256
