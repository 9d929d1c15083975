"""The numpy restatement of the robust-loss steps (tests/robust_icp_restatement.py) held against independent formulations, and the
premises of every case tests/test_robust_icp_gpu.py runs -- so that a failure there is the device's.

Tolerances.  A weight is held to its loss by a central difference of the loss with step h = 1e-5 on residuals of at most 0.2 and k of
0.02 to 0.05: the truncation error is h^2 / 6 times the third derivative (at most ~1 / k^2 = 2500 for these losses away from the kinks:
4e-8) and the rounding error 2^-53 |rho| / h (1e-13): 1e-6, as the issue sets it.  For the record, 1e-9 per term relative to the sum of that
term's |addends| (the two sums differ by reordering and by the extended precision only).
"""
import numpy as np
import pytest

import colored_icp_restatement as cr
import robust_icp_restatement as rr

STORAGES = rr.STORAGES
EST_IDS = [name for _, name in rr.ESTIMATORS]
EST = [e for e, _ in rr.ESTIMATORS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the weights
@pytest.mark.parametrize("kind,k", [(rr.L2, 0.0), (rr.L1, 0.0), (rr.HUBER, 0.02), (rr.CAUCHY, 0.02), (rr.GM, 0.01), (rr.TUKEY, 0.05)],
                         ids=lambda v: rr.LOSS_NAMES[v] if isinstance(v, int) else str(v))
def test_weight_times_residual_is_the_derivative_of_the_loss(kind, k):
    h = 1e-5
    r = np.linspace(-0.2, 0.2, 401)  # steps of 1e-3
    kinks = [0.0] if kind == rr.L1 else [-k, k] if kind in (rr.HUBER, rr.TUKEY) else []
    for x in kinks:
        r = r[np.abs(r - x) > 10 * h]
    assert len(r) >= 398
    slope = (rr.rho(kind, k, r + h) - rr.rho(kind, k, r - h)) / (2 * h)
    err = np.abs(rr.weight(kind, k, r) * r - slope)
    assert err.max() <= 1e-6, err.max()


def test_weights_at_their_special_points():
    k = rr.EDGE_K
    r = np.array([0.0, -0.0, k / 2, k, 2 * k, -2 * k, np.nan, np.inf])
    assert (rr.weight(rr.L2, k, r) == 1).all()
    np.testing.assert_array_equal(rr.weight(rr.L1, k, r), [1, 1, 2 / k, 1 / k, 0.5 / k, 0.5 / k, np.nan, 0])
    np.testing.assert_array_equal(rr.weight(rr.HUBER, k, r), [1, 1, 1, 1, 0.5, 0.5, 1, 0])      # NaN > k is false
    np.testing.assert_array_equal(rr.weight(rr.TUKEY, k, r), [1, 1, 0.5625, 0, 0, 0, 0, 0])     # NaN < 1 is false
    np.testing.assert_array_equal(rr.weight(rr.CAUCHY, k, r), [1, 1, 0.8, 0.5, 0.2, 0.2, np.nan, 0])
    assert np.isnan(rr.weight(rr.GM, k, r)[6]) and rr.weight(rr.GM, k, r)[7] == 0 and rr.weight(rr.GM, k, r)[0] == 1 / k


# ---------------------------------------------------------------------------------------------------------------- the record
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("estimator", EST, ids=EST_IDS)
@pytest.mark.parametrize("n", rr.STEP_SIZES)
def test_record_agrees_with_the_dense_longdouble_form(n, estimator, storage):
    P = rr._step_pairs(n, "near", estimator, storage)
    # premises of the GPU case: some queries have a correspondence and some have none
    assert 0.2 * n < P.have.sum() < n, P.have.sum()
    m = P.have
    for kind, k in rr.STEP_LOSSES:
        rec = rr.reference_step(n, "near", estimator, kind, k, storage)
        if estimator == rr.COLORED:
            J, res = np.concatenate([P.JG[m], P.JI[m]]), np.concatenate([P.rG[m], P.rI[m]])
        else:
            J, res = P.J[m], P.r[m]
        w = rr.weight(kind, k, res)
        want, scale = rr.dense_longdouble(J, res, w, m, P.d2)
        assert rec[28] == m.sum() and (rec[30:] == 0).all()
        assert (np.abs(rec[:30] - want) <= 1e-9 * scale).all(), (rr.LOSS_NAMES[kind], np.abs(rec[:30] - want) / np.maximum(scale, 1e-300))
        if kind != rr.L2:  # the loss does something on this case: residuals of a few centimetres against k = 0.02
            l2 = rr.reference_step(n, "near", estimator, rr.L2, k, storage)
            # (not every term moves: n.y n.y is zero on a floor and a wall at x = 0, and Huber leaves small intensity residuals alone)
            assert (_bits(rec[:27]) != _bits(l2[:27])).sum() >= 15 and (_bits(rec[27:]) == _bits(l2[27:])).all()
    assert (rr.reference_step(n, "far", estimator, rr.TUKEY, rr.STEP_K, storage) == 0).all()


@pytest.mark.parametrize("storage", STORAGES)
def test_the_three_identities(storage):
    s = cr.sliding_scene()
    grad = cr.reference_gradients("scene", storage)
    for n in rr.STEP_SIZES[:3]:
        src, col = cr.step_source(n)
        for pose, T in cr.STEP_POSES:
            # COLORED with L2 is the coloured step; POINT_TO_PLANE with L2 the geometric record
            for lam in cr.STEP_LAMBDAS:
                got = rr.step_record(rr.COLORED, rr.L2, 0.0, src, s.tgt, s.tgt_nrm, T, rr.STEP_R, storage, col, s.tgt_col, grad, lam)
                assert (_bits(got) == _bits(cr.step_record(src, col, s.tgt, s.tgt_nrm, s.tgt_col, grad, T, rr.STEP_R, lam, storage))).all()
            got = rr.step_record(rr.POINT_TO_PLANE, rr.L2, 0.0, src, s.tgt, s.tgt_nrm, T, rr.STEP_R, storage)
            assert (_bits(got) == _bits(cr.geometric_record(src, s.tgt, s.tgt_nrm, T, rr.STEP_R, storage))).all()
            # POINT_TO_PLANE with any loss is COLORED at lambda = 1 with finite gradients
            assert np.isfinite(grad).all()
            for kind, k in rr.STEP_LOSSES:
                a = rr.step_record(rr.POINT_TO_PLANE, kind, k, src, s.tgt, s.tgt_nrm, T, rr.STEP_R, storage)
                b = rr.step_record(rr.COLORED, kind, k, src, s.tgt, s.tgt_nrm, T, rr.STEP_R, storage, col, s.tgt_col, grad, 1.0)
                assert (_bits(a) == _bits(b)).all(), (n, pose, rr.LOSS_NAMES[kind])


# ---------------------------------------------------------------------------------------------------------------- edge pairs
@pytest.mark.parametrize("storage", STORAGES)
def test_premises_of_the_edge_pairs(storage):
    s, k = rr.edge_scene(), rr.EDGE_K
    assert (cr.to_storage(s.src, storage) == s.src).all() and (cr.to_storage(s.tgt, storage) == s.tgt).all()  # exact in the storage type
    P = rr.plane_pairs(s.src, s.tgt, s.tgt_nrm, np.eye(4), rr.EDGE_R, storage)
    assert P.have.all()
    assert (P.r.reshape(4, 4) == [0.0, k / 2, k, 2 * k]).all()  # exactly
    assert (P.d2 == s.heights ** 2).all()
    C = cr.pairs(s.src, s.src_col, s.tgt, s.tgt_nrm, s.tgt_col, rr.edge_gradients(storage), np.eye(4), rr.EDGE_R, 1.0, storage)
    assert (C.rG == P.r).all() and (C.rI == 0).all() and np.abs(rr.edge_gradients(storage)).max() > 0  # lambda = 1: r_I is a zero
    w = {kind: rr.weight(kind, k, P.r).reshape(4, 4)[0] for kind in range(6)}
    assert w[rr.L1][0] == 1 and w[rr.L1][1] == 2 / k     # L1's r == 0 rule
    assert (w[rr.HUBER] == [1, 1, 1, 0.5]).all()         # Huber at e == k: 1
    assert (w[rr.TUKEY] == [1, 0.5625, 0, 0]).all()      # Tukey at and beyond k: 0
    for est in EST:
        for lam in rr.EDGE_LAMBDAS:
            for kind, kk in rr.EDGE_LOSSES:
                assert np.isfinite(rr.reference_edge(est, kind, kk, lam, storage)).all()
                assert rr.reference_edge(est, kind, kk, lam, storage)[28] == 16  # a pair of weight 0 is still counted
        # every pair at or beyond Tukey's k: no normal equations, yet r^2, the count and d2 are there
        lam = 1.0
        rec = rr.reference_edge(est, rr.TUKEY, k, lam, storage, beyond_only=True)
        assert (rec[:27] == 0).all() and rec[27] == 4 * (k * k + 4 * k * k) and rec[28] == 8 and rec[29] == rec[27]
        assert (rr.reference_edge(est, rr.L2, 0.0, lam, storage, beyond_only=True)[:27] != 0).any()
    # ... and the registration takes the identity update from it
    b = s.beyond
    res = rr.register(rr.POINT_TO_PLANE, rr.TUKEY, k, s.src[b], s.tgt, s.tgt_nrm, rr.EDGE_R, storage, max_iter=2, rel_fitness=0.0, rel_rmse=0.0)
    assert (res["transformation"] == np.eye(4)).all() and res["iterations"] == 2 and res["fitness"] == 1.0


# ---------------------------------------------------------------------------------------------------------------- the outlier case
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("estimator", EST, ids=EST_IDS)
def test_the_outlier_case(estimator, storage):
    """the purpose of the feature: 300 raised floor points inside the correspondence distance pull the L2 pose by centimetres; the
    robust losses take most of that away"""
    errors = {}
    for kind, k in rr.OUTLIER_LOSSES:
        res = rr.outlier_result(estimator, kind, k, storage)
        errors[kind] = cr.translation_error(res["transformation"])
        assert res["iterations"] == rr.OUTLIER["max_iter"] and not res["converged"]
    print(f"outlier case {EST_IDS[estimator]} {storage}: " + ", ".join(f"{rr.LOSS_NAMES[kd]} {1e3 * e:.3f} mm" for kd, e in errors.items()))
    rr.outlier_conditions(errors)
    # fitness and rmse carry no weight: those of a pose, not of a loss
    s = rr.outlier_scene()
    assert len(s.src) == 2048 and len(s.tgt) == 2048
