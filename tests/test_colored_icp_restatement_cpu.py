"""The numpy restatement of coloured ICP (tests/colored_icp_restatement.py) held against independent formulations, and the premises of
every case tests/test_colored_icp_gpu.py runs -- so that a failure there is the device's.

Tolerances.  1e-9 is the project's restatement-vs-restatement bar.  For the gradients it is taken relative to
max(1, |g|_inf) on the points whose 3x3 system has a condition number below 1e6: the restatement solves the normal equations, whose
error grows like cond(M) 2^-53 (1e-10 at the cut), np.linalg.lstsq works on the rows; beyond the cut the two are not expected to agree
to nine digits and the stated departure (a failed pivot gives zero, where lstsq gives the minimum-norm solution) sets in.  For the record
it is taken per term relative to the sum of that term's |addends|: the two sums differ by reordering and by the extended precision only.
"""
import numpy as np
import pytest

import colored_icp_restatement as cr
import neighbor_restatement as nbr

STORAGES = cr.STORAGES


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["scene", "edges"])
def test_gradients_agree_with_lstsq(name, storage):
    case = next(c for c in cr.GRAD_CASES if c.name == name)
    pts, nrm, col = case.cloud()
    got = cr.reference_gradients(name, storage)
    want = cr.gradients_lstsq(pts, nrm, col, case.radius, case.max_nn, storage)
    A, _, rows = cr.gradient_rows(pts, nrm, col, case.radius, case.max_nn, storage)
    well = np.zeros(len(rows), bool)
    for i in np.flatnonzero(rows):
        a = A[i, :rows[i]]
        well[i] = np.isfinite(a).all() and np.linalg.cond(a.T @ a) < 1e6
    if name == "scene":
        assert well.mean() > 0.95, well.mean()
    assert well.sum() >= 40
    err = np.abs(got[well] - want[well]).max(axis=1) / np.maximum(1.0, np.abs(want[well]).max(axis=1))
    assert err.max() <= 1e-9, err.max()


@pytest.mark.parametrize("storage", STORAGES)
def test_a_linear_intensity_gives_its_own_tangential_gradient(storage):
    rng = np.random.default_rng(5)
    n = 400
    # a tilted plane through the origin: two tangents u, v and the normal w; I = 0.4 + 0.3 s - 0.2 t in the plane's coordinates (s, t)
    w = np.array([1.0, 2.0, 2.0]) / 3.0
    u = np.array([2.0, 1.0, -2.0]) / 3.0
    v = np.cross(w, u)
    st = rng.uniform(0.0, 2.0, (n, 2))
    pts = st[:, :1] * u + st[:, 1:] * v
    inten = 0.4 + 0.3 * st[:, 0] - 0.2 * st[:, 1]
    col = np.repeat(inten[:, None], 3, axis=1)
    nrm = np.tile(w, (n, 1))
    g = cr.gradients(pts, nrm, col, 0.4, 30, storage)
    L = nbr.search(pts, pts, 30, 0.4, storage)
    full = L.cnt >= 4
    assert full.sum() > 0.9 * n
    want = 0.3 * u - 0.2 * v
    # the stored values are rounded (f32 storage: 2^-24 relative on coordinates, normals and intensities, amplified by 1 / neighbour
    # distance ~ 1 / 0.05 on an intensity difference): 1e-9 in f64, 1e-4 in f32
    tol = 1e-9 if storage == cr.F64 else 1e-4
    assert np.abs(g[full] - want).max() <= tol, np.abs(g[full] - want).max()
    assert np.abs(g[full] @ w).max() <= tol  # tangential


def test_the_scene_texture_is_recovered_roughly():
    """the sliding case's gradients point where the analytic texture gradient's tangential part points (a sanity check of the scene, not a
    bound on the estimator: 18 to 30 neighbours over a texture of 1 m wavelength)"""
    s = cr.sliding_scene()
    g = cr.reference_gradients("scene", cr.F64)
    a = cr.texture_gradient(s.tgt)
    a = a - np.sum(a * s.tgt_nrm, axis=1, keepdims=True) * s.tgt_nrm
    cos = np.sum(g * a, axis=1) / np.maximum(np.linalg.norm(g, axis=1) * np.linalg.norm(a, axis=1), 1e-12)
    assert np.median(cos) > 0.95, np.median(cos)


@pytest.mark.parametrize("storage", STORAGES)
def test_premises_of_the_gradient_edge_cases(storage):
    pts, nrm, col = cr.edge_cloud()
    L = nbr.search(pts, pts, cr.GRADIENT_MAX_NN, cr.EDGE_RADIUS, storage)
    g = cr.reference_gradients("edges", storage)
    E = cr.EDGE
    sl = {k: slice(*v) for k, v in E.items()}
    assert (L.cnt[sl["three"]] == 3).all() and (g[sl["three"]] == 0).all()
    assert (L.cnt[sl["four"]] == 4).all() and (np.abs(g[sl["four"]]).max(axis=1) > 0).all()
    assert (L.cnt[sl["dense"]] == 30).all() and (L.total[sl["dense"]] == 50).all()
    assert (np.abs(g[sl["dense"]]).max(axis=1) > 0).all()
    d0, d1 = E["duplicates"]
    first = L.idx[d0:d1, 0]
    assert (first[4:] != np.arange(d0 + 4, d1)).all() and (first[:4] == np.arange(d0, d0 + 4)).all()  # the copy's first entry is the original
    assert (L.d2[d0:d1, 1] == 0).all() and (L.cnt[d0:d1] == 8).all()
    z0 = E["zero_normal"][0]
    assert (nrm[z0 + 4] == 0).all() and L.cnt[z0 + 4] == 9 and (g[z0 + 4] == 0).all()
    assert (np.abs(np.delete(g[sl["zero_normal"]], 4, axis=0)).max(axis=1) > 0).all()
    n0 = E["nan"][0]
    assert np.isnan(pts[n0 + 2, 1]) and L.cnt[n0 + 2] == 0 and (g[n0 + 2] == 0).all()
    assert (np.delete(L.cnt[sl["nan"]], 2) == 8).all() and np.isfinite(g).all()
    assert (L.cnt[sl["line"]] == 6).all() and (g[sl["line"]] == 0).all()


@pytest.mark.parametrize("storage", STORAGES)
def test_uniform_colours_give_zero_gradients(storage):
    assert (cr.reference_gradients("uniform", storage) == 0).all()
    assert (np.abs(cr.reference_gradients("scene", storage)).max(axis=1) > 0).mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------- the record
def test_the_sum_order():
    rng = np.random.default_rng(9)
    for n in (1, 255, 256, 257, 513):
        t = rng.integers(-1000, 1000, (n, 3)).astype(np.float64)
        assert (cr.block_tree_sum(t) == t.sum(axis=0)).all()  # (integers: exact in any order)
    # 256 + 1 terms of which the tree of the first block loses the small ones and the second block's survives
    t = np.zeros((257, 1))
    t[0] = 2.0 ** 53
    t[1:256] = 1.0     # pairs of ones meet first: the block's sum is 2^53 + 254 (the one at t = 128 meets 2^53 and is lost)
    t[256] = 1.0
    v = np.zeros(256)
    v[:] = t[:256, 0]
    s = 128
    while s >= 1:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    assert v[0] == 2.0 ** 53 + 254.0  # (added one after the other onto 2^53, every one of the ones would be lost)
    assert cr.block_tree_sum(t)[0] == v[0] + 1.0


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("lam", cr.STEP_LAMBDAS)
@pytest.mark.parametrize("pose", [p for p, _ in cr.STEP_POSES])
@pytest.mark.parametrize("n", cr.STEP_SIZES)
def test_record_agrees_with_the_dense_longdouble_form(n, pose, lam, storage):
    s = cr.sliding_scene()
    src, col = cr.step_source(n)
    T = dict(cr.STEP_POSES)[pose]
    P = cr.pairs(src, col, s.tgt, s.tgt_nrm, s.tgt_col, cr.reference_gradients("scene", storage), T, cr.STEP_R, lam, storage)
    # premises of the GPU case: some queries have a correspondence and some have none, in the last block too
    assert 0.2 * n < P.have.sum() < n, P.have.sum()
    rec = cr.reference_step(n, pose, lam, storage)
    want, scale = cr.record_dense_longdouble(P)
    assert rec[28] == P.have.sum() and (rec[30:] == 0).all()
    assert (np.abs(rec[:30] - want) <= 1e-9 * scale).all(), np.abs(rec[:30] - want) / np.maximum(scale, 1e-300)


@pytest.mark.parametrize("storage", STORAGES)
def test_premises_of_the_step_edge_cases(storage):
    s = cr.sliding_scene()
    for n in cr.STEP_SIZES:
        assert (cr.reference_step(n, "far", cr.LAMBDA_DEFAULT, storage) == 0).all()
        src, col = cr.step_source(n)
        for pose, T in cr.STEP_POSES:
            # lambda = 1: the photometric half vanishes, rows [0..27] are the pure geometric record bit for bit
            geo = cr.geometric_record(src, s.tgt, s.tgt_nrm, T, cr.STEP_R, storage)
            one = cr.reference_step(n, pose, 1.0, storage)
            assert (_bits(one[:28]) == _bits(geo[:28])).all() and one[28] > 0
            # lambda = 0: no geometric half -- the rotational rows survive through the photometric Jacobian alone
            zero = cr.reference_step(n, pose, 0.0, storage)
            assert zero[28] == one[28] and zero[29] == one[29] and not (_bits(zero[:28]) == _bits(one[:28])).all()
            # a target whose gradients are all zero: J_I = 0, the record is lambda times the geometric one plus the intensity residuals
            flat = cr.reference_step(n, pose, cr.LAMBDA_DEFAULT, storage, zero_gradients=True)
            np.testing.assert_allclose(flat[:27], cr.LAMBDA_DEFAULT * geo[:27], rtol=1e-12, atol=1e-15)
            assert flat[27] > cr.LAMBDA_DEFAULT * geo[27]


# ---------------------------------------------------------------------------------------------------------------- the registration
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("r,lam", cr.SLIDING_PARAMS)
def test_the_sliding_case(r, lam, storage):
    """the purpose of the feature: the translation along the floor / wall edge, which geometry does not see, is found from the colours"""
    res = cr.sliding_result(r, lam, storage)
    err = cr.translation_error(res["transformation"])
    print(f"sliding case r={r} lambda={lam} {storage}: translation error {err:.3e} m, fitness {res['fitness']:.4f}, rmse {res['inlier_rmse']:.4e}")
    assert res["iterations"] == 10 and not res["converged"]
    assert err < cr.SLIDE / 10.0, err


def test_geometry_alone_does_not_see_the_slide():
    """at lambda = 1 (point-to-plane) the normal matrix of the scene has no component along the edge: the translation in y is its null
    vector; with the colours it has none"""
    s = cr.sliding_scene()
    grad = cr.reference_gradients("scene", cr.F64)
    for lam, singular in ((1.0, True), (cr.LAMBDA_DEFAULT, False)):
        rec = cr.step_record(s.src, s.src_col, s.tgt, s.tgt_nrm, s.tgt_col, grad, np.eye(4), 0.15, lam, cr.F64)
        w, V = np.linalg.eigh(cr.jtj_from_record(rec))
        if singular:
            assert w[0] < 1e-12 * w[-1] and abs(V[4, 0]) > 1.0 - 1e-9, (w, V[:, 0])
        else:
            assert w[0] > 1e-6 * w[-1], w


@pytest.mark.parametrize("storage", STORAGES)
def test_the_converging_case_stops_before_max_iteration(storage):
    c = cr.CONVERGING
    res = cr.sliding_result(c["r"], c["lam"], storage, c["max_iter"], 1e-6)
    print(f"converging case {storage}: iterations {res['iterations']}, error {cr.translation_error(res['transformation']):.3e} m")
    assert res["converged"] and 1 < res["iterations"] < c["max_iter"] - 10, res["iterations"]
    assert cr.translation_error(res["transformation"]) < cr.SLIDE / 10.0


def test_loop_edge_cases():
    s = cr.sliding_scene()
    empty = cr.register(np.zeros((0, 3)), np.zeros((0, 3)), s.tgt, s.tgt_nrm, s.tgt_col, 0.15, cr.F64, init=cr.NEAR_POSE, tgt_grad=np.zeros(s.tgt.shape))
    assert empty["fitness"] == 0 and (empty["transformation"] == cr.NEAR_POSE).all()
    none = cr.register(s.src[:50], s.src_col[:50], s.tgt, s.tgt_nrm, s.tgt_col, 0.15, cr.F64, max_iter=0, tgt_grad=np.zeros(s.tgt.shape))
    assert none["iterations"] == 0 and (none["transformation"] == np.eye(4)).all() and none["fitness"] > 0
