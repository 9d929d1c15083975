"""FPFH features, feature correspondences and RANSAC global registration on the device (o3ds_compute_fpfh,
o3ds_feature_correspondences, o3ds_ransac_feature_matching) against the numpy restatement (tests/fpfh_ransac_restatement.py), and
PlaceRecognition end to end."""
import math
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402
from child_process import ROOT, run_child  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402
from open3d_slam_amd import parameters as prm  # noqa: E402
from open3d_slam_amd.place_recognition import PlaceRecognition, toRPY  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402
from open3d_slam_amd.submap import Submap  # noqa: E402

pytestmark = pytest.mark.gpu


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sparse_cloud(seed=11, n=2000):
    """a seeded sparse cloud with a duplicated point, an isolated point and a point with exactly one neighbour (radius 1.0)"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-6.0, 6.0, (n, 3)) * [1.0, 1.0, 0.3]
    N = _unit(rng.normal(size=(n, 3)))
    P = np.vstack([P, P[5:6], [[40.0, 40.0, 40.0]], [[-40.0, 0.0, 0.0]], [[-40.0, 0.5, 0.0]]])
    N = np.vstack([N, N[7:8], [[0, 0, 1.0]], [[1.0, 0, 0]], [[0, 1.0, 0]]])
    return P, N


def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def scene_points(rng, spacing=0.12):
    """ground + boxes and cylinders of varied size in a 36 m square (surface samples, a fresh draw per call)"""
    g = np.random.default_rng(1234)  # the SCENE is fixed; the samples are not
    pts = []
    area = 36.0 * 36.0
    m = int(area / spacing ** 2 * 0.5)
    pts.append(np.column_stack([rng.uniform(-18, 18, m), rng.uniform(-18, 18, m), rng.normal(0, 0.01, m)]))
    for _ in range(14):  # boxes
        c = g.uniform(-15, 15, 2)
        sx, sy, sz = g.uniform(0.6, 3.5), g.uniform(0.6, 3.5), g.uniform(0.8, 3.0)
        yaw = g.uniform(0, np.pi)
        k = int(2 * (sx * sy + sx * sz + sy * sz) / spacing ** 2 * 0.5)
        u = rng.uniform(-0.5, 0.5, (k, 3))
        face = rng.integers(0, 6, k)
        u[np.arange(k), face // 2] = np.where(face % 2 == 0, -0.5, 0.5)
        b = u * [sx, sy, sz] + [0, 0, sz / 2]
        b = b @ _rz(yaw).T + [c[0], c[1], 0]
        pts.append(b[b[:, 2] >= 0.05])
    for _ in range(10):  # cylinders
        c = g.uniform(-15, 15, 2)
        r, h = g.uniform(0.2, 1.2), g.uniform(1.0, 4.0)
        k = int(2 * np.pi * r * h / spacing ** 2 * 0.5)
        a = rng.uniform(0, 2 * np.pi, k)
        pts.append(np.column_stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a), rng.uniform(0.05, h, k)]))
    return np.vstack(pts)


def make_T(yaw_deg, t):
    T = np.eye(4)
    T[:3, :3] = _rz(math.radians(yaw_deg))
    T[:3, 3] = t
    return T


def make_submap(be, pts, params, id_):
    sm = Submap(be, id_)
    sm.setParameters(params)
    raw = PointCloud.from_numpy(be, pts)
    vox = be.voxel_down_sample(raw.id, params.mapBuilder_.mapVoxelSize_)
    raw.release()
    be.estimate_normals(vox, 1.0, 20)
    sm.mapCloud_.release()
    sm.mapCloud_ = PointCloud(be, vox)
    sm.computeFeatures()
    return sm


def pr_params():
    p = prm.lua_default_mapper_parameters()
    p.placeRecognition_ = prm.lua_place_recognition_parameters()
    return p


@pytest.fixture(scope="module")
def be64():
    be = backend.Backend(0, backend.PRECISION_F64)
    yield be
    be.close()


@pytest.fixture(scope="module")
def pair(be64):
    """two submaps of the same scene, each in its own frame: target = T_gt * (a fresh sampling of the scene)"""
    rng = np.random.default_rng(77)
    T_gt = make_T(35.0, [3.0, -2.0, 0.3])
    src = scene_points(rng)
    tgt = scene_points(rng) @ T_gt[:3, :3].T + T_gt[:3, 3]
    p = pr_params()
    a, b = make_submap(be64, src, p, 0), make_submap(be64, tgt, p, 1)
    return a, b, T_gt, p


def _pose_err(T, G):
    dt = np.linalg.norm(T[:3, 3] - G[:3, 3])
    c = (np.trace(G[:3, :3].T @ T[:3, :3]) - 1) / 2
    return dt, math.degrees(math.acos(max(-1.0, min(1.0, c))))


# ---- 1. FPFH --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,max_nn", [(1.5, 30), (0.6, 128)])  # cap-bound, radius-bound
def test_fpfh_matches_restatement_f64(be64, radius, max_nn):
    P, N = sparse_cloud()
    cid = be64.upload(P, N)
    be64.compute_fpfh(cid, radius, max_nn)
    assert be64.has_fpfh(cid)
    got = be64.fpfh(cid)
    ref = rs.fpfh(P, N, radius, max_nn, cKDTree(P))
    counts = [len(x[0]) for x in rs.neighbours(P, radius, max_nn, cKDTree(P))]
    if max_nn == 30:
        assert max(counts) == 30  # the cap binds somewhere
    else:
        assert max(counts) < 128
    assert counts[-1] == 2 and counts[-2] == 2 and counts[-3] == 1  # one neighbour each; isolated
    assert np.all(got[-3] == 0.0)
    assert np.max(np.abs(got - ref)) <= 1e-9
    be64.free(cid)


def test_fpfh_f32_storage(backend_f32):
    """f32 storage: the device widens the stored (rounded) coordinates and normals and does the same f64 arithmetic, so the restatement
    on the rounded values is held to the f64 tolerance, 1e-9 per entry"""
    P, N = sparse_cloud(seed=5)
    P32 = P.astype(np.float32).astype(np.float64)
    N32 = N.astype(np.float32).astype(np.float64)
    cid = backend_f32.upload(P, N)
    backend_f32.compute_fpfh(cid, 1.0, 50)
    got = backend_f32.fpfh(cid)
    ref = rs.fpfh(P32, N32, 1.0, 50, cKDTree(P32))
    assert np.max(np.abs(got - ref)) <= 1e-9
    backend_f32.free(cid)


# ---- 2. correspondences ---------------------------------------------------------------------------------------------------------
def _nn_ok(A, B, got):
    """got[i] is a nearest feature of A[i] among B (within 1e-9 relative of the best)"""
    d, j = cKDTree(B).query(A, k=2)
    dg = np.sum((A - B[got]) ** 2, axis=1)
    best = d[:, 0] ** 2
    return np.all((got == j[:, 0]) | (dg <= best * (1 + 1e-9) + 1e-300))


def test_feature_correspondences(be64, pair):
    a, b, _, _ = pair
    sa, sb = a.getSparseMapPointCloud().id, b.getSparseMapPointCloud().id
    Fa, Fb = a.getFeatures(), b.getFeatures()
    one, fb = be64.feature_correspondences(sa, sb, mutual=False)
    assert not fb and len(one) == len(Fa)
    assert np.array_equal(one[:, 0], np.arange(len(Fa)))
    assert _nn_ok(Fa, Fb, one[:, 1].astype(np.int64))
    mut, fb = be64.feature_correspondences(sa, sb, mutual=True, ransac_n=3)
    back = cKDTree(Fa).query(Fb, k=1)[1]
    exp = [(i, j) for i, j in zip(range(len(Fa)), one[:, 1]) if back[j] == i]
    assert not fb and len(mut) >= 9
    # near-ties may pick either winner: compare where the reverse match is unambiguous
    assert abs(len(mut) - len(exp)) <= max(2, len(exp) // 100)
    assert np.all(np.diff(mut[:, 0].astype(np.int64)) > 0)  # source order


def test_mutual_fallback(be64):
    rng = np.random.default_rng(3)
    P, N = rng.uniform(-3, 3, (40, 3)), _unit(rng.normal(size=(40, 3)))
    s, t = be64.upload(P, N), be64.upload(P[:1] + 0.01, N[:1])
    be64.compute_fpfh(s, 1.5, 20)
    be64.compute_fpfh(t, 1.5, 20)
    c, fb = be64.feature_correspondences(s, t, mutual=True, ransac_n=3)  # one target point: at most one mutual pair < 9
    assert fb and len(c) == 40 and np.all(c[:, 1] == 0)
    be64.free(s)
    be64.free(t)


# ---- 3. RANSAC replay -----------------------------------------------------------------------------------------------------------
def _place(T, P):
    """T p for every row of P, in the validate kernel's order of operations (one rounding each, no FMA)"""
    R, t = T[:3, :3], T[:3, 3]
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.column_stack([((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0], ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1],
                            ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]])


def replay_ransac(r, S, Tg, corr, seed, ransac_n, max_corr, edge, dist, n_iter, confidence, invariants=True):
    """Replays the trace of an o3ds_ransac_feature_matching call with trace=n_iter (r) on the host: the draws, the Umeyama fit, the two
    checkers, a cKDTree recount of every validated hypothesis and the serial stopping rule.  S, Tg: the stored source and target points;
    corr: the pairs feature_correspondences returned.  invariants: also assert, for every hypothesis run (degenerate samples included),
    a finite proper rotation that maps the sample's source centroid onto its target centroid and the least-squares cost of the
    restatement's Umeyama.  Returns {t: (pairs, rmse)} of the validated hypotheses."""
    tr = r["trace"]
    m = len(corr)
    run = r["iterations_run"]
    assert 0 < run <= n_iter
    tree = cKDTree(Tg)
    validated = {}
    recount = []
    for t in range(run):
        smp = rs.draw(seed, ransac_n, t, m)
        assert list(tr["sample"][t]) == smp
        ps, qs = S[corr[smp, 0]], Tg[corr[smp, 1]]
        T = tr["transformation"][t]
        sv = np.linalg.svd((qs - qs.mean(0)).T @ (ps - ps.mean(0)), compute_uv=False)
        U = rs.umeyama(ps, qs)
        if sv[1] > 1e-6 * sv[0]:  # a unique rotation (not a repeated draw or a collinear sample)
            assert np.allclose(T, U, atol=1e-9), t
        if invariants:
            R = T[:3, :3]
            assert np.all(np.isfinite(T)) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), t
            assert np.max(np.abs(R.T @ R - np.eye(3))) <= 1e-12, t
            assert abs(np.linalg.det(R) - 1.0) <= 1e-12, t  # a rotation, never a reflection
            assert np.max(np.abs(R @ ps.mean(0) + T[:3, 3] - qs.mean(0))) <= 1e-12, t
            assert abs(rs.ls_cost(T, ps, qs) - rs.ls_cost(U, ps, qs)) <= 1e-9, t
        e_ok, e_m = rs.edge_check(ps, qs, edge) if edge > 0 else (True, np.inf)
        d_ok, d_m = rs.distance_check(ps, qs, T, dist) if dist > 0 else (True, np.inf)
        if e_m > 1e-12 and d_m > 1e-12:
            assert tr["checks"][t] == (int(e_ok) | (int(d_ok) << 1)), t
        if tr["checks"][t] == 3:
            recount.append(t)
        else:
            assert tr["pairs"][t] == -1
    for k0 in range(0, len(recount), 64):  # the recount, 64 hypotheses per cKDTree call
        ts = recount[k0:k0 + 64]
        X = np.vstack([_place(tr["transformation"][t], S) for t in ts])
        _, j = tree.query(X, k=1, distance_upper_bound=max_corr * (1 + 1e-9))
        ok = j < len(Tg)
        d2 = np.full(len(X), np.inf)
        dd = Tg[j[ok]] - X[ok]
        d2[ok] = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        d2 = np.where(d2 < max_corr * max_corr, d2, np.nan).reshape(len(ts), len(S))
        for t, row in zip(ts, d2):
            inl = ~np.isnan(row)
            assert tr["pairs"][t] == int(inl.sum()), t
            if inl.any():
                assert tr["error_sum"][t] == pytest.approx(float(row[inl].sum()), rel=1e-12)
            pairs = int(tr["pairs"][t])
            validated[t] = (pairs, math.sqrt(tr["error_sum"][t] / pairs) if pairs else 0.0)
    assert np.all(tr["checks"][run:] == -1)
    exp_run, exp_best, exp_vals = rs.stopping_rule(n_iter, confidence, ransac_n, len(S), validated)
    assert (r["iterations_run"], r["best_t"], r["validations"]) == (exp_run, exp_best, exp_vals)
    assert len(validated) == r["validations"]
    bt = r["best_t"]
    if bt >= 0:
        assert np.array_equal(r["transformation"], tr["transformation"][bt])
        assert r["n_corr"] == tr["pairs"][bt] and r["fitness"] == tr["pairs"][bt] / len(S)
    return validated


def test_ransac_replay(be64, pair):
    a, b, _, p = pair
    cfg = p.placeRecognition_
    sa, sb = a.getSparseMapPointCloud(), b.getSparseMapPointCloud()
    S, _ = be64.download(sa.id)
    Tg, _ = be64.download(sb.id)
    corr, fb = be64.feature_correspondences(sa.id, sb.id, mutual=True, ransac_n=3)
    n_iter, seed = 4096, 12345
    r = be64.ransac_feature_matching(sa.id, sb.id, cfg.ransacMaxCorrespondenceDistance_, 3, True, cfg.correspondenceCheckerEdgeLength_,
                                     cfg.correspondenceCheckerDistance_, n_iter, cfg.ransacProbability_, seed, trace=n_iter)
    assert r["n_feature_corr"] == len(corr) and r["fell_back"] == fb
    validated = replay_ransac(r, S, Tg, corr, seed, 3, cfg.ransacMaxCorrespondenceDistance_, cfg.correspondenceCheckerEdgeLength_,
                              cfg.correspondenceCheckerDistance_, n_iter, cfg.ransacProbability_)
    assert len(validated) == r["validations"] and r["validations"] > 0
    assert r["best_t"] >= 0


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------
def _ransac_on(be, pts_a, pts_b, seed=99):
    p = pr_params()
    a, b = make_submap(be, pts_a, p, 0), make_submap(be, pts_b, p, 1)
    c = p.placeRecognition_
    r = be.ransac_feature_matching(a.getSparseMapPointCloud().id, b.getSparseMapPointCloud().id, c.ransacMaxCorrespondenceDistance_, 3,
                                   True, c.correspondenceCheckerEdgeLength_, c.correspondenceCheckerDistance_, 200000, c.ransacProbability_,
                                   seed)
    return r, a.getFeatures(), b.getFeatures()


def _pair_points(seed=5):
    rng = np.random.default_rng(seed)
    T = make_T(35.0, [3.0, -2.0, 0.3])
    return scene_points(rng), scene_points(rng) @ T[:3, :3].T + T[:3, 3]


def _plain(r):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items()}


def test_determinism_two_handles():
    pa, pb = _pair_points()
    outs = []
    for _ in range(2):
        be = backend.Backend(0, backend.PRECISION_F64)
        outs.append(_ransac_on(be, pa, pb))
        be.close()
    (r1, fa1, fb1), (r2, fa2, fb2) = outs
    assert np.array_equal(fa1, fa2) and np.array_equal(fb1, fb2)
    assert _plain(r1) == _plain(r2)
    assert r1["best_t"] >= 0


def _ransac_on_a_handle_of_its_own(ab):
    pa, pb = _pair_points()
    be = backend.Backend(0, backend.PRECISION_F64, ab=ab)
    r = _plain(_ransac_on(be, pa, pb)[0])
    be.close()
    return r


def test_batch_sizes_in_fresh_processes():
    """the A/B library with fixed batches of 1024 and 65536 hypotheses (the switch is read once per process: each size in a child
    process) and the shipped library's growing batches give bit-identical results"""
    outs = [run_child("test_place_recognition_gpu", "t._ransac_on_a_handle_of_its_own(True)", env=dict(O3DS_RANSAC_BATCH=batch), timeout=600, cwd=ROOT)[0]
            for batch in ("1024", "65536")]
    shipped = _ransac_on_a_handle_of_its_own(False)
    assert outs[0] == outs[1] == shipped


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------
def test_place_recognition_end_to_end(be64, pair):
    a, b, T_gt, p = pair
    p = pr_params()
    p.placeRecognition_.consistencyCheck_ = prm.PlaceRecognitionConsistencyCheckParameters()  # 90 deg: the 35 deg pair passes
    rec = PlaceRecognition(be64, p, seed=7)
    cons = rec.buildLoopClosureConstraints(a, [b], timestamp=12.5)
    r = rec.lastRansacResult
    dt, da = _pose_err(r["transformation"], T_gt)
    assert dt <= 0.5 and da <= 3.0, (dt, da, r)
    assert len(cons) == 1, r
    c = cons[0]
    dt, da = _pose_err(c.sourceToTarget_, T_gt)
    assert dt <= 0.02 and da <= 0.2, (dt, da)
    assert not c.isOdometryConstraint_ and c.isInformationMatrixValid_ and c.timestamp_ == 12.5
    assert (c.sourceSubmapIdx_, c.targetSubmapIdx_) == (0, 1)
    # the information matrix is a direct information_matrix_dev call on the same overlap clouds
    src, tgt = a.getMapPointCloud().id, b.getMapPointCloud().id
    i_s, i_t = be64.overlap_indices(src, tgt, r["transformation"], 20 * p.mapBuilder_.mapVoxelSize_, 1)
    so, to = be64.select_by_index(src, i_s.astype(np.uint32)), be64.select_by_index(tgt, i_t.astype(np.uint32))
    info = be64.information_matrix_dev(so, to, p.placeRecognition_.maxIcpCorrespondenceDistance_, c.sourceToTarget_)
    assert np.array_equal(info, c.informationMatrix_)
    be64.free(so)
    be64.free(to)


def test_no_constraint_without_shared_structure(be64, pair):
    a, _, _, p = pair
    rng = np.random.default_rng(8)
    noise = np.column_stack([rng.uniform(-18, 18, 60000), rng.uniform(-18, 18, 60000), rng.uniform(0, 4, 60000)])
    b = make_submap(be64, noise, p, 2)
    q = pr_params()
    q.placeRecognition_.consistencyCheck_ = prm.PlaceRecognitionConsistencyCheckParameters()
    assert PlaceRecognition(be64, q, seed=7).buildLoopClosureConstraints(a, [b]) == []


def test_large_yaw_rejected_by_consistency(be64):
    rng = np.random.default_rng(9)
    T = make_T(60.0, [2.0, 1.0, 0.0])
    p = pr_params()  # the shipped 30 deg drift limit
    a = make_submap(be64, scene_points(rng), p, 0)
    b = make_submap(be64, scene_points(rng) @ T[:3, :3].T + T[:3, 3], p, 1)
    rec = PlaceRecognition(be64, p, seed=7)
    assert rec.buildLoopClosureConstraints(a, [b]) == []
    r = rec.lastRansacResult
    if r["n_corr"] >= p.placeRecognition_.ransacMinCorrespondenceSetSize_:  # RANSAC found the 60 deg: the consistency check rejected it
        assert abs(math.degrees(toRPY(r["transformation"])[2])) > 30.0


# ---- 6. input errors ------------------------------------------------------------------------------------------------------------
def test_input_errors(be64):
    rng = np.random.default_rng(1)
    P = rng.uniform(-2, 2, (100, 3))
    bare = be64.upload(P)
    with pytest.raises(backend.BackendError) as e:
        be64.compute_fpfh(bare, 1.0, 30)
    assert e.value.code == backend.ERR_INVALID_ARG
    cid = be64.upload(P, _unit(rng.normal(size=(100, 3))))
    for bad in (0, 129):
        with pytest.raises(backend.BackendError) as e:
            be64.compute_fpfh(cid, 1.0, bad)
        assert e.value.code == backend.ERR_INVALID_ARG
    assert not be64.has_fpfh(cid)
    with pytest.raises(backend.BackendError) as e:  # features missing
        be64.ransac_feature_matching(cid, cid, 0.5)
    assert e.value.code == backend.ERR_INVALID_ARG
    with pytest.raises(backend.BackendError) as e:
        be64.feature_correspondences(cid, cid)
    assert e.value.code == backend.ERR_INVALID_ARG
    be64.compute_fpfh(cid, 1.0, 30)
    assert be64.has_fpfh(cid)
    r = be64.ransac_feature_matching(cid, cid, 0.5, ransac_n=2, max_iteration=1000)  # ransac_n < 3: the empty result
    assert np.array_equal(r["transformation"], np.eye(4)) and r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0
    assert r["n_corr"] == 0 and r["best_t"] == -1 and r["iterations_run"] == 0
    r = be64.ransac_feature_matching(cid, cid, 0.0, ransac_n=3)  # max_corr <= 0: empty as well
    assert r["best_t"] == -1 and r["fitness"] == 0.0
    with pytest.raises(backend.BackendError) as e:
        be64.ransac_feature_matching(cid, cid, 0.5, ransac_n=9)
    assert e.value.code == backend.ERR_INVALID_ARG
    be64.estimate_normals(cid, 1.0, 10)  # changing the normals drops the features
    assert not be64.has_fpfh(cid)
    be64.free(bare)
    be64.free(cid)
