"""FPFH, feature matching and RANSAC on the device at the shipped sizes and at their edges, against the numpy restatement
(tests/fpfh_ransac_restatement.py): kept lists longer than 64 with the cap binding, exact distance ties at the max_nn cut, more than
65,536 points (the grid-stride loop over points), reused indexes (K = 2), every pair-feature branch, exact feature nearest neighbours
with ties across tiles, the mutual fallback threshold, the capacity contract, RANSAC for ransac_n up to 8 with every checker setting,
more than 2,048 validations in one batch, the stopping rule's edges and the invariants of every hypothesis."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402
from test_place_recognition_gpu import make_submap, make_T, pr_params, replay_ransac, scene_points  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = backend.PRECISION_F64, backend.PRECISION_F32
LATTICE_DUPS = (0, 100, 364, 500)  # the lattice of test_place_recognition_edges_cpu.py: |d| = 0 pairs


@pytest.fixture(scope="module")
def be64():
    be = backend.Backend(0, F64)
    yield be
    be.close()


@pytest.fixture(scope="module")
def be32():
    be = backend.Backend(0, F32)
    yield be
    be.close()


def _features(be, P, N, radius, max_nn, cell=None):
    """upload, (optionally) index with the given cell, compute the features, download them, free the cloud"""
    cid = be.upload(P, N)
    if cell is not None:
        be.build_index(cid, 0.0, cell_size=cell)
    be.compute_fpfh(cid, radius, max_nn)
    F = be.fpfh(cid)
    be.free(cid)
    return F


def _counts(P, radius):
    """number of points with d2 < radius^2 around every point (itself included)"""
    return np.array([len(x[0]) for x in rs.neighbours(P, radius, 1 << 30, cKDTree(P))])


# ---- A. FPFH --------------------------------------------------------------------------------------------------------------------
def test_fpfh_shipped_parameters(be64, be32):
    """featureRadius_ 2.5, featureKnn_ 100: most kept lists are longer than 64 (each lane re-ranks two entries) and the cap binds for
    many points.  The cloud is exact in f32, so f32 storage gives the same bits."""
    P, N = rs.dyadic_cloud(4000, 1, half=(7.0, 7.0, 5.0))
    c = _counts(P, 2.5)
    assert np.mean(c > 64) > 0.8 and np.mean(c > 100) > 0.5, (np.mean(c > 64), np.mean(c > 100))
    got = _features(be64, P, N, 2.5, 100)
    ref = rs.fpfh(P, N, 2.5, 100, cKDTree(P))
    assert np.max(np.abs(got - ref)) <= 1e-9
    assert np.array_equal(_features(be32, P, N, 2.5, 100), got)


@pytest.fixture(scope="module")
def lattice():
    return rs.lattice(9, dups=LATTICE_DUPS)


@pytest.mark.parametrize("max_nn", [1, 7, 20, 64, 65, 100, 128])
def test_fpfh_lattice_ties_at_the_cut(be64, be32, lattice, max_nn):
    """a 0.125 lattice, radius 0.45: the cut falls at a shell boundary (1, 7) or inside a shell of equal d2 (the others), where the
    index order decides the list.  Axis normals reach every branch of pair_feature (premise: test_place_recognition_edges_cpu.py).
    Each f0 is 0, +-pi/4, +-pi/2, +-3pi/4, +-pi or atan of a lattice ratio, none of which lies at a bin edge other than the clamped
    +-pi, so the device's atan2 and the host's cannot pick different bins."""
    P, N = lattice
    full = rs.neighbours(P, 0.45, 1 << 30, cKDTree(P))
    split = sum(len(d2) > max_nn and d2[max_nn - 1] == d2[max_nn] for _, d2 in full)
    assert split > 0  # (1: a duplicated point keeps its lower-index twin, not itself; 7: points near the faces)
    if max_nn > 64:
        assert sum(len(d2) > 64 for _, d2 in full) > len(P) // 2
    got = _features(be64, P, N, 0.45, max_nn)
    ref = rs.fpfh(P, N, 0.45, max_nn, cKDTree(P))
    assert np.max(np.abs(got - ref)) <= 1e-9
    assert np.array_equal(_features(be32, P, N, 0.45, max_nn), got)  # every coordinate and normal is exact in f32


def _tile_offsets(k, seed=0):
    """k distinct offsets, multiples of 64 in [0, 2048)^3: the copies lie >= 48 m apart and span more than 2^27 cells of 1 m"""
    rng = np.random.default_rng(seed)
    cells = np.concatenate([[0, 32 ** 3 - 1], rng.choice(np.arange(1, 32 ** 3 - 1), size=k - 2, replace=False)])  # the two corners first
    return np.column_stack([cells % 32, (cells // 32) % 32, cells // 1024]) * 64.0


@pytest.mark.parametrize("prec", [F64, F32])
def test_fpfh_tiled_beyond_65536_points(prec):
    """41 copies of a 1,700-point dyadic cloud: 69,700 points, so blocks 0..4163 of fpfh_neighbours_kernel (grid min(n, 65536)) each
    rank a second point in the LDS lists the first one left.  Every difference is exact, so each copy's features are the base cloud's
    bit for bit.  The copies span 1984+ m on every axis: 1 m cells would be ~8e9 > kMaxCells = 2^27, so the index build coarsens its
    cells (to about 5 m, still K = 1)."""
    P, N = rs.dyadic_cloud(1700, 21, half=(7.0, 7.0, 3.0))
    offs = _tile_offsets(41)
    T, TN = rs.tile(P, N, offs)
    assert len(T) > 65536
    ext = T.max(0) - T.min(0)
    assert np.prod(np.floor(ext / 1.0) + 1) > 2 ** 27
    be = backend.Backend(0, prec)  # (its own handle: the 2^27 cell counters go with it)
    try:
        base = _features(be, P, N, 1.0, 40)
        tiled = _features(be, T, TN, 1.0, 40)
    finally:
        be.close()
    assert np.array_equal(tiled, np.tile(base, (len(offs), 1)))
    ref = rs.fpfh(P, N, 1.0, 40, cKDTree(P))
    assert np.max(np.abs(base - ref)) <= 1e-9 and np.any(base != 0.0)


def _reach(P, cell, radius):
    """the largest per-axis cell distance between two points closer than radius, on a grid of the given cell from the bounding box's
    minimum (the index's origin)"""
    ix = np.floor((P - P.min(0)) / cell).astype(np.int64)
    pairs = np.array(sorted(cKDTree(P).query_pairs(radius)))
    d = P[pairs[:, 0]] - P[pairs[:, 1]]
    pairs = pairs[np.einsum("ij,ij->i", d, d) < radius * radius]
    return int(np.max(np.abs(ix[pairs[:, 0]] - ix[pairs[:, 1]])))


@pytest.mark.parametrize("f", [0.55, 1.9, 0.3, 3.0])
def test_fpfh_reused_index(be64, f):
    """an index the cloud already has: cell 0.55 r is kept and searched with K = 2 (some neighbours are two cells away, so K = 1 would
    lose them), 1.9 r is kept with coarse cells; 0.3 r and 3 r are rebuilt.  The same bits as a fresh cloud either way."""
    r = 1.0
    P, N = rs.dyadic_cloud(1500, 8, half=(5.0, 5.0, 3.0))
    if f == 0.55:
        assert math.ceil(r / (f * r)) == 2 and _reach(P, f * r, r) == 2
    got = _features(be64, P, N, r, 50, cell=f * r)
    assert np.array_equal(got, _features(be64, P, N, r, 50))
    assert np.max(np.abs(got - rs.fpfh(P, N, r, 50, cKDTree(P)))) <= 1e-9


def _coincident(n=100):
    rng = np.random.default_rng(6)
    N = rng.normal(size=(n, 3))
    return np.tile([[1.5, -2.25, 0.5]], (n, 1)), N / np.linalg.norm(N, axis=1, keepdims=True)


@pytest.mark.parametrize("case", ["n1", "n2", "n63", "n64", "n65", "coincident", "isolated"])
def test_fpfh_sizes_and_degenerate_clouds(be64, case):
    if case.startswith("n"):
        P, N = rs.dyadic_cloud(int(case[1:]), 30, half=(0.6, 0.6, 0.6))
    elif case == "coincident":  # every pair has |d| = 0 and d2 = 0 (the FPFH sum skips them): the cap of 30 cuts by index alone
        P, N = _coincident()
    else:
        _, N = rs.dyadic_cloud(80, 31)
        P = np.arange(80)[:, None] * [4.0, 0.0, 0.0]  # 4 m apart: no neighbour within the radius
    got = _features(be64, P, N, 1.0, 30)
    ref = rs.fpfh(P, N, 1.0, 30, cKDTree(P))
    assert got.shape == (len(P), 33) and np.max(np.abs(got - ref)) <= 1e-9
    if case == "isolated":
        assert np.all(got == 0.0)
    if case == "coincident":  # every pair feature is zero: bins 5, 16 and 27 take 29 increments of 100 / 29
        assert np.allclose(got[:, [5, 16, 27]], 100.0, rtol=1e-13, atol=0.0)


# ---- B. feature correspondences -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(be64):
    """the submaps of test_place_recognition_gpu.py's pair fixture (same seeds)"""
    rng = np.random.default_rng(77)
    T_gt = make_T(35.0, [3.0, -2.0, 0.3])
    src = scene_points(rng)
    tgt = scene_points(rng) @ T_gt[:3, :3].T + T_gt[:3, 3]
    p = pr_params()
    a, b = make_submap(be64, src, p, 0), make_submap(be64, tgt, p, 1)
    return a, b, T_gt, p


def _device_pairs(be, s, t, mutual, ransac_n=3):
    c, fb = be.feature_correspondences(s, t, mutual=mutual, ransac_n=ransac_n)
    return c.astype(np.int64), fb


def test_feature_correspondences_exact(be64, pair):
    """against the exact reference (the kernel's ordered f64 sum, ties to the lower index): the one-way and the mutual set are equal"""
    a, b, _, _ = pair
    sa, sb = a.getSparseMapPointCloud().id, b.getSparseMapPointCloud().id
    Fa, Fb = be64.fpfh(sa), be64.fpfh(sb)
    ab, ba = rs.feature_nn(Fa, Fb), rs.feature_nn(Fb, Fa)
    one, fb = _device_pairs(be64, sa, sb, False)
    assert not fb and np.array_equal(one, rs.feature_correspondences(Fa, Fb, False, 3, ab, ba)[0])
    mut, fb = _device_pairs(be64, sa, sb, True)
    exp, efb = rs.feature_correspondences(Fa, Fb, True, 3, ab, ba)
    assert fb == efb is False and np.array_equal(mut, exp)


def _unit_cloud(units, seed, spacing=8.0):
    """points of 'units' laid out along x, one unit per `spacing` metres: a unit is ('copy', k) -- the k-th fixed shape --,
    ('rand', size) -- a fresh random cluster -- or ('iso',) -- one isolated point.  Cluster points lie within 0.45 of each other on the
    2^-10 grid, so a shape placed twice has the same features twice, bit for bit."""
    rng = np.random.default_rng(seed)
    shapes = [rs.dyadic_cloud(4, 1000 + k, half=(0.25, 0.25, 0.25)) for k in range(4)]
    P, N = [], []
    for u, unit in enumerate(units):
        if unit[0] == "copy":
            p, n = shapes[unit[1]]
        elif unit[0] == "rand":
            p, n = rs.dyadic_cloud(unit[1], int(rng.integers(1 << 30)), half=(0.25, 0.25, 0.25))
        else:
            p, n = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
        P.append(p + [u * spacing, 0.0, 0.0])
        N.append(n)
    return np.vstack(P), np.vstack(N)


@pytest.fixture(scope="module")
def mixed(be64):
    """300+ points where many features are bitwise equal (copies of 4 shapes, isolated points with the zero feature) and scattered
    over the index range; prefixes of every size of the test, each with its own features"""
    rng = np.random.default_rng(12)
    units = [("copy", k % 4) for k in range(32)] + [("rand", 3)] * 20 + [("iso",)] * 80
    units = [units[k] for k in rng.permutation(len(units))]
    P, N = _unit_cloud(units, 13)
    out = {}
    for n in (1, 31, 32, 33, 255, 256, 257):
        cid = be64.upload(P[:n], N[:n])
        be64.compute_fpfh(cid, 1.0, 30)
        out[n] = (cid, be64.fpfh(cid))
    yield out
    for cid, _ in out.values():
        be64.free(cid)


def _tie_straddles_tile(A, B, tile=32):
    """some query's set of equally nearest rows spans two 32-row tiles"""
    for a in A:
        d = np.zeros(len(B))
        for b in range(33):
            t = a[b] - B[:, b]
            d = d + t * t
        j = np.flatnonzero(d == d.min())
        if j[-1] // tile != j[0] // tile:
            return True
    return False


@pytest.mark.parametrize("na", [1, 31, 32, 33, 255, 256, 257])
def test_feature_correspondences_sizes_and_ties(be64, mixed, na):
    """na, nb in {1, 31, 32, 33, 255, 256, 257} (tile and block tails, nb < 32): every match is the exact reference's, i.e. the lowest
    index among bitwise-equal features"""
    ca, Fa = mixed[na]
    for nb in (1, 31, 32, 33, 255, 256, 257):
        cb, Fb = mixed[nb]
        ab, ba = rs.feature_nn(Fa, Fb), rs.feature_nn(Fb, Fa)
        if na >= 255 and nb >= 255:
            assert _tie_straddles_tile(Fa, Fb)
        for mutual in (False, True):
            got, fb = _device_pairs(be64, ca, cb, mutual)
            exp, efb = rs.feature_correspondences(Fa, Fb, mutual, 3, ab, ba)
            assert fb == efb and np.array_equal(got, exp), (na, nb, mutual)


def test_feature_correspondences_lattice_ties(be64, lattice):
    """the lattice with one normal (+z) everywhere: points of equal neighbourhoods (all interior points, for a start) have bitwise-equal
    features, and each matches the lowest such index"""
    P, _ = lattice
    cid = be64.upload(P, np.tile([[0.0, 0.0, 1.0]], (len(P), 1)))
    be64.compute_fpfh(cid, 0.45, 20)
    F = be64.fpfh(cid)
    one, _ = _device_pairs(be64, cid, cid, False)
    exp = rs.feature_nn(F, F)
    assert np.array_equal(one[:, 1], exp)
    assert np.sum(exp < np.arange(len(F))) > 10  # many points match an equal feature with a lower index
    be64.free(cid)


def test_feature_correspondences_tiled_ties():
    """base cloud (1,700 points) against its 41-copy tiling (69,700 points): the copies' features are the base's bit for bit, so every
    match is in the first copy, and a tiled point's match is its base point's"""
    P, N = rs.dyadic_cloud(1700, 21, half=(7.0, 7.0, 3.0))
    offs = _tile_offsets(41)
    T, TN = rs.tile(P, N, offs)
    be = backend.Backend(0, F64)
    try:
        b, t = be.upload(P, N), be.upload(T, TN)
        be.compute_fpfh(b, 1.0, 40)
        be.compute_fpfh(t, 1.0, 40)
        Fb = be.fpfh(b)
        bb = rs.feature_nn(Fb, Fb)
        one, _ = _device_pairs(be, b, t, False)
        assert np.array_equal(one[:, 1], bb)  # the lowest of 41 equal rows (ties 1,700 rows apart)
        back, _ = _device_pairs(be, t, b, False)
        assert np.array_equal(back[:, 1], np.tile(bb, len(offs)))
        mut, fb = _device_pairs(be, b, t, True)
        keep = bb[bb] == np.arange(len(P))
        assert not fb and np.array_equal(mut, np.column_stack([np.arange(len(P)), bb])[keep])
    finally:
        be.close()


def _fallback_clouds(sizes, seed):
    """source and target holding the same random clusters (the target's in another order and place) plus isolated points: each cluster
    point's nearest feature is its copy (distance 0); all isolated points share the zero feature and give one mutual pair together"""
    rng = np.random.default_rng(seed)
    seeds = [int(s) for s in rng.integers(1 << 30, size=len(sizes))]
    clusters = [rs.dyadic_cloud(k, s, half=(0.25, 0.25, 0.25)) for k, s in zip(sizes, seeds)]

    def build(order, n_iso, shift):
        P, N = [], []
        for u, k in enumerate(order):
            P.append(clusters[k][0] + [8.0 * u + shift, 0.0, 0.0])
            N.append(clusters[k][1])
        for u in range(n_iso):
            P.append(np.array([[8.0 * (len(order) + u) + shift, 16.0, 0.0]]))
            N.append(np.array([[0.0, 0.0, 1.0]]))
        return np.vstack(P), np.vstack(N)

    return build(range(len(sizes)), 3, 0.0), build(rng.permutation(len(sizes)), 2, 1024.0)


@pytest.mark.parametrize("ransac_n,target", [(3, 9), (3, 8), (8, 24), (8, 23)])
def test_mutual_fallback_threshold(be64, ransac_n, target):
    """exactly 3 ransac_n mutual pairs keep the mutual set, one fewer falls back to the one-way set"""
    sizes = {9: [4, 4], 8: [3, 4], 24: [4, 4, 5, 5, 5], 23: [4, 4, 4, 5, 5]}[target]
    (Ps, Ns), (Pt, Nt) = _fallback_clouds(sizes, target)
    s, t = be64.upload(Ps, Ns), be64.upload(Pt, Nt)
    be64.compute_fpfh(s, 1.0, 30)
    be64.compute_fpfh(t, 1.0, 30)
    Fs, Ft = be64.fpfh(s), be64.fpfh(t)
    ab, ba = rs.feature_nn(Fs, Ft), rs.feature_nn(Ft, Fs)
    assert int(np.sum(ba[ab] == np.arange(len(Fs)))) == target  # the premise, from the exact reference
    exp, efb = rs.feature_correspondences(Fs, Ft, True, ransac_n, ab, ba)
    assert efb == (target < 3 * ransac_n)
    got, fb = _device_pairs(be64, s, t, True, ransac_n)
    assert fb == efb and np.array_equal(got, exp)
    r = be64.ransac_feature_matching(s, t, 0.5, ransac_n, True, max_iteration=1)
    assert r["fell_back"] == efb and r["n_feature_corr"] == len(exp)
    be64.free(s)
    be64.free(t)


def test_feature_correspondences_capacity(be64, pair):
    """a buffer one pair too small: O3DS_ERR_CAPACITY with *n_pairs the full count; exactly the count: OK"""
    a, b, _, _ = pair
    sa, sb = a.getSparseMapPointCloud().id, b.getSparseMapPointCloud().id
    exp, _ = _device_pairs(be64, sa, sb, True)
    k = len(exp)
    lib = be64.lib
    buf = np.zeros((k, 2), np.uint32)
    n, fb = C.c_size_t(12345), C.c_int(7)
    rc = lib.o3ds_feature_correspondences(be64.h, sa, sb, 1, 3, buf.ctypes.data_as(C.POINTER(C.c_uint32)), k - 1, C.byref(n), C.byref(fb))
    assert rc == backend.ERR_CAPACITY and n.value == k
    n.value = 0
    rc = lib.o3ds_feature_correspondences(be64.h, sa, sb, 1, 3, None, 0, C.byref(n), C.byref(fb))
    assert rc == backend.ERR_CAPACITY and n.value == k
    rc = lib.o3ds_feature_correspondences(be64.h, sa, sb, 1, 3, buf.ctypes.data_as(C.POINTER(C.c_uint32)), k, C.byref(n), C.byref(fb))
    assert rc == backend.OK and n.value == k and fb.value == 0 and np.array_equal(buf.astype(np.int64), exp)


# ---- C. RANSAC ------------------------------------------------------------------------------------------------------------------
SHIPPED = pr_params().placeRecognition_
MAX_CORR = SHIPPED.ransacMaxCorrespondenceDistance_
CHECKERS = {"both": (SHIPPED.correspondenceCheckerEdgeLength_, SHIPPED.correspondenceCheckerDistance_),
            "edge": (SHIPPED.correspondenceCheckerEdgeLength_, 0.0), "dist": (0.0, SHIPPED.correspondenceCheckerDistance_),
            "off": (0.0, 0.0)}


@pytest.fixture(scope="module")
def ransac_points(pair, be64):
    """(source, source normals, target, target normals): the pair's sparse source within 9 m of a corner of the overlap (a few hundred
    points, so a recount of thousands of hypotheses stays cheap) and the whole sparse target"""
    a, b, _, _ = pair
    S, NS = be64.download(a.getSparseMapPointCloud().id)
    Tg, NT = be64.download(b.getSparseMapPointCloud().id)
    keep = np.linalg.norm(S[:, :2] - [-6.0, -6.0], axis=1) < 9.0
    return S[keep], NS[keep], Tg, NT


def _ransac_clouds(be, pts, mirror=False, reuse=False):
    S, NS, Tg, NT = pts
    if mirror:  # the target is the source's mirror image: a reflection would fit every sample exactly
        Tg, NT = S * [1.0, -1.0, 1.0], NS * [1.0, -1.0, 1.0]
    s, t = be.upload(S, NS), be.upload(Tg, NT)
    be.compute_fpfh(s, SHIPPED.featureRadius_, SHIPPED.featureKnn_)
    be.compute_fpfh(t, SHIPPED.featureRadius_, SHIPPED.featureKnn_)
    if reuse:  # kept by ransac_t (cell in [0.5, 2] max_corr), searched with K = 2
        assert math.ceil(MAX_CORR / (0.55 * MAX_CORR)) == 2
        be.build_index(t, 0.0, cell_size=0.55 * MAX_CORR)
    return s, t


def _run_replay(be, s, t, ransac_n, checkers, mutual, n_iter, confidence, seed, invariants=True):
    edge, dist = CHECKERS[checkers]
    S, _ = be.download(s)
    Tg, _ = be.download(t)
    corr, fb = _device_pairs(be, s, t, mutual, ransac_n)
    r = be.ransac_feature_matching(s, t, MAX_CORR, ransac_n, mutual, edge, dist, n_iter, confidence, seed, trace=n_iter)
    assert r["n_feature_corr"] == len(corr) and r["fell_back"] == fb
    validated = replay_ransac(r, S, Tg, corr, seed, ransac_n, MAX_CORR, edge, dist, n_iter, confidence, invariants)
    return r, validated


GRID = [  # (ransac_n, checkers, mutual, precision, reused target index, mirrored target)
    (3, "both", True, F64, False, False), (4, "both", True, F64, False, False), (5, "both", True, F64, False, False),
    (8, "both", True, F64, False, False), (3, "edge", True, F64, False, False), (3, "dist", True, F64, False, False),
    (3, "off", True, F64, False, False), (4, "edge", False, F64, False, False), (5, "dist", False, F64, False, False),
    (8, "off", False, F64, False, False), (8, "dist", True, F64, False, False), (8, "edge", False, F64, False, False),
    (3, "both", False, F64, True, False), (4, "off", True, F64, True, False), (8, "both", True, F64, True, False),
    (3, "both", True, F32, False, False), (5, "edge", False, F32, False, False), (8, "off", True, F32, True, False),
    (4, "dist", True, F32, False, False), (3, "both", True, F64, False, True), (8, "off", False, F64, False, True),
    (4, "dist", True, F32, False, True),
]


@pytest.mark.parametrize("ransac_n,checkers,mutual,prec,reuse,mirror", GRID)
def test_ransac_replay_grid(be64, be32, ransac_points, ransac_n, checkers, mutual, prec, reuse, mirror):
    """the trace replay of test_place_recognition_gpu.py over ransac_n, the checkers, the mutual filter, the storage precision, a target
    index kept with K = 2 and a mirrored target; every hypothesis is a proper rotation of the restatement Umeyama's cost.  f32: the
    restatement runs on the stored (rounded) coordinates."""
    be = be64 if prec == F64 else be32
    s, t = _ransac_clouds(be, ransac_points, mirror, reuse)
    try:
        r, validated = _run_replay(be, s, t, ransac_n, checkers, mutual, 1536, 0.999, 4242 + ransac_n)
        if checkers == "off":
            assert len(validated) == r["iterations_run"]
        if reuse:  # the kept index gives the same result as a fresh one
            s2, t2 = _ransac_clouds(be, ransac_points, mirror, False)
            edge, dist = CHECKERS[checkers]
            r2 = be.ransac_feature_matching(s2, t2, MAX_CORR, ransac_n, mutual, edge, dist, 1536, 0.999, 4242 + ransac_n)
            assert all(np.array_equal(r[k], r2[k]) for k in r2)
            be.free(s2)
            be.free(t2)
    finally:
        be.free(s)
        be.free(t)


def test_ransac_more_than_2048_validations_in_a_batch(be64, ransac_points):
    """checkers off and confidence 1 (never cuts): batches of 1024, 2048 and 4096 hypotheses; the third validates all 4096 with 2048
    workgroups, so the validate kernel's grid-stride loop runs.  Every hypothesis is recounted."""
    s, t = _ransac_clouds(be64, ransac_points)
    r, validated = _run_replay(be64, s, t, 3, "off", True, 7168, 1.0, 99, invariants=False)
    assert r["iterations_run"] == 7168
    assert sum(3072 <= k < 7168 for k in validated) > 2048
    be64.free(s)
    be64.free(t)


@pytest.mark.parametrize("max_iteration", [1, 3, 1023, 1024, 1025, 3073])
def test_ransac_max_iteration_edges(be64, ransac_points, max_iteration):
    s, t = _ransac_clouds(be64, ransac_points)
    r, _ = _run_replay(be64, s, t, 3, "both", True, max_iteration, 1.0, 5)
    assert r["iterations_run"] == max_iteration
    be64.free(s)
    be64.free(t)


def test_ransac_confidence_zero(be64, ransac_points):
    """confidence 0: est = 0 after the first improvement, the loop stops right after it"""
    s, t = _ransac_clouds(be64, ransac_points)
    r, _ = _run_replay(be64, s, t, 3, "both", True, 2048, 0.0, 6)
    assert r["best_t"] >= 0 and r["iterations_run"] == r["best_t"] + 1
    be64.free(s)
    be64.free(t)


def test_ransac_fitness_one(be64, ransac_points):
    """source and target the same cloud: a correct sample gives fitness 1 and the estimate log(1 - p) / log(0) = 0"""
    S, NS, _, _ = ransac_points
    s = be64.upload(S, NS)
    be64.compute_fpfh(s, SHIPPED.featureRadius_, SHIPPED.featureKnn_)
    r, _ = _run_replay(be64, s, s, 3, "both", True, 2048, SHIPPED.ransacProbability_, 7)
    assert r["fitness"] == 1.0 and r["iterations_run"] == r["best_t"] + 1
    be64.free(s)


# ---- D. interactions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replica", [False, True])
def test_registration_unchanged_by_feature_index_rebuilds(monkeypatch, replica):
    """a registration against a cloud gives the same bits before and after compute_fpfh or RANSAC rebuilt that cloud's index, and
    after compute_fpfh kept it (radius 0.4 on the registration's 0.25 m cells: K = 2); with the replica (built at the first registration
    in the A/B library) and without it"""
    if replica:
        monkeypatch.setenv("O3DS_NN_REPLICA_AFTER", "1")
    rng = np.random.default_rng(31)
    T = make_T(2.0, [0.2, -0.1, 0.05])
    src = scene_points(rng, spacing=0.2)
    tgt = scene_points(rng, spacing=0.2) @ T[:3, :3].T + T[:3, 3]
    be = backend.Backend(0, F64, ab=replica)
    fixed = dict(max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    try:
        s, t = be.upload(src), be.upload(tgt)
        be.estimate_normals(t, 1.0, 20)
        be.build_index(t, 1.0)
        ref = be.icp_point_to_plane_dev(s, t, 1.0, **fixed)
        assert (be.index_replica(t) > 0) == replica
        S, NS = be.download(s)
        s_feat = be.upload(S, np.tile([[0.0, 0.0, 1.0]], (len(S), 1)))
        be.compute_fpfh(s_feat, 2.5, 100)

        def same(what):
            r = be.icp_point_to_plane_dev(s, t, 1.0, **fixed)
            np.testing.assert_array_equal(r["transformation"], ref["transformation"], err_msg=what)
            assert (r["iterations"], r["n_corr"], r["fitness"], r["inlier_rmse"]) == (ref["iterations"], ref["n_corr"], ref["fitness"],
                                                                                    ref["inlier_rmse"]), what
            assert (be.index_replica(t) > 0) == replica, what

        Pt, Nt = be.download(t)
        be.compute_fpfh(t, 0.4, 50)  # the registration's index (0.25 m cells) is kept
        assert np.array_equal(be.fpfh(t), _features(be, Pt, Nt, 0.4, 50))
        same("after compute_fpfh kept the index")
        be.compute_fpfh(t, 2.5, 100)  # rebuilt (cell 2.5)
        same("after compute_fpfh rebuilt the index")
        be.ransac_feature_matching(s_feat, t, 1.5, 3, True, 0.6, 0.8, 64, 0.999, 3)  # rebuilt (cell 1.5)
        same("after RANSAC rebuilt the index")
    finally:
        be.close()
