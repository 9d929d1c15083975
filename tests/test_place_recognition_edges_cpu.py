"""Premises of tests/test_place_recognition_edges_gpu.py, checked on the numpy restatement without a GPU: the lattice's shell sizes and
the pair-feature branches it reaches, the exactness of tiled dyadic clouds, the exact feature-NN reference and the fallback inputs."""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402


def test_lattice_shell_sizes():
    """spacing 0.125 (exact in binary), radius 0.45: the cumulative shell sizes around an interior point, so that max_nn in
    {1, 7, 20, 64, 65, 100, 128} cuts at a shell boundary or inside a tie shell"""
    P, _ = rs.lattice(9)
    c = 4 * 81 + 4 * 9 + 4  # the centre: 4 spacings of margin on every side (the radius reaches 3.6)
    idx, d2 = rs.neighbours(P, 0.45, 1000, cKDTree(P))[c]
    _, cnt = np.unique(d2, return_counts=True)
    assert np.cumsum(cnt).tolist() == [1, 7, 19, 27, 33, 57, 81, 93, 123, 147, 171, 179]
    assert np.all(d2 == np.round(d2 * 64) / 64)  # every d2 is exact (a multiple of 0.125^2)


def test_lattice_reaches_every_pair_feature_branch():
    """the GPU lattice test's cloud (tests/test_place_recognition_edges_gpu.py LATTICE) takes every early return and edge of
    pair_feature.  f2 = +-1 needs d parallel to the normal that stays n1, and then d x n1 = 0 returns first: it is the zero_cross case."""
    P, N = rs.lattice(9, dups=(0, 100, 364, 500))
    for max_nn in (20, 128):
        tags = rs.pair_feature_tags(P, N, rs.neighbours(P, 0.45, max_nn, cKDTree(P)))
        assert tags >= {"zero_d", "zero_cross", "swap", "equal_no_swap", "atan2_+pi", "atan2_-pi", "f1_+1", "f1_-1"}, (max_nn, tags)


def test_tiled_dyadic_cloud_is_exact():
    """copies of a cloud on the 2^-10 grid at offsets that are multiples of 64: every difference is exact, in f32 as well, so each copy's
    features are the base cloud's bit for bit"""
    P, N = rs.dyadic_cloud(500, 3, half=(3.0, 3.0, 1.5))
    offs = np.array([[0, 0, 0], [64, 0, 0], [-128, 64, 192]], np.float64)
    T, TN = rs.tile(P, N, offs)
    assert np.array_equal(T.astype(np.float32).astype(np.float64), T)
    assert np.array_equal(TN.astype(np.float32).astype(np.float64), TN)
    base = rs.fpfh(P, N, 1.0, 30, cKDTree(P))
    tiled = rs.fpfh(T, TN, 1.0, 30, cKDTree(T))
    assert np.array_equal(tiled, np.tile(base, (3, 1)))
    assert np.any(base != 0.0)


def test_feature_nn_is_ordered_sum_and_lowest_index():
    rng = np.random.default_rng(4)
    A = rng.uniform(0, 50, (70, 33))
    B = np.vstack([A[5], rng.uniform(500, 600, (40, 33)), A[5], A[9], A[9], A[20]])  # (the far rows are nobody's mutual match)
    got = rs.feature_nn(A, B, chunk=16)
    d = np.zeros((len(A), len(B)))
    for b in range(33):
        t = A[:, b, None] - B[None, :, b]
        d = d + t * t
    assert np.array_equal(got, np.argmin(d, axis=1))
    assert got[5] == 0 and got[9] == 42  # exact ties: the lower index
    assert np.array_equal(rs.feature_nn(A, B[:0]), np.full(len(A), -1))
    # the mutual set and its fallback at exactly 3 * ransac_n pairs
    one, fb = rs.feature_correspondences(A, B, False, 3)
    assert not fb and np.array_equal(one[:, 1], got)
    mut, fb = rs.feature_correspondences(A, B, True, 1)
    assert not fb and mut.tolist() == [[5, 0], [9, 42], [20, 44]]  # 3 = 3 * ransac_n: kept
    mut, fb = rs.feature_correspondences(A, B, True, 2)  # 3 < 3 * 2: the one-way set
    assert fb and np.array_equal(mut, one)


def test_ls_cost_and_umeyama_reflection():
    """Umeyama on a mirrored sample stays a rotation (det +1); a reflection would fit better, so the cost is not zero"""
    rng = np.random.default_rng(2)
    p = rng.normal(size=(5, 3))
    q = p * [1.0, 1.0, -1.0]
    T = rs.umeyama(p, q)
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    assert rs.ls_cost(T, p, q) > 1e-3
    M = np.diag([1.0, 1.0, -1.0, 1.0])
    assert rs.ls_cost(M, p, q) < 1e-24
