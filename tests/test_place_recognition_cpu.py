"""Place recognition without a GPU: the numpy restatement the GPU tests check against (tests/fpfh_ransac_restatement.py), the
draws, the stopping rule, the consistency check and the ABI structs of o3ds_ransac_*."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402
from open3d_slam_amd import parameters as prm  # noqa: E402
from open3d_slam_amd import place_recognition as pr  # noqa: E402


def test_pair_feature_zero_distance_and_zero_cross():
    n = [0.0, 0.0, 1.0]
    assert rs.pair_feature([1.0, 2.0, 3.0], n, [1.0, 2.0, 3.0], [1.0, 0.0, 0.0]) == (0.0, 0.0, 0.0)
    # d parallel to n1 (and n2 chosen so that no swap happens): d x n1 = 0
    assert rs.pair_feature([0.0, 0.0, 0.0], n, [0.0, 0.0, 2.0], [0.0, 0.0, 1.0]) == (0.0, 0.0, 0.0)
    # zero features still fall in bins 5, 16, 27
    assert rs.bins(0.0, 0.0, 0.0) == (5, 16, 27)


def test_pair_feature_hand_computed_and_swap():
    # no swap: n1 . d / |d| = 0 (acos = pi/2) vs n2 . d / |d| = 1/sqrt2 (acos = pi/4): acos(|a1|) > acos(|a2|) -> swap
    p1, n1, p2 = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]
    n2 = [math.sqrt(0.5), 0.0, math.sqrt(0.5)]
    f0, f1, f2 = rs.pair_feature(p1, n1, p2, n2)
    # swapped: n1' = n2, n2' = n1, d' = (-1, 0, 0), f2 = -a2 = -sqrt(.5)
    assert f2 == pytest.approx(-math.sqrt(0.5), abs=1e-15)
    v = np.cross([-1.0, 0.0, 0.0], n2)
    v /= np.linalg.norm(v)
    w = np.cross(n2, v)
    assert f1 == pytest.approx(float(v @ n1), abs=1e-15)
    assert f0 == pytest.approx(math.atan2(float(w @ n1), float(np.dot(n2, n1))), abs=1e-15)
    # without the swap (n1 tilted towards d more than n2): f2 = a1
    g0, g1, g2 = rs.pair_feature(p1, n2, p2, n1)
    assert g2 == pytest.approx(math.sqrt(0.5), abs=1e-15)
    vv = np.cross([1.0, 0.0, 0.0], n2)
    vv /= np.linalg.norm(vv)
    assert g1 == pytest.approx(float(vv @ n1), abs=1e-15)


def test_bin_clamps():
    assert rs.bins(math.pi, 1.0, 1.0) == (10, 21, 32)      # the upper edges land in the last bin
    assert rs.bins(-math.pi, -1.0, -1.0) == (0, 11, 22)
    assert rs.bins(-4.0, -1.5, -2.0) == (0, 11, 22)        # below: clamped to 0
    assert rs.bins(4.0, 1.5, 2.0) == (10, 21, 32)


def _cloud(seed, n=150):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.5, 1.5, (n, 3))
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return P, N


def test_spfh_histogram_sums_and_isolated_point():
    P, N = _cloud(3, 60)
    P = np.vstack([P, [[50.0, 50.0, 50.0]]])
    N = np.vstack([N, [[0.0, 0.0, 1.0]]])
    nb = rs.neighbours(P, 1.0, 20)
    S = rs.spfh(P, N, nb)
    for i, (idx, _) in enumerate(nb):
        if len(idx) > 1:  # each of the three sub-histograms adds up to 100
            assert np.allclose([S[i, :11].sum(), S[i, 11:22].sum(), S[i, 22:].sum()], 100.0, atol=1e-9)
    F = rs.fpfh(P, N, 1.0, 20)
    assert np.all(F[-1] == 0.0)  # no neighbour: the zero vector


def test_fpfh_invariant_under_rigid_motion():
    P, N = _cloud(7)
    F = rs.fpfh(P, N, 1.0, 30)
    a, b, c = 0.7, -0.3, 1.1
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    R = Rz @ Ry @ Rx
    F2 = rs.fpfh(P @ R.T + [3.0, -2.0, 0.5], N @ R.T, 1.0, 30)
    assert np.max(np.abs(F - F2)) <= 1e-9


def test_draws_are_splitmix_of_the_hypothesis_counter():
    # splitmix64 of 0x9E3779B97F4A7C15 (the first output of the generator seeded 0)
    assert rs.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    d = rs.draw(5, 3, 2, 1000)
    assert d == [rs.mix(5 + (3 * 2 + j + 1) * rs.GOLDEN) % 1000 for j in range(3)]
    assert all(0 <= x < 1000 for x in d)


def test_stopping_rule_hand_made_trace():
    # n_src 100, ransac_n 3, confidence 0.99.  t=2: 50 pairs -> est = ceil(log(.01) / log(1 - .125)) = 35; t=10: 80 pairs -> 7 <= 10,
    # so the loop stops after t = 10; t = 40 never runs
    val = {2: (50, 0.3), 5: (50, 0.4), 10: (80, 0.2), 40: (99, 0.1)}
    run, best, vals = rs.stopping_rule(1000, 0.99, 3, 100, val)
    assert math.ceil(math.log(0.01) / math.log(1 - 0.5 ** 3)) == 35
    assert (run, best, vals) == (11, 10, 3)
    # a tie in pairs goes to the lower rmse, a full tie to the lower t
    run, best, vals = rs.stopping_rule(20, 0.0, 3, 100, {1: (10, 0.5), 3: (10, 0.4), 4: (10, 0.4)})
    assert best == 1 and run == 2  # confidence 0: est = 0 after the first improvement
    run, best, vals = rs.stopping_rule(20, 0.5, 3, 100, {1: (10, 0.5), 3: (10, 0.4), 4: (10, 0.4)})
    assert best == 3 and vals == 3 and run == 20
    assert rs.stopping_rule(7, 0.999, 3, 100, {}) == (7, -1, 0)


def test_registration_consistency():
    p = prm.lua_place_recognition_parameters().consistencyCheck_
    assert pr.isRegistrationConsistent(np.eye(4), p)
    T = np.eye(4)
    c, s = math.cos(math.radians(29.0)), math.sin(math.radians(29.0))
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [79.0, -79.0, 39.0]
    assert pr.isRegistrationConsistent(T, p)
    c, s = math.cos(math.radians(60.0)), math.sin(math.radians(60.0))
    T[:2, :2] = [[c, -s], [s, c]]
    assert not pr.isRegistrationConsistent(T, p)
    assert pr.isRegistrationConsistent(T, prm.PlaceRecognitionConsistencyCheckParameters(maxDriftX_=100.0, maxDriftY_=100.0,
                                                                                         maxDriftZ_=100.0))
    T = np.eye(4)
    T[2, 3] = -41.0
    assert not pr.isRegistrationConsistent(T, p)
    rx = np.array([[1, 0, 0, 0], [0, math.cos(0.6), -math.sin(0.6), 0], [0, math.sin(0.6), math.cos(0.6), 0], [0, 0, 0, 1.0]])
    assert pr.toRPY(rx) == pytest.approx([0.6, 0.0, 0.0], abs=1e-12)
    assert not pr.isRegistrationConsistent(rx, p)  # 34 deg of roll > 30


def test_parameter_defaults():
    d = prm.PlaceRecognitionParameters()
    assert (d.featureVoxelSize_, d.featureRadius_, d.featureKnn_, d.normalKnn_, d.ransacNumIter_) == (0.5, 2.5, 100, 10, 1000000)
    assert d.consistencyCheck_.maxDriftYaw_ == pytest.approx(math.pi / 2)
    lua = prm.lua_place_recognition_parameters()
    assert (lua.ransacNumIter_, lua.ransacProbability_, lua.correspondenceCheckerEdgeLength_, lua.normalKnn_) == (10000000, 0.999, 0.6, 20)
    assert prm.MapperParameters().placeRecognition_.ransacModelSize_ == 3


def test_ransac_struct_layouts_match_header():
    assert C.sizeof(backend.RansacParams) == 4 + 4 + 8 + 8 + 8 + 8 + 8
    assert C.sizeof(backend.RansacResult) == 16 * 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 4 + 4
    assert C.sizeof(backend.RansacTrace) == 8 * 4 + 4 + 4 + 8 + 16 * 8
    for name in ("o3ds_compute_fpfh", "o3ds_cloud_has_fpfh", "o3ds_cloud_download_fpfh", "o3ds_feature_correspondences",
                 "o3ds_ransac_feature_matching"):
        assert name in backend.SIGNATURES


def test_ransac_struct_sizes_in_c(tmp_path):
    import shutil
    import subprocess

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "o3ds_backend.h")
    src = tmp_path / "s.c"
    src.write_text(f'#include "{hdr}"\n#include <stdio.h>\nint main(void){{ printf("%zu %zu %zu", sizeof(o3ds_ransac_params), '
                   'sizeof(o3ds_ransac_result), sizeof(o3ds_ransac_trace)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call([cc, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [C.sizeof(backend.RansacParams), C.sizeof(backend.RansacResult), C.sizeof(backend.RansacTrace)]
