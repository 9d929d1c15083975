"""The restatement of o3ds_segment_plane (tests/plane_restatement.py) without a device: the winner of the block-wise evaluation is the
serial rule's over hypotheses taken one at a time, the sums in the documented order agree with math.fsum, the fit is the plane numpy's
eigh finds up to what a regression along the dominant axis differs from a total least-squares fit by, the premises of the cases
tests/test_plane_segmentation_gpu.py runs hold, and the header, the library and the Python mirror carry the new names."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_restatement as cr  # noqa: E402
import plane_restatement as pr  # noqa: E402
from plane_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(c.name, p) for c in pr.CASES for p in c.params]


@pytest.mark.parametrize("storage", pr.STORAGES)
@pytest.mark.parametrize("name,params", RUNS, ids=lambda v: str(v))
def test_the_block_wise_winner_is_the_serial_rules_one_hypothesis_at_a_time(name, params, storage):
    thr, ransac_n, num_iterations, seed = params
    want = pr.reference(name, storage, params)
    p = pr.to_storage(pr.case(name).cloud(), storage)
    n = len(p)
    samples = pr.draw(seed, ransac_n, num_iterations, n) if num_iterations else np.zeros((0, ransac_n), np.int64)
    best_t, best_f, best_r, n_deg = -1, 0.0, 0.0, 0
    for t in range(num_iterations):
        s = p[samples[t]]
        if ransac_n == 3:
            plane = pr.triangle_planes(s[0:1], s[1:2], s[2:3])[0]
        else:
            plane = pr.fit_plane(s[:, 0], s[:, 1], s[:, 2], np.ones(ransac_n, bool), float(ransac_n))
        assert plane.tobytes() == want.planes[t].tobytes()
        if not plane.any():
            n_deg += 1
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            dist = np.abs(((plane[0] * p[:, 0] + plane[1] * p[:, 1]) + plane[2] * p[:, 2]) + plane[3])
            inl = dist < thr
        count, error = int(inl.sum()), float(pr.ordered_sum(np.where(inl, dist, 0.0)))
        assert count == want.count[t] and error == want.error[t]
        f, r = pr.score(count, error, n)
        if f > best_f or (f == best_f and r < best_r):
            best_t, best_f, best_r = t, f, r
    assert (best_t, best_f, best_r, n_deg) == (want.best_t, want.fitness, want.inlier_rmse, want.n_degenerate)
    assert want.n_inliers == len(want.inliers) and (want.best_t < 0) == (want.n_inliers == 0)
    if want.best_t >= 0:
        assert want.n_inliers == want.count[want.best_t] and want.best_plane.tobytes() == want.planes[want.best_t].tobytes()


def _fsum_last(v):
    return np.array([math.fsum(row) for row in np.atleast_2d(v)])


@pytest.mark.parametrize("storage", pr.STORAGES)
def test_the_documented_order_sums_agree_with_fsum(storage):
    """to 1e-12 of the exact sum of the terms' magnitudes (the moments cancel; the errors and the coordinates of these clouds do not)"""
    for name, params in (("size-257", pr.case("size-257").params[0]), ("size-4097", pr.case("size-4097").params[0]),
                         ("offset", pr.case("offset").params[0]), ("ground-x", pr.case("ground-x").params[0])):
        want = pr.reference(name, storage, params)
        p = pr.to_storage(pr.case(name).cloud(), storage)
        with np.errstate(invalid="ignore"):
            dist = pr.distances(want.planes[:32], p)
            terms = np.where(dist < params[0], dist, 0.0)
        exact = _fsum_last(terms)
        assert np.all(np.abs(want.error[:32] - exact) <= 1e-12 * exact), name
        inl = np.zeros(len(p), bool)
        inl[want.inliers] = True
        c = np.array([math.fsum(p[inl, a]) for a in range(3)]) / inl.sum()
        r = p[inl] - c
        rows = [p[inl, 0], p[inl, 1], p[inl, 2]] + [r[:, a] * r[:, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        for row in rows:  # the same terms in the documented order of n terms, the others +0.0
            full = np.zeros(len(p))
            full[inl] = row
            assert abs(float(pr.ordered_sum(full)) - math.fsum(row)) <= 1e-12 * math.fsum(np.abs(row)), name
    # the order itself: chunks of ceil(m / 256) consecutive terms, a halving tree over them -- on terms whose sum depends on the order
    for m in (1, 3, 8, 255, 256, 257, 258, 513, 65537):
        v = np.random.default_rng(m).normal(size=m) * 10.0 ** np.random.default_rng(m + 1).integers(-8, 8, m)
        ln = max(1, -(-m // 256))
        chunks = []
        for c in range(256):
            s = 0.0
            for x in v[c * ln:(c + 1) * ln]:
                s = s + float(x)
            chunks.append(s)
        w = 128
        while w >= 1:
            chunks = [chunks[t] + chunks[t + w] for t in range(w)]
            w //= 2
        assert float(pr.ordered_sum(v)) == chunks[0], m
        assert pr.chunk_len(m) == ln


FIT_CASES = (("tilted-plane", pr.tilted_plane, None), ("ground-x", None, "x"), ("ground-y", None, "y"), ("ground-z", None, "z"))


@pytest.mark.parametrize("name,cloud,axis", FIT_CASES, ids=lambda v: getattr(v, "__name__", None) or str(v))  # (a function by its name: its repr holds an address)
def test_the_fit_is_the_plane_of_eighs_smallest_eigenvector(name, cloud, axis):
    """GetPlaneFromPoints regresses along the axis of the largest determinant; eigh's smallest eigenvector is the total least-squares
    normal.  The two differ by about (lambda_min / lambda_mid) * tan(tilt from the axis) -- the share of the spread that the plane leaves
    unexplained, eigh's own residual on the case -- and the bound is 100 times that share (1e-3 rad and less here): a wrong term or sign
    in a normal is off by degrees."""
    if cloud is not None:
        pts = np.asarray(cloud())
    else:  # the inliers of the ground of the turned scan
        pts = np.asarray(pr.case(name).cloud())[pr.reference(name, F64, pr.case(name).params[0]).inliers]
        assert pr.fit_axis(pts[:, 0], pts[:, 1], pts[:, 2]) == axis
    plane = pr.fit_plane(pts[:, 0], pts[:, 1], pts[:, 2], np.ones(len(pts), bool), float(len(pts)))
    c = pts.mean(axis=0)
    lam, vec = np.linalg.eigh(np.cov((pts - c).T, bias=True))
    v = vec[:, 0] * np.sign(vec[:, 0] @ plane[:3])
    residual = lam[0] / lam[1]
    assert 0.0 < residual < 1e-4, residual
    assert abs(np.linalg.norm(plane[:3]) - 1.0) < 1e-15
    assert np.linalg.norm(np.cross(plane[:3], v)) <= 100.0 * residual, (np.linalg.norm(np.cross(plane[:3], v)), residual)
    assert abs(plane[3] + v @ c) <= 100.0 * residual * np.abs(c).max() + 1e-12, (plane[3], -v @ c)


@pytest.mark.parametrize("storage", pr.STORAGES)
def test_the_premises_of_the_cases(storage):
    sheets = pr.to_storage(pr.sheets(), storage)
    for params in pr.TIE_PARAMS:  # ties in count AND error, and equal counts with different errors
        r = pr.reference("sheets", storage, params)
        live = [t for t in range(len(r.planes)) if r.planes[t].any()]
        pairs = {}
        for t in live:
            pairs.setdefault(int(r.count[t]), []).append(float(r.error[t]))
        assert any(len(e) - len(set(e)) >= 1 for e in pairs.values()), params
        assert any(len(set(e)) >= 2 for e in pairs.values()), params
    # at the threshold 1.5 the two sheets' own planes tie at the top: the lower index wins
    r = pr.reference("sheets", storage, pr.TIE_PARAMS[1])
    top = [t for t in range(len(r.planes)) if r.planes[t].any() and r.count[t] == r.count[r.best_t] and r.error[t] == r.error[r.best_t]]
    assert len(top) >= 2 and r.best_t == min(top) and r.n_inliers == 128
    # the threshold on the sheet spacing: distances EQUAL to it exist and are no inliers
    r = pr.reference("sheets", storage, pr.TIE_PARAMS[0])
    dist = pr.distances(r.planes, sheets)
    assert pr.TIE_PARAMS[0][0] == pr.SHEET_SPACING and int((dist == pr.SHEET_SPACING).sum()) >= 64
    loose = pr.winner(r.planes, (dist <= pr.SHEET_SPACING).sum(axis=1), pr.ordered_sum(np.where(dist <= pr.SHEET_SPACING, dist, 0.0)), len(sheets))
    assert loose[0] != r.best_t and loose[1] > r.fitness  # with <= a sheet's own plane would take the other sheet too, and win
    # every sample of a line or of one point is degenerate: no winner
    for name in ("collinear", "duplicates"):
        for params in pr.case(name).params:
            r = pr.reference(name, storage, params)
            assert r.n_degenerate == params[2] and r.best_t == -1 and r.n_inliers == 0 and not r.plane.any(), name
    for params in pr.case("no-winner").params:
        r = pr.reference("no-winner", storage, params)
        assert r.best_t == -1 and r.n_inliers == 0 and not r.plane.any() and not r.best_plane.any()
    assert sum(p[2] == 0 for p in pr.case("no-winner").params) == 1 and sum(not p[0] > 0.0 for p in pr.case("no-winner").params) == 3
    # the determinant branches
    for axis in "xyz":
        name = f"ground-{axis}"
        r = pr.reference(name, storage, pr.case(name).params[0])
        g = pr.to_storage(pr.case(name).cloud(), storage)[r.inliers]
        assert pr.fit_axis(g[:, 0], g[:, 1], g[:, 2]) == axis and abs(r.plane["xyz".index(axis)]) > 0.98 and abs(abs(r.plane[3]) - 1.5) < 0.05
    # non-finite points are never inliers; samples that hold one give planes with a NaN, which find nothing
    bad = np.flatnonzero(~np.isfinite(pr.non_finite()).all(axis=1))
    assert len(bad) == 10 and np.isinf(pr.non_finite()).sum() == 5 and np.isnan(pr.non_finite()).any()
    for params in pr.case("non-finite").params:
        r = pr.reference("non-finite", storage, params)
        nan_planes = np.isnan(r.planes).any(axis=1)
        assert nan_planes.sum() >= 2 and (r.count[nan_planes] == 0).all() and r.best_t >= 0 and not np.isin(bad, r.inliers).any()
    assert pr.reference("non-finite", storage, pr.case("non-finite").params[1]).n_inliers == 290  # an infinite threshold: every finite point
    # the sizes around the first second term of a chunk, and a batch crossed
    assert pr.SECOND_TERM == (256, 257, 258) and [pr.chunk_len(m) for m in pr.SECOND_TERM] == [1, 2, 2]
    assert max(p[2] for p in pr.case("iterations").params) == pr.BATCH + 1
    assert sorted({p[1] for c in pr.CASES for p in c.params}) == [3, 4, 8]


def test_f32_storage_decides_membership_at_an_offset():
    params = pr.case("offset").params[0]
    a, b = pr.reference("offset", F32, params), pr.reference("offset", F64, params)
    assert a.best_t >= 0 and b.best_t >= 0
    assert len(np.setxor1d(a.inliers, b.inliers)) >= 1
    # ... under ONE plane too: the f64 winner against both sets of coordinates
    d32 = pr.distances(b.best_plane[None], pr.to_storage(pr.offset_plane(), F32))[0]
    d64 = pr.distances(b.best_plane[None], pr.to_storage(pr.offset_plane(), F64))[0]
    assert int(((d32 < params[0]) != (d64 < params[0])).sum()) >= 1


def test_the_split_scan_is_one_cluster_with_its_floor_and_several_without():
    """the premise of the test through neighbors.SplitByPlane, by cluster_restatement's brute force on the same 8192-point scan"""
    pts = pr.scan(pr.SPLIT_N_AZ)
    assert len(pts) == 8192
    eps, min_points = pr.SPLIT_DBSCAN
    for storage in pr.STORAGES:
        r = pr.segment(pts, *pr.SPLIT_PARAMS, storage)
        assert np.degrees(np.arccos(abs(r.plane[2]))) < 1.0 and abs(abs(r.plane[3]) - 1.5) < 0.05 and r.n_inliers > 3000
        rest = np.delete(pts, r.inliers, axis=0)
        assert cr.closed_form(cr.adjacency(pts, eps, storage)[0], min_points).n_clusters == 1
        assert cr.closed_form(cr.adjacency(rest, eps, storage)[0], min_points).n_clusters == pr.SPLIT_REST_CLUSTERS > 1


def test_the_header_declares_the_names_and_the_mirror_binds_them():
    header = open(os.path.join(ROOT, "include", "o3ds_backend.h")).read()
    assert re.search(r"\}\s*o3ds_plane_result\s*;", header) and re.search(r"\bint\s+o3ds_segment_plane\s*\(", header)
    lib = backend.load()
    assert "o3ds_segment_plane" in backend.SIGNATURES and hasattr(lib, "o3ds_segment_plane")
    assert C.sizeof(backend.PlaneResult) == 8 * 4 + 8 * 4 + 8 + 8 + 8 + 8 + 8
    res = backend.PlaneResult()
    assert lib.o3ds_segment_plane(None, 1, 0.01, 3, 100, 0, C.byref(res), None, 0, None, None) == backend.ERR_BAD_HANDLE
    assert callable(neighbors.SegmentPlane) and callable(neighbors.SplitByPlane) and callable(backend.Backend.segment_plane)
