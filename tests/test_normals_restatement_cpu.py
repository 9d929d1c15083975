"""The brute-force restatement of the normals' neighbour selection (tests/normals_restatement.py) against the oracle's own k-d tree search,
and the premises of the cases tests/test_normals_exact_gpu.py runs on the device.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_restatement as nr  # noqa: E402
from normals_restatement import F32, F64  # noqa: E402


def _equal(got, ref, what):
    differ = np.flatnonzero(np.any(got != ref, axis=1))
    assert len(differ) == 0, (what, len(differ), differ[:5], got[differ[:3]], ref[differ[:3]])


def test_f64_restatement_is_the_oracle_on_the_scan_and_the_tie_clouds(oracle):
    """normals(..., F64) -- all pairs, stable sort, orc_normals_from_neighbours -- equals oracle.estimate_normals -- k-d tree, insertion,
    the same arithmetic -- bit for bit: on a thinned scan and on the lattice / duplicate / tiny clouds of
    test_normals_with_exact_ties_duplicates_and_tiny_clouds"""
    pts = nr.scan_thin()
    assert 2000 < len(pts) < 4500
    for radius, knn in ((3.0, 20), (1.0, 5), (0.5, 30), (2.0, 48)):
        _equal(nr.normals(pts, radius, knn, F64), oracle.estimate_normals(pts, radius, knn), ("scan", radius, knn))
    g = np.stack(np.meshgrid(np.arange(12) * 0.25, np.arange(12) * 0.25, np.arange(3) * 0.25, indexing="ij"), -1).reshape(-1, 3) + [3.0, -2.0, 1.0]
    rng = np.random.default_rng(3)
    dup = np.vstack([g, g[rng.choice(len(g), 40, replace=False)], g[:5], g[:5]])
    shuffled = dup[rng.permutation(len(dup))]
    for pts, cases in ((g, ((0.6, 7), (1.0, 20), (0.3, 30))), (shuffled, ((0.6, 7), (0.26, 5), (2.0, 40))),
                       (g[:2], ((1.0, 20),)), (g[:1], ((1.0, 5),)), (g[:7], ((5.0, 20),))):
        for radius, knn in cases:
            _equal(nr.normals(pts, radius, knn, F64), oracle.estimate_normals(pts, radius, knn), (len(pts), radius, knn))


@pytest.mark.parametrize("case", nr.ALL_CASES, ids=lambda c: c.name)
def test_f64_restatement_is_the_oracle_on_every_case(oracle, case):
    """every cloud and (radius, max_nn) of the table, f64: the restatement and the oracle agree bit for bit (for the cases the device runs in
    f32 storage as well this is the proof that the restatement's selection and hand-over are right; f32 changes the number type only)"""
    pts = case.cloud()
    for radius, knn in case.params:
        L, nrm, r = nr.reference(case.name, radius, knn, F64)
        _equal(nrm, oracle.estimate_normals(pts, r, knn), (case.name, r, knn))
        assert (L.cnt >= 1).all()  # (the point itself)


def test_raw_lists_give_the_raw_oracle(oracle):
    """raw = 1 (no normalisation, no orientation): the k-NN normals of the generalized estimator from restated lists"""
    pts = nr.scan_thin()[:600]
    L = nr.search(pts, nr.beyond_radius(pts), 20, F64)
    assert (L.cnt == 20).all()
    _equal(nr.normals_from(pts, L, F64, raw=True), oracle.estimate_normals_knn_raw(pts, 20), "knn raw")


def test_f32_selects_the_f64_lists_where_the_coordinates_are_exact():
    """on a lattice whose coordinates and squared distances are exact in f32 the two storages select the same lists"""
    for pts in (nr.lattice(), nr.face_cloud()[:700]):
        assert (pts.astype(np.float32).astype(np.float64) == pts).all()
        for radius, knn in ((0.6, 7), (1.0, 20), (0.3, 30), (1.0, 33)):
            a, b = nr.search(pts, radius, knn, F32), nr.search(pts, radius, knn, F64)
            assert (a.cnt == b.cnt).all() and (a.idx == b.idx).all() and (a.tie == b.tie).all()
        assert nr.search(nr.lattice(), 1.0, 20, F32).tie.any()


def test_the_order_is_d2_then_index_and_the_radius_is_strict():
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, 2.0], [0, 0, 1.0]])
    for st in nr.STORAGES:
        L = nr.search(pts, 2.0, 4, st)
        assert L.idx[0].tolist() == [0, 1, 2, 3] and L.cnt[0] == 4 and L.tie[0] and L.runner_up[0] == 5  # (0, 0, 2) at d2 = r^2 is out
        L = nr.search(pts, 2.0, 8, st)
        assert L.cnt[0] == 5 and L.idx[0, :5].tolist() == [0, 1, 2, 3, 5] and not L.tie[0] and L.runner_up[0] == -1
        L = nr.search(pts, 2.0 * (1 + 1e-6), 8, st)
        assert L.cnt[0] == 6


def test_premises_of_the_reuse_pairs():
    """deep: on the cell the clump leaves behind (radius / 64) the spread cloud's max_nn-th neighbours lie at least ten cells out.  crowded:
    every point of the clump has more than 128 candidates in its 3x3x3 block of cells, on its own cell and on the lonely cloud's.  The sizes
    of each pair are within 25 %, which is what lets normals_t reuse the cell."""
    radius, knn = nr.REUSE_PARAMS
    for st in nr.STORAGES:
        clump, spread, lonely = (nr.to_storage(f(), st) for f in (nr.clump_cloud, nr.spread_cloud, nr.lonely_cloud))
        for _, first, second in nr.REUSE:
            a, b = len(first()), len(second())
            assert 0.75 * a <= b <= 1.25 * a and a != b
        small = nr.expected_cell(clump, radius, knn)
        assert small == radius / 64.0
        L, _, _ = nr.reference("spread", radius, knn, st)
        assert (L.cnt == knn).all()
        kth = np.linalg.norm(spread[L.last] - spread, axis=1)
        assert kth.min() >= 10 * small and np.median(kth) >= 15 * small, (kth.min() / small, np.median(kth) / small)
        nxyz = nr.cells_of(spread, small).max(axis=0) + 1
        assert 2e6 < np.prod(nxyz) < 2 ** 27  # a table of a few million cells, within the index's limit
        large = nr.expected_cell(lonely, radius, knn)
        assert large == radius / 8.0 * np.sqrt(knn / 3.14159265358979)  # one point per occupied pilot cell
        for cell in (small, large):
            c = nr.cells_of(clump, cell)
            assert (c.max(axis=0) + 1 <= 5).all()
            block = (np.abs(c[:, None, :] - c[None, :, :]) <= 1).all(axis=2).sum(axis=1)
            assert block.min() > 128, (cell, block.min())
        assert (nr.cells_of(clump, large).max(axis=0) + 1 <= 2).all()  # all of it in one or two cells per axis: thousands of candidates a round


def test_premises_of_the_mixed_the_beyond_and_the_degenerate_cases():
    radius, knn = nr.MIXED_PARAMS
    for st in nr.STORAGES:
        m = nr.to_storage(nr.mixed_cloud(), st)
        cell = nr.expected_cell(m, radius, knn)
        assert radius / 64.0 < cell < radius
        c = nr.cells_of(m, cell)
        _, inv, per = np.unique(c, axis=0, return_inverse=True, return_counts=True)
        occ = per[inv.reshape(-1)]
        assert (occ > 128).sum() >= 1400 and (occ <= 4).sum() >= 1000  # both regimes on one grid
        L, _, _ = nr.reference("mixed", radius, knn, st)
        assert (L.cnt == knn).sum() >= 2900  # (a few points at the sheet's rim have short lists)
        s = nr.to_storage(nr.scan_thin(), st)
        L, _, r = nr.reference("beyond", None, 20, st)
        d = s.max(axis=0) - s.min(axis=0)
        assert r > np.linalg.norm(d) and (L.cnt == 20).all()
        assert len(np.unique(nr.to_storage(nr.planar_cloud(), st)[:, 2])) == 1
        col = nr.to_storage(nr.collinear_cloud(), st)
        assert len(np.unique(col[:, 1])) == 1 and len(np.unique(col[:, 2])) == 1
        f = nr.to_storage(nr.face_cloud(), st)
        assert (f == nr.face_cloud()).all()
        for radius_f, knn_f in nr.FACE_PARAMS:
            cell = nr.expected_cell(f, radius_f, knn_f)
            assert cell == 1.0 / 16.0
            fr = (f - f.min(axis=0)) * (1.0 / cell)
            assert (fr == np.floor(fr)).all()  # every point on cell faces
            c = nr.cells_of(f, cell)
            assert (c.min(axis=0) == 0).all() and (c.max(axis=0) == 15).all()  # queries in the first and the last cells


def test_the_seeded_f32_cases_hold_ties_only_f32_makes():
    """where two candidates tie for the last place in f32 d2 and do not in f64, the device must go by the index -- a neighbour taken by
    distance there would be another point.  Every seeded f32 cloud must hold such places (the lattices tie in both types)."""
    for case in nr.PER_POINT:
        if case.name not in nr.SEEDED_F32:
            continue
        pts = case.cloud()
        total = 0
        for radius, knn in case.params:
            L, _, _ = nr.reference(case.name, radius, knn, F32)
            total += int(nr.f32_only_ties(pts, L).sum())
        assert total > 0, case.name
    L, _, _ = nr.reference("offset", 3.0, 20, F32)
    assert nr.f32_only_ties(nr.offset_cloud(), L).sum() >= 20


def test_duplicates_that_only_f32_merges_change_the_lists():
    pts = nr.shuffled_duplicates()
    a, b = nr.search(pts, 0.26, 5, F32), nr.search(pts, 0.26, 5, F64)
    assert (a.idx != b.idx).any()


def test_ragged_prefixes_cover_short_and_full_lists():
    radius, knn = nr.RAGGED_PARAMS
    assert nr.RAGGED_SIZES == (1, 2, 3, 5, 15, 17, 63, 65, 4097)
    L, _, _ = nr.reference("ragged-4097", radius, knn, F32)
    assert (L.cnt == knn).all()
    L, _, _ = nr.reference("ragged-17", radius, knn, F32)
    assert (L.cnt < 3).any()


def test_the_lattices_hold_candidates_at_exactly_the_radius():
    """(0.5, 48) and (0.25, 20) on the 0.25 m lattice: lists shorter than max_nn, with lattice points at d2 == r^2 exactly in both number
    types -- a `<=` in the radius test would lengthen them"""
    g = nr.lattice()
    for radius, knn, inside in ((0.5, 48, 27), (0.25, 20, 1)):
        for st in nr.STORAGES:
            L = nr.search(g, radius, knn, st)
            d2 = ((g[:, None, :] - g[None, :, :]) ** 2).sum(axis=2)
            assert (L.cnt == (d2 < radius * radius).sum(axis=1)).all() and L.cnt.max() == inside < knn
            assert ((d2 == radius * radius).sum(axis=1) >= 2).all()
