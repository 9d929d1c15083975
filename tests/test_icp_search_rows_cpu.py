"""The inputs of tests/icp_search_rows_cases.py against the brute force of tests/icp_search_restatement.py (no GPU): every case says what
it is built to say -- which rows hold a neighbour, on which side of a split it lies, that ties are exact, that the points on the ball's
extreme decide the way f32 arithmetic on the device decides them, that the clipped queries have neighbours to find."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_search_restatement as rs  # noqa: E402
import icp_search_rows_cases as rc  # noqa: E402


def _cells(c, pts):
    return np.floor((pts - c.tgt.min(axis=0)) / c.cell).astype(int)


def test_sizes_stay_small():
    for c in rc.all_cases():
        assert len(c.src) <= 2048 and len(c.tgt) <= 20000, c.name


@pytest.mark.parametrize("K", rc.ROW_KS)
def test_every_row_of_the_cross_section_holds_one_islands_point(K):
    c = rc.row_case(K)
    assert math.ceil(c.r / c.cell) == K and len(c.src) == (2 * K + 1) ** 2
    d = _cells(c, c.tgt[1:-1]) - _cells(c, c.src)
    rows = {(int(a), int(b)) for a, b in d[:, 1:]}
    assert rows == {(a, b) for a in range(-K, K + 1) for b in range(-K, K + 1)}
    inner = (np.abs(d[:, 1]) <= 2) & (np.abs(d[:, 2]) <= 2)
    assert (d[inner, 0] == -3).all() and (d[~inner, 0] == 0).all()  # beyond the five cells of stages 1 and 2 / the own column
    for storage in rs.STORAGES:
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        hit = m.idx >= 0
        assert (m.idx[hit] == 1 + np.flatnonzero(hit)).all()                     # its own island's point, nothing else
        assert (np.isinf(m.gap[hit]) | (m.gap[hit] > c.r * c.r)).all()          # and nothing else within reach
        reach = np.hypot(np.maximum(np.abs(d[:, 1]) - 0.75, 0), np.maximum(np.abs(d[:, 2]) - 0.75, 0)) < K - 0.3
        assert hit[reach & ~inner].all() and hit.sum() >= 0.8 * len(hit) and not hit.all()  # (the corner rows are out of reach at every K)
        assert (np.abs(np.sqrt(m.best) - c.r) > 1e-3 * c.r).all()               # nobody near the radius


def test_island_normals_lie_across_the_line_to_the_query_and_stay_distinct():
    for c in rc.lattice_cases()[:-1]:  # (all but the clipping case, whose target is a random cloud)
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F64)
        hit = m.idx >= 0
        d = c.src[hit] - c.tgt[m.idx[hit]]
        nrm = rc.registration_normals(c)
        assert (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-12).all(), c.name
        assert (np.abs((nrm[m.idx[hit]] * d).sum(axis=1)) <= 1e-12 * np.linalg.norm(d, axis=1)).all(), c.name  # no residual at the start
        assert len(np.unique(nrm.round(6), axis=0)) == len(nrm), c.name                           # distinct per point
    for c in (rc.clipping_case(), rc.lists_case()):
        assert rc.registration_normals(c) is c.nrm


def test_x_split_covers_both_sides_of_both_splits():
    c = rc.xsplit_case()
    d = _cells(c, c.tgt[1:-1]) - _cells(c, c.src)
    want = [(dx, dy, dz) for dy, dz in rc.XSPLIT_ROWS for dx in rc.XSPLIT_DX]
    assert [tuple(int(v) for v in row) for row in d] == want
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F32)
    assert (m.idx == 1 + np.arange(len(c.src))).all() and (m.d2 > 0).all()


def test_ties_are_exact_and_in_both_orders():
    c = rc.ties_case()
    for storage in rs.STORAGES:
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        assert (m.gap == 0.0).all() and (m.idx == 1 + 2 * np.arange(len(c.src))).all()
        assert (np.sqrt(m.d2) / c.cell >= 3.0).all()  # the far stage's
    d = _cells(c, c.tgt[1:-1]).reshape(-1, 2, 3) - _cells(c, c.src)[:, None, :]
    assert (d[0::2, 0] == d[1::2, 1]).all() and (d[0::2, 1] == d[1::2, 0]).all()   # the same pair, swapped
    K, side = 4, 9
    row = (d[..., 2] + K) * side + d[..., 1] + K
    assert (row[0] == row[0, 0]).all() and (row[2] == row[2, 0]).all()           # one row, two halves
    assert d[0, 0, 0] < 0 < d[0, 1, 0] and d[2, 0, 0] == -3 and d[2, 1, 0] == 3
    assert sorted(row[8] % 64) == [4, 4] and row[8, 0] != row[8, 1]               # the two rows of lane 4
    assert row[4, 0] % 64 != row[4, 1] % 64                                       # two lanes


def _d2_f32(q, t):
    """dist2 of icp_kernels.hpp in f32 storage: fmaf(dz, dz, fmaf(dy, dy, dx * dx)), every step rounded to f32 (the f64 products of
    f32 values are exact)"""
    d = (t.astype(np.float32) - q.astype(np.float32)).astype(np.float64)
    a = np.float32(d[0] * d[0])
    b = np.float32(d[1] * d[1] + np.float64(a))
    return np.float32(d[2] * d[2] + np.float64(b))


@pytest.mark.parametrize("bound", rc.SUPERSET_BOUNDS)
def test_points_on_the_balls_extreme_sit_on_cell_borders_and_decide_alike_in_f32(bound):
    c = rc.superset_case(bound)
    r2 = c.r * c.r
    assert np.float32(r2) == r2
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F64)
    steps = [s for _ in range(len(c.src) // len(rc.ULP_STEPS)) for s in rc.ULP_STEPS]
    for i, step in enumerate(steps):
        q, t = c.src[i], c.tgt[1 + i]
        assert (m.idx[i] == 1 + i) == (step > 0), (i, step)
        d2 = float(np.sum((t - q) ** 2))
        assert (d2 == r2) if step == 0 else (0 < abs(d2 - r2) < 1e-4 * r2)
        assert (_d2_f32(q, t) < np.float32(r2)) == (step > 0), (i, step)        # the device's own arithmetic decides the same way
        fx = (t[0] - c.tgt[:, 0].min()) / c.cell
        off = abs(fx - round(fx))
        assert off <= rc.BORDER_INSET + 1e-3, (i, off)                          # the extreme is a border, or within the margin of one
    m32 = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F32)
    assert (m32.idx == m.idx).all()


def test_clipped_queries_have_neighbours_cells_away():
    c = rc.clipping_case()
    assert (c.tgt.min(axis=0) == 0.0).all() and (c.tgt.max(axis=0) == rc.CLIP_BOX).all()
    out = ((c.src < 0.0) | (c.src > rc.CLIP_BOX)).any(axis=1)
    assert out.sum() == 52 and (~out).sum() == 26
    cells = _cells(c, c.src[~out])
    assert ((cells == 0) | (cells == 9)).any(axis=1).all()                        # a boundary cell of the ten-cell grid
    for storage in rs.STORAGES:
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        hit = m.idx >= 0
        assert hit[out].sum() >= 10 and (~hit[out]).sum() >= 10 and hit[~out].sum() >= 20
        assert (np.sqrt(m.d2[hit]) > 2.5 * c.cell).sum() >= 10                   # matches the far stage finds
        assert (m.gap[hit] / m.d2[hit] >= 1e-5).all() and (np.abs(np.sqrt(m.best) - c.r) / c.r >= 1e-6).all()


def test_lists_case_has_hundreds_of_far_queries_with_a_match():
    c = rc.lists_case()
    assert len(c.src) == 2048 and len(c.tgt) == rc.LISTS_MAP
    from open3d_slam_amd import synthetic as syn

    dt, dr = syn.se3_error(c.T, syn.ground_truth_pose())
    # the start is millimetres from the truth: twice the motion back of the farthest scan point stays well under the 4 cm cap on a margin
    assert 1e-3 < dt < 5e-3 and 2.0 * (dt + 2.0 * math.sin(dr / 2.0) * math.sqrt(2.0) * np.linalg.norm(c.src, axis=1).max()) < 0.03
    for storage in rs.STORAGES:
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        hit = m.idx >= 0
        assert (hit & (np.sqrt(m.d2) > rc.LISTS_FAR_CELLS * c.cell)).sum() >= 200 and hit.sum() >= 1000
        assert (m.gap[hit] / m.d2[hit] >= 1e-5).all() and (np.abs(np.sqrt(m.best) - c.r) / c.r >= 1e-6).all()
