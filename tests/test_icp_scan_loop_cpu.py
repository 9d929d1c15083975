"""The premises of tests/icp_scan_loop_cases.py, on numpy alone: that the unsigned order of the 64-bit key is the order of the candidate
test, that the ties are ties in f32 arithmetic as the kernel forms d2, that the radius cases sit where they claim, that the segments have
the lengths they claim and that the stale cloud of the array-end case would be taken from the pool and would win."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_scan_loop_cases as sc  # noqa: E402
import icp_search_restatement as rs  # noqa: E402


def _before(d2, idx, bd2, bidx):
    """the candidate test as icp_kernels.hpp states it for every storage: nearer, or equally near with the smaller (signed) index"""
    with np.errstate(invalid="ignore"):
        return bool((d2 < bd2) | ((d2 == bd2) & (idx < bidx)))


def test_key_order_is_the_order_of_the_pair():
    """for float32 d2 >= 0 (and the NaNs of either sign) and indices in [0, 2^31 - 2]: key(candidate) < key(best), unsigned, exactly when
    the candidate comes before the best under the float compare with the signed index tie-break"""
    d2s = np.concatenate([sc.KEY_D2, sc.KEY_NANS])
    n = 0
    for d2 in d2s:
        for i in sc.KEY_IDX:
            for bd2 in sc.KEY_D2:  # (a bound is never a NaN: r^2 or the distance of an accepted point)
                for bi in sc.KEY_IDX:
                    assert bool(sc.key(d2, i) < sc.key(bd2, bi)) == _before(d2, i, bd2, bi), (d2, i, bd2, bi)
                    n += 1
    assert n == len(d2s) * len(sc.KEY_D2) * len(sc.KEY_IDX) ** 2
    assert (np.diff(sc.key(sc.KEY_D2, 0).astype(np.float64)) > 0).all(), "the listed distances ascend, and so do their bit patterns"
    assert sc.key(np.float32(0.0), 0) == 0 and np.signbit(np.float32(0.0) * np.float32(-1.0)), "-0 exists, but not as a square:"
    for v in (np.float32(-0.0), np.float32(-1e-30), np.float32(0.0)):
        assert not np.signbit(v * v) and not np.signbit(np.float32(v * v + np.float32(0.0) * np.float32(0.0)))


def test_key_order_with_the_empty_bound():
    """the empty bound {r^2, -1, kNoIdx}: signed, idx < -1 is never true; unsigned, the low word 0 is below no index either.  A low word
    of 0xffffffff (the -1 of the signed form, reinterpreted) WOULD admit the point on the radius: the case the encoding exists for"""
    r2 = np.float32(1.5625)
    below = np.nextafter(r2, np.float32(0.0))
    for i in sc.KEY_IDX:
        assert not sc.key(r2, i) < sc.key(r2, sc.NO_IDX) and not _before(r2, i, r2, -1)
        assert sc.key(below, i) < sc.key(r2, sc.NO_IDX) and _before(below, i, r2, -1)
        assert sc.key(r2, i) < sc.key(r2, -1), "(the reinterpreted -1 is the largest low word)"
        for nan in sc.KEY_NANS:
            assert not sc.key(nan, i) < sc.key(r2, sc.NO_IDX)
    # the multi-target search's "index infinity" (a tie against the carried match of a HIGHER slot wins): 2^31 - 1 in both forms
    for i in sc.KEY_IDX:
        assert sc.key(r2, i) < sc.key(r2, 2 ** 31 - 1) and _before(r2, i, r2, 2 ** 31 - 1)


def test_ties_are_ties_in_f32_arithmetic_as_the_kernel_forms_d2():
    case, owner = sc.ties_case()
    assert owner[0] == 0 and owner[-1] == len(case.src) - 1, "index 0 and the largest index are island points"
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, rs.F32)
    for q in range(len(case.src)):
        mine = np.flatnonzero(owner == q)
        d2, exact = sc.d2_f32_fused(case.src[q], case.tgt[mine])
        assert exact.all(), "every step of the fused form is exact on these coordinates"
        assert (d2 == d2[0]).all() and len(mine) >= 2, (q, d2)
        assert d2[0] < np.float32(case.r * case.r)
        assert m.idx[q] == mine.min(), "the smaller original index wins"
        assert m.gap[q] == 0.0
    assert m.idx[0] == 0 and m.idx[-1] == owner.size - len(sc.TIE_SPHERE), "index 0 wins its tie; the last island's winner is its first point"
    assert (owner == len(case.src) - 1).sum() == 6 and owner[-1] == len(case.src) - 1, "the largest index is among the tied points (and loses)"
    # where the pairs lie: the cells (offsets from the own cell) the descriptions name
    cells = {name: (tuple(int(np.floor(v)) for v in a), tuple(int(np.floor(v)) for v in b)) for name, a, b in sc.TIE_PAIRS}
    assert cells["same cell, neighbours in a group's lanes"] == ((0, 0, 0), (0, 0, 0))
    assert cells["stage 1 against stage 2"] == ((1, 1, 1), (2, 0, 0)) and cells["stage 2 against stage 3"] == ((2, 2, 0), (3, 0, 0))
    assert cells["two half-rows of the far stage"] == ((-3, 0, 0), (3, 0, 0))
    assert max(abs(c) for c in cells["two rows of the 3x3x3 block"][0] + cells["two rows of the 3x3x3 block"][1]) == 1
    assert max(abs(c) for c in cells["two rows of the 5x5x5 shell"][0] + cells["two rows of the 5x5x5 shell"][1]) == 2


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_radius_premises(storage):
    case, owner = sc.radius_case(storage)
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, storage)
    r2 = rs.r2_storage(case.r, storage)
    assert r2 == 1.5625
    on = int(np.flatnonzero(owner == 0)[0])
    assert m.idx[0] == -1 and m.best[0] == r2, "the only candidate lies ON the radius: no match"
    assert ((case.tgt[on] - case.src[0]) ** 2).sum() == r2
    one = np.float32 if storage == rs.F32 else np.float64
    assert m.idx[1] == int(np.flatnonzero(owner == 1)[0]) and (owner == 1).sum() == 1
    assert sc.d2_storage(case.src[1], case.tgt[m.idx[1]], storage) == np.nextafter(one(r2), one(0.0)), "one number below r^2 as the device forms it"
    if storage == rs.F64:
        assert m.d2[1] == np.nextafter(r2, 0.0), "(the brute force forms d2 the way the f64 device code does)"
    assert m.idx[2] == int(np.flatnonzero(owner == 2)[1]) and m.d2[2] == 0.25
    assert m.idx[3] == -1 and m.best[3] == r2 and m.gap[3] == 0.0, "a tie on the radius"


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_radius_still_premises(storage):
    """the fused kernel's radius case: two candidates-on-the-radius islands without a match, every matched pair with a residual that is
    zero whatever the order of its sum (each of the three products is), one of them one number below r^2"""
    case, owner = sc.radius_still_case(storage)
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, storage)
    r2 = rs.r2_storage(case.r, storage)
    assert m.idx[0] == -1 and m.best[0] == r2 and m.idx[3] == -1 and m.best[3] == r2 and m.gap[3] == 0.0
    hit = m.idx >= 0
    assert hit.sum() == 2 + sc.STILL_FILL and hit[1] and hit[2]
    one = np.float32 if storage == rs.F32 else np.float64
    assert sc.d2_storage(case.src[1], case.tgt[m.idx[1]], storage) == np.nextafter(one(r2), one(0.0))
    assert m.d2[2] == 0.25 and (m.d2[4:] == 0.0).all()
    s, t, n = (rs.to_storage(a, storage) for a in (case.src, case.tgt, case.nrm))
    prod = (s[hit] - t[m.idx[hit]]) * n[m.idx[hit]]
    assert (prod == 0.0).all(), "p - q has no component along the normal, term by term: the residual is exactly zero"
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6).all()


def test_starts_of_later_passes():
    """what the sessions begun one cell aside, or out of reach, cache before the hand-written update takes the pose back to the identity"""
    for name, t in sc.STARTS.items():
        for c in sc.lattice_cases():
            moved = c.src + np.asarray(t)
            assert (moved.astype(np.float32).astype(np.float64) == moved).all(), "the translated queries are exact in f32"
            assert (moved - np.asarray(t) == c.src).all()
            assert (c.T == np.eye(4)).all() and c.exact
    rec = sc.step_back_record(sc.ONE_CELL)
    assert (rec[[0, 6, 11, 15, 18, 20]] == 1.0).all() and (rec[24:27] == sc.ONE_CELL).all() and rec[28] > 0 and np.count_nonzero(rec) == 8
    for c in sc.lattice_cases():
        for s in c.storages:
            assert (rs.nearest_within(c.src, c.tgt, sc.translation(sc.OUT_OF_REACH), c.r, s).idx == -1).all(), "out of reach: every query caches `none`"
    for storage in rs.STORAGES:  # the radius: the cached point of islands 0 and 3 is the one that lies ON the radius at the identity
        case, owner = sc.radius_case(storage)
        ms = rs.nearest_within(case.src, case.tgt, sc.translation(sc.ONE_CELL), case.r, storage)
        for q in (0, 3):
            k = int(np.flatnonzero(owner == q)[0])
            assert ms.idx[q] == k and ((case.tgt[k] - case.src[q]) ** 2).sum() == rs.r2_storage(case.r, storage)
        assert ms.idx[1] == int(np.flatnonzero(owner == 1)[0]), "and island 1's is the point one below r^2"
    case, owner = sc.ties_case()  # ties: somewhere the cached point is a tied point of the LARGER index, which the search must replace
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, rs.F32)
    ms = rs.nearest_within(case.src, case.tgt, sc.translation(sc.ONE_CELL), case.r, rs.F32)
    loser = [q for q in range(len(case.src)) if ms.idx[q] >= 0 and owner[ms.idx[q]] == q and ms.idx[q] > m.idx[q]]
    keeper = [q for q in range(len(case.src)) if ms.idx[q] == m.idx[q]]
    assert len(loser) >= 3 and len(keeper) >= 3, (loser, keeper)


def _cells_of(case):
    return np.floor(case.tgt / case.cell).astype(np.int64)


def test_segment_lengths():
    case, owner = sc.segments_case()
    cells = _cells_of(case)
    for q, n in enumerate(sc.SEGMENT_COUNTS):
        mine = owner == q
        assert mine.sum() == n and len(np.unique(cells[mine], axis=0)) == 1, "n points in one cell"
        assert (cells[mine][0] == np.floor(case.src[q] / case.cell)).all(), "the query's own cell"
        near = np.abs(cells[~mine] - cells[mine][0]).max(axis=1) <= sc.K + 1
        assert not near.any(), "nothing else in reach of the search (K cells and the cell the query may leave by)"
    assert set(n % 16 for n in sc.SEGMENT_COUNTS) == set(range(16)), "a group scan ends at every residue mod 16"
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, rs.F32)
    assert (m.idx >= 0).all() and (m.gap > 0).sum() >= 30, "a nearest point each (an equidistant pair here or there falls to the tie rule)"
    rank = np.array([int(np.flatnonzero(np.flatnonzero(owner == q) == m.idx[q])[0]) for q in range(len(case.src))])
    n = np.array(sc.SEGMENT_COUNTS)
    assert (rank == 0).any() and (rank == n - 1).any() and ((rank > 0) & (rank < n - 1)).any(), "winners first, last and inside their cell"


def test_half_row_lengths():
    case, owner = sc.half_rows_case()
    cells = _cells_of(case)
    for q, n in enumerate(sc.HALF_ROW_COUNTS):
        mine = owner == q
        own = np.floor(case.src[q] / case.cell).astype(np.int64)
        assert mine.sum() == n and (cells[mine] == own + np.array([0, 3, 0])).all(), "n points in the cell three rows up, the own x-column"
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, rs.F32)
    assert (m.idx >= 0).all() and (np.sqrt(m.d2) > 2.0 * sc.CELL).all(), "found, and beyond the two cells of the group stages for certain"
    assert sc.HALF_ROW_COUNTS == (255, 256, 257)


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_array_end_premises(storage):
    case, stale = sc.array_end_case()
    item = 16 if storage == rs.F32 else 32
    have = sc.pool_block(item * len(stale))
    assert sc.pool_reuses(have, item * len(case.tgt)) and have >= item * (len(case.tgt) + 16), \
        "the stale cloud's block serves the target's request, with room for stale points behind the target's last element"
    assert not sc.pool_reuses(sc.pool_block(item * len(case.tgt)) * 2, item * len(case.tgt)), "(the rule has an upper end)"
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, storage)
    assert (m.idx >= 0).all()
    g = np.floor((case.tgt - case.tgt.min(axis=0)) / case.cell).astype(np.int64)
    last = g.max(axis=0)
    assert (g[m.idx] == last).all(), "every nearest neighbour lies in the last cell of the cell-sorted order"
    ms = rs.nearest_within(case.src, stale, case.T, case.r, storage)
    assert (ms.d2 < m.d2).all(), "a stale point is nearer to every query than any target point"
