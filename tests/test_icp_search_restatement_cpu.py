"""The brute-force restatement of the ICP correspondence search (tests/icp_search_restatement.py) against the oracle, and the premises of
the inputs that tests/test_icp_search_exact_gpu.py runs on the device.  No GPU: this proves the reference itself.

For every input, in both storages: the brute force and oracle.KDTree / oracle.evaluate agree on match or no match per query and on d2
(on the winner as well wherever the winner is unique), and the record of the brute-force matches agrees with oracle.compute_jtj_jtr.

Premises (asserted, cap zero), on every input that is not exact arithmetic by construction:
  * no matched query has a relative gap between its best and second-best d2 below 1e-5 -- the f32 search forms d2 within 8 * 2^-24 =
    4.8e-7 relative, so the device cannot legitimately pick another winner;
  * no query has |d - r| / r below 1e-6 (d the distance to its nearest kept point), so match / no match is not a rounding question.
The exact-arithmetic cases are exempt: their ties and boundary hits are intended."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_search_restatement as rs  # noqa: E402

CASES = rs.all_cases()
GAP_MIN, NEAR_R_MIN = 1e-5, 1e-6


def _premises(m, r, what):
    hit = m.idx >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = m.gap[hit] / m.d2[hit]
    assert rel.size == 0 or rel.min() >= GAP_MIN, f"{what}: relative gap {rel.min():.3e}"
    fin = np.isfinite(m.best)
    near = np.abs(np.sqrt(m.best[fin]) - r) / r
    assert near.size == 0 or near.min() >= NEAR_R_MIN, f"{what}: |d - r| / r = {near.min():.3e}"
    return (rel.min() if rel.size else np.inf), (near.min() if near.size else np.inf)


def _against_oracle(oracle, m, tgt_s, r, keep, exact, what):
    """match / no match and d2 per finite query against the k-d tree over the kept points"""
    kept = np.arange(len(tgt_s)) if keep is None else np.asarray(keep)
    fin = np.isfinite(m.q).all(axis=1)
    assert not (m.idx[~fin] >= 0).any(), what
    if len(kept) == 0:
        assert not (m.idx >= 0).any(), what
        return
    tree = oracle.KDTree(tgt_s[kept])
    corr, d2, _, _, nc = oracle.evaluate(tree, m.q[fin], r)
    idx = m.idx[fin]
    on_radius = m.best[fin] == r * r  # exact cases only: the boundary hit itself, which the strict test excludes by specification
    assert exact or not on_radius.any()
    sel = ~on_radius
    np.testing.assert_array_equal(corr[sel] >= 0, idx[sel] >= 0, err_msg=what)
    hit = sel & (idx >= 0)
    np.testing.assert_allclose(d2[hit], m.d2[fin][hit], rtol=1e-13, atol=0, err_msg=what)
    if not exact:  # unique winners: the same point
        np.testing.assert_array_equal(kept[corr[hit]], idx[hit], err_msg=what)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_brute_force_agrees_with_the_oracle_and_premises_hold(oracle, case):
    for storage in case.storages:
        what = f"{case.name} {storage}"
        m = rs.nearest_within(case.src, case.tgt, case.T, case.r, storage)
        tgt_s, nrm_s = rs.to_storage(case.tgt, storage), rs.to_storage(case.nrm, storage)
        _against_oracle(oracle, m, tgt_s, case.r, None, case.exact, what)
        if not case.exact:
            _premises(m, case.r, what)
        # the record of these matches (the oracle's sums run in query order: rounding of n additions)
        rec, scale = rs.record(m.p, case.tgt, case.nrm, m.idx, storage)
        fin = np.isfinite(m.p).all(axis=1)
        JTJ, JTr, r2 = oracle.compute_jtj_jtr(m.p[fin], tgt_s, nrm_s, m.idx[fin].astype(np.int32))
        A, b, s = rs.jtj_from_record(rec)
        S = rs.jtj_from_record(scale)
        tol = 4.0 * max(int((m.idx >= 0).sum()), 1) * 2.0 ** -53
        assert (np.abs(A - JTJ) <= tol * S[0] + 1e-300).all(), what
        assert (np.abs(b - JTr) <= tol * S[1] + 1e-300).all(), what
        assert abs(s - r2) <= tol * S[2] + 1e-300, what
        assert rec[28] == (m.idx >= 0).sum()


def test_inputs_reach_what_they_are_for():
    """the shapes are the ones the mechanisms need: matches and misses where the text says so, distances that span the stages"""
    d = []
    for v in rs.STAGE_VOIDS:
        c = rs.stage_case(v, 0.25)
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F64)
        d.append(np.sqrt(m.best))
    assert d[0].min() < 0.02 and d[3].max() > 0.85  # nearest distances from millimetres to beyond three default cells
    assert d[3].min() > 0.75  # void 0.9: every query lies more than three default cells from anything, whole workgroups go to stage 3
    print("nearest distances per void:", [(round(float(x.min()), 4), round(float(x.max()), 4)) for x in d])
    c = rs.stage_case(0.9, 0.25, r=0.5)
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F32)
    assert 10 < (m.idx >= 0).sum() < len(c.src) - 10  # matches and misses mixed
    c = rs.far_radius_case()
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F32)
    assert m.idx.tolist() == [0, 0, -1, 1] and abs(np.sqrt(m.d2[0]) - 3.5) < 0.01 and c.r / c.cell == 100
    c = rs.outside_case()
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F64)
    assert (m.idx[-7:] == -1).all() and (m.idx >= 0).sum() == 20  # 0.2 r and 0.9 r match, 1.1 r and 3 r do not
    c = rs.lattice_case(300)
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, rs.F32)
    assert (m.idx >= 0).all() and (m.gap == 0).all()  # every match ties at least with its duplicate
    ways = {int(round(x)) for x in (m.d2 / (rs.LATTICE_CELL / 2) ** 2)}
    assert {0, 1, 2, 3} <= ways  # on a point, edge, face and body midpoints
    for case in rs.radius_cases():
        for storage in case.storages:
            m = rs.nearest_within(case.src, case.tgt, case.T, case.r, storage)
            assert (m.idx[0] >= 0) == ("inward" in case.name), case.name
            assert "inward" in case.name or m.best[0] == rs.r2_storage(case.r, storage)


@pytest.mark.parametrize("k", range(len(rs.CROPS)))
def test_cropped_brute_force_agrees_with_the_oracle(oracle, k):
    spec = rs.CROPS[k]
    src, tgt, nrm = rs.void_cloud(rs.CROP_VOID)
    for storage in rs.STORAGES:
        tgt_s = rs.to_storage(tgt, storage)
        keep = oracle.crop_indices(tgt_s, oracle.make_crop(**spec))
        m = rs.nearest_within(src, tgt, np.eye(4), 1.0, storage, keep=keep)
        what = f"crop {spec} {storage}"
        _against_oracle(oracle, m, tgt_s, 1.0, keep, False, what)
        if len(keep):
            _premises(m, 1.0, what)
            assert np.isin(m.idx[m.idx >= 0], keep).all()
    if k == 0:  # the nearest points of every query are excluded: without the crop every winner is another point
        free = rs.nearest_within(src, tgt, np.eye(4), 1.0, rs.F64)
        assert (free.idx != m.idx).all() and (m.idx >= 0).sum() > 100


def test_later_pass_inputs_and_decode():
    """the init of the later-pass cases is off by (0.4, -0.3, 0.1) m and about 3 degrees; keys decode to what was packed"""
    R = rs.LATER_INIT[:3, :3]
    ang = np.degrees(np.arccos((np.trace(R) - 1) / 2))
    assert 2.5 < ang < 3.5 and np.allclose(R @ R.T, np.eye(3), atol=1e-15)
    d2 = np.array([0.25, 1e-9, 3.0], dtype=np.float32)
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(5) << np.uint64(28)) | np.array([0, 7, (1 << 28) - 1], dtype=np.uint64)
    keys = np.concatenate([keys, [np.uint64(rs.NO_KEY)]]).view(np.int64)
    none, dd, rank, pos = rs.decode_keys(keys)
    assert none.tolist() == [False, False, False, True] and (dd[:3] == d2).all() and (rank[:3] == 5).all() and pos[:3].tolist() == [0, 7, (1 << 28) - 1]
