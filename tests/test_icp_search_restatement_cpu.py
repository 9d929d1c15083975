"""The brute-force restatement of the ICP correspondence search (tests/icp_search_restatement.py) against the oracle, and the premises of
the inputs that tests/test_icp_search_exact_gpu.py runs on the device.  No GPU: this proves the reference itself.

For every input, in both storages: the brute force and oracle.KDTree / oracle.evaluate agree on match or no match per query and on d2
(on the winner as well wherever the winner is unique), and the record of the brute-force matches agrees with oracle.compute_jtj_jtr.

Premises (asserted, cap zero), on every input that is not exact arithmetic by construction:
  * no matched query has a relative gap between its best and second-best d2 below 1e-5 -- the f32 search forms d2 within 8 * 2^-24 =
    4.8e-7 relative, so the device cannot legitimately pick another winner;
  * no query has |d - r| / r below 1e-6 (d the distance to its nearest kept point), so match / no match is not a rounding question.
The exact-arithmetic cases are exempt: their ties and boundary hits are intended.

The generalized estimator's record (rs.record_gicp: Open3D's own form per pair, in extended precision) is proven three ways: against the
oracle's gicp_jtj_jtr fed with the oracle's covariance_from_normal (1e-12 of the scale; the largest ratio is printed), through three
iterations of the oracle's icp_generalized, and against the closed form the device documents (rs.FORM_CLOSED).  The distance between the
two forms per pair is DEFECT[case, storage]: below 1e-12 in f64 storage, a few 1e-6 in f32 storage, where the stored normals are unit
only to 6e-8 -- the GPU tests widen their comparison with Open3D's form by it and hold the closed form at full sharpness.  It compares one
reference with the other, never with the device."""
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


# ---- the generalized estimator ---------------------------------------------------------------------------------------------------------
GICP_CASES = rs.GICP_CASES
ORACLE_TOL = 1e-12   # the oracle forms M^-1/2 by Jacobi rotations in f64 and sums in query order; agreement was 4e-15 of the scale
_gicp_case, gicp_matches, defect = rs._gicp_case, rs.gicp_matches, rs.defect  # (shared with the GPU tests: tests/icp_search_restatement.py)


def _oracle_gicp(oracle, p, tgt_s, nt_s, ns_s, idx, T, eps):
    """the oracle's normal equations over the matches: covariances from covariance_from_normal, the source's rotated by R"""
    hit = np.flatnonzero(idx >= 0)
    used, corr = np.unique(idx[hit], return_inverse=True)   # (covariances of the matched target points only)
    R = np.asarray(T)[:3, :3]
    Cs = np.array([R @ oracle.covariance_from_normal(n, eps) @ R.T for n in ns_s[hit]]).reshape(-1, 9)
    Ct = np.array([oracle.covariance_from_normal(n, eps) for n in nt_s[used]]).reshape(-1, 9)
    return oracle.gicp_jtj_jtr(p[hit], Cs, tgt_s[used], Ct, corr.astype(np.int32))


def _check_against_oracle(oracle, c, m, storage, what):
    tgt_s, nt_s, ns_s = rs.to_storage(c.tgt, storage), rs.to_storage(c.nrm, storage), rs.to_storage(c.src_nrm, storage)
    rec, scale = rs.record(m.p, c.tgt, c.nrm, m.idx, storage, rs.METHOD_GENERALIZED, src_nrm=c.src_nrm, T=c.T, eps=c.eps)
    JTJ, JTr = _oracle_gicp(oracle, m.p, tgt_s, nt_s, ns_s, m.idx, c.T, c.eps)
    A, b, _ = rs.jtj_from_record(rec)
    SA, Sb, _ = rs.jtj_from_record(scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = max(np.nanmax(np.abs(A - JTJ) / (ORACLE_TOL * SA)), np.nanmax(np.abs(b - JTr) / (ORACLE_TOL * Sb)))
    print(f"GICP {what}: restated record against the oracle, deviation / bound {ratio:.3e}, {int(rec[28])} matches")
    assert ratio <= 1.0, what
    assert rec[28] == (m.idx >= 0).sum()
    return ratio


@pytest.mark.parametrize("case", GICP_CASES, ids=[c.name for c in GICP_CASES])
def test_generalized_record_equals_the_oracle(oracle, case):
    for storage in case.storages:
        what = f"{case.name} {storage}"
        m = gicp_matches(case.name, storage)
        if not case.groups and not case.name.startswith("lattice"):
            _premises(m, case.r, what)   # (the lattice ties by construction; the edge case has a test of its own below)
        _check_against_oracle(oracle, case, m, storage, what)


def test_generalized_record_under_a_crop_equals_the_oracle(oracle):
    src, tgt, nrm = rs.void_cloud(rs.CROP_VOID)
    c = rs.GicpCase("crop0", src, rs.void_source_normals(rs.CROP_VOID), tgt, nrm, 1.0, 0.25, np.eye(4))
    for storage in rs.STORAGES:
        keep = oracle.crop_indices(rs.to_storage(tgt, storage), oracle.make_crop(**rs.CROPS[0]))
        m = rs.nearest_within(src, tgt, c.T, 1.0, storage, keep=keep)
        _check_against_oracle(oracle, c, m, storage, f"crop0 {storage}")


def test_three_iterations_of_the_oracles_generalized_icp(oracle):
    """the registration-level anchor: [O3D] RegistrationGeneralizedICP restated with the brute-force search, the restated record and the
    oracle's solve reproduces the oracle's own loop (which carries the transformed points and covariances from update to update)"""
    src, tgt, nrm = rs.void_cloud(0.0)
    sn = rs.void_source_normals(0.0)
    T = rs.LATER_INIT.copy()
    for _ in range(3):
        m = rs.nearest_within(src, tgt, T, 1.0, rs.F64)
        rec, _ = rs.record_gicp(m.p, tgt, nrm, sn, m.idx, T, rs.GICP_EPSILON, rs.F64)
        JTJ, JTr, _ = rs.jtj_from_record(rec)
        U, x = oracle.solve_update(JTJ, JTr)
        assert np.abs(x).max() > 1e-3   # (the updates are no fixed point: random normals make the pose jump)
        T = U @ T
    ref = oracle.icp_generalized(src, sn, tgt, nrm, 1.0, init=rs.LATER_INIT, max_iter=3, rel_fitness=0.0, rel_rmse=0.0)
    m = rs.nearest_within(src, tgt, T, 1.0, rs.F64)
    print("GICP anchor: |T - T_oracle| max", np.abs(T - ref["transformation"]).max(), "n_corr", ref["n_corr"])
    # three solves of a system of condition ~1e3 on records that agree to 1e-14: far below 1e-10
    np.testing.assert_allclose(T, ref["transformation"], rtol=0.0, atol=1e-10)
    assert ref["n_corr"] == (m.idx >= 0).sum() and ref["iterations"] == 3


@pytest.mark.parametrize("void", [0.0, 0.6])
def test_premises_of_the_generalized_later_passes(oracle, void):
    """test_later_passes and the fused-kernel tests of tests/test_icp_search_exact_gpu.py assert the gap and radius premises at the poses
    the DEVICE reaches from LATER_INIT in 0..3 generalized updates.  Those poses depend on the source normals; here the same loop is
    played with the restated record and the oracle's solve, and the premises are held with ten times the margin, so that the device's
    poses, which differ from these by roundings, keep them."""
    src, tgt, nrm = rs.void_cloud(void)
    sn = rs.void_source_normals(void)
    for storage in rs.STORAGES:
        T = rs.LATER_INIT.copy()
        for k in range(4):
            m = rs.nearest_within(src, tgt, T, 1.0, storage)
            gap, near = _premises(m, 1.0, f"void{void} {storage} round {k}")
            assert gap >= 10 * GAP_MIN and near >= 10 * NEAR_R_MIN, (void, storage, k, gap, near)
            rec, _ = rs.record_gicp(m.p, tgt, nrm, sn, m.idx, T, rs.GICP_EPSILON, storage)
            JTJ, JTr, _ = rs.jtj_from_record(rec)
            T = oracle.solve_update(JTJ, JTr)[0] @ T


def test_closed_form_against_open3ds_form():
    """DEFECT: the closed form I - k n n^T of the device's documentation (with n := e1 for x < -0.99 and for the zero vector) against
    Rx diag(eps, 1, 1) Rx^T, per pair, relative to |B|_2"""
    for c in GICP_CASES:
        for storage in c.storages:
            d = defect(c.name, storage)
            print(f"GICP DEFECT[{c.name}, {storage}] = {d:.3e}")
            if storage == rs.F64:
                assert d < 1e-12, (c.name, d)
            else:
                assert d < 1e-3, (c.name, d)   # (f32 unit normals: 6e-8 off unit, times |B| <= 500; nothing like the 0.9 of a wrong rule)


def test_zero_normal_is_e1_in_open3ds_form(oracle):
    """[O3D] GetRotationFromE1ToX of the zero vector is the identity (c = 0, v = 0), so its covariance is diag(eps, 1, 1) -- the closed
    form's I - k n n^T would make it I.  The closed form agrees with Open3D's on the zero-normal pairs only under the rule n := e1 for
    n == 0, which is the rule write_record implements."""
    for eps in rs.GICP_EPSILONS:
        assert np.array_equal(oracle.covariance_from_normal([0.0, 0.0, 0.0], eps), np.diag([eps, 1.0, 1.0]))
        assert np.array_equal(rs.covariance_from_normals(np.zeros((1, 3)), eps)[0].astype(np.float64), np.diag([eps, 1.0, 1.0]))
    c = _gicp_case("gicp-edge")
    zero_groups = [g for g in c.groups if g[0].endswith("zero")]
    assert len(zero_groups) == 2
    for storage in rs.STORAGES:
        m = gicp_matches(c.name, storage)
        for name, first, count in zero_groups:
            idx = np.full_like(m.idx, -1)
            idx[first:first + count] = m.idx[first:first + count]
            without = rs.gicp_defect(c.nrm, c.src_nrm, idx, c.T, c.eps, storage, zero_is_e1=False)
            with_rule = rs.gicp_defect(c.nrm, c.src_nrm, idx, c.T, c.eps, storage, zero_is_e1=True)
            print(f"GICP {name} {storage}: closed form against Open3D's, without the rule {without:.3e}, with it {with_rule:.3e}")
            assert without > 0.1 and with_rule < (1e-12 if storage == rs.F64 else 1e-3)


def test_premises_of_the_edge_case():
    c = _gicp_case("gicp-edge")
    R = c.T[:3, :3]
    assert len(c.groups) == 2 * len(rs.EDGE_X) + 5 and len(c.src) == 300 and c.n_plain == 20_000
    ends = [f + n for _, f, n in c.groups]
    assert [f for _, f, _ in c.groups] == [0] + ends[:-1] and ends[-1] <= len(c.src)   # disjoint, contiguous
    ang = np.degrees(np.arccos((np.trace(R) - 1) / 2))
    assert abs(ang - 170.0) < 1e-9 and np.abs(c.T[:3, :3] @ rs.VOID_CENTRE + c.T[:3, 3] - rs.VOID_CENTRE).max() < 0.05
    # -0.99 itself: its f32-nearest value lies below -0.99, so f32 storage takes the special case where f64 storage does not; the value
    # float(f32(-0.99)) is below -0.99 in both
    assert rs.to_storage([rs.X99], rs.F32)[0] < -0.99 and not rs.to_storage([rs.X99], rs.F64)[0] < -0.99
    assert rs.to_storage([np.nextafter(rs.X99, 0.0)], rs.F32)[0] < -0.99
    assert all(rs.to_storage([float(np.float32(rs.X99))], s)[0] < -0.99 for s in rs.STORAGES)
    ref = gicp_matches(c.name, rs.F64)
    for storage in rs.STORAGES:
        m = gicp_matches(c.name, storage)
        assert (m.idx >= 0).all() and (m.idx < c.n_plain).all()   # a duplicate has the larger index and loses
        np.testing.assert_array_equal(m.idx, ref.idx)             # the groups are the same pairs in both storages
        _premises(rs.nearest_within(c.src, c.tgt[:c.n_plain], c.T, c.r, storage), c.r, f"{c.name} {storage}")
        nt, ns = rs.to_storage(c.nrm, storage)[m.idx], rs.to_storage(c.src_nrm, storage)
        fires_t, fires_s = nt[:, 0] < -0.99, ns[:, 0] < -0.99
        for (name, first, count), (_, x) in zip(c.groups, rs.EDGE_X + rs.EDGE_X):
            g = slice(first, first + count)
            assert count >= rs.EDGE_GROUP, name
            side, fires = (nt, fires_t) if name.startswith("tgt") else (ns, fires_s)
            if x is None:
                assert (side[g] == 0.0).all(), name
            else:
                stored = rs.to_storage([x], storage)[0]
                assert (side[g][:, 0] == stored).all() and (fires[g] == (stored < -0.99)).all(), name
                assert np.abs(np.linalg.norm(side[g], axis=1) - 1).max() < (1e-6 if storage == rs.F32 else 1e-15), name
            # a target-side group holds EVERY pair of its target points
            if name.startswith("tgt"):
                assert np.isin(np.flatnonzero(np.isin(m.idx, m.idx[g])), np.arange(first, first + count)).all(), name
        by_name = {name: slice(first, first + count) for name, first, count in c.groups}
        a = ns @ R.T
        for name in ("src a=b", "src a=-b", "src a orthogonal b"):   # neither side takes the special case in these groups
            g = by_name[name]
            assert not fires_t[g].any() and not fires_s[g].any(), name
        tol = 1e-6 if storage == rs.F32 else 1e-15
        assert np.abs(a[by_name["src a=b"]] - nt[by_name["src a=b"]]).max() < tol
        assert np.abs(a[by_name["src a=-b"]] + nt[by_name["src a=-b"]]).max() < tol
        g = by_name["src a orthogonal b"]
        assert np.abs((a[g] * nt[g]).sum(axis=1)).max() < tol and np.abs(np.linalg.norm(ns[g], axis=1) - 1).max() < tol
        g = by_name["src rotates to -e1"]
        assert (ns[g][:, 0] > 0.9).all() and not fires_s[g].any() and (a[g][:, 0] < -0.99).all()   # must NOT fire after the rotation
        g = by_name["src -e1 rotates away"]
        assert (ns[g] == [-1.0, 0.0, 0.0]).all() and fires_s[g].all() and (a[g][:, 0] > 0.9).all()  # must fire
        # the duplicates: had the copy won, the record would differ visibly
        dups = np.arange(c.n_plain, len(c.tgt))
        assert len(dups) == rs.EDGE_DUPLICATES
        for j in dups:
            orig = np.flatnonzero((c.tgt[:c.n_plain] == c.tgt[j]).all(axis=1))
            assert len(orig) == 1 and (m.idx == orig[0]).any()
            mine = np.where(m.idx == orig[0], m.idx, -1)
            rec, scale = rs.record_gicp(m.p, c.tgt, c.nrm, c.src_nrm, mine, c.T, c.eps, storage)
            other, _ = rs.record_gicp(m.p, c.tgt, c.nrm, c.src_nrm, np.where(mine >= 0, j, -1), c.T, c.eps, storage)
            rel = (np.abs(rec - other)[:28] / scale[:28]).max()
            assert rel > 1e-6, (j, rel)
