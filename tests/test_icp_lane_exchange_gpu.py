"""The lane exchanges of the ICP search, the scan loop's loads beyond the end of a range and the order a pass deals its queries out in, on
the device (needs an MI355X).  Inputs: tests/icp_lane_exchange_cases.py; brute force: tests/icp_search_restatement.py; the record of the
PARENT commit's library: tests/golden/icp_lane_exchange_parent.npz (the commit is named in the .txt beside it).

What is held:
  * quad, quad-radius, wave -- per query, both storages, row search and replica, point-to-plane: match or none and the float bits of d2
    as the brute force says (the lattice inputs are exact), the pass record within the bound of tests/icp_search_harness.py,
    and in every island with a tie the record of that query alone against the record each tied point would give (the winner's normal
    names the original index where d2 cannot).  Which lane scanned a winner is read back from its position: the premise that the wave
    case's winners fell on every one of the 64 lanes is asserted, the quad case's lanes are asserted to be all four;
  * the same three inputs through the crop + generalized multi-target kernel (the kernel with the fewest registers to spare): the
    correspondence count of an evaluation pass is the brute force's;
  * array-end-1 ... array-end-17: per query against the brute force on both paths with stale, nearer points behind the target's last
    element, and a registration that stands still (asserted), whose passes 1 to 3 list candidates at the corner: pose, fitness, rmse and
    the per-launch counters (O3DS_ICP_STATS) are the parent's, whose scan loop clamped its loads to the range.  The queries stand one
    cell outside the grid in y and z, so the range they scan is the LAST of the cell-sorted array on the row path and the LAST of the
    replica on the replica path (tests/test_icp_lane_exchange_cpu.py: last_super_row).  A persistent map's pool ends behind its last
    row page only when it is full to the last position; that end is not placed by this file.  For that index the claim is not needed:
    a fresh pool and the slack behind it are cleared to the far sentinel (pm_pool_clear_kernel), and a persistent map is searched per
    query in a block a cloud of nearer points has just left;
  * a target whose cell-sorted points, replica or persistent-map pool was allocated without the slack (A/B switch O3DS_NO_SCAN_SLACK) is
    refused by icp_begin with an error; an index one element above the capacity, which is 2^32 bytes less the slack, is refused (A/B
    switch O3DS_SCAN_SPACE_BYTES stands in for the 2^32), in both storages and for a persistent map's pool;
  * sources of 1 ... 4 099 points: passes 0 and 1 (the two spread orders) and the pass after them, through the fused kernel and
    through begin / accumulate / update / finish (point-to-point, whose updates land for any number of queries): results and step records are the parent's bits.  The partition of the queries into
    workgroups decides the last bit of every sum, so equal bits mean the same permutation.

Recording (parent commit's library only):
    O3DS_BACKEND_LIB=<A/B library built from the parent commit> python tests/test_icp_lane_exchange_gpu.py --record FILE"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (run as a script to record: the package)
import icp_lane_exchange_cases as lc  # noqa: E402
import icp_scan_loop_cases as sc  # noqa: E402
import icp_search_harness as harness  # noqa: E402
import icp_search_restatement as rs  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_lane_exchange_parent.npz")
PATHS, PREC = harness.PATHS, harness.PREC
FIXED = dict(rel_fitness=0.0, rel_rmse=0.0)
END_ITERS = 3


@pytest.fixture(autouse=True)
def _eager_replica(monkeypatch):
    harness.eager_replica(monkeypatch, replica="replica", clear=("O3DS_DEBUG_ACC", "O3DS_ICP_SETS", "O3DS_NO_SCAN_SLACK", "O3DS_SCAN_SPACE_BYTES"))


@pytest.fixture(scope="module")
def ab():
    yield from harness.backends(True)


@pytest.fixture(scope="module")
def shipped():
    yield from harness.backends(False)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _built(name):
    return lc.builders()[name]()


@functools.lru_cache(maxsize=None)
def _ref(name, storage):
    c = _built(name)[0]
    return rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)


def _tied(c, owner, q, storage):
    """the original indices of island q's points at the smallest distance from its query, as the device forms it"""
    mine = np.flatnonzero(owner == q)
    d2 = sc.d2_storage(c.src[q], c.tgt[mine], storage)
    return mine[d2 == d2.min()]


def _check_tie_winners(ses, c, m, owner, storage, what):
    n_ties = 0
    for q in range(len(c.src)):
        tied = _tied(c, owner, q, storage)
        if len(tied) < 2 or m.idx[q] < 0:
            continue
        n_ties += 1
        got = ses.record(q, 1).cpu().numpy()
        dist = {}
        for t in tied:
            idx = np.full_like(m.idx, -1)
            idx[q] = t
            ref, _ = rs.record(m.p, c.tgt, c.nrm, idx, storage, backend.ICP_POINT_TO_PLANE)
            dist[int(t)] = float(np.abs(got - ref)[:27].max())
        assert m.idx[q] == tied.min()
        win = dist.pop(int(tied.min()))
        assert got[28] == 1.0 and win * 1000.0 < min(dist.values()), f"{what} query {q}: the record is not that of the smallest index: {win} {dist}"
    return n_ties


def _lanes(keys, c, owner, islands, width, start_of):
    """the lane (position in its range modulo the scan's stride) that scanned the winner of each of `islands`"""
    none, _, _, pos = rs.decode_keys(keys.cpu().numpy()[:len(c.src)])
    assert not none[list(islands)].any()
    return np.array([(int(pos[i]) - start_of(i)) % width for i in islands])


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", list(lc.builders()))
def test_lane_exchange_per_query(ab, monkeypatch, name, storage):
    c, owner, want = _built(name)
    m = _ref(name, storage)
    assert np.array_equal(m.idx, lc.winners(c, owner, want)), "premise (tests/test_icp_lane_exchange_cpu.py): the brute force's winners"
    n_src = len(c.src)
    ses = harness.Session(ab[storage], c.src, c.tgt, c.nrm, c.r, c.cell)
    try:
        for path in PATHS:
            what = f"{name} {storage} {path}"
            harness.set_path(path, monkeypatch)
            ses.begin(c.T, path)
            keys = ses.keys(rank=3)
            harness.check_keys(keys, m, storage, True, 3, len(c.tgt), 0, n_src, what)
            harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, n_src, what)
            n_ties = _check_tie_winners(ses, c, m, owner, storage, what)
            ses.be.icp_finish()
            if name == "quad":
                assert n_ties == 12
            if name == "wave":
                assert n_ties == lc.WAVE
                # every match comes out of stage 3 (nn_search_wave_far, lanes_min<64>): with that stage skipped (O3DS_DEBUG_ACC=16, A/B
                # library, read when a session begins) a first pass finds none of them
                monkeypatch.setenv("O3DS_DEBUG_ACC", "16")
                ses.begin(c.T, path)
                blind = ses.keys(rank=3)
                monkeypatch.delenv("O3DS_DEBUG_ACC")
                ses.be.icp_finish()
                assert rs.decode_keys(blind.cpu().numpy()[:n_src])[0].all(), f"{what}: premise: a match was found without the far stage"
            if path != "rows":  # (a replica scan's lanes follow the replica's positions, which the keys do not carry)
                continue
            if name == "quad":
                n_one = sum(lc.QUAD_COUNTS)
                lanes = _lanes(keys, c, owner, range(n_one), 4, lambda i: lc.segment_start(owner, i))
                print(f"LANES {what}: winners per lane of the group {np.bincount(lanes, minlength=4).tolist()}")
                assert set(lanes.tolist()) == {0, 1, 2, 3}, f"{what}: premise: the winners did not fall on every lane of a group"
            if name == "wave":
                lanes = _lanes(keys, c, owner, range(lc.WAVE), 64, lambda i: 1 + lc.WAVE * i)
                print(f"LANES {what}: lanes of the wavefront that held a winner: {len(set(lanes.tolist()))} of 64")
                assert sorted(lanes.tolist()) == list(range(64)), f"{what}: premise: the winners did not fall on every lane of the wavefront"
    finally:
        ses.close()


@pytest.mark.parametrize("name", list(lc.builders()))
def test_lane_exchange_in_the_crop_generalized_multi_target_kernel(shipped, name):
    """an evaluation pass (max_iteration 0) of o3ds_icp_register_multi, generalized, under a crop that keeps everything: the count is the
    brute force's, the rmse that of its matches"""
    c = _built(name)[0]
    m = _ref(name, rs.F32)
    be = shipped[rs.F32]
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=(0.0, 0.0, 0.0), rmax=1e6)
    s = be.upload(c.src, rs.unit_normals(np.random.default_rng(9), len(c.src)))
    t = be.upload(c.tgt, c.nrm)
    try:
        be.build_index(t, c.r, c.cell)
        got = be.icp_register_multi(s, [t], form=be.MULTI_UNION, crop=crop, init=c.T, params=be._params(c.r, 0, 0.0, 0.0, backend.ICP_GENERALIZED))
        hit = m.idx >= 0
        print(f"LANES {name} generalized multi-target: n_corr {got['n_corr']} of {len(c.src)}, rmse {got['inlier_rmse']}")
        assert got["n_corr"] == hit.sum()
        mean = m.d2[hit].sum() / hit.sum()
        assert abs(got["inlier_rmse"] ** 2 - mean) <= rs.D2_F32_REL * mean
    finally:
        be.free(s)
        be.free(t)


# ---- the end of the array ---------------------------------------------------------------------------------------------------------------
def _open_end(be, c, stale):
    """the target behind the stale cloud (harness.open_behind_stale, whose session ends with icp_finish before it is closed: the calls the
    parent's record was made with)"""
    return harness.open_behind_stale(be, c, stale, finish=True)


def _end_registrations(storage):
    """{case|storage|path: (floats, ints)} of the array-end cases of a storage, on a handle of its own"""
    os.environ["O3DS_NN_REPLICA_AFTER"] = "1"
    out = {}
    be = backend.Backend(0, PREC[storage], ab=True)
    try:
        for n_last in lc.END_LENGTHS:
            c, stale = lc.array_end_case(n_last)
            ses = _open_end(be, c, stale)
            for path in PATHS:
                harness.set_path(path)
                ses.begin(c.T, path)
                out[f"{c.name}|{storage}|{path}"] = harness.pack(be.icp_point_to_plane_dev(ses.s, ses.t, c.r, init=c.T, max_iter=END_ITERS, **FIXED))
            ses.close()
    finally:
        be.close()
    return out


def _end_child(storage):
    return harness.child_with_stats("test_icp_lane_exchange_gpu", f"t._end_registrations({storage!r})", unset=("O3DS_ICP_SETS", "O3DS_DEBUG_ACC", "O3DS_NO_SCAN_SLACK"))


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_array_end_per_query(ab, monkeypatch, storage):
    for n_last in lc.END_LENGTHS:
        c, stale = lc.array_end_case(n_last)
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        ses = _open_end(ab[storage], c, stale)
        try:
            for path in PATHS:
                what = f"{c.name} {storage} {path}"
                harness.set_path(path, monkeypatch)
                ses.begin(c.T, path)
                # (the corner queries: the d2 bound is relative, and the fill queries stand AT their match -- the record counts those)
                harness.check_keys(ses.keys(0, 64, 3), m, storage, False, 3, len(c.tgt), 0, 64, what)
                harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, len(c.src), what)
                ses.be.icp_finish()
        finally:
            ses.close()


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_array_end_lists_and_registrations_equal_the_parents(golden, storage):
    res, lines = _end_child(storage)
    names = [f"array-end-{n}|{storage}|{p}" for n in lc.END_LENGTHS for p in PATHS]
    assert list(res) == names and len(lines) == len(names)
    want = dict(zip(golden["end_names"].tolist(), range(len(golden["end_names"]))))
    for k, ln in zip(names, lines):
        f, i = res[k]
        print(f"END {k}: {ln}; iterations {i[0]} n_corr {i[1]} rmse {f[17]}")
        assert np.array_equal(f[:16].reshape(4, 4), np.eye(4)), f"{k}: premise: the registration moved\n{f[:16].reshape(4, 4)}"
        n_last = int(k.split("|")[0].split("-")[-1])
        c = lc.array_end_case(n_last)[0]
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        assert i.tolist() == [END_ITERS, int((m.idx >= 0).sum())], (k, i)
        passes = harness.parse_stats(ln)
        assert passes[1]["k"] > 0, f"{k}: premise: pass 1 lists candidates: {ln}"
        g = want[k]
        assert np.array_equal(i, golden["end_ints"][g]), (k, i)
        harness.assert_bits(f, golden["end_floats"][g], k)
        assert ln == str(golden["end_stats"][g]), (k, ln, str(golden["end_stats"][g]))


PM_STALE = 4_600_000  # points of the cloud whose cell-sorted array leaves the block a persistent map's pool then takes


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_a_persistent_map_whose_pool_takes_a_block_full_of_nearer_points(ab, storage):
    """tests/test_icp_search_exact_gpu.py::test_persistent_map_target in a reused block.  Every range of a row-paged index is followed by
    page slots no point was written to, and the scan loop now loads them: a cloud of PM_STALE points around the queries, nearer to each
    than any map point, is uploaded, indexed and freed first, and its cell-sorted array is of the block class the pool asks for (asserted
    for every size the pool can have here).  The pool is cleared to the far sentinel when the map enters the persistent form
    (pm_pool_clear_kernel), so these points are gone before the first search; whatever a change leaves of them behind a range would win."""
    be = ab[storage]
    src, tgt, _ = rs.void_cloud(0.3)
    rng = np.random.default_rng(640)
    v = rng.normal(size=(PM_STALE, 3))
    stale = rs.VOID_CENTRE + v / np.linalg.norm(v, axis=1, keepdims=True) * (0.2 * rng.uniform(size=(PM_STALE, 1)) ** (1.0 / 3.0))
    near = rs.nearest_within(src, stale[:20_000], np.eye(4), 1.0, storage)
    b = lc.POINT_BYTES[storage]
    have = sc.pool_block(b * PM_STALE + lc.SCAN_SLACK_BYTES)
    for n_map in (0, len(tgt)):  # pool = 6 n + 16 scan_upper + 2^22 positions (pm_enter_t), n = the map's points when it enters
        assert sc.pool_reuses(have, b * (6 * n_map + 16 * 10_000 + (1 << 22)) + lc.SCAN_SLACK_BYTES), "premise: one block class"
    st = be.upload(stale)
    be.build_index(st, 1.0, 0.25)
    be.synchronize()
    be.free(st)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=tuple(rs.VOID_CENTRE), rmax=2.5)
    mp = be.upload(np.zeros((0, 3)))
    scans = [be.upload(tgt[:10_000]), be.upload(tgt[10_000:])]
    ses = harness.Session(be, src, None, None, 1.0, None, target_id=mp)
    try:
        for s_ in scans:
            be.map_insert_scan(mp, s_, np.eye(4), 0.1, crop, max_corr_hint=1.0)
        assert be.is_persistent_map(mp)
        ses.begin(np.eye(4), method=backend.ICP_POINT_TO_POINT)
        keys = ses.keys(rank=2)
        rec = ses.record()
        assert be.is_persistent_map(mp), "taking keys folded the map"
        pts, _ = be.download(mp)
        m = rs.nearest_within(src, pts, np.eye(4), 1.0, storage)
        assert (near.d2 < m.d2).all(), "premise: a stale point is nearer to every query than any map point"
        what = f"persistent map in a reused block {storage}"
        harness.premises(m, 1.0, what)
        harness.check_keys(keys, m, storage, False, 2, None, 0, len(src), what)
        harness.check_record(rec, m, pts, None, storage, backend.ICP_POINT_TO_POINT, 0, len(src), what)
        be.icp_finish()
    finally:
        for s_ in scans:
            be.free(s_)
        ses.close()


def _refused(ses, T, path=None, method=backend.ICP_POINT_TO_PLANE):
    with pytest.raises(backend.BackendError) as e:
        ses.begin(T, path, method=method)
    assert "kScanSlackBytes" in str(e.value), str(e.value)


def test_a_target_without_the_slack_is_refused(ab, monkeypatch):
    """O3DS_NO_SCAN_SLACK (A/B library, read when an index array is allocated) allocates the cell-sorted points, the replica and a
    persistent map's pool as a caller unaware of the scan loop would: icp_begin refuses each such target, and says why, before it runs
    anything against it"""
    c = _built("quad-radius")[0]
    be = ab[rs.F32]
    # ---- the cell-sorted points
    monkeypatch.setenv("O3DS_NO_SCAN_SLACK", "1")
    ses = harness.Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)
    monkeypatch.delenv("O3DS_NO_SCAN_SLACK")
    try:
        _refused(ses, c.T)
        be.build_index(ses.t, c.r, c.cell)  # rebuilt as the library does it: accepted
        ses.begin(c.T)
        harness.check_keys(ses.keys(rank=1), _ref("quad-radius", rs.F32), rs.F32, True, 1, len(c.tgt), 0, len(c.src), "rebuilt with the slack")
        be.icp_finish()
        # ---- the replica alone: the index has its slack, the replica built at this registration (O3DS_NN_REPLICA_AFTER=1) has none
        be.build_index(ses.t, c.r, c.cell)
        assert be.index_replica(ses.t) == 0
        monkeypatch.setenv("O3DS_NO_SCAN_SLACK", "1")
        _refused(ses, c.T)
        monkeypatch.delenv("O3DS_NO_SCAN_SLACK")
        assert be.index_replica(ses.t) > 0, "premise: the refused target is the one with the replica"
        _refused(ses, c.T)  # (and stays refused: the replica is what it is)
    finally:
        ses.close()
    # ---- a persistent map's pool
    _, tgt, _ = rs.void_cloud(0.3)
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=tuple(rs.VOID_CENTRE), rmax=2.5)
    mp = be.upload(np.zeros((0, 3)))
    scans = [be.upload(tgt[:10_000]), be.upload(tgt[10_000:])]
    ses = harness.Session(be, c.src, None, None, 1.0, None, target_id=mp)
    try:
        monkeypatch.setenv("O3DS_NO_SCAN_SLACK", "1")
        for s_ in scans:
            be.map_insert_scan(mp, s_, np.eye(4), 0.1, crop, max_corr_hint=1.0)
        monkeypatch.delenv("O3DS_NO_SCAN_SLACK")
        assert be.is_persistent_map(mp)
        _refused(ses, np.eye(4), method=backend.ICP_POINT_TO_POINT)  # (the map carries no normals)
    finally:
        for s_ in scans:
            be.free(s_)
        ses.close()


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_a_capacity_one_element_above_the_limit_is_refused(ab, monkeypatch, storage):
    """The limit of a searched array is 2^32 bytes LESS the slack (an offset into the slack must not wrap).  O3DS_SCAN_SPACE_BYTES (A/B
    library) stands in for the 2^32, the slack still comes off it: an index of exactly (space - slack) / sizeof(point) points is built,
    one point more is refused with O3DS_ERR_CAPACITY -- and a persistent map whose pool does not fit is refused alike."""
    be = ab[storage]
    n = 1000
    pts = np.random.default_rng(630).uniform(0.0, 2.0, size=(n + 1, 3))
    space = n * lc.POINT_BYTES[storage] + lc.SCAN_SLACK_BYTES
    at, above = be.upload(pts[:n]), be.upload(pts)
    try:
        monkeypatch.setenv("O3DS_SCAN_SPACE_BYTES", str(space))
        be.build_index(at, 1.0, 0.25)
        with pytest.raises(backend.BackendError) as e:
            be.build_index(above, 1.0, 0.25)
        assert "slack" in str(e.value) and e.value.code == backend.ERR_CAPACITY, str(e.value)
        monkeypatch.setenv("O3DS_SCAN_SPACE_BYTES", str(space + lc.POINT_BYTES[storage] - 1))  # (a fraction of an element is none)
        with pytest.raises(backend.BackendError):
            be.build_index(above, 1.0, 0.25)
        monkeypatch.setenv("O3DS_SCAN_SPACE_BYTES", str(space + lc.POINT_BYTES[storage]))
        be.build_index(above, 1.0, 0.25)
        # the persistent map's pool is at least 2^22 positions: it does not fit 2^22 * sizeof(point) bytes of space, less the slack
        monkeypatch.setenv("O3DS_SCAN_SPACE_BYTES", str((1 << 22) * lc.POINT_BYTES[storage]))
        _, tgt, _ = rs.void_cloud(0.3)
        crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=tuple(rs.VOID_CENTRE), rmax=2.5)
        mp = be.upload(np.zeros((0, 3)))
        scans = [be.upload(tgt[:10_000]), be.upload(tgt[10_000:])]
        try:
            with pytest.raises(backend.BackendError) as e:
                for s_ in scans:  # (as tests/test_icp_search_exact_gpu.py::test_persistent_map_target enters the persistent form)
                    be.map_insert_scan(mp, s_, np.eye(4), 0.1, crop, max_corr_hint=1.0)
            assert "slack" in str(e.value) and e.value.code == backend.ERR_CAPACITY, str(e.value)
        finally:
            for s_ in scans:
                be.free(s_)
            be.free(mp)
    finally:
        monkeypatch.delenv("O3DS_SCAN_SPACE_BYTES", raising=False)
        be.free(at)
        be.free(above)


# ---- the order the queries are dealt out in ---------------------------------------------------------------------------------------------
def _order_run(be, n_src):
    """(fused floats, fused ints, step-wise floats, step-wise ints, records [ORDER_ITERS + 1][32]) of one source size on a handle"""
    import torch

    src, tgt, nrm, T0 = lc.order_inputs(n_src)
    s, t = be.upload(src), be.upload(tgt, nrm)
    rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    try:
        be.build_index(t, 1.0, 0.25)
        kw = dict(init=T0, max_iter=lc.ORDER_ITERS, method=backend.ICP_POINT_TO_POINT, **FIXED)
        ff, fi = harness.pack(be.icp_register_dev(s, t, 1.0, **kw))
        be.icp_begin(s, t, 1.0, **kw)
        recs = []
        for _ in range(lc.ORDER_ITERS + 1):
            be.icp_accumulate(0, n_src, rec.data_ptr())
            be.synchronize()
            recs.append(rec.cpu().numpy().copy())
            be.icp_update(rec.data_ptr(), n_src)
            if be.icp_done():
                break
        sf, si = harness.pack(be.icp_finish())
    finally:
        be.free(s)
        be.free(t)
    assert len(recs) == lc.ORDER_ITERS + 1
    return ff, fi, sf, si, np.array(recs)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("n_src", lc.ORDER_COUNTS)
def test_query_order_is_the_parents(shipped, golden, n_src, storage):
    ff, fi, sf, si, recs = _order_run(shipped[storage], n_src)
    g = golden["order_names"].tolist().index(f"order-{n_src}|{storage}")
    print(f"ORDER {n_src} {storage}: iterations {fi[0]} n_corr {fi[1]} rmse {ff[17]}; pass records' counts {recs[:, 28].tolist()}")
    assert fi[0] == lc.ORDER_ITERS and (ff[:16] != rs.LATER_INIT.reshape(16)).any() and fi[1] > 0, "premise: two updates were taken, and they landed"
    for what, a, b in (("fused result", ff, golden["order_fused_floats"][g]), ("step-wise result", sf, golden["order_step_floats"][g]),
                       ("step-wise records", recs, golden["order_records"][g])):
        harness.assert_bits(a, b, (what, n_src, storage))
    assert np.array_equal(fi, golden["order_fused_ints"][g]) and np.array_equal(si, golden["order_step_ints"][g])
    assert np.array_equal(ff.view(np.uint64), sf.view(np.uint64)) and np.array_equal(fi, si), "the fused form and the step-wise form differ"


# ---- recording (parent commit's library only) -----------------------------------------------------------------------------------------
if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or not os.environ.get("O3DS_BACKEND_LIB"):
        sys.exit("usage: O3DS_BACKEND_LIB=<A/B library built from the PARENT commit> python tests/test_icp_lane_exchange_gpu.py --record FILE")
    import torch  # noqa: F401  (before the backend library is loaded: see tests/conftest.py)

    out = {}
    names, floats, ints, stats = [], [], [], []
    for storage_ in rs.STORAGES:
        res_, lines_ = _end_child(storage_)
        assert len(res_) == len(lines_)
        for (k_, (f_, i_)), ln_ in zip(res_.items(), lines_):
            names.append(k_), floats.append(f_), ints.append(i_), stats.append(ln_)
            print(k_, i_.tolist(), f_[16:].tolist(), ln_, flush=True)
    out.update(end_names=np.array(names), end_floats=np.array(floats, np.float64), end_ints=np.array(ints, np.int64), end_stats=np.array(stats))
    names, cols = [], [[], [], [], [], []]
    for storage_ in rs.STORAGES:
        be_ = backend.Backend(0, PREC[storage_])
        for n_ in lc.ORDER_COUNTS:
            names.append(f"order-{n_}|{storage_}")
            for col_, v_ in zip(cols, _order_run(be_, n_)):
                col_.append(v_)
            print(names[-1], cols[1][-1].tolist(), cols[0][-1][16:].tolist(), flush=True)
        be_.close()
    out.update(order_names=np.array(names), order_fused_floats=np.array(cols[0]), order_fused_ints=np.array(cols[1]),
               order_step_floats=np.array(cols[2]), order_step_ints=np.array(cols[3]), order_records=np.array(cols[4]))
    np.savez(sys.argv[2], **out)
    print("recorded", len(out["end_names"]), "array-end registrations and", len(out["order_names"]), "query-order runs")
