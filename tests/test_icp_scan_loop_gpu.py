"""The scan loop of the ICP search on the device (needs an MI355X): the inputs of tests/icp_scan_loop_cases.py, per query against the brute
force of tests/icp_search_restatement.py, and a three-iteration registration of each against a record made with the PARENT commit's
library (tests/golden/icp_scan_loop_parent.npz; the commit is named in tests/golden/icp_scan_loop_parent.txt).

What is held, per case, in the storages the case names, row search and replica:
  * o3ds_icp_nn_keys per query -- match or none as the brute force says, equal float bits of d2 (the lattice inputs are exact in both
    storages), a position inside the target -- in a first pass (the empty bound {r^2, none}) and in passes that start from a cached bound.
    A search reads the cache only once the session's pass count is above zero, and only an update raises it, so the pass is advanced
    with hand-written records through o3ds_icp_update (tests/icp_scan_loop_cases.py: ZERO_RECORD, step_back_record):
      - the identity update: pass 1 at the pose of pass 0, every query from what its own first search cached, its match or `none`;
      - lattice cases: a session begun one cell aside, searched there, and stepped back to the identity: pass 1 from STALE matches --
        in the tie case the tied point of the larger index, which must be replaced, in the radius case the point that now lies ON the
        radius and the one just below it; and a session begun out of reach and stepped back: pass 1 with `none` cached for every query.
    After each, icp_finish must report one iteration and the pose meant (the premise that the update was taken), and the keys must be
    those of the first pass.  That a pass above zero READS the cache, and that the cache holds the last search's positions, is shown
    once, by a search that cannot find the matches itself (test_a_search_after_an_update_starts_from_the_cached_matches);
  * the pass record over all queries within the bound of tests/icp_search_harness.py, and in the tie case the record of each query
    alone against the record each of its tied points would give: the winner's normal enters every term, which names the original index
    where d2 cannot -- under every one of the bounds above;
  * the bound formed from the candidate sets exists in the fused kernel only, which computes its own updates: radius_still_case is a
    registration whose every update is the identity, held to the brute force's count and rmse, its counters showing a set per query;
  * pose, fitness, rmse, iterations and correspondence count of three iterations (fused kernel, candidate sets on) equal the parent's
    bits.  The inputs register from the identity with free normals, so the updates jump: passes 1 and 2 start from bounds gone stale;
  * the library's per-launch counters of those registrations (O3DS_ICP_STATS: verified / searched / sets left / far queries per pass),
    read in a child process, equal the parent's lines: a candidate listed twice or not at all changes a `k` or, a pass later, a `v`.
The array-end case is built in a block the pool has just taken back from a larger cloud whose points lie nearer to every query than any
target point (tests/test_icp_scan_loop_cpu.py: same pool class, stale points nearer): no query may match a point from behind the end.

Recording (parent commit's library only):
    O3DS_BACKEND_LIB=<A/B library built from the parent commit> python tests/test_icp_scan_loop_gpu.py --record FILE"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (run as a script to record: the package)
import icp_scan_loop_cases as sc  # noqa: E402
import icp_search_harness as harness  # noqa: E402
import icp_search_restatement as rs  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_scan_loop_parent.npz")
PATHS = harness.PATHS
FIXED = dict(max_iter=3, rel_fitness=0.0, rel_rmse=0.0)
PREC = harness.PREC


@functools.lru_cache(maxsize=None)
def _cases():
    return {c.name: c for c in sc.all_cases()}


@functools.lru_cache(maxsize=None)
def _ref(name, storage):
    c = _cases()[name]
    return rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)


def _ids():
    return [(c.name, s) for c in sc.all_cases() for s in c.storages]


def _open(be, c):
    """the session of a case on a handle.  array-end: behind a larger cloud around the queries (harness.open_behind_stale, whose session is
    closed without an icp_finish: the calls the parent's record was made with)"""
    if c.name == "array-end":
        return harness.open_behind_stale(be, c, sc.array_end_case()[1], finish=False)
    return harness.Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)


def _registrations(storage):
    """{case|storage|path: (floats, ints)} of every case of a storage, in the order of sc.all_cases() x PATHS, on a handle of its own"""
    os.environ["O3DS_NN_REPLICA_AFTER"] = "1"
    out = {}
    be = backend.Backend(0, PREC[storage], ab=True)
    try:
        for c in sc.all_cases():
            if storage not in c.storages:
                continue
            ses = _open(be, c)
            for path in PATHS:
                harness.set_path(path)
                ses.begin(c.T, path)
                out[f"{c.name}|{storage}|{path}"] = harness.pack(ses.be.icp_point_to_plane_dev(ses.s, ses.t, c.r, init=c.T, **FIXED))
            ses.close()
    finally:
        be.close()
    return out


def _child(call):
    """a call of this module that returns registrations, such as "_registrations('f32')", in a child process with O3DS_ICP_STATS=1
    (looked at once per process): (results, the stats lines in order)"""
    return harness.child_with_stats("test_icp_scan_loop_gpu", f"t.{call}", unset=("O3DS_ICP_SETS", "O3DS_DEBUG_ACC"))


@pytest.fixture(autouse=True)
def _eager_replica(monkeypatch):
    harness.eager_replica(monkeypatch, replica="replica", clear=("O3DS_DEBUG_ACC", "O3DS_ICP_SETS"))


@pytest.fixture(scope="module")
def ab():
    yield from harness.backends(True)


@pytest.fixture(scope="module")
def golden():
    return harness.load_parent_record(GOLDEN)


def _golden_names():
    return sorted(f"{n}|{s}|{p}" for n, s in _ids() for p in PATHS)


def test_golden_file_lists_exactly_the_cases(golden):
    assert sorted(golden[0]) == _golden_names()
    for s in rs.STORAGES:
        assert len(golden[1][s]) == sum(1 for k in golden[0] if f"|{s}|" in k), "one line of counters per recorded registration"


def _check_tie_winners(ses, c, m, storage, what):
    """which of a query's equidistant points won, one query at a time: d2 cannot tell them apart, the record can -- the winner's normal
    (random, a different one per point) enters every term.  The record of query q alone is held against the restatement's record for
    EACH of its island's points as the winner: it must lie a thousand times nearer to the one of the smallest original index than to
    any other (the distance of two such records is of the order of the record; rounding, cancellation in p x n included, is of the
    order of 1e-12 of it -- no sharp bound is needed, and none is claimed)."""
    owner = sc.ties_case()[1]
    for q in range(len(c.src)):
        got = ses.record(q, 1).cpu().numpy()
        mine = np.flatnonzero(owner == q)
        assert m.idx[q] == mine.min()
        dist = {}
        for t in mine:
            idx = np.full_like(m.idx, -1)
            idx[q] = t
            ref, _ = rs.record(m.p, c.tgt, c.nrm, idx, storage, backend.ICP_POINT_TO_PLANE)
            dist[int(t)] = float(np.abs(got - ref)[:27].max())
        win = dist.pop(int(mine.min()))
        print(f"SCAN {what} query {q}: |record - winner's| {win:.3e}, nearest other point's {min(dist.values()):.3e}")
        assert got[28] == 1.0 and win * 1000.0 < min(dist.values()), f"{what} query {q}: the record is not that of the smallest index: {win} {dist}"


def _update(ses, record):
    """one o3ds_icp_update of the session with a hand-written record (sc.ZERO_RECORD, sc.step_back_record): the pass count goes up, the
    pose moves by the step the record states"""
    import torch

    rec = torch.from_numpy(np.ascontiguousarray(record, np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    ses.be.icp_update(rec.data_ptr(), ses.n)
    ses.be.synchronize()


def _finish_after_one_update(ses, T, what):
    """ends the session: exactly one update was taken (icp_step_block counts the pass where it counts the iteration) and it left the pose T"""
    res = ses.be.icp_finish()
    assert res["iterations"] == 1, f"{what}: premise: the update was not taken, the searches after it ran as a first pass"
    assert np.array_equal(res["transformation"], T), f"{what}: premise: the pose after the hand-written update\n{res['transformation']}"


@functools.lru_cache(maxsize=None)
def _ref_start(name, storage, start):
    c = _cases()[name]
    return rs.nearest_within(c.src, c.tgt, sc.translation(sc.STARTS[start]), c.r, storage)


@pytest.mark.parametrize("name,storage", _ids())
def test_scan_loop_per_query_and_the_parents_registration(ab, golden, monkeypatch, name, storage):
    import torch

    c, m = _cases()[name], _ref(name, storage)
    n_src = len(c.src)
    ses = _open(ab[storage], c)
    try:
        for path in PATHS:
            what = f"{name} {storage} {path}"
            harness.set_path(path, monkeypatch)
            ses.begin(c.T, path)
            first = ses.keys(rank=3)
            harness.check_keys(first, m, storage, c.exact, 3, len(c.tgt), 0, n_src, f"{what} first search")
            harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, n_src, f"{what} first pass")
            if name == "ties":
                _check_tie_winners(ses, c, m, storage, f"{what} first pass")
            # ---- pass 1 at the same pose: every query starts from what the first search cached for it, its match or `none`
            _update(ses, sc.ZERO_RECORD)
            again = ses.keys(rank=3)
            harness.check_keys(again, m, storage, c.exact, 3, len(c.tgt), 0, n_src, f"{what} from its own cached matches")
            assert torch.equal(first, again), f"{what}: the search from the cached bound finds other keys"
            harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, n_src, f"{what} from its own cached matches")
            if name == "ties":
                _check_tie_winners(ses, c, m, storage, f"{what} from its own cached matches")
            _finish_after_one_update(ses, c.T, what)
            # ---- pass 1 at the identity from the cache of a pass 0 elsewhere: stale matches (one cell aside), `none` (out of reach)
            for start in sc.STARTS if c.exact else ():
                ms, at = _ref_start(name, storage, start), f"{what} start `{start}`"
                assert (c.T == np.eye(4)).all() and ((ms.idx != m.idx).any() if start == "stale" else (ms.idx == -1).all()), at
                ses.begin(sc.translation(sc.STARTS[start]), path)
                harness.check_keys(ses.keys(rank=3), ms, storage, True, 3, len(c.tgt), 0, n_src, f"{at}, first search")
                _update(ses, sc.step_back_record(sc.STARTS[start]))
                back = ses.keys(rank=3)
                harness.check_keys(back, m, storage, True, 3, len(c.tgt), 0, n_src, f"{at}, back at the identity")
                assert torch.equal(first, back), f"{at}: the search from this bound finds other keys"
                harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, n_src, at)
                if name == "ties":
                    _check_tie_winners(ses, c, m, storage, at)
                _finish_after_one_update(ses, np.eye(4), at)
            ses.begin(c.T, path)
            got = ses.be.icp_point_to_plane_dev(ses.s, ses.t, c.r, init=c.T, **FIXED)
            print(f"SCAN {what}: iterations {got['iterations']} n_corr {got['n_corr']} fitness {got['fitness']} rmse {got['inlier_rmse']}")
            f, i = harness.pack(got)
            gf, gi = golden[0][f"{name}|{storage}|{path}"]
            assert np.array_equal(i, gi), (what, i, gi)
            harness.assert_bits(f, gf, what)
    finally:
        ses.close()


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_a_search_after_an_update_starts_from_the_cached_matches(ab, monkeypatch, storage):
    """The premise of the later-pass checks above, shown by a search that cannot find the matches itself.  O3DS_DEBUG_ACC=16 (A/B
    library, read when a session begins) skips stage 3, and every match of the half-rows case lies three rows away: a first pass finds
    none.  After a full search of an ordinary session on the same handle (the handle's match cache outlives a session), a session with
    stage 3 skipped that takes one identity update and THEN searches returns that search's keys, positions included: pass > 0 reads the
    cache, and the cache holds the positions the last search found."""
    import torch

    c, m = _cases()["half-rows"], _ref("half-rows", storage)
    n_src = len(c.src)
    ses = _open(ab[storage], c)
    try:
        for path in PATHS:
            what = f"cache premise {storage} {path}"
            harness.set_path(path, monkeypatch)
            ses.begin(c.T, path)
            full = ses.keys(rank=3)
            harness.check_keys(full, m, storage, True, 3, len(c.tgt), 0, n_src, what)
            assert (m.idx >= 0).all()
            ses.be.icp_finish()
            monkeypatch.setenv("O3DS_DEBUG_ACC", "16")
            ses.begin(c.T, path)
            _update(ses, sc.ZERO_RECORD)
            cached = ses.keys(rank=3)
            ses.begin(c.T, path)
            blind = ses.keys(rank=3)  # (a first pass again: this one overwrites the cache with what it finds)
            monkeypatch.delenv("O3DS_DEBUG_ACC")
            assert rs.decode_keys(blind.cpu().numpy()[:n_src])[0].all(), f"{what}: without stage 3 a first pass finds a match: the case proves nothing"
            assert torch.equal(cached, full), f"{what}: the search of pass 1 did not start from the matches the last search cached"
            ses.be.icp_finish()
    finally:
        monkeypatch.delenv("O3DS_DEBUG_ACC", raising=False)
        ses.close()


def _still_registrations():
    """{case|path: (floats, ints)} of the fused kernel's radius cases (both storages), each on a handle of its own"""
    os.environ["O3DS_NN_REPLICA_AFTER"] = "1"
    out = {}
    for storage in rs.STORAGES:
        c = sc.radius_still_case(storage)[0]
        be = backend.Backend(0, PREC[storage], ab=True)
        try:
            ses = harness.Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)
            for path in PATHS:
                harness.set_path(path)
                ses.begin(c.T, path)
                out[f"{c.name}|{path}"] = harness.pack(be.icp_point_to_plane_dev(ses.s, ses.t, c.r, init=c.T, **FIXED))
            ses.close()
        finally:
            be.close()
    return out


def test_the_radius_under_a_bound_from_the_candidate_sets():
    """sc.radius_still_case through the fused kernel, three iterations: every update is the identity (asserted: the pose comes back as
    the identity), so passes 1 to 3 search where pass 0 did.  Pass 1 leaves a candidate set for every query (its counters say so: the
    O3DS_ICP_STATS line, read in a child process) and the sets of islands 0 and 3 hold the points ON the radius; passes 2 and 3 form
    their bound from the listed points.  The result is the brute force's: 2 + STILL_FILL correspondences of 4 + STILL_FILL queries -- a
    point at d2 == r^2 taken from a set, or the point one below r^2 dropped, changes the count -- and the rmse of exactly those."""
    res, lines = _child("_still_registrations()")
    assert list(res) == [f"radius-still-{s}|{p}" for s in rs.STORAGES for p in PATHS] and len(lines) == len(res)
    for (k, (f, i)), ln in zip(res.items(), lines):
        print(f"SCAN {k}: {ln}; iterations {i[0]} n_corr {i[1]} fitness {f[16]} rmse {f[17]}")
        storage = rs.F32 if "f32" in k else rs.F64
        c = sc.radius_still_case(storage)[0]
        m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
        n = len(c.src)
        passes = harness.parse_stats(ln)
        assert len(passes) >= 4 and passes[0]["k"] == 0 and passes[1]["k"] == n, f"{k}: premise: pass 1 leaves a candidate set per query: {ln}"
        assert all(p["v"] + p["s"] == n for p in passes[:4]), ln
        assert np.array_equal(f[:16].reshape(4, 4), np.eye(4)), f"{k}: premise: the pose moved\n{f[:16].reshape(4, 4)}"
        hit = m.idx >= 0
        assert i.tolist() == [3, int(hit.sum())] and f[16] == hit.sum() / n, (k, i, f[16:])
        mean = m.d2[hit].sum() / hit.sum()
        bound = rs.D2_F32_REL if storage == rs.F32 else 2.0 ** -23
        assert abs(f[17] ** 2 - mean) <= bound * mean, (k, f[17], np.sqrt(mean))


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_counters_and_registrations_of_a_fresh_process_equal_the_parents(golden, storage):
    """every registration of the storage in a child process: the parent's bits, and the parent's per-launch counters line for line"""
    res, lines = _child(f"_registrations({storage!r})")
    for ln in lines:
        print(f"SCAN {storage}: {ln}")
    names = [k for k in res]
    assert names == [f"{c.name}|{storage}|{p}" for c in sc.all_cases() if storage in c.storages for p in PATHS]
    for k, (f, i) in res.items():
        gf, gi = golden[0][k]
        assert np.array_equal(i, gi), (k, i, gi)
        harness.assert_bits(f, gf, k)
    # (the array-end case's preparation registers nothing through the fused kernel: one line per registration above)
    assert lines == golden[1][storage], [(a, b) for a, b in zip(lines, golden[1][storage]) if a != b]
    assert any(" k" in ln and any(int(t[1:]) > 0 for t in ln.replace("]", "").split() if t.startswith("k")) for ln in lines), \
        "premise: some pass of some registration left candidate sets"


# ---- recording (parent commit's library only) -----------------------------------------------------------------------------------------
if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or not os.environ.get("O3DS_BACKEND_LIB"):
        sys.exit("usage: O3DS_BACKEND_LIB=<A/B library built from the PARENT commit> python tests/test_icp_scan_loop_gpu.py --record FILE")
    import torch  # noqa: F401  (before the backend library is loaded: see tests/conftest.py)

    names, floats, ints, stats = [], [], [], {}
    for storage_ in rs.STORAGES:
        res_, stats[storage_] = _child(f"_registrations({storage_!r})")
        for k_, (f_, i_) in res_.items():
            names.append(k_), floats.append(f_), ints.append(i_)
            print(k_, i_.tolist(), f_[16:].tolist(), flush=True)
        for ln_ in stats[storage_]:
            print(storage_, ln_, flush=True)
        assert len(stats[storage_]) == len(res_)
    np.savez(sys.argv[2], names=np.array(names), floats=np.array(floats, np.float64), ints=np.array(ints, np.int64),
             **{f"stats_{s}": np.array(v) for s, v in stats.items()})
    print("recorded", len(names), "cases")
