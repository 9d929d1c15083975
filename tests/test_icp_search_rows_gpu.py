"""The row geometry of the ICP search's shell and far stages on the device (needs an MI355X): the inputs of
tests/icp_search_rows_cases.py, per query against the brute force of tests/icp_search_restatement.py, and a three-iteration registration
of each against a record made with the PARENT commit's library (tests/golden/icp_search_rows_parent.npz; the commit is named in
profiles/search_rows.txt).

What is held, per case, f32 and f64 storage, row search and replica (the replica serves stage 1 only: stages 2 and 3 are the same code):
  * o3ds_icp_nn_keys per query: match or none as the brute force says; d2 within the bounds of tests/icp_search_harness.py (equal
    float bits in the exact case) -- islands hold one point within r, so d2 names the point;
  * the pass record over all queries within that file's bound: the winner's normal enters every term, which pins the original index;
    in the tie case per query, where d2 cannot tell the two candidates apart;
  * pose, fitness, rmse, iterations and correspondence count of three iterations (fused kernel, candidate sets on): the parent's bits.
The candidate sets themselves have no accessor in the ABI; what the far stage listed is held through what the next pass does with it:
the `lists-far` registration starts millimetres from the truth, so that its pass 1 lists (its far queries among them: asserted from the
library's per-launch counters) and its passes 2 and 3 verify their matches inside those sets; it must equal the parent's bits, and the
same registration with O3DS_ICP_SETS=0 (every pass searches).  The island inputs register from the identity with normals across the
line from point to query: their updates are rounding residue, so passes 1 to 3 run with the lists on as well and find the matches of
pass 0 again -- the recorded correspondence count, fitness and rmse say so.

Recording (parent commit's library only):
    O3DS_BACKEND_LIB=<A/B library built from the parent commit> python tests/test_icp_search_rows_gpu.py --record FILE"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (run as a script to record: the package)
import icp_search_harness as harness  # noqa: E402
import icp_search_restatement as rs  # noqa: E402
import icp_search_rows_cases as rc  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_search_rows_parent.npz")
PATHS = harness.PATHS
FIXED = dict(max_iter=3, rel_fitness=0.0, rel_rmse=0.0)


@functools.lru_cache(maxsize=None)
def _cases():
    return {c.name: c for c in rc.all_cases()}


@functools.lru_cache(maxsize=None)
def _ref(name, storage):
    c = _cases()[name]
    return rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)


def _names():
    return [c.name for c in rc.all_cases()]


def _register(ses, c):
    return ses.be.icp_point_to_plane_dev(ses.s, ses.t, c.r, init=c.T, **FIXED)


def _registration_session(be, c, ses):
    """the session the registration of a case runs in: the case's own, or one whose target carries rc.registration_normals"""
    nrm = rc.registration_normals(c)
    return ses if nrm is c.nrm else harness.Session(be, c.src, c.tgt, nrm, c.r, c.cell)


@pytest.fixture(autouse=True)
def _eager_replica(monkeypatch):
    harness.eager_replica(monkeypatch, clear=("O3DS_DEBUG_ACC", "O3DS_ICP_SETS"))


@pytest.fixture(scope="module")
def ab():
    yield from harness.backends(True)


@pytest.fixture(scope="module")
def golden():
    return harness.load_parent_record(GOLDEN)[0]


def test_golden_file_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(f"{n}|{s}|{p}" for n in _names() for s in rs.STORAGES for p in PATHS)


@pytest.mark.parametrize("storage", rs.STORAGES)
@pytest.mark.parametrize("name", _names())
def test_rows_per_query_and_the_parents_registration(ab, golden, monkeypatch, name, storage):
    c, m = _cases()[name], _ref(name, storage)
    ses = harness.Session(ab[storage], c.src, c.tgt, c.nrm, c.r, c.cell)
    reg = _registration_session(ab[storage], c, ses)
    try:
        for path in PATHS:
            what = f"{name} {storage} {path}"
            harness.set_path(path, monkeypatch)
            ses.begin(c.T, path)
            harness.check_keys(ses.keys(rank=3), m, storage, c.exact, 3, len(c.tgt), 0, len(c.src), what)
            harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, len(c.src), what)
            if name == "ties":  # which of the two won: one query at a time (the winner's normal is in every term)
                assert (m.idx == np.array([min(1 + 2 * i, 2 + 2 * i) for i in range(len(c.src))])).all(), "premise: the first of each pair"
                for q in range(len(c.src)):
                    harness.check_record(ses.record(q, 1), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, q, 1, f"{what} query {q}")
            reg.begin(c.T, path)
            got = _register(reg, c)
            print(f"ROWS {what}: iterations {got['iterations']} n_corr {got['n_corr']} fitness {got['fitness']} rmse {got['inlier_rmse']}")
            f, i = harness.pack(got)
            gf, gi = golden[f"{name}|{storage}|{path}"]
            assert np.array_equal(i, gi), (what, i, gi)
            harness.assert_bits(f, gf, what)
    finally:
        ses.close()
        if reg is not ses:
            reg.close()


def _lists_registration(storage):
    """the `lists-far` registration on a handle of its own (replica on, the set policy of the environment)"""
    c = _cases()["lists-far"]
    be = backend.Backend(0, harness.PREC[storage], ab=True)
    try:
        ses = harness.Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)
        out = harness.pack(_register(ses, c))
        ses.close()
    finally:
        be.close()
    return out


@pytest.mark.parametrize("storage", rs.STORAGES)
def test_sets_listed_by_the_far_stage_serve_the_next_passes(golden, monkeypatch, storage):
    """`lists-far` starts millimetres from the truth, so its updates are millimetres and its passes after the first search with the lists
    on (default policy: a query lists when twice the motion of its point under the last update is at most 4 cm), hundreds of their
    queries in the far stage; the passes after them verify their matches inside what was listed.  That this is what happens is read
    from the library's per-launch counters (O3DS_ICP_STATS is looked at once per process: a child process), not supposed.  Per pass j
    they count v_j verified matches, s_j searches, k_j sets left by searches and f_j far queries.  Pass 0 follows no update: it
    searches and lists nothing.  For a pass j >= 1:
      * at most s_j - f_j searches stayed outside the far stage, so at least  k_j - (s_j - f_j)  SETS WERE LEFT BY FAR QUERIES;
      * a match verified in pass j + 1 lies in a set carried through pass j (at most v_j of them) or in one pass j left, so at least
        v_{j+1} - v_j - (s_j - f_j)  MATCHES OF PASS j + 1 WERE VERIFIED INSIDE SETS THE FAR STAGE OF PASS j LISTED.
    Both must reach 100 for one j of 1, 2 (the brute force finds 300 matches more than three cells away at the start,
    tests/test_icp_search_rows_cpu.py; which pass it is depends on how small update 0 came out, the counters are printed).
    The registration equals the parent's record bit for bit, in the child, in this process, and with O3DS_ICP_SETS=0 (every pass
    searches: a neighbour the lists left out would show).  The listed positions themselves have no accessor in the ABI."""
    c = _cases()["lists-far"]
    monkeypatch.setenv("O3DS_NN_REPLICA", "1")
    child, lines = harness.child_with_stats("test_icp_search_rows_gpu", f"t._lists_registration({storage!r})", unset=("O3DS_ICP_SETS",))
    print(f"ROWS lists-far {storage}: {lines}")
    assert len(lines) == 1, lines
    st = [(p["v"], p["s"], p["k"], p["f"]) for p in harness.parse_stats(lines[0])]
    n = len(c.src)
    assert st[0][:3] == (0, n, 0), "pass 0 follows no update: it searches and lists nothing"
    assert all(st[j][0] + st[j][1] == n for j in range(4)), "every query of a pass is verified or searches"
    listed = {j: st[j][2] - (st[j][1] - st[j][3]) for j in (1, 2)}
    served = {j: st[j + 1][0] - st[j][0] - (st[j][1] - st[j][3]) for j in (1, 2)}
    print(f"ROWS lists-far {storage}: sets left by far queries >= {listed}, matches of the next pass verified inside them >= {served}")
    assert any(st[j][3] >= 200 and listed[j] >= 100 and served[j] >= 100 for j in (1, 2)), \
        "premise: the far stage of a pass listed at least a hundred sets in which the next pass verified its matches"
    out = {"child": child}
    for sets in ("1", "0"):
        monkeypatch.setenv("O3DS_ICP_SETS", sets)  # (read when the handle is made)
        out[sets] = _lists_registration(storage)
    gf, gi = golden[f"lists-far|{storage}|replica"]
    for which, (f, i) in out.items():
        assert np.array_equal(i, gi), (which, i, gi)
        harness.assert_bits(f, gf, which)
    assert gi[1] >= 1000, "premise: the registration keeps its correspondences"


# ---- recording (parent commit's library only) -----------------------------------------------------------------------------------------
if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or not os.environ.get("O3DS_BACKEND_LIB"):
        sys.exit("usage: O3DS_BACKEND_LIB=<A/B library built from the PARENT commit> python tests/test_icp_search_rows_gpu.py --record FILE")
    import torch  # noqa: F401  (before the backend library is loaded: see tests/conftest.py)

    os.environ["O3DS_NN_REPLICA_AFTER"] = "1"
    names, floats, ints = [], [], []
    for storage, prec in harness.PREC.items():
        be_ = backend.Backend(0, prec, ab=True)
        for c_ in rc.all_cases():
            ses_ = harness.Session(be_, c_.src, c_.tgt, c_.nrm, c_.r, c_.cell)
            reg_ = _registration_session(be_, c_, ses_)
            for path_ in PATHS:
                harness.set_path(path_)
                ses_.begin(c_.T, path_)
                ses_.keys(rank=3), ses_.record()  # (the same calls in the same order as the test)
                reg_.begin(c_.T, path_)
                res = _register(reg_, c_)
                f_, i_ = harness.pack(res)
                names.append(f"{c_.name}|{storage}|{path_}"), floats.append(f_), ints.append(i_)
                print(names[-1], res["iterations"], res["n_corr"], res["fitness"], res["inlier_rmse"], flush=True)
            ses_.close()
            if reg_ is not ses_:
                reg_.close()
        be_.close()
    np.savez(sys.argv[2], names=np.array(names), floats=np.array(floats, np.float64), ints=np.array(ints, np.int64))
    print("recorded", len(names), "cases")
