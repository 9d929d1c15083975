"""The workgroup barriers of a one-pair ICP pass (icp_kernels.hpp: icp_pass_body, icp_step_block, icp_fused_kernel) at tiny sizes.

The fused kernel's instantiation of the pass body (one batch per workgroup) leaves out the three barriers that only the batch loop and
a caller that reuses s_red need, and the far list has LDS words of its own ("The barriers of a pass").  Nothing a pass
computes moved, so every case here is held, bit for bit, to what the library of the PARENT commit produced for the same inputs on an MI355X
(tests/golden/icp_pass_sync_parent.npz; the commit is named in the .txt beside it): pose, fitness, rmse, iterations and correspondence
count of the fused form, the two-launch form (O3DS_ICP_MODE=launch) and, for the 2 048-point scans, the step-wise ABI -- and the
per-launch counters of the fused form (O3DS_ICP_STATS, read in a child process: verified / searched / sets left / far queries per
pass; the `k` column is where a last bit of the candidate-set margin would show).  Inputs are regenerated from seeds and put on a grid
of 2^-20 m, or are lattice islands (tests/icp_scan_loop_cases.py), exact in both storages.

Cases (2 048-point scan against a 20 000-point map unless the name says otherwise):
  * for each of the three estimators x f32 / f64 storage: step_*, max_iter 1, 2, 3, 10, 12 (and point-to-plane under a map crop);
    early_exit_*, an exit by the convergence test with launches queued behind it (go = 0: the update is not applied, the launches
    behind it find the state done); no_correspondence_*, a scan without a correspondence (identity update); straddle_*, a start 3 and
    4 degrees off, whose updates shrink towards the 4 cm cap of the candidate-set margin.  What the counters of that start show is
    asserted per estimator: point-to-plane has a pass in which a part of the searches gets a margin and a part does not
    (0 < k < s = 2048), so its k column depends on the margin's value; the generalized estimator's updates fall from above the cap
    for every query to below it for every query within one iteration (k: 0, 0, 0, 2048); point-to-point is still above the cap for
    every query after its ten iterations (k = 0 throughout) -- its pass with margins on both sides of the cap is in
    early_exit_point_*, which runs 25 iterations (asserted there);
  * partial_*: 1, 127, 128, 129 and 4 099 queries (lanes without a query at every barrier, a last workgroup that is almost empty), and
    count_dev_*: a scan straight out of crop + VoxelDownSample, registered behind a backlog on the stream so that the host has not
    seen its size when the registration is queued (premise, asserted: one of up to three chains on a warmed handle);
  * far_*: 384 islands dealt out by pass 0 so that one workgroup has no far query, one has five and in one all 128 queries are far
    (premise, asserted with a restatement of query_index), as a registration that stands still: pass 1 lists candidates WITH far
    queries, the later passes verify inside those sets.  The fused form is held to the parent's registration bits and counters; per
    query, against the brute force (tests/icp_search_restatement.py), only the keys and the record of pass 0 through the pass kernel
    WITH the batch loop can be read -- the library has no entry point that returns the fused form's matches or candidate sets;
  * steady_*: queries AT map points -- every update is the identity and every pass from the third on verifies all its matches.

Recording (parent commit's library only):
    O3DS_BACKEND_LIB=<A/B library built from the parent commit> python tests/test_icp_pass_sync_gpu.py --record FILE"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (run as a script to record: the package)
if __name__ == "__main__":
    import torch  # noqa: F401  (before the backend library is loaded: see tests/conftest.py)
import icp_scan_loop_cases as sc  # noqa: E402
import icp_search_harness as harness  # noqa: E402
import icp_search_restatement as rs  # noqa: E402
import test_icp_step_gpu as st  # noqa: E402  (its gridded clouds and start pose)

from open3d_slam_amd import backend, synthetic as syn  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_pass_sync_parent.npz")
MODULE = "test_icp_pass_sync_gpu"
FIXED = dict(rel_fitness=0.0, rel_rmse=0.0)
EARLY = dict(max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6)
EARLY_POINT = dict(EARLY, max_iter=120)  # (point-to-point creeps: it needs more iterations to meet the same criteria)
METHODS, PRECISIONS = st.METHODS, st.PRECISIONS
PARTIAL_COUNTS = (1, 127, 128, 129, 4099)
QPB, QPW = 128, 16  # queries per workgroup and per wavefront of a pass (512 threads, four lanes per query)
N_ISLANDS, FEW_FAR = 3 * QPB, 5
CROP = dict(center=(1.0, -2.0, 0.0), rmax=22.0)


# ---- which workgroup serves a query (icp_kernels.hpp: query_index, pass_order) ------------------------------------------------------
def query_index(count, b, ql, order):
    if order == 0:
        return b * QPB + ql
    mul = 1000003
    off, qw = b * (QPB // QPW) + ql // QPW, ql % QPW
    if order == 2:
        n_run = (count + QPW - 1) // QPW
        run = (off * mul) % n_run if n_run % mul else off
        i = run * QPW + qw
        return i if off < n_run and i < count else count
    n_off = (count + QPW - 1) // QPW
    offs = (off * mul) % n_off if n_off % mul else off
    run = qw * n_off + offs
    return run if off < n_off and run < count else count


def workgroup_of(count, order):
    """workgroup of every query in a pass of the given order"""
    out = np.full(count, -1)
    for b in range((count + QPB - 1) // QPB):
        for ql in range(QPB):
            i = query_index(count, b, ql, order)
            if i < count:
                assert out[i] == -1
                out[i] = b
    assert (out >= 0).all()
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_case():
    """(case, far): N_ISLANDS islands on the lattice.  A near island holds one point AT its query.  A far island's nearest point stands
    3 cells straight above the query, three rows up -- beyond the 5x5x5 shell's reach of 2.5 cells, so only stage 3 finds it and no
    bound of a later pass lets stage 2 prove it -- among seven more points of that cell, all higher up; it carries the normal e_x, so
    its residual (p - q) . n is exactly zero as the near islands' are: J^T r = 0 and the registration stands still.  Far are all
    queries of workgroup 2 of pass 0 and FEW_FAR queries of workgroup 1."""
    import icp_lane_exchange_cases as lc

    wg = workgroup_of(N_ISLANDS, 1)
    far = (wg == 2)
    far[np.flatnonzero(wg == 1)[:: QPB // FEW_FAR][:FEW_FAR]] = True
    rng = np.random.default_rng(701)
    c = sc.C
    islands = []
    for i in range(N_ISLANDS):
        if far[i]:
            pts = lc._sixteenths(rng, 8, (0.0, 3.0, 0.0), y_from=9)
            pts[int(rng.integers(8))] = (c, 3.5, c)
            islands.append(((c, c, c), pts))
        else:
            islands.append(((c, c, c), [(c, c, c)]))
    case, owner = sc._assemble("far-mix", islands, True, 702)
    nrm = case.nrm.copy()
    m = rs.nearest_within(case.src, case.tgt, case.T, case.r, rs.F64)
    assert (m.idx >= 0).all() and np.array_equal(owner[m.idx], np.arange(N_ISLANDS))
    nrm[m.idx[far]] = (1.0, 0.0, 0.0)
    return case._replace(nrm=nrm), far


@functools.lru_cache(maxsize=None)
def clouds(name):
    """(src, src_normals or None, tgt, tgt_normals, max_corr, cell or None)"""
    if name in ("main", "far_scan"):
        return st.clouds()[name] + (st.MAX_CORR, None)
    src, sn, tgt, nrm = st.clouds()["main"]
    if name.startswith("first"):  # the first n points of the scan
        n = int(name[5:])
        if n <= len(src):
            return src[:n], sn[:n], tgt, nrm, st.MAX_CORR, None
        wide = st._grid(syn.config2_inputs(n_map=1000, n_az=512)[0], 20)
        assert len(wide) >= n
        return wide[:n], None, tgt, nrm, st.MAX_CORR, None
    if name == "at_map":  # queries AT map points
        pick = np.random.default_rng(703).choice(len(tgt), 2048, replace=False)
        return tgt[pick], None, tgt, nrm, st.MAX_CORR, None
    if name == "far_mix":
        c = far_case()[0]
        return c.src, None, c.tgt, c.nrm, c.r, c.cell
    raise KeyError(name)


def raw_scan():
    """the 131 072-point scan the count_dev cases crop and voxel-filter, f32 on a millimetre grid (2^-10 m: exact in f32 out to 16 km)"""
    raw = syn.os128_scan(syn.make_scene(), syn.make_pose([0.3, 0.2, 0.0], [0.0, 0.0, 2.0]), frame=3)
    return np.ascontiguousarray(st._grid(raw, 10), dtype=np.float32)


def cases():
    """name -> (cloud, estimator, storage, init or None, crop or None, criteria)"""
    out = {}
    for m in METHODS:
        for p in PRECISIONS:
            for it in (1, 2, 3, 10, 12):
                out[f"step_{m}_{p}_iter{it}"] = ("main", m, p, None, None, dict(max_iter=it, **FIXED))
    for p in PRECISIONS:
        out[f"step_crop_plane_{p}"] = ("main", "plane", p, None, CROP, dict(max_iter=10, **FIXED))
        for m in METHODS:
            out[f"early_exit_{m}_{p}"] = ("main", m, p, None, None, EARLY_POINT if m == "point" else EARLY)
            out[f"no_correspondence_{m}_{p}"] = ("far_scan", m, p, None, None, dict(max_iter=3, **FIXED))
            out[f"straddle_{m}_{p}"] = ("main", m, p, st.INIT_C, None, dict(max_iter=10, **FIXED))
        for n in PARTIAL_COUNTS:
            out[f"partial_{n}_point_{p}"] = (f"first{n}", "point", p, None, None, dict(max_iter=3, **FIXED))
        for n in (129, 4099):
            out[f"partial_{n}_plane_{p}"] = (f"first{n}", "plane", p, None, None, dict(max_iter=3, **FIXED))
        out[f"count_dev_plane_{p}"] = ("count_dev", "plane", p, None, None, dict(max_iter=4, **FIXED))
        out[f"far_mix_plane_{p}"] = ("far_mix", "plane", p, None, None, dict(max_iter=10, **FIXED))
        out[f"steady_plane_{p}"] = ("at_map", "plane", p, None, None, dict(max_iter=10, **FIXED))
    return out


def cases_of(storage):
    return [n for n, c in cases().items() if c[2] == storage]


class Rig:
    """clouds on a handle, uploaded once; one registration of a case on it"""

    def __init__(self, be):
        self.be, self.ids = be, {}

    def close(self):
        self.be.close()

    def _ids(self, cloud):
        if cloud not in self.ids:
            src, sn, tgt, nrm, r, cell = clouds(cloud)
            s, t = self.be.upload(src, sn), self.be.upload(tgt, nrm)
            self.be.build_index(t, r) if cell is None else self.be.build_index(t, r, cell)
            self.ids[cloud] = (s, t, len(src), r)
        return self.ids[cloud]

    def _args(self, case):
        cloud, m, p, init, crop, kw = cases()[case]
        crop = None if crop is None else backend.make_crop(backend.CROP_MAX_RADIUS, **crop)
        return cloud, dict(init=init, method=METHODS[m], target_crop=crop, **kw)

    def run(self, case):
        cloud, kw = self._args(case)
        if cloud == "count_dev":
            return self._run_count_dev(kw)
        s, t, _, r = self._ids(cloud)
        self.n_regs = 1
        return self.be.icp_register_dev(s, t, r, **kw)

    def _run_count_dev(self, kw):
        """the head of a crop + VoxelDownSample chain, registered at once behind a backlog on the stream: its size is a bound and a
        device word when the registration is queued.  The first chain on a handle waits here and there (as in
        tests/test_icp_gpu.py), so one is run and dropped; of the three that follow, the first whose size the host had not seen is the
        case's result, and that there is one is asserted (all of them hold the same bits)."""
        be = self.be
        _, t, _, r = self._ids("main")
        if "raw" not in self.ids:
            self.ids["raw"] = (raw_scan(), be.upload(np.random.default_rng(5).uniform(-15.0, 15.0, (4_000_000, 3))))
        raw, big = self.ids["raw"]

        def chain():
            rid = be.upload_f32(raw)
            for _ in range(40):  # (queued, never waited for: what follows cannot have run when the registration is queued)
                be.free(be.transform_cloud(big, np.eye(4)))
            v = be.crop_voxel_down_sample(rid, backend.make_crop(backend.CROP_MAX_RADIUS, rmax=25.0), 0.1)
            be.free(rid)
            lazy = be.size_bound(v)[1] == len(raw)
            out = be.icp_register_dev(v, t, r, **kw)
            n = be.size(v)[0]
            be.free(v)
            return out, n, lazy

        chain()
        runs = []
        while len(runs) < 3 and not (runs and runs[-1][2]):
            runs.append(chain())
        print(f"PASS-SYNC count_dev: {runs[-1][1]} points, size unknown to the host when queued: {[x[2] for x in runs]}")
        assert runs[-1][2], "premise: the host had seen the scan's size before every registration was queued"
        assert runs[-1][1] < len(raw)
        self.n_regs = 1 + len(runs)
        return runs[-1][0]

    def run_stepwise(self, case):
        import torch

        cloud, kw = self._args(case)
        s, t, n, r = self._ids(cloud)
        rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        self.be.icp_begin(s, t, r, **kw)
        for _ in range(kw["max_iter"] + 1):
            self.be.icp_accumulate(0, n, rec.data_ptr())
            self.be.icp_update(rec.data_ptr(), n)
            if self.be.icp_done():
                break
        assert self.be.icp_done()
        return self.be.icp_finish()


def _registrations(storage):
    """({case: (floats, ints)}, registrations each case ran) of a storage's cases, fused form, on a handle of the A/B library (the child
    process: its counters)"""
    rig = Rig(backend.Backend(0, PRECISIONS[storage], ab=True))
    try:
        out, counts = {}, []
        for c in cases_of(storage):
            out[c] = harness.pack(rig.run(c))
            counts.append(rig.n_regs)
        return out, counts
    finally:
        rig.close()


def _child(storage):
    """({case: (floats, ints)}, the counters line of each case's registration -- of its LAST one where a case ran several)"""
    (res, counts), lines = harness.child_with_stats(MODULE, f"t._registrations({storage!r})", unset=("O3DS_ICP_SETS", "O3DS_DEBUG_ACC", "O3DS_ICP_MODE"))
    assert len(lines) == sum(counts), (len(lines), counts)
    return res, [lines[k - 1] for k in np.cumsum(counts)]


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused():
    rigs = {p: Rig(backend.Backend(0, v)) for p, v in PRECISIONS.items()}
    yield rigs
    for r in rigs.values():
        r.close()


@pytest.fixture(scope="module")
def launch():
    mp = pytest.MonkeyPatch()
    mp.setenv("O3DS_ICP_MODE", "launch")
    rigs = {p: Rig(backend.Backend(0, v, ab=True)) for p, v in PRECISIONS.items()}
    mp.undo()  # (the mode is read when the handle is made)
    yield rigs
    for r in rigs.values():
        r.close()


@pytest.fixture(scope="module")
def golden():
    return harness.load_parent_record(GOLDEN)


def test_golden_file_lists_exactly_the_cases(golden):
    records, stats = golden
    assert sorted(records) == sorted(cases())
    assert {s: len(v) for s, v in stats.items()} == {s: len(cases_of(s)) for s in PRECISIONS}


def test_the_far_case_deals_its_far_queries_as_it_says():
    _, far = far_case()
    per_wg = np.bincount(workgroup_of(N_ISLANDS, 1), weights=far, minlength=3).astype(int).tolist()
    assert per_wg == [0, FEW_FAR, QPB], per_wg
    for n in PARTIAL_COUNTS:  # the restatement deals every query exactly once in every order
        for order in (0, 1, 2):
            workgroup_of(n, order)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(cases()))
def test_every_form_equals_the_parent(case, fused, launch, golden):
    cloud, m, p, init, crop, kw = cases()[case]
    want = golden[0][case]
    a = fused[p].run(case)
    print(f"PASS-SYNC {case}: iterations {a['iterations']} n_corr {a['n_corr']} fitness {a['fitness']} rmse {a['inlier_rmse']}")
    harness.assert_bits(harness.pack(a)[0], want[0], (case, "fused against the parent"))
    assert np.array_equal(harness.pack(a)[1], want[1]), (case, harness.pack(a)[1], want[1])
    forms = [("two-launch", launch[p].run(case))]
    if cloud != "count_dev" and clouds(cloud)[0].shape[0] == 2048:
        forms.append(("step-wise", fused[p].run_stepwise(case)))
    for what, b in forms:
        harness.assert_bits(harness.pack(b)[0], want[0], (case, what + " against the parent"))
        assert np.array_equal(harness.pack(b)[1], want[1]), (case, what, harness.pack(b)[1], want[1])
    T = a["transformation"]
    assert np.isfinite(T).all()
    if case.startswith("early_exit"):
        assert a["converged"] and 1 < a["iterations"] < kw["max_iter"]
    if case.startswith("no_correspondence"):
        assert np.array_equal(T, np.eye(4)) and a["n_corr"] == 0 and a["fitness"] == 0.0
    if case.startswith(("far_mix", "steady")):
        assert np.array_equal(T, np.eye(4)), f"{case}: premise: the registration moved\n{T}"
        assert a["n_corr"] == len(clouds(cloud)[0]) and a["iterations"] == kw["max_iter"]
    if case.startswith("partial"):
        assert a["iterations"] == 3 and (a["n_corr"] > 0 or "_1_" in case)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", list(PRECISIONS))
def test_counters_of_every_launch_equal_the_parents(storage, golden):
    res, lines = _child(storage)
    names = cases_of(storage)
    assert list(res) == names and len(lines) == len(names), (len(res), len(lines))
    records, stats = golden
    seen = {}
    for k, ln, want in zip(names, lines, stats[storage]):
        print(f"PASS-SYNC {k}: {ln}")
        harness.assert_bits(res[k][0], records[k][0], (k, "A/B library, fused"))
        assert np.array_equal(res[k][1], records[k][1]), k
        assert ln == want, (k, ln, want)
        seen[k] = harness.parse_stats(ln)
    far = seen[f"far_mix_plane_{storage}"]
    assert far[0] == dict(v=0, s=N_ISLANDS, k=0, f=QPB + FEW_FAR), far[0]
    assert far[1]["f"] > 0 and far[1]["k"] == N_ISLANDS, f"premise: pass 1 lists candidates with far queries: {far[1]}"
    assert all(q == dict(v=N_ISLANDS, s=0, k=0, f=0) for q in far[2:10]), far
    steady = seen[f"steady_plane_{storage}"]
    assert steady[1]["k"] == 2048 and all(q == dict(v=2048, s=0, k=0, f=0) for q in steady[2:10]), steady
    # what the start 3 and 4 degrees off gives, per estimator (see the docstring)
    for name in (f"straddle_plane_{storage}", f"early_exit_point_{storage}"):
        assert any(0 < q["k"] < q["s"] == 2048 for q in seen[name]), f"premise: {name}: no pass with margins on both sides of the cap: {seen[name]}"
    gicp = [q["k"] for q in seen[f"straddle_gicp_{storage}"] if q["s"] == 2048]
    assert gicp == [0, 0, 0, 2048], f"straddle_gicp_{storage}: {gicp}"
    point = seen[f"straddle_point_{storage}"]
    assert all(q["k"] == 0 and q["v"] == 0 for q in point) and all(q["s"] == 2048 for q in point[:11]), f"straddle_point_{storage}: {point}"


@pytest.mark.gpu
@pytest.mark.parametrize("storage", rs.STORAGES)
def test_far_queries_per_query_against_brute_force(storage):
    """pass 0 of the far case through the pass kernel with the batch loop (keys and record): workgroups without, with five and with
    128 far queries in one launch"""
    c, far = far_case()
    m = rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)
    assert (m.idx >= 0).all()
    be = backend.Backend(0, harness.PREC[storage])
    ses = harness.Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)
    try:
        ses.begin(c.T)
        what = f"far-mix {storage}"
        harness.check_keys(ses.keys(rank=3), m, storage, True, 3, len(c.tgt), 0, len(c.src), what)
        harness.check_record(ses.record(), m, c.tgt, c.nrm, storage, backend.ICP_POINT_TO_PLANE, 0, len(c.src), what)
        be.icp_finish()
    finally:
        ses.close()
        be.close()


# ---- recording (parent commit's library only) -----------------------------------------------------------------------------------------
if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or not os.environ.get("O3DS_BACKEND_LIB"):
        sys.exit("usage: O3DS_BACKEND_LIB=<A/B library built from the PARENT commit> python tests/test_icp_pass_sync_gpu.py --record FILE")
    names_, floats_, ints_, out_ = [], [], [], {}
    for storage_ in PRECISIONS:
        res_, lines_ = _child(storage_)
        assert list(res_) == cases_of(storage_) and len(lines_) == len(res_), (len(res_), len(lines_))
        for (k_, (f_, i_)), ln_ in zip(res_.items(), lines_):
            names_.append(k_), floats_.append(f_), ints_.append(i_)
            print(k_, i_.tolist(), f_[16:].tolist(), ln_, flush=True)
        out_["stats_" + storage_] = np.array(lines_)
    np.savez(sys.argv[2], names=np.array(names_), floats=np.array(floats_, np.float64), ints=np.array(ints_, np.int64), **out_)
    print("recorded", len(names_), "cases")
