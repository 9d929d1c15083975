"""What the GPU tests of the ICP neighbour search share: a session of one case on a handle, the checks of its per-query keys and of its
pass record against the brute force of tests/icp_search_restatement.py, and the plumbing of the comparisons with a record made by the
parent commit's library (the A/B handles, the environment, the stale cloud parked in the pool, the packed result, the counters line).
A plain module: fixtures stay in the test modules, three lines each around the generators here.

Bounds (derived, not measured; every test prints the largest observed ratio before it asserts):
  * exact cases (coordinates small integers times a power of two, pose the identity or an exact translation): every operation is exact
    in both storages, the float bits of d2 are equal.
  * f32 storage, seeded clouds: |d2_dev - d2_ref| <= 8 * 2^-24 * d2_ref.  dist2 is fmaf(dz, dz, fmaf(dy, dy, dx * dx)): the three
    differences are each within 2^-24 relative of the exact ones (one rounding; exact when the operands are within a factor of two), so
    each SQUARE is within (1 + 2^-24)^2 - 1 < 2.0001 * 2^-24; the product dx * dx and the two fused steps add one rounding each, and as
    all terms are non-negative a relative error of the terms is a relative error of the sum: 2 + 3 = 5 units of 2^-24 to first order,
    under 8 with every higher-order term.  The reference forms d2 in f64 from the same stored coordinates (error 2^-52, nothing).
  * f64 storage: float(d2_ref) within one float ulp of the key's float -- the device's d2 differs from the reference's by a few f64 ulps
    (its own three products and two sums, and the f64 rounding of p = T s, whose multiply-adds the compiler may fuse), so the double-to-
    float cast is the only rounding that can differ, and only by landing on the other side of a rounding boundary.
  * records: |term_dev - term_ref| <= 1e-12 * sum |addends| per term: an addend carries at most about eight f64 roundings (1e-15), the
    workgroup sums add n * 2^-53, the sums across workgroups are exact by design; three orders of margin.  In f32 storage terms [27]
    and [29] take the d2 bound above instead.
The key cannot show WHICH of several equidistant points won; the record can (duplicated target points carry different normals), and it
pins the position -> point -> normal gather with it.
The generalized estimator's record is held to both forms of the restatement (check_record_gicp); REC_TOL for it is derived in the docstring
of tests/test_icp_search_exact_gpu.py, beside the figures observed."""
import contextlib
import os
import re

import numpy as np

import icp_search_restatement as rs
from child_process import run_child

from open3d_slam_amd import backend

SENTINEL = -0x0123456789ABCDEF
PREC = {rs.F32: backend.PRECISION_F32, rs.F64: backend.PRECISION_F64}
PATHS = ("rows", "replica")
REC_TOL = 1e-12
GAP_MIN, NEAR_R_MIN = 1e-5, 1e-6  # the premises of tests/test_icp_search_restatement_cpu.py, asserted here where the pose comes from the device


def backends(ab):
    """the body of a module's `ab` / `shipped` fixture: one handle per storage, of the A/B library (the switches O3DS_NN_REPLICA,
    O3DS_NN_REPLICA_AFTER, O3DS_DEBUG_ACC, ... exist only there) or of the shipped one, closed when the module is done"""
    bes = {s: backend.Backend(0, p, ab=ab) for s, p in PREC.items()}
    yield bes
    for be in bes.values():
        be.close()


def _path(monkeypatch, path):
    monkeypatch.setenv("O3DS_NN_REPLICA", "1" if path == "replica" else "0")


class _ProcessEnvironment:
    """setenv without the undo"""
    setenv = staticmethod(os.environ.__setitem__)


def set_path(path, monkeypatch=None):
    """the row search or the replica for the sessions begun from here on.  Without monkeypatch the environment itself is written:
    for child processes and recording"""
    _path(_ProcessEnvironment if monkeypatch is None else monkeypatch, path)


def eager_replica(monkeypatch, replica=None, clear=("O3DS_DEBUG_ACC",)):
    """the body of a module's autouse environment fixture: a replica from the first registration on, the path `replica` names (None:
    left as it is), and none of the switches `clear` lists"""
    monkeypatch.setenv("O3DS_NN_REPLICA_AFTER", "1")
    if replica is not None:
        set_path(replica, monkeypatch)
    for v in clear:
        monkeypatch.delenv(v, raising=False)


class Session:
    """source and target of one case on a handle, its index built with the case's cell"""

    def __init__(self, be, src, tgt, nrm, r, cell, target_id=None, src_nrm=None):
        self.be, self.r, self.n = be, r, len(src)
        self.s = be.upload(src, src_nrm)
        self.t = be.upload(tgt, nrm) if target_id is None else target_id  # (a target the caller has built keeps the index it has)
        if target_id is None:
            be.build_index(self.t, r, cell)

    def begin(self, T, path=None, crop=None, method=backend.ICP_POINT_TO_PLANE, max_iter=10):
        self.be.icp_begin(self.s, self.t, self.r, init=T, max_iter=max_iter, rel_fitness=0.0, rel_rmse=0.0, target_crop=crop, method=method)
        if path == "replica":
            assert self.be.index_replica(self.t) > 0, "the target has no replica: this run would take the row search"

    @contextlib.contextmanager
    def eps(self, epsilon):
        """the generalized estimator's epsilon for the sessions begun inside (the handles are shared by the module: always put back)"""
        try:
            self.be.set_gicp_epsilon(epsilon)
            yield
        finally:
            self.be.set_gicp_epsilon(rs.GICP_EPSILON)

    def keys(self, first=0, count=None, rank=0):
        import torch

        count = self.n - first if count is None else count
        k = torch.full((max(self.n, 1),), SENTINEL, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        self.be.icp_nn_keys(first, count, rank, k.data_ptr())
        self.be.synchronize()
        return k

    def record(self, first=0, count=None, keys=None, rank=0):
        import torch

        count = self.n - first if count is None else count
        rec = torch.full((32,), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        if keys is None:
            self.be.icp_accumulate(first, count, rec.data_ptr())
        else:
            self.be.icp_accumulate_keys(first, count, rank, keys.data_ptr(), rec.data_ptr())
        self.be.synchronize()
        return rec

    def close(self):
        self.be.free(self.s)
        self.be.free(self.t)


def open_behind_stale(be, c, stale, finish):
    """the session of case c in blocks a cloud of nearer points has just left: the stale cloud is uploaded, indexed, registered against
    once (which builds its replica) and freed, so that the pool holds its blocks when the target asks for its own
    (tests/test_icp_scan_loop_cpu.py: same pool class).  finish: end the stale session with icp_finish before it is closed.  The block
    the target then gets, and with it the bits of the parent records, follow the order of the calls, so each caller keeps its own."""
    pre = Session(be, c.src, stale, rs.unit_normals(np.random.default_rng(1), len(stale)), c.r, c.cell)
    pre.begin(c.T, "replica")
    pre.keys()
    if finish:
        pre.be.icp_finish()
    pre.close()
    return Session(be, c.src, c.tgt, c.nrm, c.r, c.cell)


def check_keys(keys, m, storage, exact, rank, n_tgt, first, count, what):
    """the keys of queries [first, first + count) against the brute-force matches m (of ALL queries); returns the largest d2 deviation
    as a fraction of its bound"""
    k = keys.cpu().numpy()[:len(m.idx)]
    outside = np.ones(len(k), dtype=bool)
    outside[first:first + count] = False
    assert (k[outside] == SENTINEL).all(), f"{what}: keys outside the range were written"
    sel = slice(first, first + count)
    none, d2, rk, pos = rs.decode_keys(k[sel])
    want_none = m.idx[sel] < 0
    bad = np.flatnonzero(none != want_none)
    assert bad.size == 0, f"{what}: {bad.size} of {count} queries differ in match / no match, first {first + bad[:8]}, reference d {np.sqrt(m.best[sel][bad[:8]])}"
    hit = ~none
    assert (rk[hit] == rank).all(), f"{what}: rank not echoed"
    if n_tgt is not None:
        assert (pos[hit] < n_tgt).all(), f"{what}: position beyond the target"
    ref = m.d2[sel][hit]
    dev = d2[hit].astype(np.float64)
    if exact:
        np.testing.assert_array_equal(d2[hit].view(np.uint32), ref.astype(np.float32).view(np.uint32), err_msg=f"{what}: float bits of d2")
        return 0.0
    if not hit.any():
        return 0.0
    if storage == rs.F32:
        ratio = np.abs(dev - ref) / (rs.D2_F32_REL * ref)
    else:
        ratio = np.abs(dev - ref.astype(np.float32).astype(np.float64)) / rs.ulp32(ref)
    worst = float(ratio.max())
    print(f"SEARCH {what}: d2 deviation / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: d2 off by {worst:.3f} x its bound at query {first + np.flatnonzero(hit)[ratio.argmax()]}"
    return worst


def check_record(rec, m, tgt, nrm, storage, method, first, count, what):
    got = rec.cpu().numpy()
    idx = np.full_like(m.idx, -1)
    idx[first:first + count] = m.idx[first:first + count]
    ref, scale = rs.record(m.p, tgt, nrm, idx, storage, method)
    tol = np.full(32, REC_TOL)
    if storage == rs.F32:
        tol[[27, 29]] = rs.D2_F32_REL
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(scale > 0, np.abs(got - ref) / (tol * scale), np.where(got == ref, 0.0, np.inf))
    worst = float(ratio.max())
    print(f"SEARCH {what}: record deviation / bound {worst:.3e} (term {int(ratio.argmax())}), {int(ref[28])} matches of {count}")
    assert got[28] == ref[28], f"{what}: {got[28]} correspondences, brute force {ref[28]}"
    assert worst <= 1.0, f"{what}: record term {int(ratio.argmax())} off by {worst:.3e} x its bound: {got[ratio.argmax()]} vs {ref[ratio.argmax()]}"
    return worst


def check_record_gicp(rec, m, tgt, nrm, src_nrm, storage, T, eps, first, count, what, defect=None):
    """the generalized record of queries [first, first + count) against both forms of the restatement; returns the largest deviation
    as a fraction of its bound (of both comparisons).  defect: the DEFECT of a set of pairs that contains these (default: of these)."""
    got = rec.cpu().numpy() if hasattr(rec, "cpu") else np.asarray(rec)
    idx = np.full_like(m.idx, -1)
    idx[first:first + count] = m.idx[first:first + count]
    if defect is None:
        defect = rs.gicp_defect(nrm, src_nrm, idx, T, eps, storage)
    worst = 0.0
    for form, extra in ((rs.FORM_O3D, 2.0 * defect), (rs.FORM_CLOSED, 0.0)):
        ref, scale = rs.record_gicp(m.p, tgt, nrm, src_nrm, idx, T, eps, storage, form)
        tol = np.full(32, REC_TOL + extra)
        if storage == rs.F32:
            tol[29] = rs.D2_F32_REL
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(scale > 0, np.abs(got - ref) / (tol * scale), np.where(got == ref, 0.0, np.inf))
        w = float(ratio.max())
        print(f"SEARCH {what}: generalized record against the {form} form, deviation / bound {w:.3e} (term {int(ratio.argmax())}), "
              f"{int(ref[28])} matches of {count}, DEFECT {defect:.3e}")
        assert got[28] == ref[28], f"{what}: {got[28]} correspondences, brute force {ref[28]}"
        assert w <= 1.0, f"{what}: {form} form, record term {int(ratio.argmax())} off by {w:.3e} x its bound: {got[ratio.argmax()]} vs {ref[ratio.argmax()]}"
        worst = max(worst, w)
    return worst


def premises(m, r, what):
    hit = m.idx >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = m.gap[hit] / m.d2[hit]
    assert rel.size == 0 or rel.min() >= GAP_MIN, f"{what}: premise: relative gap {rel.min():.3e}"
    fin = np.isfinite(m.best)
    near = np.abs(np.sqrt(m.best[fin]) - r) / r
    assert near.size == 0 or near.min() >= NEAR_R_MIN, f"{what}: premise: |d - r| / r = {near.min():.3e}"


# ---- comparisons with a record of the parent commit's library ---------------------------------------------------------------------------
def pack(r):
    """a registration result as the records hold it: (16 pose doubles, fitness, rmse), (iterations, correspondences)"""
    f = np.concatenate([np.ascontiguousarray(r["transformation"], np.float64).reshape(16), [r["fitness"], r["inlier_rmse"]]])
    return f.astype(np.float64), np.array([r["iterations"], r["n_corr"]], np.int64)


def assert_bits(got, want, what):
    """two arrays of doubles are the same bits"""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got, want)


def load_parent_record(path):
    """a record of the layout {names, floats, ints[, stats_<storage>]}: ({name: (floats, ints)}, {storage: [counters lines]})"""
    g = np.load(path)
    records = {str(n): (g["floats"][k], g["ints"][k]) for k, n in enumerate(g["names"])}
    return records, {f[len("stats_"):]: [str(x) for x in g[f]] for f in g.files if f.startswith("stats_")}


_STATS_PASS = re.compile(r"\[(\d+) v(\d+) s(\d+) k(\d+) f(\d+)\]")


def parse_stats(line):
    """the per-launch counters of one registration (an `icp stats` line of O3DS_ICP_STATS=1): per pass, in order, {v: matches verified
    inside their candidate sets, s: searches, k: sets left by searches, f: far queries}"""
    found = _STATS_PASS.findall(line)
    assert [int(p[0]) for p in found] == list(range(line.count("["))), f"not one well-formed group per pass: {line}"
    return [dict(zip("vskf", map(int, p[1:]))) for p in found]


def child_with_stats(module, expr, unset=()):
    """`expr` over test module `module` in a child process with O3DS_ICP_STATS=1 (looked at once per process) and without the variables
    of `unset`: (its value, its `icp stats` lines in order)"""
    value, err = run_child(module, expr, env={"O3DS_ICP_STATS": "1"}, unset=unset, timeout=300)
    return value, [ln.strip() for ln in err.splitlines() if ln.startswith("icp stats")]
