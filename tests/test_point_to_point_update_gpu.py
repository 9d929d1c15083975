"""The point-to-point update on the device (icp_kernels.hpp umeyama_from_record / svd3_jacobi) against Eigen's form in longdouble
(tests/point_to_point_restatement.py), pair set by pair set, in both storages.

a. Fed records: o3ds_icp_update takes the record from the caller, so every case of the catalogue -- reflections, coplanar, collinear and
   single pairs, equal singular values, slabs either side of the `tiny` switch, half turns -- reaches the one-lane SVD as written.  The
   record is formed the way the pass forms it: relative to the pivot, the multiple of 1024 m nearest to T s_0 (pp.pivot_of).
b. Parity (1e-6 rad and m in f64 storage, 1e-3 in f32) for every case that singles out a rotation and is at least 0.5 m large, the ones
   at (1e5, -2e5, 50) included.  In f32 storage the source stays near the origin and `init` carries the offset.
c. Computed records: the same pair sets as clouds, one iteration through the fused, two-launch and step-wise forms, a one-entry batch
   and a one-target multi registration: bit for bit the same, and the fed result's bits where the record sums are exact.
d. RANSAC hypotheses through the trace of o3ds_ransac_feature_matching, near the origin and at the offset: every hypothesis is held to a
   and b on its own three pairs; repeated and collinear draws (at most 5 %) to the cost assertion.
e. The one-kernel-per-iteration form (o3ds_icp_pass / o3ds_icp_pass_finish) at the offset: a finish with iterations left, the full loop,
   and two ranks of which one holds none of the source.

Measured on an MI355X, angle / (B / K) with K = 140: fed records near the origin at most 27.6 (the 1e-14 slab; below 4 elsewhere), fed
offset cases at most 0.8, computed records at the offset at most 61 (2.7e-8 rad).  Before the record had its pivot the offset patch and
triangle stood 3.1e-5 and 6.1e-5 rad off the reference (fed), 31x and 61x the f64 parity.  DESIGN.md 4.4b."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_ransac_restatement as rs  # noqa: E402
import point_to_point_restatement as pp  # noqa: E402
from open3d_slam_amd import backend  # noqa: E402
from test_icp_step_gpu import _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

STORAGES = {"f32": backend.PRECISION_F32, "f64": backend.PRECISION_F64}
FIXED = dict(rel_fitness=0.0, rel_rmse=0.0)
P2P = backend.ICP_POINT_TO_POINT
CASES = pp.cases()
COMPUTED = [n for n in CASES if CASES[n]["radius"] is not None]
# 256 dummy points on the grid for the sessions that are fed their record; point 0 is what the pivot is taken from
_g = np.arange(256, dtype=np.float64)
DUMMY = np.c_[0.5 + (_g % 8) * 0.25, -1.0 + ((_g // 8) % 8) * 0.25, 0.25 + (_g // 64) * 0.25]


def _stored(a, storage):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if storage == "f32" else a.copy()


def _translation(off):
    T = np.eye(4)
    T[:3, 3] = off
    return T


def _frame(case, storage):
    """(shift of the uploaded source against the case's p, init or None): f64 storage holds the offset cases where they are; f32 storage
    holds the source near the origin and `init` carries it"""
    if case["offset"] is None or storage == "f64":
        return np.zeros(3), None
    return case["offset"], _translation(case["offset"])


def _effective(case, storage):
    """the case as the device holds it: (uploaded source, stored target, init, p = init applied to the source -- exact, a translation of
    grid points by integers --, q)"""
    shift, init = _frame(case, storage)
    src = _stored(case["p"] - shift, storage)
    q = _stored(case["q"], storage)
    return src, q, init, src + shift, q


class Rig:
    def __init__(self):
        self.be = {s: backend.Backend(0, v) for s, v in STORAGES.items()}
        mp = pytest.MonkeyPatch()
        mp.setenv("O3DS_ICP_MODE", "launch")
        self.launch = {s: backend.Backend(0, v, ab=True) for s, v in STORAGES.items()}
        mp.undo()  # (the mode is read when the handle is made)
        self.dummies = {}

    def close(self):
        for be in list(self.be.values()) + list(self.launch.values()):
            be.close()

    def dummy(self, storage, at):
        key = (storage, tuple(at))
        if key not in self.dummies:
            be = self.be[storage]
            s, t = be.upload(DUMMY + at), be.upload(DUMMY + at + [0.0, 0.0, 0.0625])
            be.build_index(t, 1.0)
            self.dummies[key] = (s, t)
        return self.dummies[key]

    def fed(self, storage, p, q, at, init):
        """one update from the record of (p, q), fed to a session on the dummy clouds at `at`: the update U and the record's pivot"""
        import torch

        be = self.be[storage]
        s, t = self.dummy(storage, at)
        T0 = np.eye(4) if init is None else init
        piv = pp.pivot_of(DUMMY[0] + at + T0[:3, 3])
        rec = torch.from_numpy(pp.record_of(p, q, piv)).to("cuda:0")
        torch.cuda.synchronize()
        be.icp_begin(s, t, 1.0, init=init, max_iter=1, method=P2P, **FIXED)
        be.icp_update(rec.data_ptr(), 256)
        be.icp_update(rec.data_ptr(), 256)
        assert be.icp_done()
        got = be.icp_finish()
        assert got["iterations"] == 1 and got["n_corr"] == len(p)
        return got["transformation"], piv

    def computed(self, storage, src, tgt, radius, init):
        """max_iter = 1 through the five forms: name -> result"""
        import torch

        out = {}
        kw = dict(init=init, max_iter=1, method=P2P, **FIXED)
        for name, be in (("fused", self.be[storage]), ("two-launch", self.launch[storage])):
            s, t = be.upload(src), be.upload(tgt)
            be.build_index(t, radius)
            out[name] = be.icp_register_dev(s, t, radius, **kw)
            if name == "fused":
                rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
                torch.cuda.synchronize()
                be.icp_begin(s, t, radius, **kw)
                for _ in range(2):
                    be.icp_accumulate(0, len(src), rec.data_ptr())
                    be.icp_update(rec.data_ptr(), len(src))
                assert be.icp_done()
                out["step-wise"] = be.icp_finish()
                params = be._params(radius, 1, 0.0, 0.0, P2P)
                res, status = be.icp_register_batch([(s, t, None, init)], params)
                assert status == [0]
                out["batch"] = res[0]
                out["multi"] = be.icp_register_multi(s, [t], form=0, init=init, params=params)
            be.free(s)
            be.free(t)
        return out


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def refs():
    return {}


def _ref(refs, key, p, q):
    if key not in refs:
        refs[key] = pp.umeyama_reference(p, q)
    return refs[key]


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("name", list(CASES))
def test_fed_record(name, storage, rig, refs):
    """a and b.  The fed record is that of the case's exact pairs whatever the storage (the record is f64 either way); the storage decides
    where the dummy source lies and what `init` carries, hence the pivot.  With `init` carrying the offset the assertions hold the
    registration's result T = U init as the pose that maps the near-origin source onto q: nothing is inverted."""
    case = CASES[name]
    shift, init = _frame(case, storage)
    at = np.zeros(3) if case["offset"] is None or init is not None else case["offset"]
    T, piv = rig.fed(storage, case["p"], case["q"], at, init)
    held = dict(case, p=case["p"] - shift)
    got = pp.check_update(T, held, _ref(refs, (name, tuple(shift)), held["p"], held["q"]), pivot=piv - shift, pivot_q=piv, storage=storage)
    print(name, storage, "pivot", piv.tolist(), {k: v for k, v in got.items() if k != "case"})


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("name", COMPUTED)
def test_computed_record_through_every_form(name, storage, rig, refs):
    """c.  The pairs are the stored clouds' (f32 storage rounds the thin slabs' z and the offset targets); the reference is theirs."""
    case = CASES[name]
    src, q, init, p_eff, q_eff = _effective(case, storage)
    shift, _ = _frame(case, storage)
    tgt = np.vstack([q, _stored(pp.decoys(case), storage)])
    res = rig.computed(storage, src, tgt, case["radius"], init)
    for form in ("two-launch", "step-wise", "batch", "multi"):
        _same_bits(res[form], res["fused"], "%s: %s form against fused" % (name, form))
    T = res["fused"]["transformation"]
    assert res["fused"]["n_corr"] == len(src) and res["fused"]["iterations"] == 1 and res["fused"]["fitness"] == 1.0
    piv = pp.pivot_of(p_eff[0])
    held = dict(case, p=src, q=q_eff)
    got = pp.check_update(T, held, _ref(refs, (name, storage, "stored"), src, q_eff), pivot=piv - shift, pivot_q=piv, storage=storage)
    print(name, storage, {k: v for k, v in got.items() if k != "case"})
    exact = max(np.max(np.abs(p_eff - piv)), np.max(np.abs(q_eff - piv))) < 16.0 and all(
        np.array_equal(a * 2.0 ** 20, np.round(a * 2.0 ** 20)) for a in (p_eff, q_eff))
    if exact:  # products of at most 48 bits are exact, and the pass's exact sums round once, as math.fsum does: the pass's record is the
        # fed one to the bit, and so is the pose
        at = np.zeros(3) if init is not None or case["offset"] is None else case["offset"]
        T_fed, piv_fed = rig.fed(storage, p_eff, q_eff, at, init)
        assert np.array_equal(piv_fed, piv)
        assert np.array_equal(T_fed.view(np.uint64), T.view(np.uint64)), (name, T_fed, T)
    else:
        assert "near_coplanar" in name or case["offset"] is not None, name  # (everything else is exact)


def _fused_stepwise(ranks, n, radius, init, max_iter, passes):
    """o3ds_icp_begin / `passes` x o3ds_icp_pass / o3ds_icp_pass_finish, the form ShardedIcp uses by default, on one handle per rank.
    ranks: (handle, source, target, first, count) each; after every pass the ranks' sums are added and handed back to all of them, as the
    all-reduce of a source-sharded run does.  Returns one result per rank."""
    import torch

    sums = [[torch.zeros(512, dtype=torch.float64, device="cuda:0") for _ in range(3)] for _ in ranks]
    torch.cuda.synchronize()
    for be, s, t, _, _ in ranks:
        be.icp_begin(s, t, radius, init=init, max_iter=max_iter, method=P2P, **FIXED)
    for p in range(passes):
        for (be, _, _, first, count), sm in zip(ranks, sums):
            out, nxt, prev = sm[p % 3], sm[(p + 1) % 3], sm[(p + 2) % 3]
            be.icp_pass(first, count, n, prev.data_ptr() if p > 0 else None, out.data_ptr(), nxt.data_ptr())
        for be, _, _, _, _ in ranks:
            be.synchronize()
        if len(ranks) > 1:
            total = sum(sm[p % 3] for sm in sums)
            for sm in sums:
                sm[p % 3].copy_(total)
            torch.cuda.synchronize()
    return [be.icp_pass_finish(n, sm[(passes - 1) % 3].data_ptr(), sm[passes % 3].data_ptr()) for (be, _, _, _, _), sm in zip(ranks, sums)]


def _stepwise(be, s, t, n, radius, init, max_iter, updates):
    import torch

    rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    be.icp_begin(s, t, radius, init=init, max_iter=max_iter, method=P2P, **FIXED)
    for _ in range(updates):
        be.icp_accumulate(0, n, rec.data_ptr())
        be.icp_update(rec.data_ptr(), n)
    return be.icp_finish()


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("name", ["patch_20_offset", "coplanar_axis_300_offset", "patch_20"])
def test_fused_step_wise_form_and_its_tail_launch(name, storage, rig, refs):
    """The one-kernel-per-iteration form at the offset.  Its tail launch (o3ds_icp_pass_finish) and the launches of a rank with an empty
    share cover no source point of their own and still step on a record formed about the pivot of point 0: a finish with iterations left
    (one pass of max_iteration 3: the tail applies the first update) equals the step-wise ABI bit for bit and is held to the reference;
    the full loop equals the one-shot registration; and of two ranks, one with the whole source and one with none of it, both end with
    that same pose."""
    case = CASES[name]
    src, q, init, p_eff, q_eff = _effective(case, storage)
    shift, _ = _frame(case, storage)
    tgt = np.vstack([q, _stored(pp.decoys(case), storage)])
    be, n, r = rig.be[storage], len(src), case["radius"]
    s, t = be.upload(src), be.upload(tgt)
    be.build_index(t, r)
    try:
        early = _fused_stepwise([(be, s, t, 0, n)], n, r, init, 3, 1)[0]
        want = _stepwise(be, s, t, n, r, init, 3, 1)
        assert early["iterations"] == want["iterations"] == 1 and early["n_corr"] == n
        assert np.array_equal(early["transformation"].view(np.uint64), want["transformation"].view(np.uint64)), (name, early, want)
        piv = pp.pivot_of(p_eff[0])
        held = dict(case, p=src, q=q_eff)
        got = pp.check_update(early["transformation"], held, _ref(refs, (name, storage, "stored"), src, q_eff), pivot=piv - shift, pivot_q=piv,
                              storage=storage)
        print(name, storage, "tail launch with iterations left", {k: v for k, v in got.items() if k != "case"})
        one_shot = be.icp_register_dev(s, t, r, init=init, max_iter=3, method=P2P, **FIXED)
        full = _fused_stepwise([(be, s, t, 0, n)], n, r, init, 3, 4)[0]
        _same_bits(full, one_shot, name + ": fused step-wise form against the one-shot")
        other = backend.Backend(0, STORAGES[storage])  # a second rank: the same clouds, an empty share of the source
        try:
            s2, t2 = other.upload(src), other.upload(tgt)
            other.build_index(t2, r)
            for k, got2 in enumerate(_fused_stepwise([(be, s, t, 0, n), (other, s2, t2, n, 0)], n, r, init, 3, 4)):
                _same_bits(got2, one_shot, "%s: rank %d of two (shares n and 0) against the one-shot" % (name, k))
        finally:
            other.close()
    finally:
        be.free(s)
        be.free(t)


def _ransac(be, storage, off):
    P, N, Q, NQ = pp.ransac_clouds()
    s, t = be.upload(P + off, N), be.upload(Q + off, NQ)
    be.compute_fpfh(s, 3.0, 30)
    be.compute_fpfh(t, 3.0, 30)
    corr, _ = be.feature_correspondences(s, t, mutual=True, ransac_n=pp.RANSAC_N)
    # the distance checker at 1e-9 m turns every hypothesis away (three grid-rounded pairs never fit that well), so none is validated,
    # the loop never stops early, and the trace holds all of them
    r = be.ransac_feature_matching(s, t, 0.5, pp.RANSAC_N, True, 0.0, 1e-9, pp.RANSAC_ITER, 0.999, pp.RANSAC_SEED, trace=pp.RANSAC_ITER)
    S, Tg = be.download(s)[0], be.download(t)[0]
    be.free(s)
    be.free(t)
    return r, np.asarray(corr, dtype=np.int64), S, Tg


@pytest.mark.parametrize("storage,where", [("f32", "origin"), ("f64", "origin"), ("f64", "offset")])
def test_ransac_hypotheses(storage, where, rig):
    """d.  Share of exempt draws measured: 6 of 512 (1.2 %)."""
    off = pp.OFFSET if where == "offset" else np.zeros(3)
    r, corr, S, Tg = _ransac(rig.be[storage], storage, off)
    assert r["iterations_run"] == pp.RANSAC_ITER and len(corr) >= 100, (r["iterations_run"], len(corr))
    tr = r["trace"]
    exempt, worst = 0, dict(ratio=0.0, angle=0.0, placement=0.0)
    for k in range(pp.RANSAC_ITER):
        smp = rs.draw(pp.RANSAC_SEED, pp.RANSAC_N, k, len(corr))
        assert list(tr["sample"][k]) == smp
        ps, qs = S[corr[smp, 0]], Tg[corr[smp, 1]]
        ref = pp.umeyama_reference(ps, qs)
        unique = pp.is_unique(ref)
        exempt += not unique
        hyp = dict(name="hypothesis %d %s" % (k, smp), p=ps, q=qs, envelope=bool(unique and pp.extent(ps) >= pp.ENVELOPE_EXTENT))
        got = pp.check_update(tr["transformation"][k], hyp, ref, pivot=pp.pivot_of(ps[0]), pivot_q=pp.pivot_of(qs[0]), storage=storage)  # (the kernel's frame: about the first pair)
        for key in worst:
            worst[key] = max(worst[key], got.get(key, 0.0))
    print(storage, where, "pairs", len(corr), "exempt", exempt, "worst", worst)
    assert exempt <= 0.05 * pp.RANSAC_ITER
