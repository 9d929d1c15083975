"""The serial step of an ICP iteration (icp_kernels.hpp icp_step_block: fold, convergence test, 6x6 solve, U, T <- U * T) at tiny sizes.

Every case runs one registration three ways -- the fused form, the two-launch form (O3DS_ICP_MODE=launch) and the step-wise ABI
(o3ds_icp_begin / accumulate / update) -- and asserts (1) that the three agree bit for bit in transformation, fitness, inlier_rmse,
iterations and correspondence count, and (2) that they equal, bit for bit, what the library of the commit BEFORE the step was reworked
produced for the same inputs on an MI355X (tests/golden/icp_step_parent.npz, see profiles/serial_step.txt for the commit).  The inputs
are regenerated from seeds.  Signed zeros count: the comparison is on the bit patterns.

The golden file is never written from the build under test.  `python tests/test_icp_step_gpu.py --record FILE` exists to record it
with a library of the parent commit (O3DS_BACKEND_LIB names it) and refuses to run without that override.

Cases: the three estimators x f32 / f64 storage x max_iter 1, 2, 3, 10, 12 (a fold-only run, one solve, the ordered solve after a
searching one, the chunk boundary at 12 launches), an exit by the convergence test, (a) a one-plane map (a rank-deficient system
with exactly zero rows), (b) a scan with no correspondence (identity update), (c) a start pose from which the largest diagonal entry
of the normal equations changes index between iterations 1 and 2 (the handed-down pivot order fails its strict-maximum check),
(d) signed zeros, two ways.  Mirror-symmetric clouds (d_mirror_*) only come to 1e-20 of a zero: a mirrored pair of terms does not
cancel to the last bit of the device's record sums.  So the exact zeros are FED (fed_*): the step-wise ABI takes the record from
the caller's memory (o3ds_icp_update), and a hand-written record with a diagonal J^T J and J^T r entries of +0.0 and -0.0 has update
components that are exactly -0.0 and +0.0 -- all eight sign patterns of the three angles, zero translations, a permuted pivot order,
null pivots -- through the searching solve (first update) and the ordered one (the following ones).  Only the step-wise form can be
fed a record; the fused and two-launch forms compute theirs, so the fed cases compare the step-wise form with the parent's bits and
with the closed form alone.  What a signed zero can reach: sin(-0.0) = -0.0 puts a negative zero into every entry of U that is a single
product or a negation (0, 1, 2, 6, 10 and the translation lanes), but no further -- T <- U * T accumulates each entry with fma from
+0.0, and (+0.0) + (-0.0) = +0.0, and the candidate-set margin squares its terms -- so the reachable property, asserted below, is
that every zero of the result is +0.0 and every other entry is the closed form's and the parent's."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (before the backend: see tests/conftest.py)

from open3d_slam_amd import backend, synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_step_parent.npz")
MAX_CORR = 1.0
N_MAP, N_AZ = 20_000, 128  # 16 rings x 128 azimuth steps = 2048 points
METHODS = {"plane": backend.ICP_POINT_TO_PLANE, "gicp": backend.ICP_GENERALIZED, "point": backend.ICP_POINT_TO_POINT}
PRECISIONS = {"f32": backend.PRECISION_F32, "f64": backend.PRECISION_F64}
FIXED = dict(rel_fitness=0.0, rel_rmse=0.0)
# (c): truth is synthetic.ground_truth_pose(), t = (0.30, -0.20, 0.05), rpy = (0.5, -0.5, 2.0) deg.  Started 3 deg off in pitch and 4 deg
# off in yaw, about 550 of the 2048 points (the far walls) find no correspondence in iteration 1 and J^T J's largest diagonal entry is
# the roll one; from iteration 2 on everything matches and the yaw entry leads (margins 23 % and 28 %: f32 storage cannot flip them)
INIT_C = syn.make_pose([0.30, -0.20, 0.05], [0.5, 2.5, 6.0])


def _pitch_pose(deg, tx, tz):
    """x / z translation and pitch only, with exact zeros where a mirror y -> -y needs them"""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s, tx], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, tz], [0.0, 0.0, 0.0, 1.0]])


def _yz_pose(deg, ty, tz):
    """y / z translation and roll only: the same for a mirror x -> -x"""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, c, -s, ty], [0.0, s, c, tz], [0.0, 0.0, 0.0, 1.0]])


def _grid(a, bits):
    return np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits


def _mirrored(pts, axis):
    """[p0, mirror(p0), p1, mirror(p1), ...]: the half on the positive side of `axis` and its mirror image, pair by pair"""
    m = pts.copy()
    m[:, axis] = -m[:, axis]
    return np.ascontiguousarray(np.stack([pts, m], 1).reshape(-1, 3))


_CLOUDS = {}


def clouds():
    """name -> (src, src_normals or None, tgt, tgt_normals), built once"""
    if _CLOUDS:
        return _CLOUDS
    from oracle import pyoracle as po

    src, tgt, nrm, T_gt = syn.config2_inputs(n_map=N_MAP, n_az=N_AZ)
    assert len(src) == 2048 and len(tgt) == N_MAP
    # the golden record holds bits, so the inputs must not depend on how a machine's BLAS or libm rounds a last place (the ray
    # directions are a matrix product): everything is put on a grid of 2^-20 m (normals: 2^-30) before it is used
    src, tgt, nrm = _grid(src, 20), _grid(tgt, 20), _grid(nrm, 30)
    _CLOUDS["main"] = (src, _grid(po.estimate_normals(src, 3.0, 20), 30), tgt, nrm)
    # (a) one plane: x / y translation and yaw are unobservable, exactly zero rows of J^T J
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(-8, 8, 0.25), np.arange(-8, 8, 0.25)), -1).reshape(-1, 2)
    _CLOUDS["plane_map"] = (_grid(np.c_[rng.uniform(-6, 6, (500, 2)), 0.04 + 0.02 * rng.uniform(-1, 1, 500)], 20), None,
                            np.c_[g, np.zeros(len(g))], np.tile([0.0, 0.0, 1.0], (len(g), 1)))
    # (b) the scan 64 m away from every map point
    _CLOUDS["far_scan"] = (src + np.array([50.0, 0.0, 40.0]), _CLOUDS["main"][1], tgt, nrm)
    # (d) map and scan symmetric under a mirror (y -> -y, then x -> -x), the scan displaced inside the mirror's own motions: the
    # rows of the system that belong to the other three motions cancel pair by pair, so those components of the update -- two of the
    # three angles among them -- are zero up to the residue of the sums (1e-20 on the device, not a signed zero), of either sign:
    # sines of +-1e-20, single products and negations of them, in every entry of U that is one
    in_map = _grid(po.transform_points(src, T_gt), 20)
    for name, axis, S in (("mirror_y", 1, _pitch_pose(1.0, 0.2, 0.1)), ("mirror_x", 0, _yz_pose(-1.0, -0.15, 0.1))):
        keep = tgt[:, axis] > 0.0
        half = in_map[in_map[:, axis] > 0.3][:1024]
        h, R = half - S[:3, 3], S[:3, :3]  # S^-1, term by term: the registration has to find S
        half = _grid(np.stack([(h[:, 0] * R[0, k] + h[:, 1] * R[1, k]) + h[:, 2] * R[2, k] for k in range(3)], 1), 20)
        n_m = nrm[keep].copy()
        n_m[:, axis] = -n_m[:, axis]
        _CLOUDS[name] = (_mirrored(half, axis), None, _mirrored(tgt[keep], axis),
                         np.ascontiguousarray(np.stack([nrm[keep], n_m], 1).reshape(-1, 3)))
    return _CLOUDS


def cases():
    """name -> (cloud set, estimator, storage, init or None, criteria)"""
    out = {}
    for m in METHODS:
        for p in PRECISIONS:
            for it in (1, 2, 3, 10, 12):
                out["%s_%s_iter%d" % (m, p, it)] = ("main", m, p, None, dict(max_iter=it, **FIXED))
    out["early_exit_plane_f32"] = ("main", "plane", "f32", None, dict(max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6))
    out["early_exit_gicp_f64"] = ("main", "gicp", "f64", None, dict(max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6))
    for p in PRECISIONS:
        out["a_one_plane_%s" % p] = ("plane_map", "plane", p, None, dict(max_iter=5, **FIXED))
        out["b_no_correspondence_%s" % p] = ("far_scan", "plane", p, None, dict(max_iter=3, **FIXED))
        out["c_pivot_order_changes_%s" % p] = ("main", "plane", p, INIT_C, dict(max_iter=4, **FIXED))
        out["d_mirror_y_%s" % p] = ("mirror_y", "plane", p, None, dict(max_iter=3, **FIXED))
        out["d_mirror_x_%s" % p] = ("mirror_x", "plane", p, None, dict(max_iter=3, **FIXED))
    out["b_no_correspondence_gicp_f32"] = ("far_scan", "gicp", "f32", None, dict(max_iter=3, **FIXED))
    return out


def _pack(r):
    f = np.concatenate([np.ascontiguousarray(r["transformation"], np.float64).reshape(16), [r["fitness"], r["inlier_rmse"]]])
    return f.astype(np.float64), np.array([r["iterations"], r["n_corr"]], np.int64)


def _same_bits(a, b, what):
    fa, ia = _pack(a) if isinstance(a, dict) else a
    fb, ib = _pack(b) if isinstance(b, dict) else b
    assert np.array_equal(fa.view(np.uint64), fb.view(np.uint64)), (what, fa, fb)
    assert np.array_equal(ia, ib), (what, ia, ib)


class Rig:
    """One handle per storage precision and form; clouds are uploaded to a handle once."""

    def __init__(self):
        self.fused = {p: backend.Backend(0, v) for p, v in PRECISIONS.items()}
        mp = pytest.MonkeyPatch()
        mp.setenv("O3DS_ICP_MODE", "launch")
        self.launch = {p: backend.Backend(0, v, ab=True) for p, v in PRECISIONS.items()}
        mp.undo()  # (the mode is read when the handle is made)
        self.ids = {}

    def close(self):
        for be in list(self.fused.values()) + list(self.launch.values()):
            be.close()

    def _ids(self, be, cloud):
        key = (id(be), cloud)
        if key not in self.ids:
            src, sn, tgt, nrm = clouds()[cloud]
            s, t = be.upload(src, sn), be.upload(tgt, nrm)
            be.build_index(t, MAX_CORR)
            self.ids[key] = (s, t, len(src))
        return self.ids[key]

    def run(self, case):
        """(fused, two-launch, step-wise) results of one case"""
        import torch

        cloud, m, p, init, kw = cases()[case]
        out = []
        for be in (self.fused[p], self.launch[p]):
            s, t, _ = self._ids(be, cloud)
            out.append(be.icp_register_dev(s, t, MAX_CORR, init=init, method=METHODS[m], **kw))
        be = self.fused[p]
        s, t, n = self._ids(be, cloud)
        rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        be.icp_begin(s, t, MAX_CORR, init=init, method=METHODS[m], **kw)
        for _ in range(kw["max_iter"] + 1):
            be.icp_accumulate(0, n, rec.data_ptr())
            be.icp_update(rec.data_ptr(), n)
            if be.icp_done():
                break
        assert be.icp_done()
        out.append(be.icp_finish())
        return out

    def run_fed(self, case):
        """the step-wise form with a record of the caller's in place of the pass's"""
        import torch

        diag, jtr, init = fed_cases()[case]
        be = self.fused["f32"]
        s, t, n = self._ids(be, "main")
        rec = torch.from_numpy(_fed_record(diag, jtr)).to("cuda:0")
        torch.cuda.synchronize()
        be.icp_begin(s, t, MAX_CORR, init=init, max_iter=FED_ITERATIONS, **FIXED)
        for _ in range(FED_ITERATIONS + 1):
            be.icp_update(rec.data_ptr(), n)
        assert be.icp_done()
        return be.icp_finish()


FED_ITERATIONS = 3  # the first update solves with the pivot search, the second and third with the order it found


def fed_cases():
    """name -> (diagonal of J^T J, J^T r, init or None): records written by hand for o3ds_icp_update"""
    out = {}
    for bits in range(8):  # every sign pattern of three zero angles; the yaw or the translations carry the motion
        z = [(-0.0 if (bits >> k) & 1 else 0.0) for k in range(3)]
        out["fed_zero_angles_%d" % bits] = ([6.0, 5.0, 4.0, 3.0, 2.0, 1.0], z + [0.3, -0.2, 0.5], None)
        out["fed_zero_roll_pitch_%d" % bits] = ([6.0, 5.0, 4.0, 3.0, 2.0, 1.0], z[:2] + [0.04 if bits & 4 else -0.04, 0.3, -0.2, 0.5], None)
    out["fed_zero_roll_pitch_dense_init"] = ([6.0, 5.0, 4.0, 3.0, 2.0, 1.0], [-0.0, 0.0, 0.04, 0.3, -0.2, 0.5], INIT_C)
    out["fed_zero_translations"] = ([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [0.02, -0.01, 0.03, -0.0, 0.0, -0.0], None)
    out["fed_permuted_order"] = ([2.0, 6.0, 1.0, 5.0, 3.0, 4.0], [-0.0, 0.01, 0.0, -0.0, 0.4, 0.0], None)
    out["fed_null_pivots"] = ([5.0, 0.0, 3.0, 0.0, 0.0, 1.0], [0.01, 0.0, -0.0, -0.0, 0.0, 0.2], INIT_C)
    return out


def _fed_record(diag, jtr):
    rec = np.zeros(32)
    rec[[0, 6, 11, 15, 18, 20]] = diag  # the packed upper triangle's diagonal (common.hpp: 21 entries of J^T J, 6 of J^T r, ...)
    rec[21:27] = jtr
    rec[27], rec[28], rec[29] = 25.0, 100.0, 25.0  # r^2 sum, correspondence count, d^2 sum: fitness 100 / n, rmse 0.5
    return rec


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    names = [str(n) for n in g["names"]]
    return {n: (g["floats"][k], g["ints"][k]) for k, n in enumerate(names)}


def test_golden_file_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(list(cases()) + list(fed_cases()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(cases()))
def test_step_forms_agree_and_equal_the_parent(case, rig, golden):
    cloud, m, p, init, kw = cases()[case]
    fused, launch, step = rig.run(case)
    print(case, "iterations", fused["iterations"], "n_corr", fused["n_corr"], "fitness", fused["fitness"], "rmse", fused["inlier_rmse"])
    _same_bits(launch, fused, "two-launch form against fused")
    _same_bits(step, fused, "step-wise ABI against fused")
    _same_bits(fused, golden[case], "fused against the parent commit's record")
    T = fused["transformation"]
    assert np.isfinite(T).all()
    if case.startswith("early_exit"):
        assert fused["converged"] and 1 < fused["iterations"] < kw["max_iter"]
    elif not case.startswith("b_"):
        assert fused["iterations"] == kw["max_iter"] and not fused["converged"]
    if case.startswith("b_"):  # [O3D] corres.empty(): the identity update
        assert np.array_equal(T, np.eye(4)) and fused["fitness"] == 0.0 and fused["inlier_rmse"] == 0.0 and fused["n_corr"] == 0
    if case.startswith("a_"):  # the unobservable motions get no update of their own (tests/test_icp_gpu.py, rank-deficient case)
        assert abs(T[0, 3]) < 1e-5 and abs(T[1, 3]) < 1e-5 and abs(T[1, 0]) < 1e-5 and fused["n_corr"] == 500
    # (d): only the mirror's own motions; the other entries are the identity's up to the residue of the sums (f64 record sums of
    # O(1e3) terms of size O(1e2), normal equations of condition ~1e3: far below 1e-12 whatever the order of summation)
    if case.startswith("d_mirror_y"):  # pitch and x / z translation
        assert max(abs(T[0, 1]), abs(T[1, 0]), abs(T[1, 2]), abs(T[2, 1]), abs(T[1, 3]), abs(T[1, 1] - 1.0)) < 1e-12
    if case.startswith("d_mirror_x"):  # roll and y / z translation
        assert max(abs(T[0, 1]), abs(T[1, 0]), abs(T[0, 2]), abs(T[2, 0]), abs(T[0, 3]), abs(T[0, 0] - 1.0)) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(fed_cases()))
def test_fed_record_with_signed_zeros_equals_the_parent_and_the_closed_form(case, rig, golden, oracle):
    diag, jtr, init = fed_cases()[case]
    got = rig.run_fed(case)
    T = got["transformation"]
    print(case, "T", T.tolist(), "sign bits", np.signbit(T).astype(int).tolist())
    _same_bits(got, golden[case], "step-wise form against the parent commit's record")
    assert got["iterations"] == FED_ITERATIONS and got["n_corr"] == 100 and got["fitness"] == 100.0 / 2048.0 and got["inlier_rmse"] == 0.5
    # the closed form: a diagonal system, x_k = -(J^T r)_k / d_k, zero under a null pivot (Eigen's LDLT); the same record every update
    x = np.array([(-r / d if d != 0.0 else 0.0) for d, r in zip(diag, jtr)])
    want = np.eye(4) if init is None else init.copy()
    for _ in range(FED_ITERATIONS):
        want = oracle.vector6_to_matrix4(x) @ want
    np.testing.assert_allclose(T, want, rtol=0.0, atol=1e-14)  # (entries of size <= 1, a dozen roundings each)
    assert not np.signbit(T[T == 0.0]).any()  # no negative zero reaches the result (see the docstring)
    if init is None and x[0] == 0.0 and x[1] == 0.0:  # a pure yaw: the entries fed by the zero sines are zeros, exactly
        assert T[2, 0] == 0.0 and T[2, 1] == 0.0 and T[0, 2] == 0.0 and T[1, 2] == 0.0 and T[2, 2] == 1.0


# ---- the premises of (c) and (d), on the CPU with the oracle's restatement ------------------------------------------------------------
def _normal_equations(oracle, src, tgt, nrm, init, iterations):
    """[O3D] RegistrationICP restated with the oracle's pieces: (J^T J, J^T r, update vector) of every iteration"""
    tree = oracle.KDTree(tgt)
    T = np.eye(4) if init is None else init.copy()
    out = []
    for _ in range(iterations):
        p = oracle.transform_points(src, T)
        corr = oracle.evaluate(tree, p, MAX_CORR)[0]
        JTJ, JTr, _ = oracle.compute_jtj_jtr(p, tgt, nrm, corr)
        U, x = oracle.solve_update(JTJ, JTr)
        out.append((JTJ, JTr, x))
        T = U @ T
    return out, T


def test_premise_c_the_largest_diagonal_entry_changes_index(oracle):
    src, _, tgt, nrm = clouds()["main"]
    eqs, T = _normal_equations(oracle, src, tgt, nrm, INIT_C, 3)
    lead, margin = [], []
    for JTJ, JTr, x in eqs:
        d = np.diag(JTJ)
        print("diag J^T J", d, " J^T r", JTr, " x", x)
        lead.append(int(np.argmax(d)))
        s = np.sort(d)[::-1]
        margin.append(s[0] / s[1])
    assert lead == [0, 2, 2], lead
    assert min(margin) > 1.1, margin  # f32 storage moves a diagonal entry by parts in 1e-6
    ref = oracle.icp_point_to_plane(src, tgt, nrm, MAX_CORR, init=INIT_C, max_iter=3, **FIXED)
    np.testing.assert_allclose(T, ref["transformation"], atol=1e-12)  # the restatement above is the oracle's loop


@pytest.mark.parametrize("name,zero,free", [("mirror_y", (0, 2, 4), (1, 3, 5)), ("mirror_x", (1, 2, 3), (0, 4, 5))])
def test_premise_d_mirrored_inputs_leave_three_components_at_zero(oracle, name, zero, free):
    src, _, tgt, nrm = clouds()[name]
    axis = 1 if name == "mirror_y" else 0
    for a in (src, tgt):  # pairs of mirror images, exactly
        assert np.array_equal(a[0::2, axis], -a[1::2, axis]) and np.array_equal(np.delete(a[0::2], axis, 1), np.delete(a[1::2], axis, 1))
    assert np.array_equal(src.astype(np.float32)[0::2, axis], -src.astype(np.float32)[1::2, axis])
    eqs, _ = _normal_equations(oracle, src, tgt, nrm, None, 2)
    for JTJ, JTr, x in eqs:
        print("J^T r", JTr, " x", x, " sign bits", np.signbit(x))
        # pair by pair the terms cancel; what a summation order leaves is rounding residue (two of the three angles among the zeros)
        assert all(abs(JTr[k]) < 1e-9 for k in zero) and all(abs(JTJ[a, b]) < 1e-9 for a in zero for b in free)
        assert all(abs(x[k]) < 1e-12 for k in zero) and all(abs(x[k]) > 1e-5 for k in free)


# ---- recording (parent commit's library only) -----------------------------------------------------------------------------------------
if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record" or not os.environ.get("O3DS_BACKEND_LIB"):
        sys.exit("usage: O3DS_BACKEND_LIB=<A/B library built from the PARENT commit> python tests/test_icp_step_gpu.py --record FILE")
    rig_ = Rig()
    names, floats, ints = [], [], []
    for c in cases():
        res = rig_.run(c)
        _same_bits(res[1], res[0], c + ": two-launch form against fused")
        _same_bits(res[2], res[0], c + ": step-wise ABI against fused")
        f, i = _pack(res[0])
        names.append(c), floats.append(f), ints.append(i)
        print(c, res[0]["iterations"], res[0]["n_corr"], res[0]["converged"], res[0]["fitness"], res[0]["inlier_rmse"], flush=True)
        if c.startswith("d_"):
            print(res[0]["transformation"], np.signbit(res[0]["transformation"]).astype(int), flush=True)
    for c in fed_cases():
        res = rig_.run_fed(c)
        f, i = _pack(res)
        names.append(c), floats.append(f), ints.append(i)
        print(c, res["iterations"], res["n_corr"], res["transformation"].tolist(), flush=True)
    rig_.close()
    np.savez(sys.argv[2], names=np.array(names), floats=np.array(floats, np.float64), ints=np.array(ints, np.int64))
    print("recorded", len(names), "cases")
