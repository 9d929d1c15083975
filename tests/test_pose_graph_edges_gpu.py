"""o3ds_global_optimization where the LM loop and the factorisation branch, against the numpy restatement (tests/pose_graph_restatement.py):
rejected steps (rho <= 0, several in a row) and every stop reason on both sides of the one-workgroup threshold; hub graphs whose Cholesky
factor fills in completely, block and node lists in the hundreds; one LM step in isolation against a refined solve; passes without edges,
a node cut loose by pruning, poses at pitch +-pi/2, parallel edges and self-edges; the non-positive-pivot error; determinism.
tests/test_pose_graph_edges_cpu.py pins, without a GPU, that each scenario takes the branch it is here for and that every compared run is
decision-stable (the same iterations, LM steps, stop reasons and kept edges whichever way the restatement solves).

Tolerances: 1e-9 on poses (test_pose_graph_gpu._assert_same) for runs as short as the existing ones.  The long runs carry their own,
ec.LONG_RUN_MULTIPLE (16) x what the restatement differs from itself under LU and under solve_cholesky (ec.LONG_RUNS holds the figures:
poses 1.4e-11 .. 1.7e-8, so 1e-9 .. 2.7e-7).  The single step is held to c cond(H + lambda I) 2^-53 |delta| with c = ec.ONE_STEP_C = 0.15,
4 x the worst of the restatement's own LU and Cholesky solves (0.037)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as rs  # noqa: E402
import pose_graph_edge_cases as ec  # noqa: E402
from test_pose_graph_gpu import OPT, _angle, _assert_same, _edges, _run_both  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be64():
    be = backend.Backend(0, backend.PRECISION_F64)
    yield be
    be.close()


def _stats(r):
    if "passes" in r:
        return [(p["iterations"], p["lm_steps"], p["stop_reason"]) for p in r["passes"]]
    return list(zip(r["iterations"], r["lm_steps"], r["stop_reason"]))


def _assert_long(got, want, name):
    """_assert_same with the long run's own tolerances (ec.long_run_tolerances): counts, reasons and kept edges stay exact"""
    tol, ctol, rtol = ec.long_run_tolerances(name)
    assert got["valid"] and want["valid"]
    assert _stats(got) == _stats(want), (got, _stats(want))
    np.testing.assert_array_equal(got["kept"], want["kept"])
    dp = max(np.abs(a - b).max() for a, b in zip(got["poses"], want["poses"]))
    da = max(_angle(a[:3, :3].T @ b[:3, :3]) for a, b in zip(got["poses"], want["poses"]))
    dc = np.abs(got["confidence"] - want["confidence"]).max()
    dr = max(abs(g - p["residual"]) / max(abs(p["residual"]), 1e-300) for g, p in zip(got["residual"], want["passes"]))
    print(f"{name}: {_stats(want)} pose {dp:.3e} (tol {tol:.1e}) angle {da:.3e} confidence {dc:.3e} (tol {ctol:.1e}) residual {dr:.3e} (tol {rtol:.1e})")
    for k, p in enumerate(want["passes"]):
        assert got["line_process_weight"][k] == pytest.approx(p["line_process_weight"], rel=1e-15)
        assert got["residual"][k] == pytest.approx(p["residual"], rel=rtol, abs=1e-12)
    assert dc <= ctol and dp <= tol and da <= tol


def _rejections(p):
    return [t[3] <= 0 for t in p["trace"]]


# ---- rejected steps and every stop reason ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.LONG_RUNS))
def test_rejected_steps_match_the_restatement(be64, name):
    """rho <= 0: lambda *= ni, ni doubles, the same H and b are solved again and the trial's confidences, edge outputs and right-hand side
    are dropped.  21 nodes run in the one-workgroup solve, 30 in the blocked one; uncertain and all-certain edges; pass 1 ends on reason
    3, 5 or 6 and pass 2 on 4, 5, 6 or (all_outliers: no edge left) 1."""
    builder, kw, crit, _ = ec.LONG_RUNS[name]
    _, T0, E = builder(**kw)
    got, want = _run_both(be64, T0, E, ref=-1, **crit)
    assert any(_rejections(p).count(True) for p in want["passes"])
    _assert_long(got, want, name)
    if name == "all_outliers":
        assert got["n_edges_kept"] == 0 and not got["kept"].any()
        assert (got["line_process_weight"][1], got["stop_reason"][1], got["lm_steps"][1], got["iterations"][1]) == (0.0, rs.STOP_RIGHT_TERM, 0, 0)
        np.testing.assert_allclose(got["poses"], want["poses_pass1"], rtol=0, atol=ec.long_run_tolerances(name)[0])


@pytest.mark.parametrize("n,seed", [(21, 11), (30, 13)])
@pytest.mark.parametrize("lm", [1, 2])
def test_max_iteration_lm_ends_a_run_of_rejections(be64, n, seed, lm):
    """the first step of the scrambled graph is rejected, and so is the second: reason 6 after lm steps, nothing has moved"""
    _, T0, E = rs.scrambled_graph(n, seed)
    got, want = _run_both(be64, T0, E, ref=-1, max_iteration_lm=lm)
    assert _stats(want) == [(1, lm, rs.STOP_MAX_ITER_LM)] * 2
    _assert_same(got, want)
    assert np.array_equal(got["poses"], T0)


@pytest.mark.parametrize("n", [21, 30])
def test_right_term_after_an_accepted_step_and_residual(be64, n):
    """reason 1 where it is not the first thing a pass does (min_right_term raised to 3e2: false at the start of pass 1, true after
    two accepted steps), and reason 4 with min_residual raised above the converged residual"""
    _, T0, E = rs.figure_eight_graph(n_nodes=n, drift_yaw=0.15 / n, n_points=300)
    got, want = _run_both(be64, T0, E, min_right_term=3e2)
    assert want["passes"][0]["stop_reason"] == rs.STOP_RIGHT_TERM and want["passes"][0]["lm_steps"] >= 1
    _assert_same(got, want)
    got, want = _run_both(be64, T0, E, min_residual=1e3)
    assert want["passes"][0]["stop_reason"] == rs.STOP_RESIDUAL and want["passes"][0]["lm_steps"] >= 1
    _assert_same(got, want)


# ---- dense fill ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.HUB_RUNS))
def test_hub_graph_fills_the_factor(be64, name):
    """node 0 tied to every node: every tile of L is non-zero, the far ones (i - j >= 2) too, so pg_trsm_kernel, pg_syrk_kernel and the
    substitutions' off-diagonal updates all carry weight.  hub400 runs two outer iterations; many_edges is 200 nodes under 20,000
    edges, 3000 of them on the pair (1, 2) in both directions: block and node lists in the thousands, and pg_reduce_kernel strides
    twenty times over the edges."""
    kw, crit = ec.HUB_RUNS[name]
    _, T0, E = rs.hub_graph(**kw)
    got, want = _run_both(be64, T0, E, **crit)
    assert sum(got["lm_steps"]) >= 2
    _assert_same(got, want)


# ---- one LM step in isolation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.ONE_STEP_GRAPHS))
def test_one_lm_step_against_the_refined_solve(be64, name):
    """max_iteration = 0, max_iteration_lm = 1, no reference node, every edge uncertain and the prune threshold 1: pass 1 takes one
    (accepted) step, pass 2 has no edge.  delta_i = V6(pose_new_i pose_old_i^-1) against solve_refined on the restatement's H, b and
    lambda: |delta_dev - delta_ref| <= c cond(H + lambda I) 2^-53 |delta_ref|.

    c = ec.ONE_STEP_C = 4 x 0.0371 = 0.148.  Measured on the CPU in the same units, the step read back from the poses in the same way
    (band21 band30 hub21 hub30 hub60): f64 LU 0.0036 0.0099 0.0371 0.0337 0.0040, solve_cholesky 0.0118 0.0023 0.0098 0.0135 0.0035;
    cond is 1.0e5 .. 1.9e5.  21 nodes: the one-workgroup solve; the others: the blocked one."""
    _, T0, E = ec.ONE_STEP_GRAPHS[name]()
    E = rs.all_uncertain(E)
    o = ec.ONE_STEP_OPTION
    got = be64.global_optimization(T0, _edges(E), o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, -1,
                                   max_iteration=0, max_iteration_lm=1)
    assert got["valid"] and got["lm_steps"] == [1, 0] and got["n_edges_kept"] == 0
    H, b, lam = rs.first_system(T0, E, o)
    A = H + lam * np.eye(len(H))
    ref = rs.solve_refined(A, b)
    dev = rs.recovered_delta(got["poses"], T0)
    unit = np.linalg.cond(A) * 2.0 ** -53 * np.linalg.norm(ref)
    c = np.linalg.norm(dev - ref) / unit
    print(f"{name}: cond {np.linalg.cond(A):.3e} |delta| {np.linalg.norm(ref):.3e} device c {c:.4f} (bound {ec.ONE_STEP_C:.4f})")
    assert np.linalg.norm(ref) > 0.1  # a step, not a stand-still
    assert c <= ec.ONE_STEP_C


# ---- degenerate passes and poses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 25])
def test_leaf_cut_loose_by_pruning_stays_where_pass_1_left_it(be64, n):
    """max_iteration = 0: one accepted step per pass, so pass 2 moves every node that still has an edge -- and the leaf not at all"""
    _, T0, E = rs.leaf_cut_graph(n)
    got, want = _run_both(be64, T0, E, ref=-1, max_iteration=0)
    assert _stats(want) == [(1, 1, rs.STOP_MAX_ITER)] * 2
    assert not want["kept"][-1] and want["kept"][:-1].all()
    assert np.array_equal(want["poses"][n - 1], want["poses_pass1"][n - 1]) and want["passes"][1]["lm_steps"] >= 1
    _assert_same(got, want)
    assert np.abs(got["poses"][n - 1] - want["poses_pass1"][n - 1]).max() <= 1e-9
    assert np.abs(got["poses"][: n - 1] - want["poses_pass1"][: n - 1]).max() > 1e-7  # pass 2 moved the others


@pytest.mark.parametrize("n", [10, 30])
@pytest.mark.parametrize("which", [0, 1, None])
def test_gimbal_poses(be64, n, which):
    """nodes at pitch +-pi/2 exactly: |x| of stop check 2 comes from the else branch of TransformMatrix4dToVector6d there and from the
    first branch elsewhere; the two min_relative_increment values sit where a wrong branch changes `iterations`"""
    _, T0, E = rs.gimbal_graph(n)
    crit = {} if which is None else dict(min_relative_increment=ec.GIMBAL_INCREMENTS[n][which])
    got, want = _run_both(be64, T0, E, ref=-1, **crit)
    if which is not None:
        assert _stats(want)[0] == ((2, 2, rs.STOP_REL_INCREMENT), (1, 1, rs.STOP_REL_INCREMENT))[which]
    _assert_same(got, want)


@pytest.mark.parametrize("n", [8, 25])
def test_parallel_edges_and_a_self_edge(be64, n):
    _, T0, E = rs.multi_edge_graph(n)
    got, want = _run_both(be64, T0, E)
    _assert_same(got, want)
    assert got["kept"].all()


@pytest.mark.parametrize("n", [10, 30])
def test_reference_node_out_of_range_is_no_reference_node(be64, n):
    _, T0, E = rs.figure_eight_graph(n_nodes=n)
    base = be64.global_optimization(T0, _edges(E), reference_node=-1, **OPT)
    for ref in (n, n + 5):
        got, want = _run_both(be64, T0, E, ref=ref)
        _assert_same(got, want)
        assert got["poses"].tobytes() == base["poses"].tobytes()


# ---- the error path ---------------------------------------------------------------------------------------------------------------------
def _raw_call(be, T0, E):
    """the ABI called with buffers this test owns, so that it can look at them after an error"""
    P = np.ascontiguousarray(np.asarray(T0, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
    Ed = (backend.PoseGraphEdge * len(E))()
    for k, e in enumerate(E):
        Ed[k].source_node_id, Ed[k].target_node_id, Ed[k].uncertain = e.source, e.target, int(e.uncertain)
        Ed[k].transformation[:] = list(backend.colmajor(e.transformation))
        Ed[k].information[:] = [float(v) for v in np.asarray(e.information).reshape(36)]
        Ed[k].confidence = e.confidence
    o = backend.GlobalOptimizationOption(OPT["max_correspondence_distance"], OPT["edge_prune_threshold"], OPT["preference_loop_closure"], 0, 0)
    c = backend.GlobalOptimizationCriteria(100, 20, 1e-6, 1e-6, 1e-6, 1e-6, 2.0 / 3.0, 1.0 / 3.0)
    kept = np.ones(len(E), np.uint8)
    out = backend.PoseGraphResult()
    before = (P.tobytes(), bytes(Ed))
    rc = be.lib.o3ds_global_optimization(be.h, P.ctypes.data_as(C.POINTER(C.c_double)), len(T0), Ed, len(E), C.byref(o), C.byref(c),
                                         kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out))
    return rc, before, (P.tobytes(), bytes(Ed))


@pytest.mark.parametrize("n,edge,info", [(10, 0, "minus"), (10, 4, "axis"), (30, 0, "minus"), (30, 5, "axis"), (30, 20, "minus"), (43, 40, "axis")])
def test_indefinite_information_is_an_error_that_names_the_pivot(be64, n, edge, info):
    """an edge whose information matrix is -1e3 I, or PSD minus a large multiple of one axis: the first pivot of H + lambda I that is not
    positive is row 6 min(source, target) or a later one of that node -- in the one-workgroup solve (10 nodes), in block 0 of the blocked
    one (30 nodes, edges 0 and 5) and in a later block (edge 20: row 120, block 1; 43 nodes, edge 40: row 240, block 3).  The error names
    the row the restatement's Cholesky stops at, the caller's poses and edges are untouched, and the handle works on as a fresh one does."""
    _, T0, E = rs.figure_eight_graph(n_nodes=n, drift_yaw=0.15 / n, n_points=300)
    good = [rs.Edge(e.source, e.target, e.transformation, e.information, e.uncertain) for e in E]
    bad = list(good)
    I = -1e3 * np.eye(6) if info == "minus" else E[edge].information - 1e6 * np.diag([0, 0, 0, 0, 1.0, 0])
    bad[edge] = rs.Edge(E[edge].source, E[edge].target, E[edge].transformation, I, False)
    H, b, lam = rs.first_system(T0, bad, rs.Option(1.0, 0.2, 2.0, 0))
    with pytest.raises(rs.NotPositiveDefinite) as e:
        rs.cholesky_lower(H + lam * np.eye(len(H)))
    row = e.value.row
    assert 6 * edge <= row < 6 * edge + 6
    rc, before, after = _raw_call(be64, T0, bad)
    assert rc == backend.ERR_INVALID_ARG
    msg = (be64.lib.o3ds_last_error(be64.h) or b"").decode()
    assert "not positive definite" in msg and int(re.search(r"pivot of row (\d+)", msg).group(1)) == row, msg
    assert after == before
    with pytest.raises(backend.BackendError) as e:
        be64.global_optimization(T0, _edges(bad), **OPT)
    assert e.value.code == backend.ERR_INVALID_ARG
    again = be64.global_optimization(T0, _edges(good), reference_node=0, **OPT)
    fresh_be = backend.Backend(0, backend.PRECISION_F64)
    fresh = fresh_be.global_optimization(T0, _edges(good), reference_node=0, **OPT)
    fresh_be.close()
    assert again["poses"].tobytes() == fresh["poses"].tobytes() and again["confidence"].tobytes() == fresh["confidence"].tobytes()
    assert (again["iterations"], again["lm_steps"], again["stop_reason"], again["residual"]) == (fresh["iterations"], fresh["lm_steps"],
                                                                                                 fresh["stop_reason"], fresh["residual"])


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scrambled30", "certain21", "hub200"])
def test_bitwise_determinism(be64, name):
    if name == "hub200":
        (_, T0, E), crit = rs.hub_graph(200), {}
    else:
        builder, kw, crit, _ = ec.LONG_RUNS[name]
        _, T0, E = builder(**kw)
    runs = [be64.global_optimization(T0, _edges(E), reference_node=-1, **OPT, **crit) for _ in range(2)]
    be = backend.Backend(0, backend.PRECISION_F64)
    runs.append(be.global_optimization(T0, _edges(E), reference_node=-1, **OPT, **crit))
    be.close()
    for r in runs[1:]:
        assert r["poses"].tobytes() == runs[0]["poses"].tobytes() and r["confidence"].tobytes() == runs[0]["confidence"].tobytes()
        assert (r["iterations"], r["lm_steps"], r["stop_reason"], r["residual"]) == (runs[0]["iterations"], runs[0]["lm_steps"],
                                                                                     runs[0]["stop_reason"], runs[0]["residual"])
