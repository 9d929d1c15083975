"""The premises of tests/test_pose_graph_edges_gpu.py, on the restatement alone: each scenario takes the branch it is there for, every
compared run is decision-stable under three solvers, and the figures the GPU tolerances are derived from are what the restatement gives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as rs  # noqa: E402
import pose_graph_edge_cases as ec  # noqa: E402

OPT = rs.Option(1.0, 0.2, 2.0, -1)  # test_pose_graph_gpu.OPT, no reference node
SOLVERS = (np.linalg.solve, rs.solve_cholesky, rs.solve_refined)


def _run(T0, E, solve=np.linalg.solve, opt=OPT, **crit):
    return rs.global_optimization(T0, E, criteria=rs.Criteria(**crit), option=opt, solve=solve)


def _stats(r):
    return [(p["iterations"], p["lm_steps"], p["stop_reason"]) for p in r["passes"]]


def _rejections(p):
    return [t[3] <= 0 for t in p["trace"]]


def _assert_decision_stable(T0, E, opt=OPT, **crit):
    runs = [_run(T0, E, s, opt, **crit) for s in SOLVERS]
    for r in runs[1:]:
        assert _stats(r) == _stats(runs[0])
        assert np.array_equal(r["kept"], runs[0]["kept"])
    return runs


# ---- the solvers ------------------------------------------------------------------------------------------------------------------------
def test_solvers_agree_and_the_refined_one_is_the_most_accurate():
    rng = np.random.default_rng(0)
    for m in (7, 60, 300):  # 300 rows: the longdouble residual; below: mpmath's where it imports
        B = rng.integers(-3, 4, (m, m)).astype(np.float64)  # integers: A, x and b = A x are exact in f64
        A = B @ B.T + np.eye(m)
        x = rng.integers(-9, 10, m).astype(np.float64)
        b = A @ x
        err = [np.linalg.norm(s(A, b) - x) / np.linalg.norm(x) for s in SOLVERS]
        bound = np.linalg.cond(A) * 2.0 ** -53
        assert err[0] <= bound and err[1] <= bound
        assert err[2] <= 2.0 ** -52  # the true solution, rounded
        L = rs.cholesky_lower(A)
        np.testing.assert_allclose(L @ L.T, A, rtol=0, atol=1e-12 * np.abs(A).max())
    with pytest.raises(rs.NotPositiveDefinite) as e:
        rs.cholesky_lower(np.diag([1.0, 2.0, -1.0, 3.0]))
    assert e.value.row == 2


# ---- rejected steps, stop reasons, decision stability ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.LONG_RUNS))
def test_long_runs_reject_steps_are_decision_stable_and_carry_their_own_figures(name):
    builder, kw, crit, recorded = ec.LONG_RUNS[name]
    _, T0, E = builder(**kw)
    lu, ch, _ = _assert_decision_stable(T0, E, **crit)
    rej = [_rejections(p) for p in lu["passes"]]
    assert sum(r.count(True) for r in rej) >= 2
    assert any(a and b for r in rej for a, b in zip(r, r[1:]))  # two in a row: ni only matters from the second
    measured = (np.abs(lu["poses"] - ch["poses"]).max(), np.abs(lu["confidence"] - ch["confidence"]).max(),
                max(abs(p["residual"] - q["residual"]) / max(abs(p["residual"]), 1e-300) for p, q in zip(lu["passes"], ch["passes"])))
    print(name, _stats(lu), [r.count(True) for r in rej], "LU vs Cholesky: pose %.2e confidence %.2e residual %.2e" % measured)
    # the recorded figures are the measurement (to a factor 10: they are rounding noise), and the multiple stays below 1e-6
    assert recorded[0] / 10 <= measured[0] <= recorded[0] * 10
    assert measured[1] <= max(recorded[1] * 10, 1e-13) and measured[2] <= max(recorded[2] * 10, 1e-10)
    assert ec.long_run_tolerances(name)[0] <= 1e-6


def test_long_runs_reach_their_stop_reasons():
    want = {"scrambled21": (5, 4), "scrambled30": (3, 4), "certain21": (5, 5), "certain30": (5, 5), "lm2_certain30": (6, 6), "all_outliers": (3, 1)}
    for name, (builder, kw, crit, _) in ec.LONG_RUNS.items():
        _, T0, E = builder(**kw)
        r = _run(T0, E, **crit)
        assert tuple(p["stop_reason"] for p in r["passes"]) == want[name], (name, _stats(r))
    # reason 6 in lm2_certain30 comes in an outer iteration after accepted ones: lm_count starts again in each (a count kept across them
    # would have stopped at the second step)
    assert _stats(r := _run(*rs.scrambled_graph(30, 11, True)[1:], max_iteration=12, max_iteration_lm=2))[0] == (4, 5, rs.STOP_MAX_ITER_LM)
    assert _rejections(r["passes"][0]) == [False, False, False, True, True]


@pytest.mark.parametrize("n,seed", [(21, 11), (30, 13)])
@pytest.mark.parametrize("lm", [1, 2])
def test_max_iteration_lm_premise(n, seed, lm):
    _, T0, E = rs.scrambled_graph(n, seed)
    runs = _assert_decision_stable(T0, E, max_iteration_lm=lm)
    assert _stats(runs[0]) == [(1, lm, rs.STOP_MAX_ITER_LM)] * 2
    assert all(_rejections(p) == [True] * lm for p in runs[0]["passes"])


@pytest.mark.parametrize("n", [21, 30])
def test_right_term_after_an_accepted_step_and_residual_premise(n):
    _, T0, E = rs.figure_eight_graph(n_nodes=n, drift_yaw=0.15 / n, n_points=300)
    opt = rs.Option(1.0, 0.2, 2.0, 0)
    r = _assert_decision_stable(T0, E, opt, min_right_term=3e2)[0]
    assert r["passes"][0]["stop_reason"] == rs.STOP_RIGHT_TERM and r["passes"][0]["lm_steps"] >= 1
    assert all(t[3] > 0 for t in r["passes"][0]["trace"])  # after accepted steps only
    r = _assert_decision_stable(T0, E, opt, min_residual=1e3)[0]
    assert r["passes"][0]["stop_reason"] == rs.STOP_RESIDUAL and r["passes"][0]["lm_steps"] >= 1


# ---- structure ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [22, 43, 60])
def test_hub_graph_factor_has_far_tiles(n):
    _, T0, E = rs.hub_graph(n)
    assert sum(1 for e in E if 0 in (e.source, e.target)) >= n - 1
    assert {e.source == 0 for e in E if 0 in (e.source, e.target)} == {True, False}  # both directions
    H, b, lam = rs.first_system(T0, E, OPT)
    L = rs.cholesky_lower(H + lam * np.eye(len(H)))
    nb = (len(L) + 63) // 64
    Lp = np.zeros((64 * nb, 64 * nb))
    Lp[: len(L), : len(L)] = L
    tiles = Lp.reshape(nb, 64, nb, 64).transpose(0, 2, 1, 3)
    far = [(i, j) for i in range(nb) for j in range(nb) if i - j >= 2]
    assert far and all(np.abs(tiles[i, j]).max() > 1e-3 * np.abs(L).max() for i, j in far)
    # the figure-eight's far tiles, for contrast, are fill from the four loop closures at most: most are exactly zero
    _, T8, E8 = rs.figure_eight_graph(n_nodes=60, n_points=300)
    H8, _, l8 = rs.first_system(T8, E8, OPT)
    L8 = rs.cholesky_lower(H8 + l8 * np.eye(len(H8)))[:320, :320].reshape(5, 64, 5, 64).transpose(0, 2, 1, 3)
    assert sum(1 for i in range(5) for j in range(5) if i - j >= 2 and not L8[i, j].any()) >= 1


@pytest.mark.parametrize("name", list(ec.HUB_RUNS))
def test_hub_runs_are_decision_stable(name):
    kw, crit = ec.HUB_RUNS[name]
    _, T0, E = rs.hub_graph(**kw)
    runs = _assert_decision_stable(T0, E, rs.Option(1.0, 0.2, 2.0, 0), **crit)
    assert sum(p["lm_steps"] for p in runs[0]["passes"]) >= 2


def test_many_edges_graph_has_lists_in_the_hundreds():
    _, T0, E = rs.hub_graph(**ec.HUB_RUNS["many_edges"][0])
    assert len(E) == 20000
    on_pair = [e for e in E if {e.source, e.target} == {1, 2}]
    assert len(on_pair) >= 3000 and {e.source for e in on_pair} == {1, 2} and {e.uncertain for e in on_pair} == {True, False}
    ends = np.bincount([v for e in E for v in (e.source, e.target)], minlength=200)
    assert ends.max() >= 3000 and ends.min() >= 100


def test_multi_edge_graph_structure():
    for n in (8, 25):
        _, T0, E = rs.multi_edge_graph(n)
        pair = [e for e in E if {e.source, e.target} == {2, 5}]
        assert len(pair) >= 3 and {(e.source, e.uncertain) for e in pair} >= {(2, False), (5, True), (2, True)}
        assert sum(1 for e in E if e.source == e.target) == 1
        H, b, _ = rs.first_system(T0, E, OPT)
        assert np.abs(H[12:18, 30:36]).max() > 0 and np.abs(b).max() > 0
        r = _assert_decision_stable(T0, E, rs.Option(1.0, 0.2, 2.0, 0))[0]
        assert r["kept"].all()


def _swapped(T):  # TransformMatrix4dToVector6d with its two branches exchanged
    R = T[:3, :3]
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if sy < 1e-6:
        r = [np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])]
    else:
        r = [np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0]
    return np.array([*r, T[0, 3], T[1, 3], T[2, 3]])


def _first_branch_always(T):
    R = T[:3, :3]
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0]), T[0, 3], T[1, 3], T[2, 3]])


@pytest.mark.parametrize("n", [10, 30])
def test_gimbal_graph_takes_the_else_branch_and_the_branch_decides_the_iterations(n, monkeypatch):
    _, T0, E = rs.gimbal_graph(n)
    for i in (1, n - 2):
        R = T0[i][:3, :3]
        assert np.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2) < 1e-9 and abs(abs(R[2, 0]) - 1.0) < 1e-15  # pitch +-pi/2: the else branch
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)
        v = rs.matrix4_to_vector6(T0[i])
        assert v[2] == 0.0 and abs(abs(v[1]) - np.pi / 2) < 1e-15
        np.testing.assert_allclose(rs.vector6_to_matrix4(v), T0[i], atol=1e-15)
    lo, hi = ec.GIMBAL_INCREMENTS[n]
    for inc in (lo, hi, 1e-6):
        _assert_decision_stable(T0, E, min_relative_increment=inc)
    true = [_stats(_run(T0, E, min_relative_increment=inc))[0] for inc in (lo, hi)]
    ratio = [d / x for d, x in _run(T0, E)["passes"][0]["norms"]]
    assert ratio[0] > lo * 1.05 and ratio[0] < hi * 0.999 and ratio[1] < lo / 10  # not on an edge
    assert true == [(2, 2, rs.STOP_REL_INCREMENT), (1, 1, rs.STOP_REL_INCREMENT)]
    monkeypatch.setattr(rs, "matrix4_to_vector6", _swapped)
    assert _stats(_run(T0, E, min_relative_increment=lo))[0] == (1, 1, rs.STOP_REL_INCREMENT)
    monkeypatch.setattr(rs, "matrix4_to_vector6", _first_branch_always)
    assert _stats(_run(T0, E, min_relative_increment=hi))[0][:2] != (1, 1)


def test_all_outliers_graph_keeps_no_edge():
    builder, kw, crit, _ = ec.LONG_RUNS["all_outliers"]
    _, T0, E = builder(**kw)
    assert all(e.uncertain for e in E)
    r = _run(T0, E, **crit)
    assert not r["kept"].any() and r["confidence"].max() < 1e-6
    p = r["passes"][1]
    assert (p["line_process_weight"], p["stop_reason"], p["lm_steps"], p["iterations"], p["residual"]) == (0.0, rs.STOP_RIGHT_TERM, 0, 0, 0.0)
    assert np.array_equal(r["poses"], r["poses_pass1"]) and np.abs(r["poses"] - T0).max() > 1.0


@pytest.mark.parametrize("n", [8, 25])
def test_leaf_cut_graph_loses_exactly_its_leaf_edge(n):
    _, T0, E = rs.leaf_cut_graph(n)
    assert sum(1 for e in E if n - 1 in (e.source, e.target)) == 1 and E[-1].uncertain
    r = _assert_decision_stable(T0, E, max_iteration=0)[0]
    assert not r["kept"][-1] and r["kept"][:-1].all()
    assert _stats(r) == [(1, 1, rs.STOP_MAX_ITER)] * 2 and all(t[3] > 0 for p in r["passes"] for t in p["trace"])  # both steps accepted
    assert np.array_equal(r["poses"][n - 1], r["poses_pass1"][n - 1])
    assert np.abs(r["poses"][: n - 1] - r["poses_pass1"][: n - 1]).max() > 1e-7  # pass 2 moved the others
    H, _, lam = rs.first_system(r["poses_pass1"], [e for e, k in zip(E, r["kept"]) if k], OPT)
    assert not H[6 * (n - 1):].any() and lam > 0  # the leaf's pivots are lambda alone


# ---- one LM step ------------------------------------------------------------------------------------------------------------------------
def test_one_step_bound_is_four_times_the_restatements_own_solves():
    worst = 0.0
    for name, make in ec.ONE_STEP_GRAPHS.items():
        _, T0, E = make()
        E = rs.all_uncertain(E)
        r = _run(T0, E, opt=ec.ONE_STEP_OPTION, max_iteration=0, max_iteration_lm=1)
        assert [(p["lm_steps"], len(p["trace"])) for p in r["passes"]] == [(1, 1), (0, 0)] and r["passes"][0]["trace"][0][3] > 0
        assert not r["kept"].any()
        H, b, lam = rs.first_system(T0, E, ec.ONE_STEP_OPTION)
        A = H + lam * np.eye(len(H))
        ref = rs.solve_refined(A, b)
        unit = np.linalg.cond(A) * 2.0 ** -53 * np.linalg.norm(ref)
        assert np.linalg.norm(ref - rs.solve_refined(A, b, rounds=10)) <= 1e-3 * unit  # the refinement has converged
        c = [np.linalg.norm(rs.recovered_delta(rs.update_pose_graph(list(T0), s(A, b)), T0) - ref) / unit for s in (np.linalg.solve, rs.solve_cholesky)]
        back = np.linalg.norm(rs.recovered_delta(rs.update_pose_graph(list(T0), ref), T0) - ref) / unit
        print(f"{name}: cond {np.linalg.cond(A):.3e} LU {c[0]:.4f} Cholesky {c[1]:.4f} read-back alone {back:.4f}")
        worst = max(worst, *c)
        assert back <= 0.1 * ec.ONE_STEP_C
    assert ec.ONE_STEP_C == 4.0 * ec.ONE_STEP_C_CPU and ec.ONE_STEP_C_CPU / 3 <= worst <= ec.ONE_STEP_C_CPU * 1.5


@pytest.mark.parametrize("n", [10, 30])
def test_reference_node_out_of_range_is_no_reference_node(n):
    _, T0, E = rs.figure_eight_graph(n_nodes=n)
    base = _assert_decision_stable(T0, E)[0]
    for ref in (n, n + 5):
        assert np.array_equal(rs.global_optimization(T0, E, option=rs.Option(1.0, 0.2, 2.0, ref))["poses"], base["poses"])


@pytest.mark.parametrize("n,edge,info", [(10, 0, "minus"), (10, 4, "axis"), (30, 0, "minus"), (30, 5, "axis"), (30, 20, "minus"), (43, 40, "axis")])
def test_indefinite_information_fails_a_pivot_of_the_edges_first_node(n, edge, info):
    _, T0, E = rs.figure_eight_graph(n_nodes=n, drift_yaw=0.15 / n, n_points=300)
    I = -1e3 * np.eye(6) if info == "minus" else E[edge].information - 1e6 * np.diag([0, 0, 0, 0, 1.0, 0])
    bad = list(E)
    bad[edge] = rs.Edge(E[edge].source, E[edge].target, E[edge].transformation, I, False)
    H, b, lam = rs.first_system(T0, bad, rs.Option(1.0, 0.2, 2.0, 0))
    assert b.max() >= 1e-6 and lam > 0  # the pass gets as far as its first solve
    with pytest.raises(rs.NotPositiveDefinite) as e:
        rs.cholesky_lower(H + lam * np.eye(len(H)))
    assert 6 * edge <= e.value.row < 6 * edge + 6
