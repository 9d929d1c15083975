"""The pose-graph restatement (tests/pose_graph_restatement.py) and the host logic of OptimizationProblem / applyOptimizedTransforms,
without a GPU: the Jacobians against finite differences, the LM stop paths, pruning, the reference node, the reference's graph
building over two builds and the submap update's walk up the parents."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as rs  # noqa: E402

from open3d_slam_amd import parameters as prm  # noqa: E402
from open3d_slam_amd.optimization_problem import OptimizationProblem, OptimizedTransform, applyOptimizedTransforms  # noqa: E402
from open3d_slam_amd.place_recognition import Constraint  # noqa: E402


def _expm(A):
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ A / k
        out = out + term
    return out


def _random_pose(rng):
    v = rng.normal(size=6) * [0.5, 0.5, 0.5, 3, 3, 3]
    return rs.vector6_to_matrix4(v)


def test_jacobians_are_the_derivative_under_a_left_perturbation():
    rng = np.random.default_rng(0)
    for _ in range(5):
        X, Ts, Tt = _random_pose(rng), _random_pose(rng), _random_pose(rng)
        Js, Jt = rs.jacobian(np.linalg.inv(X), Ts, np.linalg.inv(Tt))
        h = 1e-5
        for i, G in enumerate(rs.JACOBIAN_OPERATOR):
            zs = [rs.misalignment(np.linalg.inv(X), _expm(s * h * G) @ Ts, np.linalg.inv(Tt)) for s in (1, -1)]
            zt = [rs.misalignment(np.linalg.inv(X), Ts, np.linalg.inv(_expm(s * h * G) @ Tt)) for s in (1, -1)]
            np.testing.assert_allclose((zs[0] - zs[1]) / (2 * h), Js[:, i], atol=1e-7)
            np.testing.assert_allclose((zt[0] - zt[1]) / (2 * h), Jt[:, i], atol=1e-7)
        assert np.array_equal(Jt, -Js)  # the generators enter negated: exact


def test_vector6_round_trip():
    v = np.array([0.1, -0.2, 0.3, 1.0, 2.0, -3.0])
    np.testing.assert_allclose(rs.matrix4_to_vector6(rs.vector6_to_matrix4(v)), v, atol=1e-15)


def test_consistent_odometry_chain_stops_at_once():
    G, _, E = rs.figure_eight_graph(n_nodes=12, drift_yaw=0.0, drift_fwd=0.0)
    odo = [e for e in E if not e.uncertain]
    r = rs.global_optimization(G, odo, option=rs.Option(1.0, 0.2, 2.0, 0))
    assert r["valid"] == 1
    for p in r["passes"]:
        assert p["iterations"] == 0 and p["lm_steps"] == 0 and p["stop_reason"] == rs.STOP_RIGHT_TERM
        assert p["residual"] < 1e-12
    np.testing.assert_allclose(r["poses"], G, atol=1e-12)


def test_outlier_loop_closure_is_pruned_and_drift_drops():
    G, T0, E = rs.figure_eight_graph()
    r = rs.global_optimization(T0, E, option=rs.Option(1.0, 0.2, 2.0, 0))
    assert r["kept"][:-1].all() and not r["kept"][-1]
    assert r["confidence"][-1] <= 0.2 and (r["confidence"][-4:-1] > 0.9).all()
    assert (r["confidence"][:-4] == 1.0).all()
    assert rs.drift(r["poses"], G) < rs.drift(T0, G) / 8


@pytest.mark.parametrize("ref", [-1, 0, 7, 11])
def test_reference_node_keeps_its_pose(ref):
    G, T0, E = rs.figure_eight_graph(n_nodes=12)
    r = rs.global_optimization(T0, E, option=rs.Option(1.0, 0.2, 2.0, ref))
    if ref >= 0:
        np.testing.assert_allclose(r["poses"][ref], T0[ref], atol=1e-12)
    else:
        assert not np.allclose(r["poses"][0], T0[0], atol=1e-6)


def test_invalid_graphs_are_returned_unchanged():
    G, T0, E = rs.figure_eight_graph(n_nodes=6)
    r = rs.global_optimization(T0, E[1:5], option=rs.Option())  # node 0 unreachable
    assert r["valid"] == 0 and np.array_equal(r["poses"], T0)
    E2 = [rs.Edge(e.source, e.target, e.transformation, e.information, e.uncertain, 0.5 if k == 0 else 1.0) for k, e in enumerate(E)]
    assert rs.global_optimization(T0, E2)["valid"] == 0
    with pytest.raises(ValueError):
        rs.global_optimization(T0, [rs.Edge(0, 9, np.eye(4), np.eye(6))])


# ---- OptimizationProblem --------------------------------------------------------------------------------------------------------
class _HostBackend:
    """global_optimization through the restatement (the graph logic under test is the host's)"""

    def global_optimization(self, poses, edges, max_correspondence_distance, edge_prune_threshold, preference_loop_closure, reference_node):
        E = [rs.Edge(s, t, np.array(X), np.array(I), bool(u), c) for s, t, X, I, u, c in edges]
        r = rs.global_optimization(poses, E, option=rs.Option(max_correspondence_distance, edge_prune_threshold, preference_loop_closure,
                                                              reference_node))
        return dict(poses=r["poses"], kept=r["kept"], confidence=r["confidence"], valid=bool(r["valid"]))


def _c(s, t, T, loop=False):
    return Constraint(sourceToTarget_=T, sourceSubmapIdx_=s, targetSubmapIdx_=t, informationMatrix_=np.eye(6) * 100.0,
                      isInformationMatrixValid_=True, isOdometryConstraint_=not loop)


def test_optimization_problem_builds_the_references_graph_over_two_builds():
    p = prm.MapperParameters()
    assert (p.globalOptimization_.maxCorrespondenceDistance_, p.globalOptimization_.loopClosurePreference_,
            p.globalOptimization_.edgePruneThreshold_, p.globalOptimization_.referenceNode_) == (10.0, 2.0, 0.2, 0)
    assert prm.lua_global_optimization_parameters().maxCorrespondenceDistance_ == 1000.0
    op = OptimizationProblem(_HostBackend(), p)
    step = rs.rz(0.1)
    step[0, 3] = 1.0
    op.insertOdometryConstraints([_c(1, 2, step), _c(0, 1, step)])  # out of order: the sort puts (0, 1) first
    op.buildOptimizationProblem()
    g = op.poseGraph_
    assert [(e.source_node_id_, e.target_node_id_, e.uncertain_) for e in g.edges_] == [(0, 1, False), (1, 2, False)]
    assert len(g.nodes_) == 3
    np.testing.assert_allclose(g.nodes_[0].pose_, np.eye(4))
    np.testing.assert_allclose(g.nodes_[2].pose_, np.linalg.inv(step @ step), atol=1e-15)
    op.solve()
    assert len(op.poseGraphOptimized_.edges_) == 2 and len(op.poseGraphNonOptimized_.nodes_) == 3
    inc = op.getOptimizedTransformIncrements()
    assert [t.submapId_ for t in inc] == [0, 1, 2]
    np.testing.assert_allclose(inc[2].dT_, op.poseGraphOptimized_.nodes_[2].pose_)  # the "increment" is the absolute pose
    # second build: nodes accumulate, the chain continues from the last optimised node over the new constraints only
    op.addOdometryConstraint(_c(2, 3, step))
    op.insertLoopClosureConstraints([_c(3, 0, np.eye(4), loop=True), _c(3, 0, np.eye(4), loop=True)])
    op.insertLoopClosureConstraints([_c(3, 0, rs.rz(0.5), loop=True)])  # (3, 0) is held already
    assert len(op.getLoopClosureConstraints()) == 1  # de-duplicated on (source, target), within one insertion too
    op.clearLoopClosureConstraints()
    op.addLoopClosureConstraint(_c(3, 1, np.eye(4), loop=True))
    last = op.poseGraphOptimized_.nodes_[-1].pose_.copy()
    op.buildOptimizationProblem()
    g = op.poseGraph_
    assert len(g.nodes_) == 4
    np.testing.assert_allclose(g.nodes_[3].pose_, np.linalg.inv(step @ np.linalg.inv(last)), atol=1e-12)
    assert [(e.source_node_id_, e.target_node_id_, e.uncertain_) for e in g.edges_] == [(0, 1, False), (1, 2, False), (2, 3, False),
                                                                                         (3, 1, True)]
    op.updateLoopClosureConstraint(0, _c(3, 2, np.eye(4), loop=True))
    assert op.getLoopClosureConstraints()[0].targetSubmapIdx_ == 2
    op.clearOdometryConstraints()
    assert op.odometryConstraints_ == [] and op.numOdometryEdgesPrev_ == 3
    with pytest.raises(RuntimeError):
        bad = OptimizationProblem(_HostBackend())
        bad.addLoopClosureConstraint(_c(0, 3, np.eye(4), loop=True))  # a loop closure must point backwards
        bad.buildOptimizationProblem()


class _StubSubmap:
    def __init__(self, parent):
        self.parentId_ = parent
        self.moves = []

    def transform(self, T):
        self.moves.append(np.array(T))


def test_apply_optimized_transforms_walks_up_the_parents():
    subs = [_StubSubmap(p) for p in (0, 0, 1, 2, 3, 1)]  # 0..2 in the graph; 3 -> 2; 4 -> 3 -> 2; 5 -> 1
    inc = [OptimizedTransform(rs.rz(0.1 * (k + 1)), k) for k in range(3)] + [OptimizedTransform(np.eye(4), 9)]  # 9: no such submap
    applyOptimizedTransforms(subs, inc)
    for k in range(3):
        assert len(subs[k].moves) == 1 and np.array_equal(subs[k].moves[0], inc[k].dT_)
    assert np.array_equal(subs[3].moves[0], inc[2].dT_) and np.array_equal(subs[4].moves[0], inc[2].dT_)
    assert np.array_equal(subs[5].moves[0], inc[1].dT_)
    loop = [_StubSubmap(0), _StubSubmap(2), _StubSubmap(2)]  # 1 -> 2 -> 2: neither in the graph
    with pytest.raises(RuntimeError, match="Stuck in a loop"):
        applyOptimizedTransforms(loop, [OptimizedTransform(np.eye(4), 0)])
