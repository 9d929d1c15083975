"""Loop closure's back half: OptimizationProblem (include/open3d_slam/OptimizationProblem.hpp, src/OptimizationProblem.cpp), the
constraint builders (src/constraint_builders.cpp:33-90) and the submap update of SubmapCollection::transform
(src/SubmapCollection.cpp:284-330).  The pose graph lives on the host, as Open3D's PoseGraph does; OptimizationProblem.solve runs
GlobalOptimization on the device (o3ds_global_optimization).  The reference's quirks are kept and marked where they are odd.
Candidate selection and the cycle that calls this are submap_collection.py and loop_closure.py; the PoseGraph JSON dump is not
modelled (DESIGN.md sections 7.2, 7.3)."""
from __future__ import annotations

import copy
import dataclasses
import functools

import numpy as np

from . import backend as _b
from .parameters import MapperParameters
from .place_recognition import (ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS, VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION,
                                VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO, Constraint, getMapVoxelSize)
from .pointcloud import PointCloud

VOXEL_EXPANSION_FACTOR_ICP_CORRESPONDENCE_DISTANCE = 1.5  # magic.hpp:15


@dataclasses.dataclass
class PoseGraphNode:  # [O3D] PoseGraphNode
    pose_: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(4))


@dataclasses.dataclass
class PoseGraphEdge:  # [O3D] PoseGraphEdge
    source_node_id_: int = -1
    target_node_id_: int = -1
    transformation_: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(4))
    information_: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(6))
    uncertain_: bool = False
    confidence_: float = 1.0


@dataclasses.dataclass
class PoseGraph:  # [O3D] PoseGraph
    nodes_: list = dataclasses.field(default_factory=list)
    edges_: list = dataclasses.field(default_factory=list)


@dataclasses.dataclass
class OptimizedTransform:  # Constraint.hpp:26-29
    dT_: np.ndarray
    submapId_: int


def _odometry_order(c1: Constraint, c2: Constraint) -> bool:
    # OptimizationProblem.cpp:65: the reference sorts with `c1.sourceSubmapIdx_ < c2.targetSubmapIdx_` -- source against TARGET, not a
    # strict weak ordering.  For odometry chains (target = source + 1) it orders by source; read as a three-way comparison below.
    return c1.sourceSubmapIdx_ < c2.targetSubmapIdx_


def _cmp(a, b) -> int:
    ab, ba = _odometry_order(a, b), _odometry_order(b, a)
    return -1 if ab and not ba else (1 if ba and not ab else 0)


class OptimizationProblem:
    def __init__(self, be, params: MapperParameters | None = None):
        self.be = be
        self.params_ = params if params is not None else MapperParameters()
        self.poseGraph_ = PoseGraph()
        self.poseGraphOptimized_ = PoseGraph()
        self.poseGraphNonOptimized_ = PoseGraph()
        self.odometryConstraints_: list = []
        self.loopClosureConstraints_: list = []
        self.numOdometryEdgesPrev_ = 0
        self.numLoopClosuresPrev_ = 0
        self.lastResult = None  # the o3ds_global_optimization result of the last solve (diagnostics)

    def setParameters(self, p: MapperParameters):
        self.params_ = p

    # -- constraints (OptimizationProblem.cpp:145-188)
    def addOdometryConstraint(self, c: Constraint):
        self.odometryConstraints_.append(c)

    def addLoopClosureConstraint(self, c: Constraint):
        self.loopClosureConstraints_.append(c)

    def insertOdometryConstraints(self, cs):
        self.odometryConstraints_.extend(cs)

    def insertLoopClosureConstraints(self, cs):
        for c in cs:  # de-duplicated on (source, target) against what is held, including what this call has just added
            if not any(c.sourceSubmapIdx_ == c2.sourceSubmapIdx_ and c.targetSubmapIdx_ == c2.targetSubmapIdx_ for c2 in self.loopClosureConstraints_):
                self.loopClosureConstraints_.append(c)

    def clearOdometryConstraints(self):
        self.odometryConstraints_.clear()

    def clearLoopClosureConstraints(self):
        self.loopClosureConstraints_.clear()

    def getLoopClosureConstraints(self) -> list:
        return self.loopClosureConstraints_

    def updateLoopClosureConstraint(self, idx: int, c: Constraint):
        self.loopClosureConstraints_[idx] = c

    # -- the graph (OptimizationProblem.cpp:50-120)
    def buildOptimizationProblem(self, submaps=None):
        """Clears the EDGES only: nodes accumulate across builds (the reference never clears poseGraph_.nodes_)."""
        self.poseGraph_.edges_.clear()
        self.setupOdometryEdgesAndPoseGraphNodes()
        self.setupLoopClosureEdges()

    def setupOdometryEdgesAndPoseGraphNodes(self):
        self.odometryConstraints_.sort(key=functools.cmp_to_key(_cmp))
        for c in self.odometryConstraints_:
            if not c.targetSubmapIdx_ > c.sourceSubmapIdx_:
                raise RuntimeError("id_source should always be less than id_target for the odometry constraints")
            self.poseGraph_.edges_.append(PoseGraphEdge(c.sourceSubmapIdx_, c.targetSubmapIdx_, np.array(c.sourceToTarget_, dtype=np.float64),
                                                        np.array(c.informationMatrix_, dtype=np.float64), uncertain_=False))
        if len(self.poseGraphOptimized_.edges_) > 0:
            # a later build continues the chain from the last OPTIMISED node, and only over the odometry constraints added since
            odometry = np.linalg.inv(self.poseGraphOptimized_.nodes_[-1].pose_)
        else:
            self.poseGraph_.nodes_.append(PoseGraphNode(np.eye(4)))
            odometry = np.eye(4)
        for i in range(self.numOdometryEdgesPrev_, len(self.odometryConstraints_)):
            odometry = np.array(self.odometryConstraints_[i].sourceToTarget_, dtype=np.float64) @ odometry
            self.poseGraph_.nodes_.append(PoseGraphNode(np.linalg.inv(odometry)))
        self.numOdometryEdgesPrev_ = len(self.odometryConstraints_)

    def setupLoopClosureEdges(self):
        self.numLoopClosuresPrev_ = len(self.loopClosureConstraints_)
        for c in self.loopClosureConstraints_:
            if not c.isInformationMatrixValid_:
                raise RuntimeError(f"Invalid information matrix between: {c.sourceSubmapIdx_} and {c.targetSubmapIdx_}")
            if not c.sourceSubmapIdx_ > c.targetSubmapIdx_:
                raise RuntimeError("Optimization problem, loop closure constraints: ")
            self.poseGraph_.edges_.append(PoseGraphEdge(c.sourceSubmapIdx_, c.targetSubmapIdx_, np.array(c.sourceToTarget_, dtype=np.float64),
                                                        np.array(c.informationMatrix_, dtype=np.float64), uncertain_=True))

    # -- solve (OptimizationProblem.cpp:26-44)
    def solve(self):
        p = self.params_.globalOptimization_
        self.poseGraphNonOptimized_ = copy.deepcopy(self.poseGraph_)
        g = self.poseGraph_
        r = self.be.global_optimization(
            [n.pose_ for n in g.nodes_], [(e.source_node_id_, e.target_node_id_, e.transformation_, e.information_, e.uncertain_, e.confidence_)
                                         for e in g.edges_],
            max_correspondence_distance=p.maxCorrespondenceDistance_, edge_prune_threshold=p.edgePruneThreshold_,
            preference_loop_closure=p.loopClosurePreference_, reference_node=p.referenceNode_)
        self.lastResult = r
        if r["valid"] and len(g.nodes_) > 1:
            # GlobalOptimization assigns the pruned graph back: the kept edges with their final confidences, the new poses
            for node, T in zip(g.nodes_, r["poses"]):
                node.pose_ = np.array(T)
            for e, c in zip(g.edges_, r["confidence"]):
                e.confidence_ = float(c)
            g.edges_ = [e for e, k in zip(g.edges_, r["kept"]) if k]
        self.poseGraphOptimized_ = copy.deepcopy(g)

    def getOptimizedTransformIncrements(self) -> list:
        """OptimizationProblem.cpp:167-178: the "increment" is the optimised node's ABSOLUTE pose (deltaT = tNew)."""
        if len(self.poseGraphOptimized_.nodes_) != len(self.poseGraph_.nodes_):
            raise RuntimeError("Graphs are not of same size, did you run the optimization?")
        return [OptimizedTransform(np.array(self.poseGraphOptimized_.nodes_[i].pose_), i) for i in range(len(self.poseGraph_.nodes_))]


def applyOptimizedTransforms(submaps, transformIncrements) -> None:
    """SubmapCollection::transform (SubmapCollection.cpp:284-330) over `submaps` (indexable by id, each with parentId_ and transform):
    every submap in the graph moves by its increment; every other one by the increment of its first ancestor (walking parentId_) that
    is in the graph -- looked up by POSITION in transformIncrements, as the reference's .at(currentNode) does."""
    optimized = []
    for update in transformIncrements:
        if update.submapId_ < len(submaps):
            submaps[update.submapId_].transform(update.dT_)
            optimized.append(update.submapId_)
        else:
            print(f"tying to update submap: {update.submapId_} but the there are only: {len(submaps)}submaps!!!! This should not happen!")
    optimized.sort()
    toUpdate = sorted(set(range(len(submaps))) - set(optimized))
    for idx in toUpdate:
        current = idx
        while transformIncrements:
            current = submaps[current].parentId_
            if current not in toUpdate:  # the parent is in the pose graph
                submaps[idx].transform(transformIncrements[current].dT_)
                break
            if current == submaps[current].parentId_:
                raise RuntimeError("Stuck in a loop, this should not happen")


def buildConstraint(be, sourceIdx: int, targetIdx: int, submaps, params: MapperParameters, isComputeOverlap: bool,
                    icpMaxCorrespondenceDistance: float, voxelSizeOverlapCompute: float, isEstimateInformationMatrix: bool,
                    isSkipIcpRefinement: bool) -> Constraint:
    """constraint_builders.cpp:45-90 on the device: the overlap crop at identity (o3ds_overlap_indices), point-to-plane ICP run to
    convergence (the target map needs normals) and the information matrix."""
    source = submaps[sourceIdx].getMapPointCloud()
    target = submaps[targetIdx].getMapPointCloud()
    held = []
    try:
        if isComputeOverlap:
            i_s, i_t = be.overlap_indices(source.id, target.id, np.eye(4), voxelSizeOverlapCompute, 1)
            source = PointCloud(be, be.select_by_index(source.id, i_s.astype(np.uint32)))
            target = PointCloud(be, be.select_by_index(target.id, i_t.astype(np.uint32)))
            held = [source, target]
        T = np.eye(4)
        if not isSkipIcpRefinement:
            r = be.icp_point_to_plane_dev(source.id, target.id, icpMaxCorrespondenceDistance, init=np.eye(4),
                                          max_iter=ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS)
            T = np.array(r["transformation"])
        info = np.eye(6)
        if isEstimateInformationMatrix:
            info = be.information_matrix_dev(source.id, target.id, icpMaxCorrespondenceDistance, T)
    finally:
        for c in held:
            c.release()
    return Constraint(sourceToTarget_=T, sourceSubmapIdx_=sourceIdx, targetSubmapIdx_=targetIdx, informationMatrix_=info,
                      isInformationMatrixValid_=isEstimateInformationMatrix, isOdometryConstraint_=True)


def buildConstraintsBatch(be, pairs, submaps, params: MapperParameters, isComputeOverlap: bool, icpMaxCorrespondenceDistance: float,
                          voxelSizeOverlapCompute: float, isEstimateInformationMatrix: bool) -> list:
    """buildConstraint with ICP refinement for every (sourceIdx, targetIdx) of `pairs`, the registrations in ONE device call
    (o3ds_icp_register_batch, a capability beyond the reference): the overlap crops of all pairs first, one batch of point-to-plane
    ICPs from identity, then the information matrices in order.  Every entry is its one-pair registration bit for bit, so the
    constraints are those of buildConstraint called pair by pair."""
    held, clouds = [], []
    try:
        for sourceIdx, targetIdx in pairs:
            source = submaps[sourceIdx].getMapPointCloud()
            target = submaps[targetIdx].getMapPointCloud()
            if isComputeOverlap:
                i_s, i_t = be.overlap_indices(source.id, target.id, np.eye(4), voxelSizeOverlapCompute, 1)
                source = PointCloud(be, be.select_by_index(source.id, i_s.astype(np.uint32)))
                held.append(source)
                target = PointCloud(be, be.select_by_index(target.id, i_t.astype(np.uint32)))
                held.append(target)
            clouds.append((source, target))
        p = be._params(icpMaxCorrespondenceDistance, ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS, 1e-6, 1e-6, _b.ICP_POINT_TO_PLANE)
        results, status = be.icp_register_batch([(s.id, t.id, None, np.eye(4)) for s, t in clouds], p, split=True)
        for k, st in enumerate(status):
            if st != 0:
                raise _b.BackendError(st, f"buildConstraintsBatch: the registration of pair {pairs[k]} did not run")
        out = []
        for (sourceIdx, targetIdx), (source, target), r in zip(pairs, clouds, results):
            T = np.array(r["transformation"])
            info = np.eye(6)
            if isEstimateInformationMatrix:
                info = be.information_matrix_dev(source.id, target.id, icpMaxCorrespondenceDistance, T)
            out.append(Constraint(sourceToTarget_=T, sourceSubmapIdx_=sourceIdx, targetSubmapIdx_=targetIdx, informationMatrix_=info,
                                  isInformationMatrixValid_=isEstimateInformationMatrix, isOdometryConstraint_=True))
        return out
    finally:
        for c in held:
            c.release()


def buildOdometryConstraintsBatch(be, pairs, submaps, params: MapperParameters) -> list:
    """buildOdometryConstraint for every pair; with isRefineOdometryConstraintsBetweenSubmaps_ the pairs' ICPs go in one batch."""
    pairs = list(pairs)
    if not pairs:
        return []
    if not params.isRefineOdometryConstraintsBetweenSubmaps_:  # nothing to batch: the per-pair form
        return [buildOdometryConstraint(be, s, t, submaps, params) for s, t in pairs]
    v = getMapVoxelSize(params.mapBuilder_, VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO)
    return buildConstraintsBatch(be, pairs, submaps, params, True, VOXEL_EXPANSION_FACTOR_ICP_CORRESPONDENCE_DISTANCE * v,
                                 VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION * v, True)


def buildOdometryConstraint(be, sourceIdx: int, targetIdx: int, submaps, params: MapperParameters) -> Constraint:
    """constraint_builders.cpp:33-43."""
    v = getMapVoxelSize(params.mapBuilder_, VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO)
    c = buildConstraint(be, sourceIdx, targetIdx, submaps, params, True, VOXEL_EXPANSION_FACTOR_ICP_CORRESPONDENCE_DISTANCE * v,
                        VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION * v, True, not params.isRefineOdometryConstraintsBetweenSubmaps_)
    c.isOdometryConstraint_ = True
    return c
