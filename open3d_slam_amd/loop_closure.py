"""SlamWrapper's loop-closure sequence (src/SlamWrapper.cpp:386-485) run synchronously, in the order its workers run it: features of the
finished submaps and their odometry constraints (computeFeaturesIfReady, attemptLoopClosuresIfReady), the loop-closure constraints and
the pose graph (loopClosureWorker), the submaps and the mapper's pose moved by the solution (updateSubmapsAndTrajectory).  The threads
and the wall-clock throttle of the feature computation are not modelled; the RANSAC seed is the collection's (fixed), so one cycle is
a function of its inputs."""
from __future__ import annotations

import dataclasses

import numpy as np

from .optimization_problem import OptimizationProblem
from .submap_collection import computeOdometryConstraints


class LoopClosure:
    def __init__(self, be, mapper, params=None, batchRegistrations: bool = False):
        """mapper: a Mapper built with submaps=SubmapCollection(...); params: its MapperParameters (default: the mapper's).
        batchRegistrations: the independent ICPs of a cycle -- the refinements of a finished submap's loop-closure candidates, the
        odometry constraints -- run as batched registrations (PlaceRecognition.batchRefinement, computeOdometryConstraints(batch=True));
        the constraints are the same.  Off by default: the call sequence of the reference."""
        if mapper.getSubmaps() is None:
            raise ValueError("LoopClosure needs a Mapper that maps into a SubmapCollection")
        self.be = be
        self.mapper_ = mapper
        self.submaps_ = mapper.getSubmaps()
        self.params_ = params if params is not None else mapper.params_
        self.optimizationProblem_ = OptimizationProblem(be, self.params_)
        self.loopClosureCandidates_: list = []
        self.lastLoopClosureConstraints_: list = []
        self.numLatestLoopClosureConstraints_ = 0
        self.isOptimizedGraphAvailable_ = False
        self.batchRegistrations = bool(batchRegistrations)
        if self.batchRegistrations:
            self.submaps_.placeRecognition_.batchRefinement = True
        self.lastIncrement = None  # the dT handed to Mapper.loopClosureUpdate by the last update (diagnostics)

    def computeFeaturesIfReady(self):  # SlamWrapper.cpp:386-393
        if self.submaps_.numFinishedSubmaps() > 0:
            self.submaps_.computeFeatures(self.submaps_.popFinishedSubmapIds(), batch=self.batchRegistrations)

    def attemptLoopClosuresIfReady(self):  # SlamWrapper.cpp:394-404
        if self.submaps_.numLoopClosureCandidates() > 0:
            self.loopClosureCandidates_.extend(self.submaps_.popLoopClosureCandidates())

    def loopClosureWorker(self) -> list:
        """One pass of SlamWrapper.cpp:406-449: the constraints of the queued candidates; with any, the pose graph over them and the
        odometry constraints (the collection's, then those of every pair that does not touch the active submap) is built and solved."""
        if not self.loopClosureCandidates_ or self.isOptimizedGraphAvailable_:
            return []
        lcc, self.loopClosureCandidates_ = self.loopClosureCandidates_, []
        loopClosureConstraints = self.submaps_.buildLoopClosureConstraints(lcc)
        self.numLatestLoopClosureConstraints_ = len(loopClosureConstraints)
        if not loopClosureConstraints:
            return []
        odometryConstraints = list(self.submaps_.getOdometryConstraints())
        computeOdometryConstraints(self.be, self.submaps_, odometryConstraints, batch=self.batchRegistrations)
        op = self.optimizationProblem_
        op.clearOdometryConstraints()
        op.insertLoopClosureConstraints(loopClosureConstraints)
        op.insertOdometryConstraints(odometryConstraints)
        op.buildOptimizationProblem(self.submaps_)
        op.solve()
        self.lastLoopClosureConstraints_ = loopClosureConstraints
        self.isOptimizedGraphAvailable_ = True
        return loopClosureConstraints

    def updateSubmapsAndTrajectory(self):
        """SlamWrapper.cpp:451-485: the submaps move by the optimised increments; the mapper's pose by the increment of the source submap
        of the latest loop-closure constraint (by timestamp, the first of equal ones); the loop-closure constraints are reset to identity
        and enter the adjacency matrix."""
        op = self.optimizationProblem_
        increments = op.getOptimizedTransformIncrements()
        self.submaps_.transform(increments)
        latest = max(self.lastLoopClosureConstraints_, key=lambda c: c.timestamp_)
        if not latest.sourceSubmapIdx_ > latest.targetSubmapIdx_:
            raise RuntimeError("Wrapper ros, update submaps and trajectory: ")
        dT = increments[latest.sourceSubmapIdx_].dT_
        self.mapper_.loopClosureUpdate(dT)
        self.lastIncrement = np.array(dT)
        constraints = op.getLoopClosureConstraints()
        for i, old in enumerate(list(constraints)):
            op.updateLoopClosureConstraint(i, dataclasses.replace(old, sourceToTarget_=np.eye(4)))
        self.submaps_.updateAdjacencyMatrix(op.getLoopClosureConstraints())
        self.isOptimizedGraphAvailable_ = False

    def run(self) -> list:
        """The whole cycle once: returns the loop-closure constraints built (empty: nothing was closed and nothing moved).  Does nothing
        when isAttemptLoopClosures_ is off."""
        if not self.params_.isAttemptLoopClosures_:
            return []
        self.computeFeaturesIfReady()
        self.attemptLoopClosuresIfReady()
        constraints = self.loopClosureWorker()
        if self.isOptimizedGraphAvailable_:
            self.updateSubmapsAndTrajectory()
        return constraints
