"""SubmapCollection (include/open3d_slam/SubmapCollection.hpp, src/SubmapCollection.cpp): the submaps of one mapping session -- a new
one every submaps_.radius_ metres, the finished ones queued for features, loop-closure candidates picked among them
(PlaceRecognition::getLoopClosureCandidatesIdxs, PlaceRecognition.cpp:231-283) and every submap moved once the pose graph is solved.

Everything that touches a map runs on the device through the existing entry points (map insertion and carving, the centre, the voxel
map of the switch check, features, RANSAC, ICP, the information matrix, the transforms); only centres, counts, poses and constraints
come back to the host.  The overlap ring holds the pre-processed scans themselves (PointCloud.retain()), not copies.  The reference's
worker threads are not modelled: loop_closure.py runs their sequence in one thread."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from .adjacency_matrix import AdjacencyMatrix
from .optimization_problem import applyOptimizedTransforms, buildOdometryConstraint, buildOdometryConstraintsBatch
from .parameters import MapperParameters
from .place_recognition import PlaceRecognition
from .pointcloud import PointCloud
from .submap import Submap


@dataclasses.dataclass
class TimestampedSubmapId:  # typedefs.hpp: TimestampedSubmapId {submapId_, time_}
    submapId_: int
    time_: float


@dataclasses.dataclass
class ScanTimeTransform:  # SubmapCollection.hpp:26-30
    cloud_: PointCloud
    timestamp_: float
    mapToRangeSensor_: np.ndarray


def _hasConstraint(sourceIdx: int, targetIdx: int, constraints) -> bool:  # constraint_builders.cpp:23-30
    return any(c.sourceSubmapIdx_ == sourceIdx and c.targetSubmapIdx_ == targetIdx for c in constraints)


def computeOdometryConstraints(be, submaps: "SubmapCollection", constraints: list, candidates=None, batch: bool = False) -> None:
    """constraint_builders.cpp:92-118.  candidates given: the odometry constraint (parent -> submap) of every candidate but submap 0
    (the form SubmapCollection::computeFeatures uses); None: of every submap 1..N-1 whose pair does not touch the active submap (the
    form of the loop-closure worker).  Constraints already in `constraints` (same source and target) are not built again.
    batch (a capability beyond the reference, off by default): the pairs are collected first and, with
    isRefineOdometryConstraintsBetweenSubmaps_, their ICPs run as one batched registration; the constraints appended are the same."""
    params = submaps.getParameters()
    pairs = []  # batch: the (source, target) pairs in the order the loop below would build them

    def build(source, target):
        if batch:
            if (source, target) not in pairs:  # (the sequential form sees its own earlier constraint in `constraints`)
                pairs.append((source, target))
        else:
            constraints.append(buildOdometryConstraint(be, source, target, submaps.submaps_, params))

    if candidates is not None:
        for candidate in candidates:
            if candidate.submapId_ < 1:
                continue
            target = candidate.submapId_
            source = submaps.getSubmap(target).parentId_
            if not _hasConstraint(source, target, constraints):
                build(source, target)
    else:
        active = submaps.getActiveSubmap().id_
        for target in range(1, submaps.getNumSubmaps()):
            source = submaps.getSubmap(target).parentId_
            if not _hasConstraint(source, target, constraints) and source != active and target != active:
                build(source, target)
    if batch:
        constraints.extend(buildOdometryConstraintsBatch(be, pairs, submaps.submaps_, params))


def getLoopClosureCandidatesIdxs(submaps, adjMatrix: AdjacencyMatrix, lastFinishedSubmapIdx: int, activeSubmapIdx: int,
                                 params: MapperParameters) -> list:
    """PlaceRecognition::getLoopClosureCandidatesIdxs (PlaceRecognition.cpp:231-283), its six filters in the reference's order.  `submaps`:
    a list indexed by submap index, each with id_ and getMapToSubmapCenter()."""
    idxs = []
    n = len(submaps)
    lastCenter = np.asarray(submaps[lastFinishedSubmapIdx].getMapToSubmapCenter(), dtype=np.float64)
    maxDistance = params.placeRecognition_.loopClosureSearchRadius_
    for i in range(n):
        if i == activeSubmapIdx:  # 1. the active submap
            continue
        if adjMatrix.isAdjacent(submaps[i].id_, submaps[activeSubmapIdx].id_):  # 2. adjacent to the active one (by id)
            continue
        if abs(i - lastFinishedSubmapIdx) == 1 or adjMatrix.isAdjacent(i, lastFinishedSubmapIdx):  # 3. next to the finished one
            continue
        center = np.asarray(submaps[i].getMapToSubmapCenter(), dtype=np.float64)
        if np.linalg.norm(lastCenter - center) > maxDistance:  # 4. too far
            continue
        consecutiveThreshold = int(math.ceil(maxDistance / params.submaps_.radius_))
        if abs(i - lastFinishedSubmapIdx) <= consecutiveThreshold:  # 5. consecutive
            continue
        if adjMatrix.getDistanceToNearestLoopClosureSubmap(lastFinishedSubmapIdx) < params.placeRecognition_.minSubmapsBetweenLoopClosures_:
            continue  # 6. a loop was closed too few submaps ago
        idxs.append(i)
    return idxs


class SubmapCollection:
    def __init__(self, be, params: MapperParameters | None = None, seed: int = 0):
        """seed: the RANSAC draws of place recognition (fixed, so that a loop-closure cycle is a function of its inputs)."""
        self.be = be
        self.mapToRangeSensor_ = np.eye(4)
        self.timestamp_ = 0.0
        self.submaps_: list[Submap] = []
        self.activeSubmapIdx_ = 0
        self.params_ = MapperParameters()
        self.numScansMergedInActiveSubmap_ = 0
        self.lastFinishedSubmapIdx_ = 0
        self.adjacencyMatrix_ = AdjacencyMatrix()
        self.submapId_ = 0
        self.placeRecognition_ = PlaceRecognition(be, self.params_, seed=seed)
        self.loopClosureCandidatesIdxs_: list[TimestampedSubmapId] = []
        self.finishedSubmapsIdxs_: list[TimestampedSubmapId] = []
        self.odometryConstraints_: list = []
        self.overlapScansBuffer_: list[ScanTimeTransform] = []
        self.overlapScansBufferLimit_ = 5  # SubmapCollection.cpp:31, until setParameters
        self.isForceNewSubmapCreation_ = False
        self.createNewSubmap(self.mapToRangeSensor_)  # SubmapCollection.cpp:28-32: submap 0 exists before the first scan
        self.setParameters(params if params is not None else MapperParameters())

    # -- accessors (SubmapCollection.cpp:34-81)
    def setMapToRangeSensor(self, T):
        self.mapToRangeSensor_ = np.array(T, dtype=np.float64)

    def isEmpty(self) -> bool:
        return not self.submaps_

    def getSubmap(self, idx: int) -> Submap:
        return self.submaps_[idx]

    def getSubmapPtr(self, idx: int) -> Submap:
        return self.submaps_[idx]

    def getNumSubmaps(self) -> int:
        return len(self.submaps_)

    def getActiveSubmap(self) -> Submap:
        return self.submaps_[self.activeSubmapIdx_]

    def getSubmapsForScanMatching(self, k: int) -> list:
        """The submaps one scan is registered against when the mapper is asked for more than the active one (a capability beyond the
        reference, which registers against the active submap only, Mapper.cpp:141): the active submap first, then up to k - 1 others
        among the non-empty submaps adjacent to it in the AdjacencyMatrix, the one whose centre is nearest to the sensor position
        (mapToRangeSensor_, what findClosestSubmap measures from) first; equally near: the lower id.  k <= 1: the active submap alone."""
        active = self.getActiveSubmap()
        out = [active]
        if k <= 1:
            return out
        p0 = np.asarray(self.mapToRangeSensor_, dtype=np.float64)[:3, 3]
        others = []
        for i, s in enumerate(self.submaps_):
            if i == self.activeSubmapIdx_ or s.isEmpty() or not self.adjacencyMatrix_.isAdjacent(s.id_, active.id_):
                continue
            others.append((float(np.linalg.norm(p0 - s.getMapToSubmapCenter())), s.id_, i))
        others.sort()
        return out + [self.submaps_[i] for _, _, i in others[:k - 1]]

    def getParameters(self) -> MapperParameters:
        return self.params_

    def getOdometryConstraints(self) -> list:
        return self.odometryConstraints_

    def popFinishedSubmapIds(self) -> list:
        out, self.finishedSubmapsIdxs_ = self.finishedSubmapsIdxs_, []
        return out

    def popLoopClosureCandidates(self) -> list:
        out, self.loopClosureCandidatesIdxs_ = self.loopClosureCandidatesIdxs_, []
        return out

    def numFinishedSubmaps(self) -> int:
        return len(self.finishedSubmapsIdxs_)

    def numLoopClosureCandidates(self) -> int:
        return len(self.loopClosureCandidatesIdxs_)

    def updateAdjacencyMatrix(self, loopClosureConstraints):
        for c in loopClosureConstraints:
            self.adjacencyMatrix_.addEdge(c.sourceSubmapIdx_, c.targetSubmapIdx_)
            self.adjacencyMatrix_.markAsLoopClosureSubmap(c.sourceSubmapIdx_)
            self.adjacencyMatrix_.markAsLoopClosureSubmap(c.targetSubmapIdx_)

    def setParameters(self, p: MapperParameters):  # SubmapCollection.cpp:209-217
        self.params_ = p
        for submap in self.submaps_:
            submap.setParameters(p)
        self.placeRecognition_.setParameters(p)
        if not p.submaps_.numScansOverlap_ > 0:
            raise RuntimeError("Num scan overlap has to be > 0")
        self.overlapScansBufferLimit_ = int(p.submaps_.numScansOverlap_)
        self._trimBuffer()

    # -- the overlap ring (CircularBuffer: push at the back, the oldest falls out at the front)
    def addScanToBuffer(self, scan: PointCloud, mapToRangeSensor, timestamp: float):
        self.overlapScansBuffer_.append(ScanTimeTransform(scan.retain(), timestamp, np.array(mapToRangeSensor, dtype=np.float64)))
        self._trimBuffer()

    def _trimBuffer(self):
        while len(self.overlapScansBuffer_) > self.overlapScansBufferLimit_:
            self.overlapScansBuffer_.pop(0).cloud_.release()

    def clearOverlapBuffer(self):
        while self.overlapScansBuffer_:
            self.overlapScansBuffer_.pop(0).cloud_.release()

    def insertBufferedScans(self, submap: Submap):  # SubmapCollection.cpp:87-92
        while self.overlapScansBuffer_:
            scan = self.overlapScansBuffer_.pop(0)
            submap.insertScan(scan.cloud_, scan.cloud_, scan.mapToRangeSensor_, scan.timestamp_, isPerformCarving=False)
            scan.cloud_.release()

    # -- switching (SubmapCollection.cpp:94-157, 352-364)
    def findClosestSubmap(self, mapToRangeSensor) -> int:
        """std::min_element with a strict `<` on the distance to each centre: the first of equally close submaps wins."""
        p0 = np.asarray(mapToRangeSensor, dtype=np.float64)[:3, 3]
        best, bestDistance = 0, None
        for i, s in enumerate(self.submaps_):
            d = np.linalg.norm(p0 - s.getMapToSubmapCenter())
            if bestDistance is None or d < bestDistance:
                best, bestDistance = i, d
        return best

    def isSwitchingSubmapsConsistant(self, scan: PointCloud, newActiveSubmapCandidate: int, mapToRangeSensor) -> bool:
        """hits / scan size > adjacencyBasedRevisitingMinFitness_ (strictly); the hits are counted on the device."""
        hits = self.submaps_[newActiveSubmapCandidate].countVoxelMapHits(scan, mapToRangeSensor)
        n = len(scan)
        fitness = hits / n if n else float("nan")  # (0 / 0 in the reference: NaN, and NaN > x is false)
        return fitness > self.params_.submaps_.adjacencyBasedRevisitingMinFitness_

    def updateActiveSubmap(self, mapToRangeSensor, scan: PointCloud):
        sp = self.params_.submaps_
        if self.isForceNewSubmapCreation_:
            self.createNewSubmap(self.mapToRangeSensor_)
            self.isForceNewSubmapCreation_ = False
            return
        if self.numScansMergedInActiveSubmap_ < sp.minNumRangeData_:
            return
        if self.params_.isUseInitialMap_:
            return
        closestMapIdx = self.findClosestSubmap(self.mapToRangeSensor_)
        closestSubmap = self.submaps_[closestMapIdx]
        activeSubmap = self.submaps_[self.activeSubmapIdx_]
        position = self.mapToRangeSensor_[:3, 3]
        isAnotherSubmapWithinRange = np.linalg.norm(position - closestSubmap.getMapToSubmapCenter()) < sp.radius_
        if isAnotherSubmapWithinRange:
            if closestMapIdx == self.activeSubmapIdx_:
                return
            if self.adjacencyMatrix_.isAdjacent(closestSubmap.id_, activeSubmap.id_) and \
                    self.isSwitchingSubmapsConsistant(scan, closestSubmap.id_, mapToRangeSensor):
                self.activeSubmapIdx_ = closestMapIdx
            else:
                isTraveledSufficientDistance = np.linalg.norm(position - activeSubmap.getMapToSubmapCenter()) > sp.radius_
                if isTraveledSufficientDistance:
                    self.createNewSubmap(self.mapToRangeSensor_)
        else:
            self.createNewSubmap(self.mapToRangeSensor_)

    def createNewSubmap(self, mapToSubmap):  # SubmapCollection.cpp:133-145
        submapId = self.submapId_
        self.submapId_ += 1
        submapParentId = self.activeSubmapIdx_
        newSubmap = Submap(self.be, submapId, submapParentId)
        newSubmap.setMapToSubmapOrigin(mapToSubmap)
        newSubmap.setParameters(self.params_)
        self.submaps_.append(newSubmap)
        self.activeSubmapIdx_ = len(self.submaps_) - 1
        self.numScansMergedInActiveSubmap_ = 0

    def forceNewSubmapCreation(self):  # SubmapCollection.cpp:163-170
        if not self.submaps_:
            return
        self.isForceNewSubmapCreation_ = True
        empty = PointCloud.from_numpy(self.be, np.zeros((0, 3)))
        try:
            self.insertScan(empty, empty, self.mapToRangeSensor_, self.timestamp_)
        finally:
            empty.release()
        self.isForceNewSubmapCreation_ = False

    def insertScan(self, rawScan: PointCloud, preProcessedScan: PointCloud, mapToRangeSensor, timestamp: float) -> bool:
        """SubmapCollection.cpp:172-207."""
        T = np.array(mapToRangeSensor, dtype=np.float64)
        self.mapToRangeSensor_ = T
        self.timestamp_ = timestamp
        if not self.submaps_:
            self.createNewSubmap(self.mapToRangeSensor_)
            self.submaps_[self.activeSubmapIdx_].insertScan(rawScan, preProcessedScan, T, timestamp, isPerformCarving=True)
            self.numScansMergedInActiveSubmap_ += 1
            return True
        self.addScanToBuffer(preProcessedScan, T, timestamp)
        prevActiveSubmapIdx = self.activeSubmapIdx_
        self.updateActiveSubmap(T, preProcessedScan)
        if prevActiveSubmapIdx != self.activeSubmapIdx_:
            prev = self.submaps_[prevActiveSubmapIdx]
            prev.insertScan(rawScan, preProcessedScan, T, timestamp, isPerformCarving=True)
            prev.computeSubmapCenter()
            self.lastFinishedSubmapIdx_ = prevActiveSubmapIdx
            self.finishedSubmapsIdxs_.append(TimestampedSubmapId(prevActiveSubmapIdx, timestamp))
            self.numScansMergedInActiveSubmap_ = 0
            self.adjacencyMatrix_.addEdge(prev.id_, self.submaps_[self.activeSubmapIdx_].id_)
            self.insertBufferedScans(self.submaps_[self.activeSubmapIdx_])
            if self.submaps_[self.activeSubmapIdx_].isEmpty():
                raise RuntimeError("submap should not be empty after switching")
        else:
            self.submaps_[self.activeSubmapIdx_].insertScan(rawScan, preProcessedScan, T, timestamp, isPerformCarving=True)
        self.numScansMergedInActiveSubmap_ += 1
        return True

    # -- loop closure (SubmapCollection.cpp:219-267, 284-335)
    def computeFeatures(self, finishedSubmapIds, batch: bool = False):
        for tid in finishedSubmapIds:
            self.submaps_[tid.submapId_].computeFeatures()
            self.loopClosureCandidatesIdxs_.append(tid)
        computeOdometryConstraints(self.be, self, self.odometryConstraints_, candidates=finishedSubmapIds, batch=batch)

    def getLoopClosureCandidatesIdxs(self, lastFinishedSubmapIdx: int) -> list:
        return getLoopClosureCandidatesIdxs(self.submaps_, self.adjacencyMatrix_, lastFinishedSubmapIdx, self.activeSubmapIdx_,
                                            self.placeRecognition_.params_)

    def buildLoopClosureConstraints(self, loopClosureCandidatesIdxs) -> list:
        """SubmapCollection.cpp:253-267 with PlaceRecognition::buildLoopClosureConstraints (PlaceRecognition.cpp:49-70): the candidates of
        every finished submap, then the existing per-candidate body."""
        retVal = []
        for tid in loopClosureCandidatesIdxs:
            idxs = self.getLoopClosureCandidatesIdxs(tid.submapId_)
            if not idxs:
                continue
            retVal.extend(self.placeRecognition_.buildLoopClosureConstraints(
                self.submaps_[tid.submapId_], [self.submaps_[i] for i in idxs], timestamp=tid.time_, sourceSubmapIdx=tid.submapId_,
                candidateIdxs=idxs))
        return retVal

    def transform(self, transformIncrements):
        """SubmapCollection.cpp:284-335: the submaps of the pose graph by their increments, every other one by that of its first ancestor
        in the graph (parentId_ walk); then the overlap ring is flushed."""
        applyOptimizedTransforms(self.submaps_, transformIncrements)
        self.clearOverlapBuffer()
