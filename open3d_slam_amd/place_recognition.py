"""PlaceRecognition (include/open3d_slam/PlaceRecognition.hpp, src/PlaceRecognition.cpp:38-226) over the HIP backend: loop-closure
constraints between a finished submap and candidate submaps, with every data-parallel step on the device -- FPFH features
(Submap.computeFeatures), feature correspondences and the RANSAC hypothesis search (o3ds_ransac_feature_matching), the overlap crop
(o3ds_overlap_indices), the ICP refinement and the information matrix.  Candidate selection (getLoopClosureCandidatesIdxs) is
submap_collection.py's, which passes the candidates here."""
from __future__ import annotations

import dataclasses

import numpy as np

from .cloud_registration import cloudRegistrationFactory
from .parameters import MapperParameters
from .pointcloud import PointCloud
from .scan_to_map_registration import toCloudRegistrationType

ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS = 100  # magic.hpp:13
VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION = 20.0     # magic.hpp:14
VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO = 0.04  # magic.hpp:12


@dataclasses.dataclass
class Constraint:  # Constraint.hpp:14-22
    sourceToTarget_: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(4))
    sourceSubmapIdx_: int = 0
    targetSubmapIdx_: int = 0
    informationMatrix_: np.ndarray = dataclasses.field(default_factory=lambda: np.eye(6))
    isInformationMatrixValid_: bool = False
    isOdometryConstraint_: bool = True
    timestamp_: float = 0.0


def toRPY(R) -> np.ndarray:
    """math.cpp:39-46 toRPY(Quaterniond(R)): the normalised quaternion of R, then roll / pitch / yaw as getRollFromQuat &c. (math.hpp:30-42)."""
    R = np.asarray(R, dtype=np.float64)[:3, :3]
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:  # Eigen's Quaternion from rotation matrix
        t = np.sqrt(tr + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        x, y, z = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = [0.0, 0.0, 0.0]
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
        x, y, z = q
    nq = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / nq, x / nq, y / nq, z / nq
    roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    pitch = np.arcsin(np.clip(2 * (w * y - x * z), -1.0, 1.0))
    yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return np.array([roll, pitch, yaw])


def isRegistrationConsistent(mat, p) -> bool:
    """PlaceRecognition::isRegistrationConsistent (PlaceRecognition.cpp:182-226): |roll|, |pitch|, |yaw| and |x|, |y|, |z| of the
    registration against the drift limits of PlaceRecognitionConsistencyCheckParameters `p`."""
    T = np.asarray(mat, dtype=np.float64)
    roll, pitch, yaw = toRPY(T)
    t = T[:3, 3]
    return not (abs(roll) > p.maxDriftRoll_ or abs(pitch) > p.maxDriftPitch_ or abs(yaw) > p.maxDriftYaw_ or abs(t[0]) > p.maxDriftX_
                or abs(t[1]) > p.maxDriftY_ or abs(t[2]) > p.maxDriftZ_)


def getMapVoxelSize(mapBuilder, valueIfZero: float) -> float:  # helpers.cpp:343-345
    return valueIfZero if abs(mapBuilder.mapVoxelSize_) <= 1e-3 else mapBuilder.mapVoxelSize_


class PlaceRecognition:
    def __init__(self, be, params: MapperParameters | None = None, seed: int = 0, batchRefinement: bool = False):
        """batchRefinement: refine the candidates that pass the RANSAC gates with ONE batched registration instead of one ICP per
        candidate (a capability beyond the reference; the constraints are the sequential form's, bit for bit).  Off by default."""
        self.be = be
        self.batchRefinement = bool(batchRefinement)
        self.seed = int(seed)  # RANSAC's draws (Open3D seeds from std::random_device; here the seed is the caller's)
        self.lastRansacResult = None  # the RANSAC result of the last candidate examined (diagnostics)
        self.setParameters(params if params is not None else MapperParameters())

    def setParameters(self, p: MapperParameters):  # PlaceRecognition.cpp:38-41
        self.params_ = dataclasses.replace(p)
        self.updateRegistrationAlgorithm(self.params_)

    def updateRegistrationAlgorithm(self, p: MapperParameters):  # PlaceRecognition.cpp:43-47
        sm = dataclasses.replace(p.scanMatcher_, icp_=dataclasses.replace(p.scanMatcher_.icp_))
        sm.icp_.maxNumIter_ = ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS
        sm.icp_.maxCorrespondenceDistance_ = p.placeRecognition_.maxIcpCorrespondenceDistance_
        self.params_ = dataclasses.replace(p, scanMatcher_=sm)
        self.cloudRegistration = cloudRegistrationFactory(toCloudRegistrationType(sm))

    def isRegistrationConsistent(self, mat) -> bool:
        return isRegistrationConsistent(mat, self.params_.placeRecognition_.consistencyCheck_)

    def ransac(self, sourceSubmap, targetSubmap) -> dict:
        """RegistrationRANSACBasedOnFeatureMatching of the two sparse maps (PlaceRecognition.cpp:77-84): mutual filter, point-to-point
        estimation, the distance and edge-length checkers, RANSACConvergenceCriteria(ransacNumIter_, ransacProbability_)."""
        cfg = self.params_.placeRecognition_
        return self.be.ransac_feature_matching(
            sourceSubmap.getSparseMapPointCloud().id, targetSubmap.getSparseMapPointCloud().id, cfg.ransacMaxCorrespondenceDistance_,
            ransac_n=cfg.ransacModelSize_, mutual=True, edge_length=cfg.correspondenceCheckerEdgeLength_,
            distance=cfg.correspondenceCheckerDistance_, max_iteration=cfg.ransacNumIter_, confidence=cfg.ransacProbability_, seed=self.seed)

    def buildLoopClosureConstraints(self, sourceSubmap, candidateSubmaps, timestamp: float = 0.0, sourceSubmapIdx: int | None = None,
                                    candidateIdxs=None) -> list:
        """The per-candidate body of PlaceRecognition::buildLoopClosureConstraints (PlaceRecognition.cpp:71-176).  Both submaps must
        have run computeFeatures; the map clouds need normals when the scan matcher is point-to-plane."""
        be = self.be
        cfg = self.params_.placeRecognition_
        constraints = []
        if not candidateSubmaps:
            return constraints
        source = sourceSubmap.getMapPointCloud()
        src_idx = sourceSubmap.id_ if sourceSubmapIdx is None else sourceSubmapIdx
        ids = candidateIdxs if candidateIdxs is not None else [s.id_ for s in candidateSubmaps]
        if self.batchRefinement:
            return self._buildLoopClosureConstraintsBatch(sourceSubmap, candidateSubmaps, ids, src_idx, timestamp)
        for target_submap, tid in zip(candidateSubmaps, ids):
            r = self.ransac(sourceSubmap, target_submap)
            self.lastRansacResult = r
            if r["n_corr"] < cfg.ransacMinCorrespondenceSetSize_:
                continue
            if not self.isRegistrationConsistent(r["transformation"]):
                continue
            target = target_submap.getMapPointCloud()
            voxel = VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION * getMapVoxelSize(
                self.params_.mapBuilder_, VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO)
            i_s, i_t = be.overlap_indices(source.id, target.id, r["transformation"], voxel, 1)
            src_ov = PointCloud(be, be.select_by_index(source.id, i_s.astype(np.uint32)))
            tgt_ov = PointCloud(be, be.select_by_index(target.id, i_t.astype(np.uint32)))
            try:
                icp = self.cloudRegistration.registerClouds(src_ov, tgt_ov, r["transformation"])
                if icp.fitness_ < cfg.minRefinementFitness_:
                    continue
                if not self.isRegistrationConsistent(icp.transformation_):
                    continue
                info = be.information_matrix_dev(src_ov.id, tgt_ov.id, cfg.maxIcpCorrespondenceDistance_, icp.transformation_)
                constraints.append(Constraint(sourceToTarget_=np.array(icp.transformation_), sourceSubmapIdx_=src_idx, targetSubmapIdx_=tid,
                                              informationMatrix_=info, isInformationMatrixValid_=True, isOdometryConstraint_=False,
                                              timestamp_=timestamp))
            finally:
                src_ov.release()
                tgt_ov.release()
        return constraints

    def _buildLoopClosureConstraintsBatch(self, sourceSubmap, candidateSubmaps, ids, src_idx: int, timestamp: float) -> list:
        """buildLoopClosureConstraints with the refinements of all candidates in one device call: the RANSAC step, both of its gates and
        the overlap selection run for every candidate first; the survivors are refined by one registerCloudsBatch, each from its own
        RANSAC transform; the fitness and consistency gates and the information matrices follow in candidate order.  Every entry of
        the batch is its one-pair registration bit for bit (o3ds_icp_register_batch), so the list is the sequential form's."""
        be = self.be
        cfg = self.params_.placeRecognition_
        source = sourceSubmap.getMapPointCloud()
        constraints = []
        survivors = []  # (tid, RANSAC transform, source overlap, target overlap)
        try:
            for target_submap, tid in zip(candidateSubmaps, ids):
                r = self.ransac(sourceSubmap, target_submap)
                self.lastRansacResult = r
                if r["n_corr"] < cfg.ransacMinCorrespondenceSetSize_:
                    continue
                if not self.isRegistrationConsistent(r["transformation"]):
                    continue
                target = target_submap.getMapPointCloud()
                voxel = VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION * getMapVoxelSize(
                    self.params_.mapBuilder_, VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO)
                i_s, i_t = be.overlap_indices(source.id, target.id, r["transformation"], voxel, 1)
                src_ov = PointCloud(be, be.select_by_index(source.id, i_s.astype(np.uint32)))
                survivors.append([tid, r["transformation"], src_ov, None])
                survivors[-1][3] = PointCloud(be, be.select_by_index(target.id, i_t.astype(np.uint32)))
            if not survivors:
                return constraints
            icps = self.cloudRegistration.registerCloudsBatch([s[2] for s in survivors], [s[3] for s in survivors], [s[1] for s in survivors])
            for (tid, _, src_ov, tgt_ov), icp in zip(survivors, icps):
                if icp.fitness_ < cfg.minRefinementFitness_:
                    continue
                if not self.isRegistrationConsistent(icp.transformation_):
                    continue
                info = be.information_matrix_dev(src_ov.id, tgt_ov.id, cfg.maxIcpCorrespondenceDistance_, icp.transformation_)
                constraints.append(Constraint(sourceToTarget_=np.array(icp.transformation_), sourceSubmapIdx_=src_idx, targetSubmapIdx_=tid,
                                              informationMatrix_=info, isInformationMatrixValid_=True, isOdometryConstraint_=False,
                                              timestamp_=timestamp))
        finally:
            for _, _, src_ov, tgt_ov in survivors:
                src_ov.release()
                if tgt_ov is not None:
                    tgt_ov.release()
        return constraints
