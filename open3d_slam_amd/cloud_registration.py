"""CloudRegistration seam of the reference (include/open3d_slam/CloudRegistration.hpp:19-42,
src/CloudRegistration.cpp:44-65,85-100) over the HIP backend: same class names, members, factory and error behaviour."""
from __future__ import annotations

import dataclasses

import numpy as np

from . import backend as _b
from .parameters import CloudRegistrationParameters, CloudRegistrationType
from .pointcloud import PointCloud


@dataclasses.dataclass
class RegistrationResult:
    """open3d::pipelines::registration::RegistrationResult fields open3d_slam reads
    (Odometry.cpp:51-72, Mapper.cpp:151-159); correspondence_set_ is never consumed and is not materialised."""
    transformation_: np.ndarray
    fitness_: float
    inlier_rmse_: float
    iterations_: int = 0
    converged_: bool = False


@dataclasses.dataclass
class ICPConvergenceCriteria:
    """[O3D] defaults; the reference only overrides max_iteration_ (CloudRegistration.cpp:63)."""
    relative_fitness_: float = 1e-6
    relative_rmse_: float = 1e-6
    max_iteration_: int = 30


class CloudRegistration:  # CloudRegistration.hpp:19-27
    def registerClouds(self, source: PointCloud, target: PointCloud, init) -> RegistrationResult:
        raise NotImplementedError

    def registerCloudsBatch(self, sources, targets, inits) -> list:
        raise NotImplementedError

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:
        return None


def _register_clouds_batch(reg, method: int, sources, targets, inits, target_crops=None) -> list:
    """registerClouds of `reg` for every (sources[k], targets[k], inits[k]) in ONE o3ds_icp_register_batch call (a capability beyond the
    reference): the results of the per-pair calls, bit for bit, in order.  Raises as the per-pair call raises: on what
    the library refuses for the whole batch, and on the first entry that did not run (an empty target, a missing normal set).
    Generalized ICP: a pair with a cloud that carries no normals takes the per-pair call, which estimates them on a copy
    (o3ds_icp_generalized_dev) -- the batch entry point registers clouds as they are."""
    sources, targets, inits = list(sources), list(targets), list(inits)
    if not (len(sources) == len(targets) == len(inits)):
        raise ValueError("registerCloudsBatch: sources, targets and inits differ in length")
    if not sources:
        return []
    crops = list(target_crops) if target_crops is not None else [None] * len(sources)
    be = sources[0].be
    if method == _b.ICP_GENERALIZED:
        single = [k for k, (s, t) in enumerate(zip(sources, targets)) if not (be.has_normals(s.id) and be.has_normals(t.id))]
        if single:
            out = [None] * len(sources)
            for k in single:
                out[k] = reg.registerClouds(sources[k], targets[k], inits[k], crops[k])
            rest = [k for k in range(len(sources)) if out[k] is None]
            done = _register_clouds_batch(reg, method, [sources[k] for k in rest], [targets[k] for k in rest], [inits[k] for k in rest],
                                          [crops[k] for k in rest])
            for k, r in zip(rest, done):
                out[k] = r
            return out
    c = reg.icpConvergenceCriteria_
    params = be._params(reg.maxCorrespondenceDistance_, c.max_iteration_, c.relative_fitness_, c.relative_rmse_, method)
    try:
        results, status = be.icp_register_batch([(s.id, t.id, crop, init) for s, t, crop, init in zip(sources, targets, crops, inits)], params, split=True)
    except _b.BackendError as e:
        raise RuntimeError(str(e)) from e
    for k, st in enumerate(status):
        if st != 0:
            raise RuntimeError(f"registerCloudsBatch: entry {k} failed with status {st}")
    return [RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"]) for r in results]


class RegistrationIcpPointToPlane(CloudRegistration):  # CloudRegistration.hpp:29-42
    def __init__(self):
        self.maxCorrespondenceDistance_ = 1.0
        self.knnNormalEstimation_ = 10
        self.maxRadiusNormalEstimation_ = 2.0
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()

    def registerClouds(self, source: PointCloud, target: PointCloud, init, target_crop=None) -> RegistrationResult:
        """CloudRegistration.cpp:44-48 -> [O3D] RegistrationICP(source, target, maxCorrespondenceDistance_, init,
        TransformationEstimationPointToPlane, icpConvergenceCriteria_).  Raises (like Open3D's LogError -> runtime_error)
        on max_correspondence_distance <= 0 or a target without normals."""
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_point_to_plane_dev(source.id, target.id, self.maxCorrespondenceDistance_, init=init,
                                                 max_iter=c.max_iteration_, rel_fitness=c.relative_fitness_,
                                                 rel_rmse=c.relative_rmse_, target_crop=target_crop)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    def registerCloudsBatch(self, sources, targets, inits, target_crops=None) -> list:
        """registerClouds for every pair, in one device call: the same results in order (see _register_clouds_batch)"""
        return _register_clouds_batch(self, _b.ICP_POINT_TO_PLANE, sources, targets, inits, target_crops)

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:
        """CloudRegistration.cpp:49-56: assert_gt on both parameters, then EstimateNormals(Hybrid) + NormalizeNormals +
        OrientNormalsTowardsCameraLocation."""
        if not self.maxRadiusNormalEstimation_ > 0.0:
            raise RuntimeError("maxRadiusNormalEstimation_")  # assert_gt (assert.hpp)
        if not self.knnNormalEstimation_ > 0:
            raise RuntimeError("knnNormalEstimation_")
        cloud.be.estimate_normals(cloud.id, self.maxRadiusNormalEstimation_, self.knnNormalEstimation_)


class RegistrationIcpGeneralized(CloudRegistration):  # CloudRegistration.hpp:56-69
    def __init__(self):
        self.maxCorrespondenceDistance_ = 1.0
        self.knnNormalEstimation_ = 10
        self.maxRadiusNormalEstimation_ = 2.0
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()

    def registerClouds(self, source: PointCloud, target: PointCloud, init, target_crop=None) -> RegistrationResult:
        """CloudRegistration.cpp:16-21 -> [O3D] RegistrationGeneralizedICP(source, target, maxCorrespondenceDistance_, init,
        TransformationEstimationForGeneralizedICP(), icpConvergenceCriteria_); covariances are built from the clouds' normals."""
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_generalized_dev(source.id, target.id, self.maxCorrespondenceDistance_, init=init, max_iter=c.max_iteration_,
                                              rel_fitness=c.relative_fitness_, rel_rmse=c.relative_rmse_, target_crop=target_crop)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    def registerCloudsBatch(self, sources, targets, inits, target_crops=None) -> list:
        """registerClouds for every pair, in one device call: the same results in order (see _register_clouds_batch)"""
        return _register_clouds_batch(self, _b.ICP_GENERALIZED, sources, targets, inits, target_crops)

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:  # CloudRegistration.cpp:22-30
        if not self.maxRadiusNormalEstimation_ > 0.0:
            raise RuntimeError("maxRadiusNormalEstimation_")
        if not self.knnNormalEstimation_ > 0:
            raise RuntimeError("knnNormalEstimation_")
        cloud.be.estimate_normals(cloud.id, self.maxRadiusNormalEstimation_, self.knnNormalEstimation_)


class RegistrationIcpPointToPoint(CloudRegistration):  # CloudRegistration.hpp:30-41
    def __init__(self):
        self.maxCorrespondenceDistance_ = 1.0
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()

    def registerClouds(self, source: PointCloud, target: PointCloud, init, target_crop=None) -> RegistrationResult:
        """CloudRegistration.cpp:69-74 -> [O3D] RegistrationICP(source, target, maxCorrespondenceDistance_, init,
        TransformationEstimationPointToPoint(), icpConvergenceCriteria_): closed-form Umeyama update per iteration."""
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_point_to_point_dev(source.id, target.id, self.maxCorrespondenceDistance_, init=init, max_iter=c.max_iteration_,
                                                 rel_fitness=c.relative_fitness_, rel_rmse=c.relative_rmse_, target_crop=target_crop)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    def registerCloudsBatch(self, sources, targets, inits, target_crops=None) -> list:
        """registerClouds for every pair, in one device call: the same results in order (see _register_clouds_batch)"""
        return _register_clouds_batch(self, _b.ICP_POINT_TO_POINT, sources, targets, inits, target_crops)

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:  # base-class no-op (CloudRegistration.hpp:26)
        return None


class RegistrationIcpColored(CloudRegistration):
    """[O3D] RegistrationColoredICP, the fourth RegistrationICP estimator, on device clouds (o3ds_icp_colored_dev).  The reference has no
    such class and no CloudRegistrationType for it: it is offered beside the three it has and is not made by cloudRegistrationFactory."""

    def __init__(self):
        self.maxCorrespondenceDistance_ = 1.0
        self.knnNormalEstimation_ = 10
        self.maxRadiusNormalEstimation_ = 2.0
        self.lambdaGeometric_ = 0.968  # [O3D] TransformationEstimationForColoredICP's default
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()

    def registerClouds(self, source: PointCloud, target: PointCloud, init) -> RegistrationResult:
        """[O3D] RegistrationColoredICP(source, target, maxCorrespondenceDistance_, init,
        TransformationEstimationForColoredICP(lambdaGeometric_), icpConvergenceCriteria_).  Both clouds need colours, the target normals;
        the target's colour gradients are computed on the first call and stay on it.  Raises as Open3D's LogError does."""
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_colored_dev(source.id, target.id, self.maxCorrespondenceDistance_, init=init, max_iter=c.max_iteration_,
                                          rel_fitness=c.relative_fitness_, rel_rmse=c.relative_rmse_, lambda_geometric=self.lambdaGeometric_)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:
        """point-to-plane's normals (CloudRegistration.cpp:49-56)"""
        if not self.maxRadiusNormalEstimation_ > 0.0:
            raise RuntimeError("maxRadiusNormalEstimation_")
        if not self.knnNormalEstimation_ > 0:
            raise RuntimeError("knnNormalEstimation_")
        cloud.be.estimate_normals(cloud.id, self.maxRadiusNormalEstimation_, self.knnNormalEstimation_)


def createColoredIcp(p: CloudRegistrationParameters) -> RegistrationIcpColored:  # as createPointToPlaneIcp; lambdaGeometric_ keeps its default
    ret = RegistrationIcpColored()
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.knnNormalEstimation_ = p.icp_.knn_
    ret.maxRadiusNormalEstimation_ = p.icp_.maxDistanceKnn_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    return ret


# [O3D] pipelines::registration::RobustKernel and its six losses (RobustKernel.h), by Open3D's names; `k_` is Open3D's scaling parameter
@dataclasses.dataclass(frozen=True)
class RobustKernel:
    kind_ = _b.LOSS_L2

    def toBackend(self) -> _b.RobustLoss:
        return _b.RobustLoss(self.kind_, 0, float(getattr(self, "k_", 0.0)))


@dataclasses.dataclass(frozen=True)
class L2Loss(RobustKernel):
    kind_ = _b.LOSS_L2


@dataclasses.dataclass(frozen=True)
class L1Loss(RobustKernel):
    kind_ = _b.LOSS_L1


@dataclasses.dataclass(frozen=True)
class HuberLoss(RobustKernel):
    k_: float
    kind_ = _b.LOSS_HUBER


@dataclasses.dataclass(frozen=True)
class CauchyLoss(RobustKernel):
    k_: float
    kind_ = _b.LOSS_CAUCHY


@dataclasses.dataclass(frozen=True)
class GMLoss(RobustKernel):
    k_: float
    kind_ = _b.LOSS_GM


@dataclasses.dataclass(frozen=True)
class TukeyLoss(RobustKernel):
    k_: float
    kind_ = _b.LOSS_TUKEY


ROBUST_ESTIMATORS = {"point_to_plane": _b.ROBUST_POINT_TO_PLANE, "colored": _b.ROBUST_COLORED}


class RegistrationIcpRobust(CloudRegistration):
    """[O3D] RegistrationICP with TransformationEstimationPointToPlane(kernel) or TransformationEstimationForColoredICP(lambda, kernel) on
    device clouds (o3ds_icp_robust_dev).  Like RegistrationIcpColored it is offered beside the reference's three and is not made by
    cloudRegistrationFactory."""

    def __init__(self):
        self.maxCorrespondenceDistance_ = 1.0
        self.knnNormalEstimation_ = 10
        self.maxRadiusNormalEstimation_ = 2.0
        self.estimator_ = "point_to_plane"  # or "colored"
        self.kernel_: RobustKernel = L2Loss()
        self.lambdaGeometric_ = 0.968  # "colored" only
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()

    def registerClouds(self, source: PointCloud, target: PointCloud, init) -> RegistrationResult:
        """The target needs normals; "colored" needs colours on both clouds as well, and leaves its gradients on the target."""
        if self.estimator_ not in ROBUST_ESTIMATORS:
            raise RuntimeError(f"estimator_ {self.estimator_!r}: one of {sorted(ROBUST_ESTIMATORS)}")
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_robust_dev(source.id, target.id, self.maxCorrespondenceDistance_, ROBUST_ESTIMATORS[self.estimator_],
                                         self.kernel_.toBackend(), init=init, max_iter=c.max_iteration_, rel_fitness=c.relative_fitness_,
                                         rel_rmse=c.relative_rmse_, lambda_geometric=self.lambdaGeometric_)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    estimateNormalsOrCovariancesIfNeeded = RegistrationIcpColored.estimateNormalsOrCovariancesIfNeeded  # point-to-plane's normals


def createRobustIcp(p: CloudRegistrationParameters, kernel: RobustKernel, estimator: str = "point_to_plane") -> RegistrationIcpRobust:
    ret = RegistrationIcpRobust()  # as createColoredIcp; lambdaGeometric_ keeps its default
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.knnNormalEstimation_ = p.icp_.knn_
    ret.maxRadiusNormalEstimation_ = p.icp_.maxDistanceKnn_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    ret.kernel_, ret.estimator_ = kernel, estimator
    return ret


class RegistrationIcpDegeneracyAware(RegistrationIcpRobust):
    """RegistrationIcpRobust whose update is solved only in the directions the pass constrains (o3ds_icp_degeneracy_aware_dev): a direction
    of the rotation or of the translation whose normalised eigenvalue lies below its minimum is left where the initial guess put it.  With
    both minima 0 -- the only default -- it is RegistrationIcpRobust to the byte.  `lastReport` holds the report of the last call."""

    def __init__(self):
        super().__init__()
        self.minEigenvalueRotation_ = 0.0     # m^2 per correspondence
        self.minEigenvalueTranslation_ = 0.0  # the point-to-plane values of a pass sum to 1
        self.lastReport = None

    def registerClouds(self, source: PointCloud, target: PointCloud, init) -> RegistrationResult:
        if self.estimator_ not in ROBUST_ESTIMATORS:
            raise RuntimeError(f"estimator_ {self.estimator_!r}: one of {sorted(ROBUST_ESTIMATORS)}")
        c = self.icpConvergenceCriteria_
        try:
            r, self.lastReport = source.be.icp_degeneracy_aware(
                source.id, target.id, self.maxCorrespondenceDistance_, self.minEigenvalueRotation_, self.minEigenvalueTranslation_,
                ROBUST_ESTIMATORS[self.estimator_], self.kernel_.toBackend(), init=init, max_iter=c.max_iteration_,
                rel_fitness=c.relative_fitness_, rel_rmse=c.relative_rmse_, lambda_geometric=self.lambdaGeometric_)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])


def createDegeneracyAwareIcp(p: CloudRegistrationParameters, estimator: str = "point_to_plane", kernel: RobustKernel = L2Loss(),
                             minEigenvalueRotation: float = 0.0, minEigenvalueTranslation: float = 0.0) -> RegistrationIcpDegeneracyAware:
    ret = RegistrationIcpDegeneracyAware()  # as createRobustIcp
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.knnNormalEstimation_ = p.icp_.knn_
    ret.maxRadiusNormalEstimation_ = p.icp_.maxDistanceKnn_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    ret.kernel_, ret.estimator_ = kernel, estimator
    ret.minEigenvalueRotation_, ret.minEigenvalueTranslation_ = float(minEigenvalueRotation), float(minEigenvalueTranslation)
    return ret


class RegistrationNdt(CloudRegistration):
    """Search-free registration against the voxel Gaussians of the target (the normal-distributions transform; o3ds_icp_ndt_dev).  Offered
    beside the reference's three like the classes above and not made by cloudRegistrationFactory.  The Gaussians of the last target it saw
    are kept and rebuilt only when it is handed another cloud (by handle and id) or other build parameters; they are a snapshot, so after
    changing that cloud in place call invalidate()."""

    def __init__(self):
        self.voxelSize_ = 1.0
        self.minPoints_ = 6             # PCL's NormalDistributionsTransform defaults
        self.minEigenvalueRatio_ = 0.01
        self.neighbourhood_ = 7         # 1: the query's own voxel; 7: and its six face neighbours
        self.kernel_: RobustKernel = CauchyLoss(1.0)  # on r = sqrt(e^T B e), in standard deviations
        self.icpConvergenceCriteria_ = ICPConvergenceCriteria()
        self._be, self._key, self._gaussians = None, None, None
        self.lastInfo = None  # the counters of the Gaussians in use

    def invalidate(self) -> None:
        if self._gaussians is not None and getattr(self._be, "h", None):
            self._be.voxel_gaussians_free(self._gaussians)
        self._be, self._key, self._gaussians = None, None, None

    def __del__(self):
        try:
            self.invalidate()
        except Exception:
            pass

    def _targetGaussians(self, target: PointCloud) -> int:
        key = (target.id, self.voxelSize_, self.minPoints_, self.minEigenvalueRatio_)
        if self._gaussians is None or self._be is not target.be or self._key != key:
            self.invalidate()
            self._gaussians, self.lastInfo = target.be.voxel_gaussians_create(target.id, self.voxelSize_, self.minPoints_, self.minEigenvalueRatio_)
            self._be, self._key = target.be, key
        return self._gaussians

    def registerClouds(self, source: PointCloud, target: PointCloud, init) -> RegistrationResult:
        c = self.icpConvergenceCriteria_
        try:
            r = source.be.icp_ndt(source.id, self._targetGaussians(target), self.neighbourhood_, self.kernel_.toBackend(), init=init,
                                  max_iter=c.max_iteration_, rel_fitness=c.relative_fitness_, rel_rmse=c.relative_rmse_)
        except _b.BackendError as e:
            raise RuntimeError(str(e)) from e
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"], r["converged"])

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: PointCloud) -> None:  # nothing per point: the covariances are the voxels'
        return None


def createNdt(p: CloudRegistrationParameters, voxelSize: float, neighbourhood: int = 7, kernel: RobustKernel = CauchyLoss(1.0)) -> RegistrationNdt:
    ret = RegistrationNdt()
    ret.voxelSize_, ret.neighbourhood_, ret.kernel_ = float(voxelSize), int(neighbourhood), kernel
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    return ret


def createPointToPointIcp(p: CloudRegistrationParameters) -> RegistrationIcpPointToPoint:  # CloudRegistration.cpp:76-81
    ret = RegistrationIcpPointToPoint()
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    return ret


def createGeneralizedIcp(p: CloudRegistrationParameters) -> RegistrationIcpGeneralized:  # CloudRegistration.cpp:32-39
    ret = RegistrationIcpGeneralized()
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.knnNormalEstimation_ = p.icp_.knn_
    ret.maxRadiusNormalEstimation_ = p.icp_.maxDistanceKnn_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    return ret


def createPointToPlaneIcp(p: CloudRegistrationParameters) -> RegistrationIcpPointToPlane:  # CloudRegistration.cpp:58-65
    ret = RegistrationIcpPointToPlane()
    ret.maxCorrespondenceDistance_ = p.icp_.maxCorrespondenceDistance_
    ret.knnNormalEstimation_ = p.icp_.knn_
    ret.maxRadiusNormalEstimation_ = p.icp_.maxDistanceKnn_
    ret.icpConvergenceCriteria_.max_iteration_ = p.icp_.maxNumIter_
    return ret


def cloudRegistrationFactory(p: CloudRegistrationParameters) -> CloudRegistration:  # CloudRegistration.cpp:85-100
    if p.regType_ == CloudRegistrationType.PointToPlaneIcp:
        return createPointToPlaneIcp(p)
    if p.regType_ == CloudRegistrationType.GeneralizedIcp:
        return createGeneralizedIcp(p)
    if p.regType_ == CloudRegistrationType.PointToPointIcp:
        return createPointToPointIcp(p)
    raise RuntimeError("cloud: unknown type of cloud registration")
