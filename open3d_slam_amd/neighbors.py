"""Neighbour queries and outlier filters on device clouds: what callers of the reference reach for next to every cloud operation --
[O3D] KDTreeFlann::SearchKNN / SearchRadius / SearchHybrid, PointCloud::RemoveStatisticalOutliers / RemoveRadiusOutliers / ClusterDBSCAN / SegmentPlane -- and
o3d_slam::computePointCloudDistance (helpers.hpp:29, helpers.cpp:185-218).  Same names; the search runs in the HIP kernel behind
o3ds_neighbor_search on the target's grid index, no k-d tree is built and no cloud is downloaded.

Where Open3D's searches take one query point, these take a cloud of queries and answer all of them in one launch: row i of the result
belongs to query i.  The result of a query is defined in include/o3ds_backend.h (the order (d2, index), strict radius, storage-type d2).
The filters are offered, not switched on: nothing in the frame loop calls them."""
from __future__ import annotations

import numpy as np

from .pointcloud import PointCloud


def _check(queries: PointCloud, target: PointCloud):
    if queries.be is not target.be:
        raise ValueError("the query cloud and the target live on different handles")
    return target.be


def SearchKNN(target: PointCloud, queries: PointCloud, knn: int, T=None, query_idx=None):
    """[O3D] KDTreeFlann::SearchKNN for every query: (indices (n, knn), distance2 (n, knn), count (n,)) -- the knn nearest points of
    `target` in the order (distance2, index), count[i] of them valid (fewer than knn only if the target is smaller)."""
    be = _check(queries, target)
    idx, d2, count, _ = be.neighbor_search(queries.id, target.id, int(knn), 0.0, T, query_idx)
    return idx, d2, count


def SearchRadius(target: PointCloud, queries: PointCloud, radius: float, max_nn: int = 0, T=None, query_idx=None):
    """[O3D] KDTreeFlann::SearchRadius for every query: (indices, distance2, count, total).  total[i] is the number of target points with
    distance2 < radius^2 -- what SearchRadius returns.  The lists are capped at max_nn <= 128 places (nearest first); the default 0 only
    counts, which is what the radius filter needs."""
    be = _check(queries, target)
    if not radius > 0.0:
        raise ValueError("SearchRadius: radius must be > 0")
    return be.neighbor_search(queries.id, target.id, int(max_nn), float(radius), T, query_idx)


def SearchHybrid(target: PointCloud, queries: PointCloud, radius: float, max_nn: int, T=None, query_idx=None):
    """[O3D] KDTreeFlann::SearchHybrid for every query: (indices (n, max_nn), distance2, count) -- at most max_nn points with
    distance2 < radius^2, nearest first."""
    be = _check(queries, target)
    if not radius > 0.0 or int(max_nn) < 1:
        raise ValueError("SearchHybrid: radius must be > 0 and max_nn >= 1")
    idx, d2, count, _ = be.neighbor_search(queries.id, target.id, int(max_nn), float(radius), T, query_idx)
    return idx, d2, count


def RemoveStatisticalOutliers(cloud: PointCloud, nb_neighbors: int, std_ratio: float):
    """[O3D] PointCloud::RemoveStatisticalOutliers: (the kept points as a new cloud -- normals and colours carried --, their indices)"""
    cid, kept = cloud.be.remove_statistical_outliers(cloud.id, nb_neighbors, std_ratio)
    return PointCloud(cloud.be, cid), kept


def RemoveRadiusOutliers(cloud: PointCloud, nb_points: int, search_radius: float):
    """[O3D] PointCloud::RemoveRadiusOutliers: (the kept points as a new cloud -- normals and colours carried --, their indices)"""
    cid, kept = cloud.be.remove_radius_outliers(cloud.id, nb_points, search_radius)
    return PointCloud(cloud.be, cid), kept


def ClusterDBSCAN(cloud: PointCloud, eps: float, min_points: int):
    """[O3D] PointCloud::ClusterDBSCAN: the label of every point, -1 for noise (int32; defined in include/o3ds_backend.h)"""
    return cloud.be.cluster_dbscan(cloud.id, eps, min_points)[0]


def RemoveSmallClusters(cloud: PointCloud, eps: float, min_points: int, min_cluster_size: int):
    """ClusterDBSCAN(eps, min_points), then the points of the clusters of at least min_cluster_size points: (the kept points as a new
    cloud -- normals and colours carried --, their indices).  What the two outlier filters keep by construction -- a compact group of
    points is locally dense -- this drops; the labels never leave the device."""
    cid, kept = cloud.be.remove_small_clusters(cloud.id, eps, min_points, min_cluster_size)
    return PointCloud(cloud.be, cid), kept


def SegmentPlane(cloud: PointCloud, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 100, seed: int = 0):
    """[O3D] PointCloud::SegmentPlane: (plane (a, b, c, d) refitted on the inliers, their indices, the result record with the winning
    hypothesis, fitness and inlier_rmse).  Seeded: the same seed gives the same bytes (defined in include/o3ds_backend.h).  No plane found:
    zeros and no inliers, where Open3D returns NaNs."""
    return cloud.be.segment_plane(cloud.id, distance_threshold, ransac_n, num_iterations, seed)


def SplitByPlane(cloud: PointCloud, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 100, seed: int = 0):
    """SegmentPlane, then SelectByIndex(inliers) and SelectByIndex(inliers, invert=True) without the indices leaving the device: (plane,
    the inliers, the rest) -- normals and colours carried.  What a scan needs before ClusterDBSCAN: with its ground it is one cluster."""
    plane, _, _, inl, rest = cloud.be.segment_plane(cloud.id, distance_threshold, ransac_n, num_iterations, seed, split=True)
    return plane, PointCloud(cloud.be, inl), PointCloud(cloud.be, rest)


def computePointCloudDistance(reference: PointCloud, cloud: PointCloud, idsInReference):
    """helpers.cpp:185-218: for every id, the distance from reference.points_[id] to its nearest point of `cloud` (an unbounded 1-NN);
    returns (distances, ids), entries dropped from both where nothing was found (an empty `cloud`, a non-finite point)."""
    ids = np.asarray(idsInReference, dtype=np.int64).ravel()
    if len(ids) == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    be = _check(reference, cloud)
    _, d2, count, _ = be.neighbor_search(reference.id, cloud.id, 1, 0.0, None, ids.astype(np.uint32))
    found = count > 0
    return np.sqrt(d2[found, 0]), ids[found]
