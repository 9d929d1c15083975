"""The brute-force restatement of o3ds_neighbor_search and the outlier filters (tests/neighbor_restatement.py) against independent sources,
the premises of the cases tests/test_neighbor_search_gpu.py and tests/test_outlier_filters_gpu.py run on the device, and the part of the
ABI that needs no device.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_search_restatement as isr  # noqa: E402
import neighbor_restatement as nb  # noqa: E402
import normals_restatement as nr  # noqa: E402
from neighbor_restatement import F32, F64  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("o3ds_neighbor_search", "o3ds_remove_statistical_outliers", "o3ds_remove_radius_outliers")


# ---------------------------------------------------------------------------------------------------------------- independent sources
@pytest.mark.parametrize("storage", nb.STORAGES)
@pytest.mark.parametrize("cloud,radius,knn", [(nr.lattice, 0.6, 7), (nr.lattice, 0.5, 48), (nr.shuffled_duplicates, 0.6, 7), (nr.offset_cloud, 3.0, 20),
                                              (lambda: nr.ragged_cloud()[:700], 3.0, 20), (nr.mixed_cloud, 3.0, 33)])
def test_same_cloud_hybrid_is_the_normals_selection(cloud, radius, knn, storage):
    """normals_restatement.search -- what estimate_normals is held to -- and the Hybrid mode on one cloud are the same lists"""
    pts = cloud()
    a, b = nr.search(pts, radius, knn, storage), nb.search(pts, pts, knn, radius, storage)
    assert (a.cnt == b.cnt).all() and (a.idx == b.idx).all() and (a.tie == b.tie).all()
    assert (b.total >= b.cnt).all() and ((b.total > b.cnt) == (b.total > knn)).all()


@pytest.mark.parametrize("storage", nb.STORAGES)
def test_one_neighbour_with_a_pose_is_the_icp_search(storage):
    """icp_search_restatement.nearest_within -- what the ICP search is held to -- is max_nn = 1 within the radius, pose included;
    non-finite queries among them"""
    src, tgt, _ = isr.void_cloud(0.3, n_tgt=3000, n_src=200)
    src = np.vstack([src, [[np.nan, 0, 0], [np.inf, 1, 1]], src[:20] + 5.0])
    for T, r in ((nb.NEAR_POSE, 0.4), (nb.NEAR_POSE, 0.05), (nb.OFF_GRID_POSE, 1.0), (np.eye(4), 0.4)):
        m = isr.nearest_within(src, tgt, T, r, storage)
        L = nb.search(src, tgt, 1, r, storage, T=T)
        found = m.idx >= 0
        assert (L.cnt == found).all()
        assert (L.idx[found, 0] == m.idx[found]).all()
        if storage == F64:  # (nearest_within reports the f64 distance between the stored values: the storage-type d2 of f64 storage alone)
            assert (L.d2[found, 0] == m.d2[found]).all()
        else:
            assert (np.abs(L.d2[found, 0] - m.d2[found]) <= isr.D2_F32_REL * m.d2[found]).all()
        assert (L.idx[~found] == 0).all() and (L.d2[~found] == 0).all()
        assert not found.all() and (found.any() or T is nb.OFF_GRID_POSE or r < 0.1), r  # (off the grid nothing is within a metre)
        assert (nb.stored_queries(src, storage, T)[:200] == m.q[:200]).all()


def test_f64_lists_are_the_oracles_kd_tree_neighbourhoods(oracle):
    """the oracle's k-d tree (the search under its normals) returns the restated lists: Hybrid and KNN, f64, ties included"""
    for tgt, qs, radius, knn in ((nr.lattice(), nr.lattice()[::5], 0.6, 7), (nr.ragged_cloud()[:900], nb.other_sheet()[:150], 1.0, 20),
                                 (nr.shuffled_duplicates(), nr.shuffled_duplicates()[::9], 0.26, 5)):
        tree = oracle.KDTree(tgt)
        H, K = nb.search(qs, tgt, knn, radius, F64), nb.search(qs, tgt, knn, 0.0, F64)
        for i, q in enumerate(qs):
            idx, d2 = tree.search_hybrid(q, radius, knn)
            assert len(idx) == H.cnt[i] and (np.sort(idx) == np.sort(H.idx[i, :H.cnt[i]])).all() and (np.sort(d2) == H.d2[i, :H.cnt[i]]).all()
            idx, d2 = tree.search_knn(q, knn)
            assert len(idx) == K.cnt[i] and (np.sort(d2) == K.d2[i, :K.cnt[i]]).all()
            if not K.tie[i]:
                assert (np.sort(idx) == np.sort(K.idx[i, :K.cnt[i]])).all()


def test_unbounded_lists_are_scipys_kd_tree_where_nothing_ties():
    """scipy.spatial.cKDTree, f64, on clouds without equal distances: the same indices in the same order, the same distances to the
    rounding of its own arithmetic; queries in a void and far outside the cloud among them"""
    from scipy.spatial import cKDTree

    for tgt, qs, k in ((nr.ragged_cloud(), nb.other_sheet()[:400], 20), (nb.void_target(), nb.void_queries(), 20),
                       (nr.ragged_cloud()[:1000], nb.outside_queries(), 5), (nr.mixed_cloud(), nr.mixed_cloud()[::10], 33)):
        L = nb.search(qs, tgt, k, 0.0, F64)
        assert (L.cnt == k).all() and (L.total == len(tgt)).all()
        gaps = np.diff(L.d2, axis=1)
        assert (gaps > 0).all() and not L.tie.any()  # no ties: the order is the distance's alone
        d, i = cKDTree(tgt).query(qs, k=k)
        assert (i == L.idx).all()
        np.testing.assert_allclose(d * d, L.d2, rtol=1e-12, atol=0)


def test_the_order_is_d2_then_index_the_radius_is_strict_and_total_counts_everything():
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, 2.0], [0, 0, 1.0], [np.nan, 0, 0]])
    q = np.array([[0.0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]])
    for st in nb.STORAGES:
        L = nb.search(q, pts, 4, 2.0, st)
        assert L.idx[0].tolist() == [0, 1, 2, 3] and L.cnt[0] == 4 and L.total[0] == 5 and L.tie[0]  # (0, 0, 2) at d2 = r^2 is out
        assert L.d2[0].tolist() == [0.0, 1.0, 1.0, 1.0]
        assert L.cnt[1:].tolist() == [0, 0] and L.total[1:].tolist() == [0, 0]
        L = nb.search(q, pts, 8, 0.0, st)
        assert L.cnt[0] == 6 and L.total[0] == 6 and L.idx[0].tolist() == [0, 1, 2, 3, 5, 4, 0, 0] and L.d2[0, 5] == 4.0  # the NaN point never
        L = nb.search(q, pts, 0, 2.0, st)
        assert L.idx.shape == (3, 0) and L.total.tolist() == [5, 0, 0]
        assert nb.search(q, pts[:0], 3, 0.0, st).cnt.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- premises
def test_the_tie_cases_tie_at_the_last_place_kept():
    for name in nb.TIE_CASES:
        case = next(c for c in nb.CASES if c.name == name)
        sts = (F32,) if name in nb.F32_TIE_CASES else nb.STORAGES
        for st in sts:
            assert any(nb.reference(name, k, r, st).tie.any() for k, r in case.params if k), (name, st)
    # ... some of which f32 storage alone makes: the two candidates' d2 differ in f64
    for name in nb.F32_TIE_CASES:
        case = next(c for c in nb.CASES if c.name == name)
        k, r = case.params[0]
        a, b = nb.reference(name, k, r, F32), nb.reference(name, k, r, F64)
        assert (a.tie & ~b.tie).any(), name


def test_every_case_is_well_formed_and_the_edges_are_where_the_names_say():
    names = [c.name for c in nb.CASES]
    assert len(set(names)) == len(names)
    for c in nb.CASES:
        for k, r in c.params:
            assert 0 <= k <= 128 and (k > 0 or r > 0)
    L = nb.reference("lattice", 7, 0.5, F32)  # 0.5 = two lattice steps: the six points at exactly that distance are out
    M = nb.search(nr.lattice(), nr.lattice(), 7, 0.5 * (1 + 1e-6), F32)
    assert (M.total > L.total).all() and L.total.max() == 27
    assert (nb.reference("lattice", 128, 100.0, F32).total == len(nr.lattice())).all()
    assert (nb.reference("lattice", 5, 0.1, F32).total == 1).all()          # below the spacing: self alone
    assert (nb.reference("lattice-other", 5, 0.1, F32).total == 0).all()    # ... and nothing for a query between the points
    tot = nb.reference("outside", 5, 50.0, F32).total  # (queries 13 and 40 are the one in the middle of the cloud)
    assert (np.delete(tot, [13, 40]) == 0).all() and tot[13] == 1000 and (nb.reference("outside", 5, 0.0, F32).cnt == 5).all()
    d = np.sqrt(nb.reference("void", 1, 0.0, F64).d2[:, 0])
    assert d.min() > 0.7  # the nearest target is beyond the void: rings of empty cells on any cell a search would choose
    L = nb.reference("non-finite", 5, 0.0, F32)
    assert (L.cnt[[3, 4, 9, 10, 15]] == 0).all() and (L.total[[3, 4, 9, 10, 15]] == 0).all()
    assert (np.delete(L.total, [3, 4, 9, 10, 15]) == 300 - 6).all()
    q = nb.stored_queries(nr.ragged_cloud()[1000:1100], F32, nb.OFF_GRID_POSE)
    tgt = nr.ragged_cloud()[:1000]
    off = np.maximum(np.maximum(tgt.min(axis=0) - q, q - tgt.max(axis=0)), 0.0)
    assert (np.linalg.norm(off, axis=1) > 10.0).all()  # every moved query is more than 10 m outside the target's box
    idx = nb.ragged_query_idx()
    assert len(np.unique(idx)) < len(idx) and (np.diff(idx.astype(np.int64)) < 0).any()


@pytest.mark.parametrize("storage", nb.STORAGES)
@pytest.mark.parametrize("case", nb.FILTER_CASES, ids=lambda c: c.name)
def test_the_statistical_cases_leave_a_margin(case, storage):
    """no a_i within 1e-9 of the threshold (relative): the verdict of every point is the same whatever order the two sums are taken in --
    their rounding moves the threshold by parts in 1e-13.  The pairs cloud stands on exact sums instead."""
    pts = case.cloud()
    for nb_neighbors, ratio in case.statistical:
        v = nb.statistical(pts, nb_neighbors, ratio, storage)
        if case.exact_sums:
            assert (v.a == 0.5).all() and v.threshold == 0.5 and not v.keep.any()
        else:
            assert v.margin > nb.MARGIN, (case.name, nb_neighbors, ratio, v.margin)
    if case.name == "scan":
        v = nb.statistical(pts, 20, 2.0, storage)
        far = pts[:, 2] > 5.0
        assert far.sum() == 30 and not v.keep[far].any() and v.keep[~far].mean() > 0.9
        w = nb.radius_filter(pts, 5, 0.5, storage)
        assert not w.keep[far].any() and w.keep.any() and not w.keep.all()
    if case.name in ("one-valid", "single"):
        v = nb.statistical(pts, *case.statistical[0], storage)
        assert np.isnan(v.threshold) and not v.keep.any()


def test_point_cloud_distance_drops_ids_and_distances_together():
    ref = np.array(nb.odd_queries())
    d, ids = nb.point_cloud_distance(ref, nr.ragged_cloud()[:300], [19, 3, 0, 9, 7, 7], F64)
    assert ids.tolist() == [19, 0, 7, 7] and len(d) == 4 and (d > 0).all()
    d, ids = nb.point_cloud_distance(ref, np.zeros((0, 3)), [1, 2], F64)
    assert len(d) == 0 and len(ids) == 0


# ---------------------------------------------------------------------------------------------------------------- ABI, no device
def test_the_three_entry_points_are_declared_bound_and_exported():
    from open3d_slam_amd import backend

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "o3ds_backend.h")).read(), flags=re.S)
    lib = backend.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in backend.SIGNATURES and hasattr(lib, n), n
    from open3d_slam_amd import neighbors

    for n in ("SearchKNN", "SearchRadius", "SearchHybrid", "RemoveStatisticalOutliers", "RemoveRadiusOutliers", "computePointCloudDistance"):
        assert callable(getattr(neighbors, n))


def test_a_null_handle_is_rejected():
    from open3d_slam_amd import backend

    lib = backend.load()
    n_kept, out = C.c_size_t(), C.c_uint64()
    cnt = (C.c_uint32 * 1)()
    assert lib.o3ds_neighbor_search(None, 1, 1, None, None, 1, 0, 1.0, None, None, cnt, None) == backend.ERR_BAD_HANDLE
    assert b"null handle" in lib.o3ds_last_error(None)
    assert lib.o3ds_remove_statistical_outliers(None, 1, 20, 2.0, C.byref(out), None, 0, C.byref(n_kept)) == backend.ERR_BAD_HANDLE
    assert lib.o3ds_remove_radius_outliers(None, 1, 5, 0.5, C.byref(out), None, 0, C.byref(n_kept)) == backend.ERR_BAD_HANDLE
