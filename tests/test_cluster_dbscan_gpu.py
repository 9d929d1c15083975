"""o3ds_cluster_dbscan / o3ds_remove_small_clusters on the device against the restated definition (tests/cluster_restatement.py): labels,
n_clusters and sizes are equal; the filter's kept indices and the downloaded points, normals and colours of the kept points are equal.
Both storages, no tolerance; every case on an index built beforehand with a cell of eps / 8, with one of eps * 8, and with no index (no
result may depend on the cell).  The premises of the cases are asserted without a device in tests/test_cluster_restatement_cpu.py.
Needs an MI355X.  Not reached here: the refusal of a cloud of 2^31 points (32 GiB of points)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_restatement as cr  # noqa: E402
import neighbor_restatement as nb  # noqa: E402
from cluster_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors, synthetic as syn  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu

INDEX_MODES = (("cell eps/8", 1.0 / 8.0), ("cell eps*8", 8.0), ("no index", 0.0))


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


def _compare(got, want: cr.Clustering, what):
    labels, n_clusters, sizes = got
    assert labels.dtype == np.int32 and labels.shape == want.labels.shape, what
    differ = np.flatnonzero(labels != want.labels)
    if len(differ) or n_clusters != want.n_clusters:
        d = differ[:8]
        raise AssertionError(f"{what}: {n_clusters} clusters, restated {want.n_clusters}; {len(differ)} labels differ at {d.tolist()}: got "
                             f"{labels[d].tolist()}, restated {want.labels[d].tolist()} (core {want.core[d].tolist()}, |N| {want.degree[d].tolist()})")
    assert sizes.dtype == np.uint32 and sizes.tolist() == want.sizes.tolist(), what


def _check_filter(be, cid, out, kept, keep, what):
    want = np.flatnonzero(keep)
    got = np.asarray(kept, dtype=np.int64)
    if got.tolist() != want.tolist():
        extra, missing = np.setdiff1d(got, want), np.setdiff1d(want, got)
        raise AssertionError(f"{what}: kept {len(got)}, restated {len(want)}; kept in error {extra[:8].tolist()}, dropped in error {missing[:8].tolist()}")
    assert be.size(out)[0] == len(want), what
    if len(want) == 0:
        return
    p_in, n_in = be.download(cid)
    p_out, n_out = be.download(out)
    assert p_out.tobytes() == p_in[want].tobytes() and n_out.tobytes() == n_in[want].tobytes(), what
    assert be.get_colors(out).tobytes() == be.get_colors(cid)[want].tobytes(), what


@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_labels_sizes_and_the_filter_are_the_restated_ones_whatever_the_index(handles, case, storage):
    be = handles[storage]
    pts = case.cloud()
    nrm, col = nb.attributes(len(pts))
    for eps, min_points in case.params:
        want = cr.reference(case.name, eps, min_points, storage)
        for mode, factor in INDEX_MODES:
            cid = be.upload(pts, nrm if len(pts) else None)
            try:
                if len(pts):
                    be.set_colors(cid, col)
                    if factor > 0.0:
                        be.build_index(cid, 0.0, eps * factor)
                what = (case.name, storage, eps, min_points, mode)
                _compare(be.cluster_dbscan(cid, eps, min_points), want, what)
                _compare(be.cluster_dbscan(cid, eps, min_points), want, what + ("again, on the index left behind",))
                for size in cr.MIN_CLUSTER_SIZES:
                    out, kept = be.remove_small_clusters(cid, eps, min_points, size)
                    try:
                        _check_filter(be, cid, out, kept, cr.keep_mask(want, size), what + ("filter", size))
                    finally:
                        be.free(out)
            finally:
                be.free(cid)


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_a_persistent_map_is_clustered_as_its_array(handles, storage):
    """a submap left in the persistent form by two insertions is folded first, as the search does: the clustering of the array a download
    gives"""
    be = handles[storage]
    scene = syn.make_scene()
    m = be.upload(np.zeros((0, 3)))
    try:
        for k in range(2):
            T = syn.make_pose([1.5 * k, 0.4 * k, 0.0], [0.0, 0.0, 4.0 * k])
            s = be.upload(syn.vlp16_scan(scene, T, frame=k, n_az=256))
            v = be.voxel_down_sample(s, 0.1)
            be.estimate_normals(v, 2.0, 10)
            be.map_insert_scan(m, v, T, 0.2, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=12.0), max_corr_hint=1.0)
            be.free(s)
            be.free(v)
        assert be.is_persistent_map(m)
        got = be.cluster_dbscan(m, 0.5, 6)
        assert not be.is_persistent_map(m)
        pts = be.download(m)[0]
        assert 1000 < len(pts) <= 8192
        want = cr.closed_form(cr.adjacency(pts, 0.5, storage)[0], 6)
        assert want.n_clusters >= 2 and (want.labels < 0).any()
        _compare(got, want, ("persistent map", storage))
        out, kept = be.remove_small_clusters(m, 0.5, 6, 20)
        assert kept.tolist() == np.flatnonzero(cr.keep_mask(want, 20)).tolist()
        be.free(out)
    finally:
        be.free(m)


def test_the_python_names_the_empty_cloud_and_the_argument_errors(handles):
    be = handles[F32]
    pts = nb.scan_with_outliers()
    want = cr.reference("scan", 0.3, 10, F32)
    cloud, empty, inf = PointCloud.from_numpy(be, pts), PointCloud.from_numpy(be, np.zeros((0, 3))), PointCloud.from_numpy(be, cr.inf_cloud())
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    try:
        labels = neighbors.ClusterDBSCAN(cloud, 0.3, 10)
        assert labels.dtype == np.int32 and labels.tolist() == want.labels.tolist()
        out, kept = neighbors.RemoveSmallClusters(cloud, 0.3, 10, 40)  # a cloud without normals or colours
        keep = np.flatnonzero(cr.keep_mask(want, 40))
        assert 0 < len(keep) < int((want.labels >= 0).sum())
        assert kept.tolist() == keep.tolist() and len(out) == len(keep) and not out.HasNormals() and not out.HasColors()
        assert out.points_.tobytes() == cloud.points_[keep].tobytes()
        out.release()
        # the empty cloud: no cluster, no error
        lab, n_clusters, sizes = be.cluster_dbscan(empty.id, 0.3, 10)
        assert len(lab) == 0 and n_clusters == 0 and len(sizes) == 0
        nc = C.c_size_t(7)
        assert be.lib.o3ds_cluster_dbscan(be.h, empty.id, 0.3, 10, None, 0, C.byref(nc), None, 0) == backend.OK and nc.value == 0
        assert len(neighbors.ClusterDBSCAN(empty, 0.3, 10)) == 0
        out, kept = neighbors.RemoveSmallClusters(empty, 0.3, 10, 1)
        assert len(out) == 0 and len(kept) == 0
        out.release()

        def refused(fn, code, text):
            with pytest.raises(backend.BackendError) as e:
                fn()
            assert e.value.code == code and text in str(e.value), str(e.value)

        bad = backend.ERR_INVALID_ARG
        for eps in (0.0, -1.0, float("inf"), float("nan")):
            refused(lambda: be.cluster_dbscan(cloud.id, eps, 10), bad, "cluster_dbscan: eps must be a finite number greater than 0")
            refused(lambda: be.remove_small_clusters(cloud.id, eps, 10, 5), bad, "remove_small_clusters: eps must be a finite number greater than 0")
        refused(lambda: be.cluster_dbscan(cloud.id, 0.3, 0), bad, "cluster_dbscan: min_points < 1")
        refused(lambda: be.remove_small_clusters(cloud.id, 0.3, 0, 5), bad, "remove_small_clusters: min_points < 1")
        refused(lambda: be.remove_small_clusters(cloud.id, 0.3, 10, 0), bad, "remove_small_clusters: min_cluster_size < 1")
        refused(lambda: be.cluster_dbscan(987654, 0.3, 10), bad, "unknown cloud id")  # (the mirror asks for the size first)
        refused(lambda: be.remove_small_clusters(987654, 0.3, 10, 5), bad, "unknown cloud id")
        refused(lambda: be.cluster_dbscan(inf.id, 0.3, 10), bad, "build_index: non-finite coordinates")
        refused(lambda: be.remove_small_clusters(inf.id, 0.3, 10, 5), bad, "build_index: non-finite coordinates")
        n = len(pts)
        nc, lab, sizes = C.c_size_t(0), np.zeros(n, np.int32), np.zeros(n, np.uint32)
        out_id, n_kept = C.c_uint64(0), C.c_size_t(0)
        refused(lambda: be._ck(be.lib.o3ds_cluster_dbscan(be.h, 987654, 0.3, 10, lab.ctypes.data_as(i32p), n, C.byref(nc), None, 0)), bad,
                "cluster_dbscan: unknown cloud id")
        refused(lambda: be._ck(be.lib.o3ds_remove_small_clusters(be.h, 987654, 0.3, 10, 5, C.byref(out_id), None, 0, C.byref(n_kept))), bad,
                "remove_small_clusters: unknown cloud id")
        refused(lambda: be._ck(be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, None, n, C.byref(nc), None, 0)), bad, "cluster_dbscan: labels is NULL")
        refused(lambda: be._ck(be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, lab.ctypes.data_as(i32p), n, None, None, 0)), bad, "n_clusters is required")
        # sizes are optional; too little room for the labels or the sizes is reported with the number of clusters, and nothing is written
        assert be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, lab.ctypes.data_as(i32p), n, C.byref(nc), None, 0) == backend.OK
        assert nc.value == want.n_clusters and lab.tolist() == want.labels.tolist()
        lab[:] = -7
        sizes[:] = 7
        nc.value = 0
        refused(lambda: be._ck(be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, lab.ctypes.data_as(i32p), n - 1, C.byref(nc), None, 0)),
                backend.ERR_CAPACITY, "cluster_dbscan: labels has room for fewer entries than the cloud has points")
        assert nc.value == want.n_clusters and (lab == -7).all()
        nc.value = 0
        refused(lambda: be._ck(be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, lab.ctypes.data_as(i32p), n, C.byref(nc), sizes.ctypes.data_as(u32p),
                                                          want.n_clusters - 1)),
                backend.ERR_CAPACITY, "cluster_dbscan: cluster_sizes is too small for the clusters")
        assert nc.value == want.n_clusters and (lab == -7).all() and (sizes == 7).all()
        assert be.lib.o3ds_cluster_dbscan(be.h, cloud.id, 0.3, 10, lab.ctypes.data_as(i32p), n, C.byref(nc), sizes.ctypes.data_as(u32p),
                                          want.n_clusters) == backend.OK
        assert sizes[: want.n_clusters].tolist() == want.sizes.tolist() and (sizes[want.n_clusters:] == 7).all()
        # the filter: kept_idx may be NULL; one that is too small is reported with the number it would have needed, and no cloud is made
        n_keep = int(cr.keep_mask(want, 5).sum())
        out_id, n_kept = C.c_uint64(0), C.c_size_t(0)
        assert be.lib.o3ds_remove_small_clusters(be.h, cloud.id, 0.3, 10, 5, C.byref(out_id), None, 0, C.byref(n_kept)) == backend.OK
        assert n_kept.value == n_keep and be.size(out_id.value)[0] == n_keep
        be.free(out_id.value)
        small = np.zeros(4, np.uint32)
        refused(lambda: be._ck(be.lib.o3ds_remove_small_clusters(be.h, cloud.id, 0.3, 10, 5, C.byref(out_id), small.ctypes.data_as(u32p), 4, C.byref(n_kept))),
                backend.ERR_CAPACITY, "remove_small_clusters: kept_idx is too small for the kept points")
        assert n_kept.value == n_keep
        refused(lambda: be._ck(be.lib.o3ds_remove_small_clusters(be.h, cloud.id, 0.3, 10, 5, None, None, 0, C.byref(n_kept))), bad,
                "remove_small_clusters: out and n_kept are required")
    finally:
        cloud.release()
        empty.release()
        inf.release()
