"""The restatement of o3ds_cluster_dbscan (tests/cluster_restatement.py) without a device: the closed form of the header equals Open3D's
sequential procedure on every case in both storages, the premises of the cases tests/test_cluster_dbscan_gpu.py runs hold, and where
scikit-learn is installed its DBSCAN finds the same core points and the same partition of them (f64, cases without a d2 within 1e-9
relative of eps^2; its border points are not compared: it gives them to the first cluster that reaches them in ITS walk)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_restatement as cr  # noqa: E402
import neighbor_restatement as nb  # noqa: E402
from cluster_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors  # noqa: E402

PAIRS = [(c.name, eps, mp) for c in cr.CASES for eps, mp in c.params]


@pytest.mark.parametrize("storage", cr.STORAGES)
@pytest.mark.parametrize("name,eps,min_points", PAIRS, ids=lambda v: str(v))
def test_the_closed_form_is_open3ds_sequential_procedure(name, eps, min_points, storage):
    adj = cr._adjacency(name, eps, storage)[0]
    assert (adj != adj.T).nnz == 0, "the relation is symmetric bit for bit"
    a, b = cr.reference(name, eps, min_points, storage), cr.sequential(adj, min_points)
    assert a.n_clusters == b.n_clusters
    assert a.labels.tolist() == b.labels.tolist()
    assert a.sizes.tolist() == b.sizes.tolist() and int(a.sizes.sum()) == int((a.labels >= 0).sum())
    # the degrees are the Radius-mode counts of the neighbour search
    assert a.degree.tolist() == nb.search(cr.case(name).cloud(), cr.case(name).cloud(), 0, eps, storage).total.tolist()


def _border(c):
    return ~c.core & (c.labels >= 0)


@pytest.mark.parametrize("storage", cr.STORAGES)
def test_the_premises_of_the_cases(storage):
    for name in ("chain", "chain-shuffled"):
        c = cr.reference(name, 0.1, 3, storage)
        assert c.n_clusters == 1 and c.sizes.tolist() == [4096] and int(_border(c).sum()) == 2 and int(c.degree.max()) == 3, name
    for name in ("chain-gap", "chain-gap-shuffled"):
        c = cr.reference(name, 0.1, 3, storage)
        assert c.n_clusters == 2 and int(_border(c).sum()) == 4 and int(c.sizes.sum()) == 4094, name
    c = cr.reference("ring", 0.1, 3, storage)
    assert c.n_clusters == 1 and c.core.all()
    # the bridge point: its lowest-index core neighbour lies in cluster 1 and its label is 0
    c = cr.reference("bridge", 0.1, 10, storage)
    adj = cr._adjacency("bridge", 0.1, storage)[0]
    assert c.n_clusters == 2 and not c.core[2] and c.core[0] and c.core[1] and c.labels[0] == 0 and c.labels[1] == 1
    nbrs = adj.indices[adj.indptr[2]:adj.indptr[3]]
    cores = nbrs[c.core[nbrs]]
    assert cores.tolist() == [1, 15] and c.labels[15] == 0 and c.labels[2] == 0
    assert cr.discriminating(adj, c).tolist() == [2]
    assert c.sizes.tolist() == [14, 13]
    # the scan: one cluster at (0.5, 5); many, with border points that tell the smallest id from the lowest-index neighbour's, at (0.3, 10)
    c = cr.reference("scan", 0.5, 5, storage)
    assert c.n_clusters == 1
    c = cr.reference("scan", 0.3, 10, storage)
    assert c.n_clusters == 72 and int(_border(c).sum()) == 829
    assert len(cr.discriminating(cr._adjacency("scan", 0.3, storage)[0], c)) >= 1
    c = cr.reference("dense-blobs", 0.4, 150, storage)
    assert int(c.degree.max()) > 128 and c.n_clusters >= 1 and int(_border(c).sum()) >= 1 and int((c.labels < 0).sum()) >= 1
    # the radius is strict: at eps = the step exactly nobody has a neighbour but itself; one f32 ulp above, the six of the lattice
    assert cr.reference("lattice", cr.LATTICE_STEP, 1, storage).degree.tolist() == [1] * 216
    assert cr.reference("lattice", cr.LATTICE_STEP, 1, storage).n_clusters == 216 and cr.reference("lattice", cr.LATTICE_STEP, 2, storage).n_clusters == 0
    c = cr.reference("lattice", cr.STEP_PLUS_ULP, 7, storage)
    assert int(c.degree.max()) == 7 and int(c.core.sum()) == 64 and c.n_clusters == 1 and int(_border(c).sum()) == 96 and int((c.labels < 0).sum()) == 56
    c = cr.reference("duplicates", 0.05, 50, storage)
    assert c.n_clusters == 40 and c.sizes.tolist() == [50] * 40 and c.core.all()
    c = cr.reference("pairs", 0.5, 2, storage)
    assert c.n_clusters == 4096 and c.sizes.tolist() == [2] * 4096  # more roots than one block of the rank scan holds (1024)
    # points with a NaN coordinate are noise and unite nothing
    bad = np.flatnonzero(~np.isfinite(nb.nan_target()).all(axis=1))
    for eps, mp in cr.case("non-finite").params:
        c = cr.reference("non-finite", eps, mp, storage)
        assert len(bad) == 6 and (c.labels[bad] == -1).all() and (c.degree[bad] == 0).all() and c.n_clusters >= 1
    assert np.isinf(cr.inf_cloud()).sum() == 1
    # every size of the filter cuts somewhere
    c = cr.reference("scan", 0.3, 10, storage)
    kept = [int(cr.keep_mask(c, m).sum()) for m in cr.MIN_CLUSTER_SIZES]
    assert kept[0] == int((c.labels >= 0).sum()) and kept == sorted(kept, reverse=True) and len(set(kept)) >= 3


@pytest.mark.parametrize("name,eps,min_points", PAIRS, ids=lambda v: str(v))
def test_scikit_learn_finds_the_same_core_points_and_the_same_partition_of_them(name, eps, min_points):
    sklearn_cluster = pytest.importorskip("sklearn.cluster")
    pts = np.asarray(cr.case(name).cloud())
    if len(pts) == 0 or not np.isfinite(pts).all():
        return  # (scikit-learn takes neither)
    lo, hi = (cr.adjacency(pts, eps * np.sqrt(1.0 + s * 1e-9), F64)[0].nnz for s in (-1.0, 1.0))
    if lo != hi:
        return  # a d2 within 1e-9 relative of eps^2: `<` here, `<=` there
    c = cr.reference(name, eps, min_points, F64)
    sk = sklearn_cluster.DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(pts)
    assert sorted(sk.core_sample_indices_.tolist()) == np.flatnonzero(c.core).tolist()
    core = np.flatnonzero(c.core)
    pairs = set(zip(c.labels[core].tolist(), sk.labels_[core].tolist()))
    assert len(pairs) == c.n_clusters == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def test_the_symbols_exist_and_reject_a_null_handle():
    lib = backend.load()
    for n in ("o3ds_cluster_dbscan", "o3ds_remove_small_clusters"):
        assert n in backend.SIGNATURES and hasattr(lib, n)
    nc, out, n_kept = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
    lab = np.zeros(4, np.int32)
    assert lib.o3ds_cluster_dbscan(None, 1, 0.5, 5, lab.ctypes.data_as(C.POINTER(C.c_int32)), 4, C.byref(nc), None, 0) == backend.ERR_BAD_HANDLE
    assert lib.o3ds_remove_small_clusters(None, 1, 0.5, 5, 10, C.byref(out), None, 0, C.byref(n_kept)) == backend.ERR_BAD_HANDLE
    assert callable(neighbors.ClusterDBSCAN) and callable(neighbors.RemoveSmallClusters)
    assert callable(backend.Backend.cluster_dbscan) and callable(backend.Backend.remove_small_clusters)
