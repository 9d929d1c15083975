"""o3ds_neighbor_search on the device against the brute-force restatement (tests/neighbor_restatement.py), per query and without a
tolerance: idx, count, total and the bits of d2 are equal.  Both storages; needs an MI355X.

The cases and what each is there for are in neighbor_restatement.CASES; their premises (ties at the last place, radii on lattice
distances, voids, queries off the grid) are asserted without a device in tests/test_neighbor_restatement_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_restatement as nb  # noqa: E402
import normals_restatement as nr  # noqa: E402
from neighbor_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors, synthetic as syn  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


def _compare(got, L, what):
    idx, d2, count, total = got
    assert idx.shape == L.idx.shape and d2.shape == L.d2.shape, what
    bad = (count != L.cnt) | (total != L.total)
    if idx.shape[1]:
        bad |= np.any(idx != L.idx, axis=1) | np.any(d2.view(np.uint64) != L.d2.view(np.uint64), axis=1)
    differ = np.flatnonzero(bad)
    if len(differ):
        i = differ[0]
        raise AssertionError(f"{what}: {nb.describe(differ, L)}; query {i}: got idx {idx[i].tolist()} count {count[i]} total {total[i]}, "
                             f"restated idx {L.idx[i].tolist()} count {L.cnt[i]} total {L.total[i]}")


@pytest.mark.parametrize("storage", nb.STORAGES)
@pytest.mark.parametrize("case", nb.CASES, ids=lambda c: c.name)
def test_every_query_has_the_restated_list(handles, case, storage):
    be = handles[storage]
    tgt = case.target()
    t = be.upload(tgt)
    q = t if case.queries is None else be.upload(case.queries())
    try:
        if case.index_cell > 0.0:
            be.build_index(t, 0.0, case.index_cell)
        qi = None if case.query_idx is None else case.query_idx()
        for k, r in case.params:
            got = be.neighbor_search(q, t, k, r, T=case.T, query_idx=qi)
            _compare(got, nb.reference(case.name, k, r, storage), (case.name, storage, k, r))
    finally:
        be.free(t)
        if q != t:
            be.free(q)


@pytest.mark.parametrize("storage", nb.STORAGES)
def test_repeated_searches_reuse_the_index_and_give_the_same_lists(handles, storage):
    """the first search builds the target's index and leaves it; the second finds it; a search with other parameters runs on it whatever
    its cell; estimate_normals replaces it with its own and the lists stay the same"""
    be = handles[storage]
    t, q = be.upload(nr.ragged_cloud()), be.upload(nb.other_sheet()[:500])
    try:
        L = nb.reference("ragged-other", 20, 0.0, storage)
        first = be.neighbor_search(q, t, 20, 0.0)
        again = be.neighbor_search(q, t, 20, 0.0)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
        ref = nb.search(nb.other_sheet()[:500], nr.ragged_cloud(), 20, 0.0, storage)
        _compare(first, ref, ("first", storage))
        assert (L.idx[:500] == ref.idx).all()
        _compare(be.neighbor_search(q, t, 5, 0.2), nb.search(nb.other_sheet()[:500], nr.ragged_cloud(), 5, 0.2, storage), ("small radius", storage))
        be.estimate_normals(t, 3.0, 20)
        _compare(be.neighbor_search(q, t, 20, 0.0), ref, ("after normals", storage))
    finally:
        be.free(t)
        be.free(q)


@pytest.mark.parametrize("storage", nb.STORAGES)
def test_a_persistent_map_is_searched_as_its_array(handles, storage):
    """a submap in the persistent form is folded first, as estimate_normals does: the lists are those of the array a download gives"""
    be = handles[storage]
    scene = syn.make_scene()
    m = be.upload(np.zeros((0, 3)))
    q = be.upload(nb.other_sheet()[:200] * [1.0, 1.0, 0.5])
    try:
        for k in range(3):
            T = syn.make_pose([1.5 * k, 0.4 * k, 0.0], [0.0, 0.0, 4.0 * k])
            s = be.upload(syn.vlp16_scan(scene, T, frame=k, n_az=256))
            v = be.voxel_down_sample(s, 0.1)
            be.estimate_normals(v, 2.0, 10)
            be.map_insert_scan(m, v, T, 0.2, backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=0.0, rmax=12.0), max_corr_hint=1.0)
            be.free(s)
            be.free(v)
        assert be.is_persistent_map(m)
        got = be.neighbor_search(q, m, 5, 0.0)
        assert not be.is_persistent_map(m)
        pts = be.download(m)[0]
        assert len(pts) > 1000
        _compare(got, nb.search(nb.other_sheet()[:200] * [1.0, 1.0, 0.5], pts, 5, 0.0, storage), ("persistent map", storage))
        _compare(be.neighbor_search(m, m, 3, 0.5, query_idx=np.arange(0, len(pts), 7)),
                 nb.search(pts, pts, 3, 0.5, storage, query_idx=np.arange(0, len(pts), 7)), ("map on itself", storage))
    finally:
        be.free(m)
        be.free(q)


def test_argument_errors_and_the_optional_outputs(handles):
    import ctypes as C

    be = handles[F32]
    t, q = be.upload(nr.lattice()), be.upload(nr.lattice()[:10])
    try:
        def code(fn):
            with pytest.raises(backend.BackendError) as e:
                fn()
            assert str(e.value).split(": ", 1)[1]  # a text in o3ds_last_error
            return e.value.code

        assert code(lambda: be.neighbor_search(q, t, 129, 0.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.neighbor_search(q, t, -1, 1.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.neighbor_search(q, t, 0, 0.0)) == backend.ERR_INVALID_ARG          # a count needs a radius
        assert code(lambda: be.neighbor_search(q, 987654, 3, 0.0)) == backend.ERR_INVALID_ARG      # unknown ids
        assert code(lambda: be.neighbor_search(987654, t, 3, 0.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.neighbor_search(q, t, 3, 0.0, query_idx=[0, 10])) == backend.ERR_INVALID_ARG  # out of range
        # clouds of two storage types on one handle
        be.lib.o3ds_set_precision(be.h, backend.PRECISION_F64)
        q64 = be.upload(nr.lattice()[:10])
        be.lib.o3ds_set_precision(be.h, backend.PRECISION_F32)
        assert code(lambda: be.neighbor_search(q64, t, 3, 0.0)) == backend.ERR_INVALID_ARG
        be.free(q64)
        # d2 and total may be NULL; the lists are the same
        u32p, k, n = C.POINTER(C.c_uint32), 4, 10
        idx, cnt = np.zeros((n, k), np.uint32), np.zeros(n, np.uint32)
        assert be.lib.o3ds_neighbor_search(be.h, q, t, None, None, n, k, 0.5, idx.ctypes.data_as(u32p), None, cnt.ctypes.data_as(u32p), None) == backend.OK
        L = nb.search(nr.lattice()[:10], nr.lattice(), k, 0.5, F32)
        assert (idx == L.idx).all() and (cnt == L.cnt).all()
        # no queries: nothing to do, no error
        got = be.neighbor_search(q, t, 3, 0.0, query_idx=np.zeros(0, np.uint32))
        assert got[0].shape == (0, 3) and got[2].shape == (0,)
    finally:
        be.free(t)
        be.free(q)


@pytest.mark.parametrize("storage", nb.STORAGES)
def test_the_python_searches_and_point_cloud_distance(handles, storage):
    be = handles[storage]
    tgt, qs = nr.ragged_cloud()[:800], np.array(nb.odd_queries())
    target, queries, empty = PointCloud.from_numpy(be, tgt), PointCloud.from_numpy(be, qs), PointCloud.from_numpy(be, np.zeros((0, 3)))
    try:
        L = nb.search(qs, tgt, 6, 0.0, storage)
        idx, d2, cnt = neighbors.SearchKNN(target, queries, 6)
        assert (idx == L.idx).all() and (d2 == L.d2).all() and (cnt == L.cnt).all()
        L = nb.search(qs, tgt, 6, 0.7, storage)
        idx, d2, cnt = neighbors.SearchHybrid(target, queries, 0.7, 6)
        assert (idx == L.idx).all() and (d2 == L.d2).all() and (cnt == L.cnt).all()
        idx, d2, cnt, tot = neighbors.SearchRadius(target, queries, 0.7)
        assert idx.shape == (20, 0) and (tot == L.total).all() and (cnt == 0).all()
        ids = [19, 3, 0, 9, 7, 7, 15, 1]  # out of order, with a repeat, NaN and infinite points among them
        d, kept = neighbors.computePointCloudDistance(queries, target, ids)
        rd, rk = nb.point_cloud_distance(qs, tgt, ids, storage)
        assert kept.tolist() == rk.tolist() == [19, 0, 7, 7, 1] and (d == rd).all()
        d, kept = neighbors.computePointCloudDistance(queries, empty, ids)  # nothing to find: everything is dropped
        assert len(d) == 0 and len(kept) == 0
    finally:
        for c in (target, queries, empty):
            c.release()
