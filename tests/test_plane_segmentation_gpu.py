"""o3ds_segment_plane on the device against the restated definition (tests/plane_restatement.py), bit for bit in both storages: best_t,
n_degenerate, n_inliers and the inlier indices; fitness and inlier_rmse; best_plane and plane by their bytes; the downloaded points,
normals and colours of the inlier cloud and of the rest against the rows of the input.  The premises of the cases are asserted without a
device in tests/test_plane_restatement_cpu.py.  Needs an MI355X.  Not reached here: the refusal of a cloud of 2^31 points (32 GiB of
points) and of more than 16 777 216 iterations' worth of work (only the refusal itself is)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_restatement as nb  # noqa: E402
import plane_restatement as pr  # noqa: E402
from plane_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors, synthetic as syn  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


def _f64(x):
    return np.float64(x).tobytes()


def _compare(got, want: pr.Result, what):
    plane, idx, res = got
    head = (res.best_t, res.n_degenerate, res.n_inliers)
    assert head == (want.best_t, want.n_degenerate, want.n_inliers), (what, head, (want.best_t, want.n_degenerate, want.n_inliers))
    assert idx.dtype == np.uint32 and idx.tolist() == want.inliers.tolist(), what
    assert _f64(res.fitness) == _f64(want.fitness) and _f64(res.inlier_rmse) == _f64(want.inlier_rmse), (what, res.fitness, want.fitness, res.inlier_rmse,
                                                                                                       want.inlier_rmse)
    assert np.array(res.best_plane).tobytes() == want.best_plane.tobytes(), (what, list(res.best_plane), want.best_plane.tolist())
    assert plane.tobytes() == np.array(res.plane).tobytes() == want.plane.tobytes(), (what, plane.tolist(), want.plane.tolist())


def _check_split(be, cid, inl, rest, want: pr.Result, what):
    n = be.size(cid)[0]
    keep = np.zeros(n, bool)
    keep[want.inliers] = True
    p_in, n_in = be.download(cid)
    c_in = be.get_colors(cid)
    for out, rows in ((inl, np.flatnonzero(keep)), (rest, np.flatnonzero(~keep))):
        assert be.size(out)[0] == len(rows), what
        if len(rows) == 0:
            continue
        p_out, n_out = be.download(out)
        assert p_out.tobytes() == p_in[rows].tobytes() and n_out.tobytes() == n_in[rows].tobytes(), what
        assert be.get_colors(out).tobytes() == c_in[rows].tobytes(), what


@pytest.mark.parametrize("storage", pr.STORAGES)
@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c.name)
def test_the_plane_the_inliers_and_the_split_are_the_restated_ones(handles, case, storage):
    be = handles[storage]
    pts = case.cloud()
    nrm, col = nb.attributes(len(pts))
    cid = be.upload(pts, nrm)
    try:
        be.set_colors(cid, col)
        for params in case.params:
            want = pr.reference(case.name, storage, params)
            what = (case.name, storage, params)
            got = be.segment_plane(cid, *params, split=True)
            try:
                _compare(got[:3], want, what)
                _check_split(be, cid, got[3], got[4], want, what)
            finally:
                be.free(got[3])
                be.free(got[4])
            again = be.segment_plane(cid, *params)  # the same seed, the same bytes; no cloud asked for
            _compare(again, want, what + ("again",))
            assert bytes(again[2]) == bytes(got[2]), what
    finally:
        be.free(cid)


@pytest.mark.parametrize("storage", pr.STORAGES)
def test_another_seed_gives_another_winner(handles, storage):
    be = handles[storage]
    name = "ground-z"
    (a, b) = pr.case(name).params  # the same but for the seed
    assert a[:3] == b[:3] and a[3] != b[3]
    wa, wb = pr.reference(name, storage, a), pr.reference(name, storage, b)
    assert wa.best_t != wb.best_t
    cid = be.upload(pr.case(name).cloud())
    try:
        ga, gb = be.segment_plane(cid, *a), be.segment_plane(cid, *b)
        assert ga[2].best_t == wa.best_t and gb[2].best_t == wb.best_t and ga[2].best_t != gb[2].best_t
    finally:
        be.free(cid)


@pytest.mark.parametrize("storage", pr.STORAGES)
def test_a_persistent_map_is_segmented_as_its_array(handles, storage):
    """a submap left in the persistent form by two insertions is folded first, as the search does: the result of the array a download
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
        got = be.segment_plane(m, 0.05, 3, 100, 21, split=True)
        assert not be.is_persistent_map(m)
        pts = be.download(m)[0]
        assert 1000 < len(pts) <= 8192
        want = pr.segment(pts, 0.05, 3, 100, 21, storage)
        assert want.best_t >= 0 and 100 < want.n_inliers < len(pts)
        _compare(got[:3], want, ("persistent map", storage))
        assert be.size(got[3])[0] == want.n_inliers and be.size(got[4])[0] == len(pts) - want.n_inliers
        assert be.download(got[4])[0].tobytes() == np.delete(pts, want.inliers, axis=0).tobytes()
        be.free(got[3])
        be.free(got[4])
    finally:
        be.free(m)


def test_split_by_plane_takes_the_floor_out_of_a_scan_and_the_rest_falls_into_clusters(handles):
    """through neighbors: the 8192-point VLP-16 scan, range noise 0.01 m, threshold 0.05 m; the floor lies 1.5 m below the sensor.  With
    the floor the scan is one DBSCAN cluster, without it several (both counts confirmed by brute force on the CPU)."""
    be = handles[F32]
    eps, min_points = pr.SPLIT_DBSCAN
    cloud = PointCloud.from_numpy(be, pr.scan(pr.SPLIT_N_AZ))
    try:
        plane, inliers, rest = neighbors.SplitByPlane(cloud, *pr.SPLIT_PARAMS)
        assert np.degrees(np.arccos(abs(plane[2]))) < 1.0 and abs(abs(plane[3]) - syn.SENSOR_HEIGHT) < 0.05, plane
        assert len(inliers) + len(rest) == len(cloud) and len(inliers) > 3000
        assert (np.abs(inliers.points_[:, 2] + syn.SENSOR_HEIGHT) < 0.06).all()
        p2, idx, res = neighbors.SegmentPlane(cloud, *pr.SPLIT_PARAMS)
        assert p2.tobytes() == plane.tobytes() and len(idx) == len(inliers) == res.n_inliers
        assert inliers.points_.tobytes() == cloud.points_[idx].tobytes()
        assert neighbors.ClusterDBSCAN(cloud, eps, min_points).max() + 1 == 1
        assert neighbors.ClusterDBSCAN(rest, eps, min_points).max() + 1 == pr.SPLIT_REST_CLUSTERS > 1
        inliers.release()
        rest.release()
    finally:
        cloud.release()


def test_the_argument_errors_the_capacity_and_the_optional_outputs(handles):
    be = handles[F32]
    name, params = "ground-z", pr.case("ground-z").params[0]
    want = pr.reference(name, F32, params)
    cid, empty, two = be.upload(pr.case(name).cloud()), be.upload(np.zeros((0, 3))), be.upload(np.arange(6.0).reshape(2, 3))
    u32p = C.POINTER(C.c_uint32)
    n = len(pr.case(name).cloud())

    def call(cloud, thr, ransac_n, iters, seed, res, idx=None, cap=0, inl=None, rest=None):
        return be.lib.o3ds_segment_plane(be.h, cloud, thr, ransac_n, iters, seed, C.byref(res) if res is not None else None,
                                         idx.ctypes.data_as(u32p) if idx is not None else None, cap, C.byref(inl) if inl is not None else None,
                                         C.byref(rest) if rest is not None else None)

    def refused(rc, code, text):
        assert rc == code and text in be.lib.o3ds_last_error(be.h).decode(), (rc, be.lib.o3ds_last_error(be.h))

    try:
        bad, res = backend.ERR_INVALID_ARG, backend.PlaneResult()
        refused(call(cid, 0.05, 2, 10, 0, res), bad, "ransac_n should be set to higher than or equal to 3.")
        refused(call(empty, 0.05, 3, 10, 0, res), bad, "There must be at least 'ransac_n' points.")
        refused(call(two, 0.05, 3, 10, 0, res), bad, "There must be at least 'ransac_n' points.")
        refused(call(cid, 0.05, 9, 10, 0, res), bad, "segment_plane: ransac_n > 8 unsupported")
        refused(call(cid, 0.05, 3, -1, 0, res), bad, "segment_plane: num_iterations is negative or above 16777216")
        refused(call(cid, 0.05, 3, (1 << 24) + 1, 0, res), bad, "segment_plane: num_iterations is negative or above 16777216")
        refused(call(987654, 0.05, 3, 10, 0, res), bad, "segment_plane: unknown cloud id")
        refused(call(cid, 0.05, 3, 10, 0, None), bad, "segment_plane: out is required")
        refused(call(cid, 0.05, 3, 10, 0, res, None, 4), bad, "segment_plane: inlier_idx is NULL with capacity > 0")
        with pytest.raises(backend.BackendError) as e:
            neighbors.SegmentPlane(PointCloud(be, two, owns=False), 0.05, 3, 10)
        assert e.value.code == bad and "There must be at least 'ransac_n' points." in str(e.value)
        # every output but the record is optional
        assert call(cid, *params, res) == backend.OK
        assert (res.best_t, res.n_inliers) == (want.best_t, want.n_inliers) and np.array(res.plane).tobytes() == want.plane.tobytes()
        rest = C.c_uint64(0)
        assert call(cid, *params, res, rest=rest) == backend.OK and be.size(rest.value)[0] == n - want.n_inliers
        be.free(rest.value)
        # too little room for the indices: the record is complete, nothing is written, no cloud is made
        small, inl, rest = np.full(4, 7, np.uint32), C.c_uint64(0), C.c_uint64(0)
        refused(call(cid, *params, res, small, 4, inl, rest), backend.ERR_CAPACITY, "segment_plane: inlier_idx is too small for the inliers")
        assert res.n_inliers == want.n_inliers and res.best_t == want.best_t and np.array(res.plane).tobytes() == want.plane.tobytes()
        assert (small == 7).all() and inl.value == 0 and rest.value == 0
        room = np.zeros(want.n_inliers, np.uint32)
        assert call(cid, *params, res, room, len(room)) == backend.OK and room.tolist() == want.inliers.tolist()
    finally:
        for c in (cid, empty, two):
            be.free(c)
