"""o3ds_remove_statistical_outliers / o3ds_remove_radius_outliers on the device against the restated rules
(tests/neighbor_restatement.py): the kept indices, and the downloaded points, normals and colours of the kept points, are equal.  Both
storages; needs an MI355X.  The margin that makes the statistical verdicts independent of the order of the two sums is asserted without
a device in tests/test_neighbor_restatement_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_restatement as nb  # noqa: E402
from neighbor_restatement import F32, F64  # noqa: E402

from open3d_slam_amd import backend, neighbors  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {F32: backend.Backend(0, backend.PRECISION_F32), F64: backend.Backend(0, backend.PRECISION_F64)}
    yield hs
    for be in hs.values():
        be.close()


def _check(be, cid, out, kept, verdict, what):
    want = np.flatnonzero(verdict.keep)
    got = np.asarray(kept, dtype=np.int64)
    if got.tolist() != want.tolist():
        extra, missing = np.setdiff1d(got, want), np.setdiff1d(want, got)
        raise AssertionError(f"{what}: kept {len(got)}, restated {len(want)}; kept in error {extra[:8].tolist()} (a {verdict.a[extra[:8]].tolist()}), "
                             f"dropped in error {missing[:8].tolist()} (a {verdict.a[missing[:8]].tolist()}), threshold {verdict.threshold}")
    assert be.size(out)[0] == len(want), what
    if len(want) == 0:
        return
    p_in, n_in = be.download(cid)
    p_out, n_out = be.download(out)
    assert p_out.tobytes() == p_in[want].tobytes() and n_out.tobytes() == n_in[want].tobytes(), what
    assert be.get_colors(out).tobytes() == be.get_colors(cid)[want].tobytes(), what


@pytest.mark.parametrize("storage", nb.STORAGES)
@pytest.mark.parametrize("case", nb.FILTER_CASES, ids=lambda c: c.name)
def test_the_filters_keep_the_restated_points_with_their_attributes(handles, case, storage):
    be = handles[storage]
    pts = case.cloud()
    nrm, col = nb.attributes(len(pts))
    cid = be.upload(pts, nrm)
    be.set_colors(cid, col)
    try:
        for k, ratio in case.statistical:
            out, kept = be.remove_statistical_outliers(cid, k, ratio)
            try:
                _check(be, cid, out, kept, nb.statistical(pts, k, ratio, storage), (case.name, storage, "statistical", k, ratio))
            finally:
                be.free(out)
        for k, radius in case.radius:
            out, kept = be.remove_radius_outliers(cid, k, radius)
            try:
                _check(be, cid, out, kept, nb.radius_filter(pts, k, radius, storage), (case.name, storage, "radius", k, radius))
            finally:
                be.free(out)
    finally:
        be.free(cid)


def test_plain_clouds_empty_clouds_the_python_names_and_the_argument_errors(handles):
    be = handles[F32]
    pts = nb.scan_with_outliers()
    cloud, empty = PointCloud.from_numpy(be, pts), PointCloud.from_numpy(be, np.zeros((0, 3)))
    try:
        # a cloud without normals or colours
        out, kept = neighbors.RemoveStatisticalOutliers(cloud, 20, 2.0)
        want = np.flatnonzero(nb.statistical(pts, 20, 2.0, F32).keep)
        assert kept.tolist() == want.tolist() and not out.HasNormals() and not out.HasColors()
        assert out.points_.tobytes() == cloud.points_[want].tobytes()
        out.release()
        out, kept = neighbors.RemoveRadiusOutliers(cloud, 5, 0.5)
        assert kept.tolist() == np.flatnonzero(nb.radius_filter(pts, 5, 0.5, F32).keep).tolist() and len(out) == len(kept)
        n_radius = len(kept)
        assert 0 < n_radius < len(pts)
        out.release()
        for fn, args in ((neighbors.RemoveStatisticalOutliers, (20, 2.0)), (neighbors.RemoveRadiusOutliers, (5, 0.5))):
            out, kept = fn(empty, *args)
            assert len(out) == 0 and len(kept) == 0
            out.release()

        def code(fn):
            with pytest.raises(backend.BackendError) as e:
                fn()
            assert str(e.value).split(": ", 1)[1]
            return e.value.code

        assert code(lambda: be.remove_statistical_outliers(cloud.id, 0, 2.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_statistical_outliers(cloud.id, 20, 0.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_statistical_outliers(cloud.id, 20, -1.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_statistical_outliers(cloud.id, 129, 2.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_statistical_outliers(987654, 20, 2.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_radius_outliers(cloud.id, 0, 0.5)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_radius_outliers(cloud.id, 5, 0.0)) == backend.ERR_INVALID_ARG
        assert code(lambda: be.remove_radius_outliers(987654, 5, 0.5)) == backend.ERR_INVALID_ARG
        # kept_idx may be NULL; one that is too small is reported with the number it would have needed, and no cloud is made
        out_id, n_kept = C.c_uint64(0), C.c_size_t(0)
        assert be.lib.o3ds_remove_radius_outliers(be.h, cloud.id, 5, 0.5, C.byref(out_id), None, 0, C.byref(n_kept)) == backend.OK
        assert n_kept.value == n_radius and be.size(out_id.value)[0] == n_radius
        be.free(out_id.value)
        small = np.zeros(4, np.uint32)
        rc = be.lib.o3ds_remove_radius_outliers(be.h, cloud.id, 5, 0.5, C.byref(out_id), small.ctypes.data_as(C.POINTER(C.c_uint32)), 4, C.byref(n_kept))
        assert rc == backend.ERR_CAPACITY and n_kept.value == n_radius
    finally:
        cloud.release()
        empty.release()
