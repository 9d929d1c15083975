"""The neighbourhood-major replica of a registration target's index (common.hpp GridDev::rpts, icp_kernels.hpp nn_search_group): the
search on it must find the same matches as the search on the rows of cell_start, hence bit-identical poses, fitness, rmse and
correspondence counts.  Both paths run in the A/B library: O3DS_NN_REPLICA_AFTER=1 builds the replica at the first registration against
an index (the shipped policy waits for the fourth), O3DS_NN_REPLICA=0 searches without it (both read at every registration), and every
comparison first checks that the replica exists, so that a skipped build cannot make the two runs the same path."""
import numpy as np
import pytest

from open3d_slam_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu

FIXED = dict(max_iter=10, rel_fitness=0.0, rel_rmse=0.0)


def _same(a, b, what):
    np.testing.assert_array_equal(a["transformation"], b["transformation"], err_msg=what)
    assert (a["iterations"], a["n_corr"], a["fitness"], a["inlier_rmse"]) == (b["iterations"], b["n_corr"], b["fitness"], b["inlier_rmse"]), what


@pytest.fixture(autouse=True)
def _eager_replica(monkeypatch):
    monkeypatch.setenv("O3DS_NN_REPLICA_AFTER", "1")


def _both(monkeypatch, run, be, t_id):
    """run() with the replica and without it; returns the two results"""
    monkeypatch.setenv("O3DS_NN_REPLICA", "1")
    on = run()
    assert be.index_replica(t_id) > 0, "the target has no replica: both runs would take the row search"
    monkeypatch.setenv("O3DS_NN_REPLICA", "0")
    off = run()
    monkeypatch.delenv("O3DS_NN_REPLICA")
    return on, off


@pytest.fixture(scope="module")
def normals_src(small_c2):
    from oracle import pyoracle

    return pyoracle.estimate_normals(small_c2[0], 3.0, 20)


def _set_env(monkeypatch, env):
    for k in ("O3DS_ICP_SETS", "O3DS_SET_GAIN", "O3DS_SET_MIN", "O3DS_SET_CAP", "O3DS_ICP_MODE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("prec", [backend.PRECISION_F32, backend.PRECISION_F64])
@pytest.mark.parametrize("env", [{}, {"O3DS_ICP_SETS": "0"}, {"O3DS_SET_MIN": "1e-6", "O3DS_SET_GAIN": "0.01"},
                                 {"O3DS_SET_MIN": "0.3", "O3DS_SET_CAP": "10"}, {"O3DS_ICP_MODE": "launch"}])
def test_replica_is_bitwise_the_row_search(small_c2, normals_src, monkeypatch, prec, env):
    """point-to-plane with and without a map crop, generalized, point-to-point; fixed iterations and the default criteria; candidate
    sets off, tiny margins, margins that overflow the lists; the two-launch form"""
    src, tgt, nrm, _ = small_c2
    crop = backend.make_crop(backend.CROP_MAX_RADIUS, center=(1.0, -2.0, 0.0), rmax=22.0)
    _set_env(monkeypatch, env)
    be = backend.Backend(0, prec, ab=True)
    try:
        s_id, t_id = be.upload(src, normals_src), be.upload(tgt, nrm)
        be.build_index(t_id, 1.0)

        def run():
            out = []
            for kw in (FIXED, dict(max_iter=30)):
                out.append(be.icp_point_to_plane_dev(s_id, t_id, 1.0, **kw))
                out.append(be.icp_point_to_plane_dev(s_id, t_id, 1.0, target_crop=crop, **kw))
                out.append(be.icp_generalized_dev(s_id, t_id, 1.0, **kw))
                out.append(be.icp_point_to_point_dev(s_id, t_id, 1.0, **kw))
            return out

        on, off = _both(monkeypatch, run, be, t_id)
    finally:
        be.close()
    assert on[0]["iterations"] == 10 and on[0]["fitness"] > 0.5
    for k, (a, b) in enumerate(zip(on, off)):
        _same(a, b, f"{env} #{k}")


def test_replica_stepwise(small_c2, monkeypatch):
    import torch

    src, tgt, nrm, _ = small_c2
    be = backend.Backend(0, backend.PRECISION_F32, ab=True)
    try:
        s, t = be.upload(src), be.upload(tgt, nrm)
        be.build_index(t, 1.0)

        def run():
            rec = torch.zeros(32, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            be.icp_begin(s, t, 1.0, max_iter=6, rel_fitness=0.0, rel_rmse=0.0)
            for _ in range(7):
                be.icp_accumulate(0, len(src), rec.data_ptr())
                be.icp_update(rec.data_ptr(), len(src))
            assert be.icp_done()
            return be.icp_finish()

        on, off = _both(monkeypatch, run, be, t)
        one = be.icp_point_to_plane_dev(s, t, 1.0, max_iter=6, rel_fitness=0.0, rel_rmse=0.0)
    finally:
        be.close()
    _same(on, off, "step-wise")
    np.testing.assert_array_equal(on["transformation"], one["transformation"])


def _grid_cloud(rng, n, extent):
    pts = rng.uniform(0.0, 1.0, size=(n, 3)) * np.asarray(extent)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm


@pytest.mark.parametrize("prec", [backend.PRECISION_F32, backend.PRECISION_F64])
def test_replica_thin_grids_outside_queries_and_ties(monkeypatch, prec):
    """grids one and two cells thick on an axis, queries outside the grid, exact distance ties between duplicated points (the smaller
    original index wins on both paths)"""
    rng = np.random.default_rng(7)
    be = backend.Backend(0, prec, ab=True)
    try:
        cases = []
        for extent in ((6.0, 6.0, 0.1), (6.0, 0.4, 6.0), (0.1, 6.0, 0.4), (6.0, 6.0, 6.0)):
            tgt, nrm = _grid_cloud(rng, 20_000, extent)
            src = tgt[rng.choice(len(tgt), 3000, replace=False)] + rng.normal(scale=0.05, size=(3000, 3))
            cases.append((src, tgt, nrm))
        # duplicates: every target point twice (exact ties everywhere), queries straddling the grid's faces and far outside it
        tgt, nrm = _grid_cloud(rng, 8000, (3.0, 3.0, 3.0))
        tgt, nrm = np.concatenate([tgt, tgt[::-1]]), np.concatenate([nrm, nrm[::-1]])
        src = np.concatenate([rng.uniform(-1.5, 4.5, size=(4000, 3)), rng.uniform(40.0, 50.0, size=(64, 3))])
        cases.append((src, tgt, nrm))
        for k, (src, tgt, nrm) in enumerate(cases):
            s_id, t_id = be.upload(src), be.upload(tgt, nrm)
            be.build_index(t_id, 1.0)

            def run():
                return [be.icp_point_to_plane_dev(s_id, t_id, 1.0, max_iter=5, rel_fitness=0.0, rel_rmse=0.0),
                        be.icp_point_to_point_dev(s_id, t_id, 1.0, max_iter=5, rel_fitness=0.0, rel_rmse=0.0)]

            on, off = _both(monkeypatch, run, be, t_id)
            for a, b in zip(on, off):
                assert a["n_corr"] > 0
                _same(a, b, f"case {k}")
            be.free(s_id)
            be.free(t_id)
    finally:
        be.close()


def test_replica_is_built_for_reused_indexes_only(small_c2, monkeypatch):
    """Shipped policy: the fourth registration against one index builds its replica; a rebuilt index starts without one; the results
    before and after the build are the same bits."""
    monkeypatch.delenv("O3DS_NN_REPLICA_AFTER")
    src, tgt, nrm, _ = small_c2
    be = backend.Backend(0, backend.PRECISION_F32, ab=True)
    try:
        s_id, t_id = be.upload(src), be.upload(tgt, nrm)
        be.build_index(t_id, 1.0)
        out = []
        for k in range(5):
            out.append(be.icp_point_to_plane_dev(s_id, t_id, 1.0, **FIXED))
            assert (be.index_replica(t_id) > 0) == (k >= 3), k
        for r in out[1:]:
            _same(out[0], r, "with and without the replica")
        be.build_index(t_id, 1.0)
        assert be.index_replica(t_id) == 0
        be.icp_point_to_plane_dev(s_id, t_id, 1.0, **FIXED)
        assert be.index_replica(t_id) == 0
    finally:
        be.close()
