"""The last launch of a fused registration only folds: when the state it loads already has iterations == max_iter, no update can be
applied, so the 6x6 solve, the sincos and U * T are skipped (icp_step_block, fold_only).  Fitness, rmse, the correspondence count and
the flags come from the other wavefront as before.  The two-launch form (O3DS_ICP_MODE=launch) never takes that path and sums in the
same order, so it is the bitwise reference; the CPU oracle is the independent one (tolerances of tests/test_icp_gpu.py)."""
import numpy as np
import pytest

from open3d_slam_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu

TOL_T, TOL_R = 1e-3, 1e-3  # f32 point storage against the f64 oracle, as in tests/test_icp_gpu.py

# criteria 0: the loop runs out of iterations and the tail skips the solve; default criteria: it converges first and the tail keeps it
CASES = {
    "max_iter_1": dict(max_iter=1, rel_fitness=0.0, rel_rmse=0.0),
    "max_iter_2": dict(max_iter=2, rel_fitness=0.0, rel_rmse=0.0),
    "max_iter_10": dict(max_iter=10, rel_fitness=0.0, rel_rmse=0.0),
    "converges_before_max_iter": dict(max_iter=30),
}


def _same_bits(a, b):
    np.testing.assert_array_equal(a["transformation"], b["transformation"])
    for k in ("fitness", "inlier_rmse", "iterations", "converged", "n_corr"):
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.fixture(scope="module")
def second_init():
    """A start pose for the registration that follows the one under test on the same handle."""
    T = np.eye(4)
    c, s = np.cos(0.01), np.sin(0.01)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [0.05, -0.03, 0.02]
    return T


@pytest.fixture(scope="module")
def tree(oracle, small_c2):
    return oracle.KDTree(small_c2[1])


@pytest.fixture(scope="module")
def two_launch():
    mp = pytest.MonkeyPatch()
    mp.setenv("O3DS_ICP_MODE", "launch")
    be = backend.Backend(0, backend.PRECISION_F32, ab=True)
    mp.undo()  # (the mode is read when the handle is made)
    yield be
    be.close()


@pytest.mark.parametrize("case", list(CASES))
def test_tail_that_only_folds_changes_no_bit(case, small_c2, oracle, tree, two_launch, second_init):
    src, tgt, nrm, _ = small_c2
    kw = CASES[case]
    be = backend.Backend(0, backend.PRECISION_F32)
    fresh = backend.Backend(0, backend.PRECISION_F32)
    try:
        got = be.icp_point_to_plane(src, tgt, nrm, 1.0, **kw)
        ref = oracle.icp_point_to_plane(src, tgt, nrm, 1.0, tree=tree, **kw)
        if case == "converges_before_max_iter":
            assert got["converged"] and got["iterations"] < kw["max_iter"]
        else:
            assert not got["converged"] and got["iterations"] == kw["max_iter"]
        assert got["converged"] == ref["converged"] and abs(got["iterations"] - ref["iterations"]) <= (1 if got["converged"] else 0)
        dt, dr = syn.se3_error(got["transformation"], ref["transformation"])
        assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
        assert abs(got["fitness"] - ref["fitness"]) <= 4.0 / len(src)
        assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-3 * max(ref["inlier_rmse"], 1e-9)
        _same_bits(got, two_launch.icp_point_to_plane(src, tgt, nrm, 1.0, **kw))
        # the pivot order (IcpStateDev::pad) is written only by a solve: the registration that follows on the same handle must not see
        # whether the previous one's last launch solved
        again = be.icp_point_to_plane(src, tgt, nrm, 1.0, init=second_init, max_iter=4, rel_fitness=0.0, rel_rmse=0.0)
        clean = fresh.icp_point_to_plane(src, tgt, nrm, 1.0, init=second_init, max_iter=4, rel_fitness=0.0, rel_rmse=0.0)
        _same_bits(again, clean)
    finally:
        be.close()
        fresh.close()
