"""Multi-submap registration without a device: the ABI surface of o3ds_icp_register_multi, SubmapCollection.getSubmapsForScanMatching on
hand-built collections, and the host restatement of both forms (tests/multi_submap_restatement.py) against the CPU oracle's own
registration -- the yardstick of tests/test_multi_submap_gpu.py, checked here so that it does not rest on the code under test."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from open3d_slam_amd import backend
from open3d_slam_amd import synthetic as syn
from open3d_slam_amd.adjacency_matrix import AdjacencyMatrix
from open3d_slam_amd.submap_collection import SubmapCollection

from multi_submap_restatement import register_multi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle

    pyoracle.build()
    return pyoracle


# ------------------------------------------------------------------------------------------------------------------ 1. the ABI
def test_the_entry_point_is_declared_exported_and_mirrored():
    text = open(os.path.join(ROOT, "include", "o3ds_backend.h")).read()
    assert re.search(r"#define\s+O3DS_MULTI_MAX_TARGETS\s+16\b", text)
    assert re.search(r"#define\s+O3DS_MULTI_UNION\s+0\b", text) and re.search(r"#define\s+O3DS_MULTI_JOINT\s+1\b", text)
    assert re.search(r"int\s+o3ds_icp_register_multi\s*\(\s*o3ds_handle h,\s*int form,\s*o3ds_cloud source,\s*const o3ds_cloud\*\s*targets,"
                     r"\s*size_t n_targets,\s*const o3ds_crop\*\s*target_crop,\s*const double init\[16\],\s*const o3ds_icp_params\*\s*params,"
                     r"\s*o3ds_icp_result\*\s*out\)", text)
    assert "o3ds_icp_register_multi" in backend.SIGNATURES
    res, args = backend.SIGNATURES["o3ds_icp_register_multi"]
    assert len(args) == 9
    assert (backend.Backend.MULTI_UNION, backend.Backend.MULTI_JOINT, backend.Backend.MULTI_MAX_TARGETS) == (0, 1, 16)
    assert shutil.which("nm") is not None
    for lib in (backend.LIB_PATH, backend.LIB_AB_PATH):
        assert os.path.exists(lib), lib + " (build first)"
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
        assert re.search(r"\bT o3ds_icp_register_multi\b", syms), lib


# ------------------------------------------------------------------------------------------------------------------ 2. which submaps
class _Stub:
    def __init__(self, id_, center, empty=False):
        self.id_, self.center, self.empty = id_, np.array(center, dtype=np.float64), empty

    def getMapToSubmapCenter(self):
        return self.center

    def isEmpty(self):
        return self.empty


class _Collection(SubmapCollection):
    def __init__(self, stubs, active, edges, sensor=(0.0, 0.0, 0.0)):  # (no device: the selection only)
        self.submaps_, self.activeSubmapIdx_ = stubs, active
        self.adjacencyMatrix_ = AdjacencyMatrix()
        for a, b in edges:
            self.adjacencyMatrix_.addEdge(a, b)
        self.mapToRangeSensor_ = np.eye(4)
        self.mapToRangeSensor_[:3, 3] = sensor


def _ids(subs):
    return [s.id_ for s in subs]


def test_the_active_submap_comes_first_and_alone_for_k_1():
    stubs = [_Stub(0, [0, 0, 0]), _Stub(1, [1, 0, 0]), _Stub(2, [2, 0, 0])]
    c = _Collection(stubs, 1, [(0, 1), (1, 2)])
    assert _ids(c.getSubmapsForScanMatching(1)) == [1]
    assert _ids(c.getSubmapsForScanMatching(0)) == [1]
    assert c.getSubmapsForScanMatching(3)[0] is stubs[1]


def test_only_submaps_adjacent_to_the_active_one_are_taken():
    stubs = [_Stub(i, [float(i), 0, 0]) for i in range(5)]
    c = _Collection(stubs, 2, [(0, 1), (1, 2), (2, 3), (3, 4)], sensor=(2.0, 0.0, 0.0))
    assert sorted(_ids(c.getSubmapsForScanMatching(5))) == [1, 2, 3]  # 0 and 4 are two hops away
    assert _ids(c.getSubmapsForScanMatching(5))[0] == 2


def test_the_others_are_ordered_by_the_distance_of_their_centre_to_the_sensor():
    stubs = [_Stub(0, [0, 0, 0]), _Stub(1, [5, 0, 0]), _Stub(2, [1, 0, 0]), _Stub(3, [3, 0, 0])]
    c = _Collection(stubs, 0, [(0, 1), (0, 2), (0, 3)], sensor=(0.5, 0.0, 0.0))
    assert _ids(c.getSubmapsForScanMatching(4)) == [0, 2, 3, 1]
    assert _ids(c.getSubmapsForScanMatching(2)) == [0, 2]
    c.mapToRangeSensor_[:3, 3] = [4.5, 0.0, 0.0]
    assert _ids(c.getSubmapsForScanMatching(3)) == [0, 1, 3]


def test_equally_near_centres_go_by_the_lower_id():
    stubs = [_Stub(0, [0, 0, 0]), _Stub(7, [1, 0, 0]), _Stub(3, [-1, 0, 0]), _Stub(5, [0, 1, 0])]
    c = _Collection(stubs, 0, [(0, 7), (0, 3), (0, 5)])
    assert _ids(c.getSubmapsForScanMatching(4)) == [0, 3, 5, 7]
    assert _ids(c.getSubmapsForScanMatching(3)) == [0, 3, 5]


def test_k_larger_than_the_collection_and_empty_submaps():
    stubs = [_Stub(0, [0, 0, 0]), _Stub(1, [1, 0, 0], empty=True), _Stub(2, [2, 0, 0])]
    c = _Collection(stubs, 0, [(0, 1), (0, 2)])
    assert _ids(c.getSubmapsForScanMatching(16)) == [0, 2]  # the empty one is skipped, nothing is repeated
    assert _ids(_Collection([_Stub(0, [0, 0, 0])], 0, []).getSubmapsForScanMatching(8)) == [0]


def test_the_mapper_registers_against_one_submap_by_default():
    import inspect

    from open3d_slam_amd.mapper import Mapper

    assert inspect.signature(Mapper.__init__).parameters["numSubmapsForScanMatching"].default == 1


# ------------------------------------------------------------------------------------------------------------------ 3. the yardstick
def _inputs(n_maps, n_pts=20_000):
    scene = syn.make_scene()
    src = syn.vlp16_scan(scene, syn.ground_truth_pose(), n_az=128)
    maps = [syn.sample_map(scene, n_pts, seed=syn.SEED_MAP + k) for k in range(n_maps)]
    return src, maps


@pytest.mark.parametrize("n_maps", [2, 3])
def test_union_restatement_is_the_registration_against_the_concatenation(oracle, n_maps):
    src, maps = _inputs(n_maps)
    maps.insert(1, (np.zeros((0, 3)), np.zeros((0, 3))))  # an empty target contributes nothing
    maps.append((maps[0][0][:1] + 0.123, maps[0][1][:1]))  # a one-point target
    cat_p, cat_n = np.concatenate([m[0] for m in maps]), np.concatenate([m[1] for m in maps])
    # exact correspondences under the first pose: the union of per-map searches is the search of the concatenation
    from multi_submap_restatement import union_correspondences

    T = np.eye(4)
    trees = [oracle.KDTree(m[0]) if len(m[0]) else None for m in maps]
    got, got_d2 = union_correspondences(oracle, trees, maps, src @ T[:3, :3].T + T[:3, 3], 1.0)
    want, want_d2 = oracle.evaluate(oracle.KDTree(cat_p), src, 1.0)[:2]
    assert np.array_equal(got, np.asarray(want, dtype=np.int64))
    assert np.array_equal(got_d2[got >= 0], want_d2[want >= 0])
    got = register_multi(oracle, "union", src, maps, 1.0, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    ref = oracle.icp_point_to_plane(src, cat_p, cat_n, 1.0, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    np.testing.assert_allclose(got["transformation"], ref["transformation"], atol=1e-9, rtol=0)
    assert got["iterations"] == ref["iterations"] == 10
    assert got["n_corr"] == round(ref["fitness"] * len(src))
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) < 1e-9


def test_joint_restatement_of_one_map_is_the_registration_and_of_two_finds_the_pose(oracle):
    src, maps = _inputs(2, n_pts=40_000)
    one = register_multi(oracle, "joint", src, maps[:1], 1.0, max_iter=30)
    ref = oracle.icp_point_to_plane(src, maps[0][0], maps[0][1], 1.0, max_iter=30)
    np.testing.assert_allclose(one["transformation"], ref["transformation"], atol=1e-9, rtol=0)
    assert one["iterations"] == ref["iterations"] and one["converged"] == ref["converged"]
    two = register_multi(oracle, "joint", src, maps, 1.0, max_iter=30)
    dt, dr = syn.se3_error(two["transformation"], syn.ground_truth_pose())
    assert dt < 5e-3 and dr < 1e-3, (dt, dr)  # the bound tests/test_sharded_cpu.py holds the "submap" partitioning to
    # the same map twice: the record doubles, the pose is the one-map pose
    twice = register_multi(oracle, "joint", src, [maps[0], maps[0]], 1.0, max_iter=30)
    np.testing.assert_allclose(twice["transformation"], one["transformation"], atol=1e-9, rtol=0)
    assert abs(twice["fitness"] - one["fitness"]) < 1e-12
