"""Stage-by-stage wall time of place recognition on one MI355X for the end-to-end pair of tests/test_place_recognition_gpu.py (two
submaps of a boxes-and-cylinders scene, 35 deg / 3.6 m apart): FPFH per submap, feature matching, RANSAC (hypotheses run, validations)
and the ICP refinement, next to the wall time of the numpy / scipy restatement of the FPFH and the matching for scale.  Prints one JSON
line.  Under `rocprofv3 --kernel-trace --stats -- python scripts/place_recognition_timing.py` the kernel table is what
profiles/place_recognition.txt holds.  No Open3D number exists on this machine: none is compared against."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fpfh_ransac_restatement as rs  # noqa: E402
import test_place_recognition_gpu as t  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

from open3d_slam_amd import backend, parameters as prm  # noqa: E402
from open3d_slam_amd.place_recognition import PlaceRecognition  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402


def ms(t0):
    return round((time.perf_counter() - t0) * 1e3, 3)


def main():
    be = backend.Backend(0, backend.PRECISION_F64)
    rng = np.random.default_rng(77)
    T_gt = t.make_T(35.0, [3.0, -2.0, 0.3])
    p = t.pr_params()
    p.placeRecognition_.consistencyCheck_ = prm.PlaceRecognitionConsistencyCheckParameters()
    c = p.placeRecognition_
    out = {}
    subs = []
    for k, pts in enumerate((t.scene_points(rng), t.scene_points(rng) @ T_gt[:3, :3].T + T_gt[:3, 3])):
        sm = t.make_submap(be, pts, p, k)  # warm-up of every kernel on the way
        be.synchronize()
        t0 = time.perf_counter()
        sm.computeFeatures()
        be.synchronize()
        out[f"features_submap{k}_ms"] = ms(t0)
        out[f"sparse_points_submap{k}"] = len(sm.getSparseMapPointCloud())
        subs.append(sm)
    a, b = subs
    sa, sb = a.getSparseMapPointCloud(), b.getSparseMapPointCloud()
    t0 = time.perf_counter()
    be.compute_fpfh(sa.id, c.featureRadius_, c.featureKnn_)
    be.synchronize()
    out["fpfh_only_submap0_ms"] = ms(t0)
    t0 = time.perf_counter()
    corr, fb = be.feature_correspondences(sa.id, sb.id, True, c.ransacModelSize_)
    out["matching_ms"] = ms(t0)
    out["feature_correspondences"] = len(corr)
    rec = PlaceRecognition(be, p, seed=7)
    t0 = time.perf_counter()
    r = rec.ransac(a, b)
    out["ransac_ms"] = ms(t0)
    out["ransac_hypotheses_run"] = r["iterations_run"]
    out["ransac_validations"] = r["validations"]
    out["ransac_fitness"] = r["fitness"]
    src, tgt = a.getMapPointCloud(), b.getMapPointCloud()
    t0 = time.perf_counter()
    i_s, i_t = be.overlap_indices(src.id, tgt.id, r["transformation"], 20 * p.mapBuilder_.mapVoxelSize_, 1)
    so = PointCloud(be, be.select_by_index(src.id, i_s.astype(np.uint32)))
    to = PointCloud(be, be.select_by_index(tgt.id, i_t.astype(np.uint32)))
    icp = rec.cloudRegistration.registerClouds(so, to, r["transformation"])
    out["refinement_ms"] = ms(t0)
    out["refinement_fitness"] = icp.fitness_
    t0 = time.perf_counter()
    cons = rec.buildLoopClosureConstraints(a, [b])
    out["build_loop_closure_constraints_ms"] = ms(t0)
    out["constraints"] = len(cons)
    # the restatement, for scale (one core of the host)
    P, _ = be.download(sa.id)
    N = be.download(sa.id)[1]
    t0 = time.perf_counter()
    rs.fpfh(P, N, c.featureRadius_, c.featureKnn_, cKDTree(P))
    out["restatement_fpfh_submap0_ms"] = ms(t0)
    Fa, Fb = a.getFeatures(), b.getFeatures()
    t0 = time.perf_counter()
    cKDTree(Fb).query(Fa, k=1)
    cKDTree(Fa).query(Fb, k=1)
    out["restatement_matching_ms"] = ms(t0)
    be.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
