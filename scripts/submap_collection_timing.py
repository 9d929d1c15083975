"""Scans/s of the configs[2] stream (bench.stream_parameters(), the OS-128 figure-eight) through the single-submap Mapper and through a
Mapper that maps into a SubmapCollection, at the shipped 20 m radius and at 2 m (several switches); and the wall time of one
loop-closure cycle (loop_closure.py: features, odometry constraints, place recognition, the pose graph, the submap update) on the 2 m
run.  Each leg runs the stream once untimed on its own handle first (kernel loading, pools).  Prints one JSON line.  No number of the
reference's SubmapCollection exists on this machine: none is compared against."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from open3d_slam_amd import backend, synthetic as syn  # noqa: E402
from open3d_slam_amd.loop_closure import LoopClosure  # noqa: E402
from open3d_slam_amd.mapper import Mapper  # noqa: E402
from open3d_slam_amd.odometry import LidarOdometry  # noqa: E402
from open3d_slam_amd.pointcloud import PointCloud  # noqa: E402
from open3d_slam_amd.submap_collection import SubmapCollection  # noqa: E402

FRAMES = 200


def run(scans, radius, collection, loop_closures=False):
    mp, op = bench.stream_parameters()
    mp.submaps_.radius_ = radius
    mp.isAttemptLoopClosures_ = loop_closures
    mp.placeRecognition_.loopClosureSearchRadius_ = 2.0 * radius
    be = backend.Backend(0)
    odo = LidarOdometry(be)
    odo.setParameters(op)
    mapper = Mapper(be, odo, submaps=SubmapCollection(be) if collection else None)
    mapper.setParameters(mp)
    lc = LoopClosure(be, mapper) if loop_closures else None
    cycles = []
    t0 = time.perf_counter()
    for k, raw in enumerate(scans):
        cloud = PointCloud.from_pointcloud2(be, raw)
        odo.addRangeScan(cloud, 0.1 * k) and mapper.addRangeMeasurement(cloud, 0.1 * k)
        cloud.release()
        if lc is not None and mapper.getSubmaps().numFinishedSubmaps() > 0:
            c0 = time.perf_counter()
            n = len(lc.run())
            be.synchronize()
            cycles.append((round((time.perf_counter() - c0) * 1e3, 3), n))
    be.synchronize()
    wall = time.perf_counter() - t0
    n_sub = mapper.getSubmaps().getNumSubmaps() if collection else 1
    be.close()
    return {"scans_per_s": round(len(scans) / wall, 2), "submaps": n_sub, "cycles_ms_and_constraints": cycles}


def main():
    scene = syn.make_scene()
    poses = syn.figure_eight_poses(FRAMES, 0.1)
    scans = [np.asarray(syn.os128_scan(scene, poses[k], frame=k), dtype=np.float32) for k in range(FRAMES)]
    out = {"frames": FRAMES}
    for name, radius, collection in (("mapper", 20.0, False), ("collection_20m", 20.0, True), ("collection_2m", 2.0, True)):
        run(scans[:20], radius, collection)  # warm-up
        out[name] = run(scans, radius, collection)
    run(scans[:40], 2.0, True, loop_closures=True)
    lc = run(scans, 2.0, True, loop_closures=True)
    out["collection_2m_with_loop_closure"] = lc
    closing = [ms for ms, n in lc["cycles_ms_and_constraints"] if n > 0]
    out["loop_closure_cycle_ms"] = closing[0] if closing else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
