"""Times o3ds_icp_register_batch against B sequential o3ds_icp_register_dev calls in the same process, on one GPU: B = 1, 2, 4, 8, 16
entries, sources of 4 096, 18 000 and 65 536 points (prefixes of a shuffled 65 536-point scan, each entry from its own initial guess
near the ground truth), a 100 000-point and a 1 000 000-point target, point-to-plane and generalized ICP, 10 iterations
(relative_* = 0).  Every registration ends with the host reading the final state, so host wall time around the call (after a stream
synchronise) spans the device work; each cell is the median of --reps runs after --warmup, with the spread (min .. max).
Which caller should use which: a batch of SMALL sources (a few thousand points: loop-closure refinements, odometry constraints between
submaps, several guesses for one pair) fills the device where one of them cannot; LARGE sources already fill it, and the one-pair call
has candidate sets and the fused loop, which the batch has not -- see the cells below where the batch loses.
    python scripts/batch_icp_timing.py [--reps 9] [--warmup 2] [--out profiles/batch_icp.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from open3d_slam_amd import backend  # noqa: E402
from open3d_slam_amd import synthetic as syn  # noqa: E402

R = 1.0


def timed(be, fn, reps, warmup):
    t = []
    for k in range(warmup + reps):
        be.synchronize()
        t0 = time.perf_counter()
        fn()
        be.synchronize()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return np.array(t)


def fmt(t):
    return f"{np.median(t):8.3f} ms ({t.min():.3f} .. {t.max():.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "batch_icp.txt"))
    ap.add_argument("--targets", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--sources", type=int, nargs="+", default=[4096, 18_000, 65_536])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    a = ap.parse_args()
    scene = syn.make_scene()
    gt = syn.ground_truth_pose()
    scan = syn.vlp16_scan(scene, gt, n_az=4096)
    scan = scan[np.random.default_rng(3).permutation(len(scan))]
    rng = np.random.default_rng(4)
    inits = [syn.make_pose(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.5, 0.5, 3)) @ gt for _ in range(max(a.batches))]
    be = backend.Backend(0)
    lines = [f"batch_icp_timing: 10 iterations, median of {a.reps} runs after {a.warmup} (min .. max); batch = one o3ds_icp_register_batch, "
             "sequential = B x o3ds_icp_register_dev"]
    for n_tgt in a.targets:
        tp, tn = syn.sample_map(scene, n_tgt)
        t = be.upload(tp, tn)
        be.build_index(t, R)
        for n_src in a.sources:
            s = be.upload(scan[:n_src])
            be.estimate_normals(s, 2.0, 10)
            for method, name in ((backend.ICP_POINT_TO_PLANE, "point-to-plane"), (backend.ICP_GENERALIZED, "generalized")):
                params = backend.Backend._params(R, 10, 0.0, 0.0, method)
                for nb in a.batches:
                    entries = [(s, t, None, inits[k]) for k in range(nb)]
                    t_batch = timed(be, lambda: be.icp_register_batch(entries, params), a.reps, a.warmup)
                    t_seq = timed(be, lambda: [be.icp_register_dev(s, t, R, init=e[3], max_iter=10, rel_fitness=0.0, rel_rmse=0.0, method=method)
                                               for e in entries], a.reps, a.warmup)
                    lines.append(f"target {n_tgt:8d} source {n_src:6d} {name:15s} B={nb:2d}  batch {fmt(t_batch)}  sequential {fmt(t_seq)}  "
                                 f"ratio {np.median(t_batch) / np.median(t_seq):.2f}")
                    print(lines[-1], flush=True)
            be.free(s)
        be.free(t)
    be.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
