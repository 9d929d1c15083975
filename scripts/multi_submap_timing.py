"""Times o3ds_icp_register_multi against what was available before it, on one GPU: K = 1, 2, 4, 8 resident maps of 1 M points, the
65 536-point scan of configs[1], 10 iterations (relative_* = 0), point-to-plane and generalized ICP.  Rows per K and estimator:
  union / joint        one o3ds_icp_register_multi call;
  append+index+reg     the alternative without it: append the K maps into a copy, o3ds_cloud_build_index, o3ds_icp_register_dev on the
                       copy (the three parts reported separately and summed; the copy's index is rebuilt every time, as a caller would
                       have to after any submap changed);
  K x register_dev     K one-target registrations in sequence (what JOINT replaces in device time).
Every registration ends with the host reading the final state, so host wall time around the call (after a stream synchronise) spans
the device work; each row is the median of --reps runs after --warmup, with the spread (min .. max).
    python scripts/multi_submap_timing.py [--reps 15] [--warmup 3] [--ks 1 2 4 8] [--out profiles/multi_submap.txt]"""
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
    return f"{np.median(t):9.3f} ms  ({t.min():.3f} .. {t.max():.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_submap.txt"))
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    a = ap.parse_args()
    scene = syn.make_scene()
    src, tgt0, nrm0, _ = syn.config2_inputs(n_map=a.points, n_az=4096)
    maps = [(tgt0, nrm0)] + [syn.sample_map(scene, a.points, seed=syn.SEED_MAP + k) for k in range(1, max(a.ks))]
    be = backend.Backend(0)
    lines = [f"multi_submap_timing: {a.points} points per map, scan {len(src)} points, 10 iterations, median of {a.reps} runs after {a.warmup} (min .. max)"]
    s = be.upload(src)
    be.estimate_normals(s, 2.0, 10)
    ids = []
    for p, n in maps:
        cid = be.upload(p, n)
        be.build_index(cid, R)
        ids.append(cid)
    everything = backend.make_crop(backend.CROP_MAX_RADIUS, rmax=1e9)
    for method, name in ((backend.ICP_POINT_TO_PLANE, "point-to-plane"), (backend.ICP_GENERALIZED, "generalized")):
        params = backend.Backend._params(R, 10, 0.0, 0.0, method)
        for K in a.ks:
            sub = ids[:K]
            t_union = timed(be, lambda: be.icp_register_multi(s, sub, form=be.MULTI_UNION, params=params), a.reps, a.warmup)
            t_joint = timed(be, lambda: be.icp_register_multi(s, sub, form=be.MULTI_JOINT, params=params), a.reps, a.warmup)
            t_seq = timed(be, lambda: [be.icp_register_dev(s, c, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0, method=method) for c in sub],
                          a.reps, a.warmup)
            parts = {"append": [], "index": [], "register": []}
            for k in range(a.warmup + a.reps):
                be.synchronize()
                t0 = time.perf_counter()
                cat = be.crop_cloud(sub[0], everything)
                for c in sub[1:]:
                    be.cloud_append(cat, c)
                be.synchronize()
                t1 = time.perf_counter()
                be.build_index(cat, R)
                be.synchronize()
                t2 = time.perf_counter()
                be.icp_register_dev(s, cat, R, max_iter=10, rel_fitness=0.0, rel_rmse=0.0, method=method)
                be.synchronize()
                t3 = time.perf_counter()
                be.free(cat)
                if k >= a.warmup:
                    parts["append"].append((t1 - t0) * 1e3)
                    parts["index"].append((t2 - t1) * 1e3)
                    parts["register"].append((t3 - t2) * 1e3)
            pa = {k: np.array(v) for k, v in parts.items()}
            total = pa["append"] + pa["index"] + pa["register"]
            lines += [f"{name} K={K}",
                      f"  register_multi UNION        {fmt(t_union)}",
                      f"  register_multi JOINT        {fmt(t_joint)}",
                      f"  append + index + register   {fmt(total)}   = append {np.median(pa['append']):.3f} + index {np.median(pa['index']):.3f} + register {np.median(pa['register']):.3f}",
                      f"  K x register_dev            {fmt(t_seq)}"]
            print("\n".join(lines[-5:]), flush=True)
    be.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
