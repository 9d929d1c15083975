"""Device time of o3ds_segment_plane for the whole call (host clock around the call, which waits for its result) and of its evaluation
kernel alone (hipEvents around its launches: the library's internal span 14, summed over the batches of a call) on the config-2 inputs --
the 65 536-point VLP-16 scan and the 1 M-point map -- with num_iterations 100 and 1 000, distance_threshold 0.05, ransac_n 3, in both
storages.  Beside each time, two floors:
  * one read of the points: o3ds_cloud_center on the same cloud in the same process (host clock around the call, minimum of 7);
  * the VALU issue bound of the evaluation loop: instructions per point per wavefront (EVAL_VALU, counted in the gfx950 disassembly of
    plane_eval_kernel's unrolled loop body: total VALU instructions / 8 points) * 4 cycles per wavefront instruction * n points * groups of
    64 hypotheses / (1024 SIMDs * 2.4 GHz).
The first call of every configuration is not timed; minimum of 7 after it.  Prints one block per configuration.  DESIGN.md 7.8."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

REPS = 7
THRESHOLD, RANSAC_N, SEED = 0.05, 3, 0
EVAL_VALU = {"f32": 116 / 8, "f64": 92 / 8}  # VALU instructions per point per wavefront in the unrolled loop of plane_eval_kernel
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 256 * 4, 2.4e9, 4
SPAN_EVAL = 14


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e6, out


def main():
    src, tgt, _, T = syn.config2_inputs()
    src = (np.c_[src, np.ones(len(src))] @ T.T)[:, :3]  # the scan where it was taken
    for storage, precision in (("f32", backend.PRECISION_F32), ("f64", backend.PRECISION_F64)):
        be = backend.Backend(0, precision)
        be.profile_enable(2)
        for name, pts in (("scan", src), ("map", tgt)):
            cid, n = be.upload(pts), len(pts)
            be.cloud_center(cid)
            center = min(wall(lambda: be.cloud_center(cid))[0] for _ in range(REPS))
            for iters in (100, 1000):
                plane, idx, res = be.segment_plane(cid, THRESHOLD, RANSAC_N, iters, SEED)  # (untimed)
                be.span_read(SPAN_EVAL)
                whole, kern = [], []
                for _ in range(REPS):
                    whole.append(wall(lambda: be.segment_plane(cid, THRESHOLD, RANSAC_N, iters, SEED))[0])
                    kern.append(be.span_read(SPAN_EVAL)[1] * 1e3)
                split, got = wall(lambda: be.segment_plane(cid, THRESHOLD, RANSAC_N, iters, SEED, split=True))
                be.free(got[3])
                be.free(got[4])
                be.span_read(SPAN_EVAL)
                groups = (iters + 63) // 64
                valu = EVAL_VALU[storage] * CYCLES_PER_VALU * n * groups / (SIMDS * CLOCK_HZ) * 1e6
                floor = max(center, valu)
                print(f"{name}, {storage}, num_iterations {iters}: {n} points, {res.n_inliers} inliers, best_t {res.best_t}, "
                      f"plane {np.round(plane, 4).tolist()}")
                print(f"  whole call (indices downloaded, no cloud made): min {min(whole):.1f} us median {np.median(whole):.1f} us; "
                      f"once with both clouds made: {split:.1f} us")
                print(f"  evaluation kernel (span {SPAN_EVAL}): min {min(kern):.1f} us median {np.median(kern):.1f} us")
                print(f"  floors: one read of the points (o3ds_cloud_center, whole call) {center:.1f} us; VALU issue bound {valu:.1f} us "
                      f"({EVAL_VALU[storage]:.1f} instructions per point per wavefront, {groups} groups)")
                print(f"  evaluation kernel / larger floor = {min(kern) / floor:.2f}")
                sys.stdout.flush()
            be.free(cid)
        be.close()


if __name__ == "__main__":
    main()
