"""Device time of o3ds_cluster_dbscan per kernel and for the whole call (hipEvents around the launches: the library's internal spans 10 --
the count of |N_i| --, 11 -- hooking --, 12 -- flatten and the rank scan --, 13 -- the border walk, labels and sizes) on the config-2
inputs, the 65 536-point scan and the 1 M-point map, eps 0.3 and 1.0, min_points 10, f32 storage.  The yardstick is the count-only Radius
search of the same eps on the same cloud (o3ds_neighbor_search, max_nn = 0; span 10), timed in the same process on the same index.  The
first call of every configuration builds the index and is not timed; minimum of 7 after it.  Prints one block per configuration.
DESIGN.md 7.7."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

REPS = 7
U32P = C.POINTER(C.c_uint32)
MIN_POINTS = 10


def count_search(be, cid, n, eps):
    cnt, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    be._ck(be.lib.o3ds_neighbor_search(be.h, cid, cid, None, None, n, 0, eps, None, None, cnt.ctypes.data_as(U32P), tot.ctypes.data_as(U32P)))
    return tot


def main():
    src, tgt, _, T = syn.config2_inputs()
    src = (np.c_[src, np.ones(len(src))] @ T.T)[:, :3]  # the scan where it was taken
    be = backend.Backend(0, backend.PRECISION_F32)
    be.profile_enable(2)
    for name, pts in (("scan", src), ("map", tgt)):
        for eps in (0.3, 1.0):
            cid, n = be.upload(pts), len(pts)
            tot = count_search(be, cid, n, eps)  # (builds the index; untimed)
            be.span_read(10)
            yard = []
            for _ in range(REPS):
                count_search(be, cid, n, eps)
                yard.append(be.span_read(10)[1])
            labels, n_clusters, sizes = be.cluster_dbscan(cid, eps, MIN_POINTS)  # (untimed)
            for tag in (10, 11, 12, 13):
                be.span_read(tag)
            rows = []
            for _ in range(REPS):
                be.cluster_dbscan(cid, eps, MIN_POINTS)
                rows.append([be.span_read(tag)[1] for tag in (10, 11, 12, 13)])
            rows = np.asarray(rows)
            whole = rows.sum(axis=1)
            k = int(np.argmin(whole))
            core = int((tot >= MIN_POINTS).sum())
            print(f"{name}, eps {eps}, min_points {MIN_POINTS}: {n} points, mean |N| {tot.mean():.1f}, max |N| {tot.max()}, {core} core, "
                  f"{n_clusters} clusters, {int((labels < 0).sum())} noise, largest cluster {int(sizes.max()) if n_clusters else 0}")
            print(f"  yardstick (count-only Radius search): min {min(yard) * 1e3:.1f} us median {np.median(yard) * 1e3:.1f} us")
            print(f"  whole call on the device: min {whole[k] * 1e3:.1f} us median {np.median(whole) * 1e3:.1f} us = {whole[k] / min(yard):.2f} x the yardstick")
            for tag, what, v in zip((10, 11, 12, 13), ("count |N_i|", "hooking", "flatten + rank scan", "border walk, labels, sizes"), rows.T):
                print(f"    span {tag} {what}: min {v.min() * 1e3:.1f} us, in the fastest call {v[k] * 1e3:.1f} us")
            sys.stdout.flush()
            be.free(cid)
    be.close()


if __name__ == "__main__":
    main()
