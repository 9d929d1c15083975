"""Time of the neighbour-search kernel (hipEvents around its launch: the library's internal span 10) on the config-2 inputs: the 65 536-point
scan against the 1 M-point map, KNN at max_nn 1 and 20, and the scan against itself in Hybrid mode (r = 3.0, max_nn 20) with and
without `total`; beside it the two kernels of estimate_normals(3.0, 20) on the same scan (span 8), the yardstick of the same-cloud case.
The first call of every configuration builds or finds the index and is not timed.  Prints one line per configuration.  DESIGN.md 7.6."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

REPS = 7
U32P = C.POINTER(C.c_uint32)


def search(be, q, t, n, k, radius, want_total):
    idx, cnt, tot = np.zeros((n, k), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    be._ck(be.lib.o3ds_neighbor_search(be.h, q, t, None, None, n, k, radius, idx.ctypes.data_as(U32P), None, cnt.ctypes.data_as(U32P),
                                       tot.ctypes.data_as(U32P) if want_total else None))
    return cnt


def main():
    src, tgt, _, T = syn.config2_inputs()
    src = (np.c_[src, np.ones(len(src))] @ T.T)[:, :3]  # the scan where it was taken: inside the map
    be = backend.Backend(0, backend.PRECISION_F32)
    scan, world = be.upload(src), be.upload(tgt)
    n = len(src)
    be.profile_enable(2)
    for name, q, t, k, r, want_total in (("scan -> map, KNN 1", scan, world, 1, 0.0, False), ("scan -> map, KNN 20", scan, world, 20, 0.0, False),
                                         ("scan -> scan, Hybrid (3.0, 20), lists only", scan, scan, 20, 3.0, False),
                                         ("scan -> scan, Hybrid (3.0, 20), with total", scan, scan, 20, 3.0, True)):
        cnt = search(be, q, t, n, k, r, want_total)
        be.span_read(10)
        ms = []
        for _ in range(REPS):
            search(be, q, t, n, k, r, want_total)
            ms.append(be.span_read(10)[1])
        print(f"{name}: {n} queries, kernel min {min(ms) * 1e3:.1f} us median {np.median(ms) * 1e3:.1f} us "
              f"({min(ms) * 1e6 / n:.2f} ns per query; mean count {cnt.mean():.2f})", flush=True)
    be.estimate_normals(scan, 3.0, 20)
    be.span_read(8)
    ms = []
    for _ in range(REPS):
        be.estimate_normals(scan, 3.0, 20)
        ms.append(be.span_read(8)[1])
    print(f"estimate_normals(3.0, 20) on the scan: {n} points, kernels min {min(ms) * 1e3:.1f} us median {np.median(ms) * 1e3:.1f} us "
          f"({min(ms) * 1e6 / n:.2f} ns per point)", flush=True)
    be.close()


if __name__ == "__main__":
    main()
