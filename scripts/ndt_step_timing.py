"""Device time of the search-free (NDT) step beside the search-based robust step, on the pair of profiles/robust_icp.txt -- the
65 536-point VLP-16 scan against the 1 M-point map of configs[1], f32 storage -- read from the library's own profile spans:
  build        span 18: the kernels of o3ds_voxel_gaussians_create (keys, sort, segment heads, statistics), once per target
  ndt 1 / 7    span 19: the two kernels of one o3ds_ndt_step, neighbourhood 1 and 7, Cauchy(1)
  search+step  span 10 + span 17 of one o3ds_robust_icp_step (point-to-plane, Cauchy(0.1), r = 1.0): the neighbour search and the two
               kernels of the weighted step -- what a pass of the coloured, robust and degeneracy-aware registrations pays (the tuned
               passes of o3ds_icp_register_dev are another search and are not measured here)
each under the identity (a first pass, 0.36 m and 2 degrees off) and under the ground truth (a last pass).  WARMUP rounds are not read;
within every one of ROUNDS rounds the settings are taken in turn, so that whatever else the machine does falls on all alike; minimum, median and maximum.
The spans are device events around the kernels: host overheads of a call are not in them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

WARMUP, ROUNDS = 3, 20
R, VOXEL = 1.0, 1.0
SPAN_SEARCH, SPAN_ROBUST, SPAN_BUILD, SPAN_NDT = 10, 17, 18, 19


def main():
    src, tgt, nrm, T_true = syn.config2_inputs()
    be = backend.Backend(0, backend.PRECISION_F32)
    s, t = be.upload(src), be.upload(tgt, nrm)
    be.profile_enable(2)
    poses = (("identity", np.eye(4)), ("truth", np.asarray(T_true, dtype=np.float64)))
    times, info = {}, None

    def read(name, *tags):
        us = 0.0
        for tag in tags:
            n, ms = be.span_read(tag)
            assert n == 1, (name, tag, n)
            us += 1e3 * ms
        times.setdefault(name, []).append(us)

    records = {}
    for rnd in range(WARMUP + ROUNDS):
        g, info = be.voxel_gaussians_create(t, VOXEL)
        read("build", SPAN_BUILD)
        for pname, T in poses:
            for nb in (1, 7):
                records[(pname, nb)] = be.ndt_step(s, g, nb, (backend.LOSS_CAUCHY, 1.0), T=T)
                read(f"ndt {nb} ({pname})", SPAN_NDT)
            records[(pname, "robust")] = be.robust_icp_step(s, t, R, backend.ROBUST_POINT_TO_PLANE, (backend.LOSS_CAUCHY, 0.1), T=T)
            read(f"search+step ({pname})", SPAN_SEARCH, SPAN_ROBUST)
        be.voxel_gaussians_free(g)
    be.profile_enable(0)
    print(f"{len(src)} source points, {len(tgt)} target points, f32 storage; voxel {VOXEL} m: {info}; r {R} m; device spans, "
          f"{ROUNDS} rounds after {WARMUP}:")
    for name, v in times.items():
        v = v[WARMUP:]
        print(f"  {name:24s} min {min(v):9.1f} us  median {np.median(v):9.1f} us  max {max(v):9.1f} us")
    for pname, _ in poses:
        base = min(times[f"search+step ({pname})"][WARMUP:])
        for nb in (1, 7):
            print(f"  ndt {nb} / search+step ({pname}): {min(times[f'ndt {nb} ({pname})'][WARMUP:]) / base:.3f}")
        print(f"  matched ({pname}): ndt 1 {int(records[(pname, 1)][28])}, ndt 7 {int(records[(pname, 7)][28])}, "
              f"search {int(records[(pname, 'robust')][28])} of {len(src)}")
    be.close()


if __name__ == "__main__":
    main()
