"""Time per registration of o3ds_icp_degeneracy_aware_dev beside o3ds_icp_robust_dev, the entry point it is modelled on, on the pair of
profiles/robust_icp.txt -- the 65 536-point VLP-16 scan against the 1 M-point map, point-to-plane, L2 loss, r = 1.0, 10 iterations,
convergence thresholds 0, f32 storage.  A host clock around each call (every call ends in the read of its last state), in ONE run on
one device, the four settings taken in turn within every round so that whatever else the machine does falls on all alike:
  robust          o3ds_icp_robust_dev
  robust again    the same call a second time: what two measurements of the same code differ by in this run
  aware (0, 0)    o3ds_icp_degeneracy_aware_dev with both minima 0: the analysis of every pass, then the ordinary tail
  aware (0, 0.34) a translation minimum above 1/3, which the smallest of three values that sum to 1 never reaches: every pass takes
                  the constrained solve (and ends elsewhere: the point is the cost, not the pose)
The first round is not timed; minimum, median and maximum of ROUNDS after it, and each setting's minimum over the first's."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

ROUNDS = 15
R, ITERS = 1.0, 10


def main():
    src, tgt, nrm, T = syn.config2_inputs()
    be = backend.Backend(0, backend.PRECISION_F32)
    s, t = be.upload(src), be.upload(tgt, nrm)
    kw = dict(max_iter=ITERS, rel_fitness=0.0, rel_rmse=0.0)
    settings = (("robust", lambda: be.icp_robust_dev(s, t, R, **kw)),
                ("robust again", lambda: be.icp_robust_dev(s, t, R, **kw)),
                ("aware (0, 0)", lambda: be.icp_degeneracy_aware(s, t, R, 0.0, 0.0, **kw)[0]),
                ("aware (0, 0.34)", lambda: be.icp_degeneracy_aware(s, t, R, 0.0, 0.34, **kw)))
    times = {name: [] for name, _ in settings}
    last = {}
    for rnd in range(ROUNDS + 1):
        for name, call in settings:
            t0 = time.perf_counter()
            last[name] = call()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e6)
    print(f"{len(src)} source points, {len(tgt)} target points, r {R}, {ITERS} iterations ({ITERS + 1} passes), f32 storage; "
          f"whole call, host clock, {ROUNDS} rounds:")
    base = min(times["robust"])
    for name, _ in settings:
        v = times[name]
        print(f"  {name:16s} min {min(v):8.1f} us  median {np.median(v):8.1f} us  max {max(v):8.1f} us  = {min(v) / base:.3f} x robust "
              f"({(min(v) - base) / (ITERS + 1):+.2f} us per pass)")
    same = last["robust"]["transformation"].tobytes() == last["aware (0, 0)"]["transformation"].tobytes()
    res, rep = last["aware (0, 0.34)"]
    dt, dr = syn.se3_error(last["robust"]["transformation"], T)
    print(f"  robust and aware (0, 0) end at the same pose bit for bit: {same}; |dt| {dt:.2e} m, angle {dr:.2e} rad")
    print(f"  aware (0, 0.34): {rep['n_passes_constrained']} of {res['iterations']} updates constrained, dropped ever {rep['ever_degenerate'].tolist()}, "
          f"last normalised eigenvalues {np.array2string(rep['eigenvalues'], precision=4)}")
    be.close()


if __name__ == "__main__":
    main()
