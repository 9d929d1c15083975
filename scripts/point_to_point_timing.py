"""Time of a point-to-point registration (o3ds_icp_register_dev, method point-to-point) on the configs[1] pair -- the 65 536-point VLP-16
scan against the 1 M-point map --, 10 iterations (11 passes), thresholds 0, for two builds of the library in ONE run:
    python scripts/point_to_point_timing.py LIB_A LIB_B [rounds]
Every round starts one child process per library, A and B in turn (a process loads one library); a child uploads the pair, runs the
registration 3 times untimed and 30 times under a host clock (the call returns after the device has finished), and prints the times.
Reported per library: the median of every round, then the median and the spread (max - min) of those medians.  The spread of A's own
rounds is what a difference between A and B has to exceed to mean anything.  The poses of the two builds are compared bit for bit, near
the origin (f32 and f64 storage) -- profiles/point_to_point_pivot.txt."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS, ITERS = 3, 30, 10


def child():
    import time

    import numpy as np
    import torch  # noqa: F401  (before the backend: tests/conftest.py)

    from open3d_slam_amd import backend, synthetic as syn

    src, tgt, _, _ = syn.config2_inputs()
    out = {}
    for name, prec in (("f32", backend.PRECISION_F32), ("f64", backend.PRECISION_F64)):
        be = backend.Backend(0, prec)
        s, t = be.upload(src), be.upload(tgt)
        be.build_index(t, 1.0)
        kw = dict(max_iter=ITERS, rel_fitness=0.0, rel_rmse=0.0, method=backend.ICP_POINT_TO_POINT)
        times = []
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            r = be.icp_register_dev(s, t, 1.0, **kw)
            if k >= WARM:
                times.append((time.perf_counter() - t0) * 1e6)
        out[name] = dict(us=times, T=np.asarray(r["transformation"]).view(np.uint64).reshape(-1).tolist(), n_corr=r["n_corr"])
        be.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    import numpy as np

    libs = sys.argv[1:3]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    med = {lib: {"f32": [], "f64": []} for lib in libs}
    poses = {lib: None for lib in libs}
    for _ in range(rounds):
        for lib in libs:
            env = dict(os.environ, O3DS_BACKEND_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:
                sys.exit("child failed (%s): %s" % (lib, p.stderr[-2000:]))
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
            for st in ("f32", "f64"):
                med[lib][st].append(float(np.median(res[st]["us"])))
            pose = {st: (res[st]["T"], res[st]["n_corr"]) for st in ("f32", "f64")}
            assert poses[lib] is None or poses[lib] == pose, "a build differs from itself between rounds"
            poses[lib] = pose
    for st in ("f32", "f64"):
        for lib in libs:
            m = med[lib][st]
            print("%s %s: medians of %d rounds (us, %d passes each) %s -> median %.1f, spread %.1f" % (
                st, lib, rounds, ITERS + 1, " ".join("%.1f" % v for v in m), np.median(m), max(m) - min(m)))
    print("poses of the two builds bit-identical:", poses[libs[0]] == poses[libs[1]])


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
