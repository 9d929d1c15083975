"""Per-LM-step time of o3ds_global_optimization on one MI355X at N = 20, 100, 500, 1000, 2000 nodes (the figure-eight graph of
tests/pose_graph_restatement.py, drift scaled to N), next to the numpy / LAPACK restatement's time for the same step on the host CPU:
ComputeLinearSystem plus one dense solve of the 6N system.  A device step is one solve, the pose update, the per-edge pass, the b
assembly and the record read-back (plus an H assembly after an accepted step).  Prints one JSON line per N.  Under
`rocprofv3 --kernel-trace --stats -- python scripts/pose_graph_timing.py` the kernel table splits the step into assembly, factorisation,
substitution and update; profiles/pose_graph.txt holds it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_graph_restatement as rs  # noqa: E402

from open3d_slam_amd import backend  # noqa: E402

OPT = dict(max_correspondence_distance=1.0, edge_prune_threshold=0.2, preference_loop_closure=2.0, reference_node=0)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [20, 100, 500, 1000, 2000]
    cpu = os.environ.get("PG_TIMING_CPU", "1") != "0"
    be = backend.Backend(0, backend.PRECISION_F64)
    for n in sizes:
        _, T0, E = rs.figure_eight_graph(n_nodes=n, drift_yaw=0.15 / n, n_points=300)
        edges = [(e.source, e.target, e.transformation, e.information, e.uncertain) for e in E]
        be.global_optimization(T0, edges, max_iteration=0, **OPT)  # warm-up
        reps, best = 3, None
        for _ in range(reps):
            t0 = time.perf_counter()
            r = be.global_optimization(T0, edges, max_iteration=4, **OPT)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        steps = sum(r["lm_steps"])
        out = dict(n=n, rows=6 * n, call_ms=round(best * 1e3, 3), lm_steps=steps, ms_per_step=round(best * 1e3 / max(steps, 1), 3))
        if cpu and n <= 2000:
            nodes = [T.copy() for T in T0]
            zeta = rs.compute_zeta(nodes, E)
            t0 = time.perf_counter()
            H, b = rs.compute_linear_system(nodes, E, zeta)
            t1 = time.perf_counter()
            np.linalg.solve(H + 1e-5 * H.diagonal().max() * np.eye(len(H)), b)
            t2 = time.perf_counter()
            out.update(cpu_assembly_ms=round((t1 - t0) * 1e3, 3), cpu_solve_ms=round((t2 - t1) * 1e3, 3), cpu_threads=os.cpu_count())
        print(json.dumps(out), flush=True)
    be.close()


if __name__ == "__main__":
    main()
