"""What tests/test_pose_graph_edges_cpu.py and tests/test_pose_graph_edges_gpu.py share: which scenarios of the restatement are run with
which criteria, and the figures, measured on the restatement alone, that the GPU tolerances are derived from."""
from pose_graph_restatement import Option, all_outliers_graph, figure_eight_graph, hub_graph, scrambled_graph

# The long runs with rejected steps: name -> (builder, its arguments, criteria, and what the restatement itself gives when its solve is LU
# and when it is solve_cholesky: the largest differences in a pose entry, in a confidence and in a pass's relative residual).  Rounding is
# amplified over tens of LM steps, so the device is held to LONG_RUN_MULTIPLE times these figures (the inherited 1e-9, 1e-12 and 1e-9
# where that is more); test_pose_graph_edges_cpu.py measures them again and pins that every run is decision-stable.
LONG_RUN_MULTIPLE = 16.0
LONG_RUNS = {
    "scrambled21": (scrambled_graph, dict(n_nodes=21, seed=11), dict(max_iteration=20), (1.43e-11, 1.30e-16, 3.98e-10)),
    "scrambled30": (scrambled_graph, dict(n_nodes=30, seed=13), dict(), (1.58e-9, 1.65e-15, 4.47e-10)),
    "certain21": (scrambled_graph, dict(n_nodes=21, seed=13, certain=True), dict(max_iteration=20), (4.27e-9, 0.0, 5.18e-10)),
    "certain30": (scrambled_graph, dict(n_nodes=30, seed=11, certain=True), dict(max_iteration=20), (1.58e-8, 0.0, 9.52e-9)),
    "lm2_certain30": (scrambled_graph, dict(n_nodes=30, seed=11, certain=True), dict(max_iteration=12, max_iteration_lm=2), (9.61e-9, 0.0, 1.80e-11)),
    "all_outliers": (all_outliers_graph, dict(seed=9), dict(), (1.66e-8, 1.48e-20, 0.0)),
}


def long_run_tolerances(name):
    pose, conf, res = LONG_RUNS[name][3]
    return max(1e-9, LONG_RUN_MULTIPLE * pose), max(1e-12, LONG_RUN_MULTIPLE * conf), max(1e-9, LONG_RUN_MULTIPLE * res)


# One LM step in isolation: every edge uncertain and edge_prune_threshold = 1, so pass 2 has no edge and the poses are pass 1's single step.
ONE_STEP_GRAPHS = {
    "band21": lambda: figure_eight_graph(21, 0.15 / 21, n_points=300),
    "band30": lambda: figure_eight_graph(30, 0.15 / 30, n_points=300),
    "hub21": lambda: hub_graph(21),
    "hub30": lambda: hub_graph(30),
    "hub60": lambda: hub_graph(60),
}
ONE_STEP_OPTION = Option(1.0, 1.0, 2.0, -1)
# |delta - solve_refined| / (cond(H + lambda I) 2^-53 |delta|) of the restatement's own f64 solves, the step read back from the poses as
# the device's is: LU 0.0036 0.0099 0.0371 0.0337 0.0040 and solve_cholesky 0.0118 0.0023 0.0098 0.0135 0.0035 over the graphs above
# (the read-back alone: 0.0005).  The device's summation order differs from both: it gets 4 x the worst.
ONE_STEP_C_CPU = 0.0371
ONE_STEP_C = 4.0 * ONE_STEP_C_CPU

# gimbal_graph(n): min_relative_increment values that stop check 2 tells apart.  The first |delta| / |x| of pass 1 is 8.68e-3 (n = 10) and
# 1.66e-2 (n = 30); with the two branches of TransformMatrix4dToVector6d swapped it is 6.73e-3 and 1.33e-2, with the first branch taken
# for every node 8.76e-3 and 1.67e-2.  [0] lies between the first two (the true x goes on, the swapped one stops at step 1), [1] between
# the first and the last (the true x stops at step 1).
GIMBAL_INCREMENTS = {10: (7.7e-3, 8.72e-3), 30: (1.49e-2, 1.665e-2)}

# The hub graphs the device is compared on, and the one with far more edges than nodes: 200 nodes and 20,000 edges, 3000 of them on the
# pair (1, 2), so block lists and node lists run into the hundreds and thousands and pg_reduce_kernel strides twenty times.
HUB_RUNS = {
    "hub22": (dict(n=22), dict()),
    "hub43": (dict(n=43), dict()),
    "hub60": (dict(n=60), dict()),
    "hub200": (dict(n=200), dict()),
    "hub400": (dict(n=400), dict(max_iteration=1)),
    "many_edges": (dict(n=200, extra=16801, bundle=3000), dict(max_iteration=0)),
}
