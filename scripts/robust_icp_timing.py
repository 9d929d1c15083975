"""Device time of the robust-loss step (o3ds_icp_robust_dev) beside the coloured step it is modelled on, on the pair of
profiles/colored_icp.txt -- the 65 536-point VLP-16 scan against the 1 M-point map, the grey texture of tests/colored_icp_restatement.py
as colours on both clouds, r = 1.0, 10 iterations, thresholds 0, f32 storage.  In ONE run on one device:
  * o3ds_icp_colored_dev: the two kernels of a step (span 16) per pass;
  * o3ds_icp_robust_dev with the Tukey and the Huber loss on both estimators: the two kernels of a step (span 17) per pass, and their
    ratio to the coloured step's span of this same run (DESIGN.md 7.10 holds the ratio to 1.3: the weights and 56 multiplies per pair).
Spans are summed over a call's 11 passes and divided by 11.  The first call of everything is not timed; minimum and median of 7 after it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

REPS = 7
R, LAMBDA, ITERS = 1.0, 0.968, 10
SPAN_SEARCH, SPAN_COLORED_STEP, SPAN_ROBUST_STEP = 10, 16, 17
# (Tukey's k above the pair's initial residuals of a few decimetres: below them every weight is 0 and the pose stays where it started)
LOSSES = (("tukey", backend.LOSS_TUKEY, 1.0), ("huber", backend.LOSS_HUBER, 0.02))
ESTIMATORS = (("point_to_plane", backend.ROBUST_POINT_TO_PLANE), ("colored", backend.ROBUST_COLORED))


def texture(p):
    v = 0.5 + 0.2 * np.sin(2.0 * np.pi * p[:, 1]) + 0.1 * np.cos(2.0 * np.pi * (p[:, 0] + p[:, 2]) / 1.5)
    return np.repeat(v[:, None], 3, axis=1)


def stats(v):
    return f"min {min(v):.1f} us median {np.median(v):.1f} us"


def per_pass(be, call, tag):
    """the span `tag` and the search's span per pass over REPS calls after one untimed call; the result of the untimed call"""
    passes = ITERS + 1
    res = call()
    for t in (SPAN_SEARCH, tag):
        be.span_read(t)
    step, search = [], []
    for _ in range(REPS):
        call()
        n, ms = be.span_read(tag)
        assert n == passes, (n, passes)
        step.append(ms * 1e3 / passes)
        search.append(be.span_read(SPAN_SEARCH)[1] * 1e3 / passes)
    return step, search, res


def main():
    src, tgt, nrm, T = syn.config2_inputs()
    placed = (np.c_[src, np.ones(len(src))] @ T.T)[:, :3]  # the scan where it was taken: its colours are the texture's there
    be = backend.Backend(0, backend.PRECISION_F32)
    be.profile_enable(2)
    s, t = be.upload(src), be.upload(tgt, nrm)
    be.set_colors(s, texture(placed))
    be.set_colors(t, texture(tgt))
    be.compute_color_gradients(t, 2.0 * R, 30)  # (once, for every registration below)
    kw = dict(max_iter=ITERS, rel_fitness=0.0, rel_rmse=0.0)

    print(f"{len(src)} source points, {len(tgt)} target points, r {R}, {ITERS} iterations ({ITERS + 1} passes), f32 storage; per pass:")
    base, search, res = per_pass(be, lambda: be.icp_colored_dev(s, t, R, lambda_geometric=LAMBDA, **kw), SPAN_COLORED_STEP)
    dt, dr = syn.se3_error(res["transformation"], T)
    print(f"  coloured ICP (o3ds_icp_colored_dev): step kernels (span 16) {stats(base)}; search (span 10) {stats(search)}; "
          f"|dt| {dt:.2e} m, angle {dr:.2e} rad")
    worst = 0.0
    for ename, est in ESTIMATORS:
        for lname, kind, k in LOSSES:
            step, search, res = per_pass(be, lambda: be.icp_robust_dev(s, t, R, est, (kind, k), lambda_geometric=LAMBDA, **kw), SPAN_ROBUST_STEP)
            dt, dr = syn.se3_error(res["transformation"], T)
            ratio = min(step) / min(base)
            worst = max(worst, ratio)
            print(f"  robust {ename} {lname}({k}): step kernels (span 17) {stats(step)} = {ratio:.2f} x span 16; search (span 10) {stats(search)}; "
                  f"fitness {res['fitness']:.4f}, |dt| {dt:.2e} m, angle {dr:.2e} rad")
    print(f"largest ratio of the minima, robust step to coloured step: {worst:.2f} (bound 1.3)")
    be.close()


if __name__ == "__main__":
    main()
