"""Device time of coloured ICP (o3ds_icp_colored_dev) on the configs[1] pair -- the 65 536-point VLP-16 scan against the 1 M-point map --
with the grey texture of tests/colored_icp_restatement.py as colours on both clouds, 10 iterations, thresholds 0, f32 storage:
  * the one-off colour gradients of the map at (2 r, 30): host clock around o3ds_compute_color_gradients and the wait for the device (the
    call itself returns with its kernels queued), and its two parts on the device,
    the Hybrid search (the library's span 10) and the gradient kernel (span 15);
  * one registration with the gradients in place: host clock around the call, a hipEvent span around it (caller tag 0), and per pass the
    search (span 10) and the two step kernels (span 16), both summed over the call's 11 passes and divided by 11; `host` is what is left of
    the host clock: the update kernel, the read-back of the state and the launches, per pass;
  * beside it o3ds_icp_register_dev, point-to-plane, on the same pair with the same parameters (the fused loop: one launch per pass).
The first call of everything is not timed; minimum and median of 7 after it.  DESIGN.md 7.9."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from open3d_slam_amd import backend, synthetic as syn

REPS = 7
R, LAMBDA, ITERS = 1.0, 0.968, 10
SPAN_CALL, SPAN_SEARCH, SPAN_GRADIENT, SPAN_STEP = 0, 10, 15, 16


def texture(p):
    v = 0.5 + 0.2 * np.sin(2.0 * np.pi * p[:, 1]) + 0.1 * np.cos(2.0 * np.pi * (p[:, 0] + p[:, 2]) / 1.5)
    return np.repeat(v[:, None], 3, axis=1)


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e6, out


def stats(v):
    return f"min {min(v):.1f} us median {np.median(v):.1f} us"


def main():
    src, tgt, nrm, T = syn.config2_inputs()
    placed = (np.c_[src, np.ones(len(src))] @ T.T)[:, :3]  # the scan where it was taken: its colours are the texture's there
    be = backend.Backend(0, backend.PRECISION_F32)
    be.profile_enable(2)
    s, t = be.upload(src), be.upload(tgt, nrm)
    be.set_colors(s, texture(placed))
    be.set_colors(t, texture(tgt))
    passes = ITERS + 1

    be.compute_color_gradients(t, 2.0 * R, 30)  # (untimed; leaves the map's index)
    for tag in (SPAN_SEARCH, SPAN_GRADIENT):
        be.span_read(tag)
    whole, search, kern = [], [], []
    for _ in range(REPS):
        whole.append(wall(lambda: (be.compute_color_gradients(t, 2.0 * R, 30), be.synchronize()))[0])
        search.append(be.span_read(SPAN_SEARCH)[1] * 1e3)
        kern.append(be.span_read(SPAN_GRADIENT)[1] * 1e3)
    print(f"gradients of the map ({len(tgt)} points, radius {2.0 * R}, max_nn 30), one-off:")
    print(f"  whole call and the wait for it: {stats(whole)}; search (span 10): {stats(search)}; gradient kernel (span 15): {stats(kern)}")

    kw = dict(max_iter=ITERS, rel_fitness=0.0, rel_rmse=0.0)
    res = be.icp_colored_dev(s, t, R, lambda_geometric=LAMBDA, **kw)  # (untimed)
    for tag in (SPAN_CALL, SPAN_SEARCH, SPAN_GRADIENT, SPAN_STEP):
        be.span_read(tag)
    whole, dev, search, step = [], [], [], []
    for _ in range(REPS):
        def call():
            with be.span(SPAN_CALL):
                return be.icp_colored_dev(s, t, R, lambda_geometric=LAMBDA, **kw)

        whole.append(wall(call)[0])
        dev.append(be.span_read(SPAN_CALL)[1] * 1e3)
        search.append(be.span_read(SPAN_SEARCH)[1] * 1e3 / passes)
        step.append(be.span_read(SPAN_STEP)[1] * 1e3 / passes)
        assert be.span_read(SPAN_GRADIENT)[0] == 0  # the gradients were reused
    dt, dr = syn.se3_error(res["transformation"], T)
    print(f"coloured ICP, {len(src)} source points, r {R}, lambda {LAMBDA}, {res['iterations']} iterations: fitness {res['fitness']:.4f}, "
          f"rmse {res['inlier_rmse']:.4f}, |dt| {dt:.2e} m, angle {dr:.2e} rad against the ground truth")
    print(f"  whole call, host clock: {stats(whole)}; hipEvent span around it: {stats(dev)}")
    host = [(w - (a + b) * passes) / passes for w, a, b in zip(whole, search, step)]
    print(f"  per pass ({passes} passes): search (span 10) {stats(search)}; step kernels (span 16) {stats(step)}; host and update {stats(host)}")

    ref = be.icp_register_dev(s, t, R, **kw)  # (untimed)
    be.span_read(SPAN_CALL)
    whole, dev = [], []
    for _ in range(REPS):
        def call():
            with be.span(SPAN_CALL):
                return be.icp_register_dev(s, t, R, **kw)

        whole.append(wall(call)[0])
        dev.append(be.span_read(SPAN_CALL)[1] * 1e3)
    dt, dr = syn.se3_error(ref["transformation"], T)
    print(f"point-to-plane (o3ds_icp_register_dev) on the same pair, {ref['iterations']} iterations: fitness {ref['fitness']:.4f}, "
          f"|dt| {dt:.2e} m, angle {dr:.2e} rad")
    print(f"  whole call, host clock: {stats(whole)}; hipEvent span around it: {stats(dev)}")
    be.close()


if __name__ == "__main__":
    main()
