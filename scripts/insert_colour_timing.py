"""Device time of o3ds_map_insert_scan per scan into a growing map, coloured or not: bench.run_insert_sweep's loop (the stream's
pre-processed scans inserted at their true poses, every insertion under a hipEvent span while the device is kept busy) with a colour per raw
point, the rows taken where the map holds about 250 k and 1 M points.

  python scripts/insert_colour_timing.py [--coloured] [--array] [--lib PATH] [--repeats N] [--stream-cache FILE.npz]

--coloured  every raw scan carries colours (a PointCloud2 with an rgb / intensity field)
--array     the A/B library with O3DS_NO_PERSISTENT_MAP=1: the array form at every insertion (what a coloured map took before it could
            stay persistent)
--lib PATH  another build of libo3ds_backend.so (e.g. the parent commit's) instead of this tree's
--repeats N whole sweeps, each in this process one after the other; the spread of the medians is the run-to-run spread to quote

Prints one JSON line per repeat and a summary line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sweep(backend, syn, scans32, coloured, ab, marks):
    poses = syn.figure_eight_poses(200, 0.1)
    be = backend.Backend(0, ab=ab)
    m = be.upload(np.zeros((0, 3)))
    crop_scan = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, rmin=2.0, rmax=30.0)
    be.profile_enable(True)
    rec, form = [], []
    for k in range(len(scans32)):
        raw = be.upload_f32(np.ascontiguousarray(np.hstack([scans32[k], np.zeros((len(scans32[k]), 1), np.float32)])))
        if coloured:
            n = len(scans32[k])
            be.set_colors(raw, np.stack([np.full(n, (k % 32) / 32.0), (np.arange(n) % 251) / 251.0, (np.arange(n) % 7) / 7.0], axis=1))
        v = be.crop_voxel_down_sample(raw, crop_scan, 0.1)
        be.estimate_normals(v, 3.0, 20)
        be.free(raw)
        n_scan = be.size(v)[0]
        T = np.linalg.inv(poses[0]) @ poses[k]
        crop = backend.make_crop(backend.CROP_MIN_MAX_RADIUS, center=T[:3, 3], rmin=2.0, rmax=30.0)
        n_before = be.size(m)[0]
        be.estimate_normals(v, 3.0, 20)  # the device is busy while the call queues its launches: the span is the kernels' time
        with be.span(0):
            be.map_insert_scan(m, v, T, 0.1, crop, max_corr_hint=1.0)
        _, ms = be.span_read(0)
        rec.append((n_before, 1e3 * ms, n_scan))
        if hasattr(be.lib, "o3ds_cloud_is_persistent_map"):
            form.append(be.is_persistent_map(m))
        be.free(v)
    has_col = be.has_colors(m)
    be.profile_enable(False)
    be.close()
    rows = {}
    for mark in marks:
        sel = [r for r in rec[2:] if 0.8 * mark <= r[0] <= 1.2 * mark]
        if sel:
            rows[int(mark)] = {"insertions": len(sel), "median_us": float(np.median([r[1] for r in sel])), "avg_us": float(np.mean([r[1] for r in sel])),
                               "max_us": float(np.max([r[1] for r in sel])), "scan_points": int(np.mean([r[2] for r in sel]))}
    return {"rows": rows, "map_has_colours": bool(has_col), "persistent_after": int(sum(form)), "insertions": len(rec)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coloured", action="store_true")
    ap.add_argument("--array", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stream-cache", default=None)
    a = ap.parse_args()
    if a.array:
        os.environ["O3DS_NO_PERSISTENT_MAP"] = "1"
    if a.lib:
        os.environ["O3DS_BACKEND_LIB"] = os.path.abspath(a.lib)  # (backend.py's development override: an older build may lack the newest entry points)
    import bench
    from open3d_slam_amd import backend, synthetic as syn
    if a.stream_cache and os.path.exists(a.stream_cache):  # (ray-casting 200 scans takes longer than the sweeps: several runs share one file)
        with np.load(a.stream_cache) as z:
            scans = [z[f"s{k}"] for k in range(200)]
    else:
        scans = bench.make_stream(200)
        if a.stream_cache:
            np.savez(a.stream_cache, **{f"s{k}": sc for k, sc in enumerate(scans)})
    marks = (250_000, 1_000_000)
    runs = []
    for r in range(a.repeats):
        runs.append(sweep(backend, syn, scans, a.coloured, a.array, marks))
        print(json.dumps({"repeat": r, **runs[-1]}), flush=True)
    summary = {"coloured": a.coloured, "array_form": a.array, "lib": a.lib or "this tree"}
    for mark in marks:
        med = [run["rows"][mark]["median_us"] for run in runs if mark in run["rows"]]
        if med:
            summary[f"median_us_at_{mark}"] = {"runs": [round(x, 1) for x in med], "median": round(float(np.median(med)), 1),
                                               "spread": round(float(max(med) - min(med)), 1)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
