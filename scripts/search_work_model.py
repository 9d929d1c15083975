#!/usr/bin/env python
"""CPU model of the work of the searching passes of configs[1] (numpy only; development script, no GPU).

For every pass 0..10 of the bench's registration (65 536-pt VLP-16 scan vs the 1 M-pt map, cell r / 4, poses entering each pass from
the CPU oracle's point-to-plane ICP with max_iter = k) and every query it computes, the way icp_kernels.hpp nn_search_group does:
  - the bound: r in pass 0, else the distance to the previous pass's match (nn_cache);
  - stage 1 on the rows of cell_start: the rows of the 3x3 cross-section in reach, their trimmed segments and candidates;
  - stage 1 on the 9x replica (one range of the super-row, trimmed by the widest row) and on the 3x one (dz merged: one range per dy);
  - the lockstep rounds of a wavefront (16 queries x 4 lanes, 16 candidates per round and query): per segment the max over the
    wavefront's queries today (sum over the segment slots), per range with a replica;
  - how many queries go on to stage 2 (their nearest neighbour is not proven inside the 3x3x3 block) and to stage 3 (not proven inside
    the 5x5x5 block); for stage 3 the half-row geometries and lockstep rounds of its wavefront today (2 (2K+1)^2 = 162 half-rows, K = 4)
    and on 3x3 tiles of super-rows (18 half-tiles; tiles other than the centre one rescan the stage-1/2 cells of their inner rows);
  - the issue's gate: stage-1 + stage-3 rounds plus row work of passes 0-4, per wavefront, in shader cycles.  The weights are calibrated
    on round 6's per-phase cycle counts of pass 1 (profiles/r06_search_experiments.txt section 3: stage-1 rows 4.9 k cycles for three row
    iterations per lane, stage-1 scans 8.6 k cycles for this model's 6.9 lockstep rounds of that pass).
Candidate sets are left out: the model treats every query of passes 0-4 as searching (the bench verifies from sets from pass 5 on).
Nearest neighbours come from the grid itself (every point of the 9x9x9 block, chunked), no k-d tree.

    python scripts/search_work_model.py [--out profiles/search_work_model.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 1.0
CELL = R / 4
G, QPW = 4, 16           # lanes per query, queries per wavefront
PER_ROUND = 4 * G        # candidates per query and scan round (four in flight per lane)
K = 4                    # ceil(r / cell)
C_ROW = 4900.0 / 3       # cycles per row iteration of a lane (round 6, pass 1: 4.9 k cycles, three iterations per lane)
C_ROUND = 8600.0 / 6.92  # cycles per lockstep scan round (round 6, pass 1: 8.6 k cycles; this model: 6.92 rounds)


def ragged(starts_, lens):
    """flat positions of the ranges [starts_, starts_ + lens) and the number of the range each belongs to"""
    tot = int(lens.sum())
    rid = np.repeat(np.arange(lens.size), lens)
    off = np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(starts_, lens) + (np.arange(tot) - off), rid


def nearest(q, tgt, mn, n, cs, chunk=2048):
    """per query: distance to the nearest target point within R (inf: none) and its index, and the nearest inside the 5x5x5 block"""
    nx, ny, nz = n
    ic = np.floor((q - mn) / CELL).astype(np.int64)
    d_all = np.full(len(q), np.inf)
    j_all = np.full(len(q), -1)
    d_5 = np.full(len(q), np.inf)
    for c0 in range(0, len(q), chunk):
        qq, ii = q[c0 : c0 + chunk], ic[c0 : c0 + chunk]
        st, ln, qi, five = [], [], [], []
        for dz in range(-K, K + 1):
            for dy in range(-K, K + 1):
                y, z = ii[:, 1] + dy, ii[:, 2] + dz
                xa, xb = np.maximum(ii[:, 0] - K, 0), np.minimum(ii[:, 0] + K, nx - 1)
                ok = (y >= 0) & (y < ny) & (z >= 0) & (z < nz) & (xa <= xb)
                row = (np.clip(z, 0, nz - 1) * ny + np.clip(y, 0, ny - 1)) * nx
                a, b = cs[np.where(ok, row + xa, 0)], cs[np.where(ok, row + xb + 1, 0)]
                st.append(a)
                ln.append(np.where(ok, b - a, 0))
                qi.append(np.arange(len(qq)))
                five.append(np.full(len(qq), abs(dy) <= 2 and abs(dz) <= 2))
        st, ln, qi, five = (np.concatenate(v) for v in (st, ln, qi, five))
        pos, rid = ragged(st, ln)
        qid = qi[rid]
        d = np.linalg.norm(tgt[pos] - qq[qid], axis=1)
        d[d > R] = np.inf
        inb = five[rid] & (np.abs(np.floor((tgt[pos] - mn) / CELL).astype(np.int64)[:, 0] - ii[qid, 0]) <= 2)
        best = np.full(len(qq), np.inf)
        np.minimum.at(best, qid, d)
        b5 = np.full(len(qq), np.inf)
        np.minimum.at(b5, qid, np.where(inb, d, np.inf))
        hit = np.isfinite(d) & (d == best[qid])
        first = np.unique(qid[hit], return_index=True)
        j = np.full(len(qq), -1)
        j[first[0]] = pos[hit][first[1]]
        d_all[c0 : c0 + chunk], j_all[c0 : c0 + chunk], d_5[c0 : c0 + chunk] = best, j, b5
    return d_all, j_all, d_5


def far_wave(lens, c_per_lane_rows):
    """stage 3 of one far query on a wavefront: row-geometry iterations per lane and lockstep rounds (the lanes regroup: 64 / pow2(#listed,
    at most 16) lanes per listed range, each group strides over its share of the list)"""
    lens = lens[lens > 0]
    if lens.size == 0:
        return c_per_lane_rows, 0
    groups = 1
    while groups < lens.size and groups < 16:
        groups <<= 1
    W = 64 // groups
    rounds_g = [int(sum(-(-int(L) // (4 * W)) for L in lens[g::groups])) for g in range(groups)]
    return c_per_lane_rows, max(rounds_g)


def grid_of(tgt):
    mn, mx = tgt.min(0), tgt.max(0)
    n = (np.floor((mx - mn) / CELL) + 1).astype(np.int64)
    cid = np.clip(np.floor((tgt - mn) / CELL).astype(np.int64), 0, n - 1)
    return mn, n, cid


def starts(counts):
    cs = np.zeros(counts.size + 1, np.int64)
    np.cumsum(counts, out=cs[1:])
    return cs


def slab(d, u):
    return np.where(d == 0, 0.0, np.where(d < 0, u + (-d - 1), (1.0 - u) + (d - 1)))


def extent(b2, rowd2, ux):
    w2 = b2 - rowd2
    ok = w2 >= 0
    w = np.sqrt(np.maximum(w2, 0)) + 1e-4
    return ok, np.floor(np.maximum(ux - w, -64)).astype(np.int64), np.floor(np.minimum(ux + w, 64)).astype(np.int64)


def wave_order(n, pass_no):
    """query indices of each wavefront (pass_order: pass 0 single queries spread over the scan, later passes runs of 16)"""
    n_w = (n + QPW - 1) // QPW
    if pass_no == 0:
        idx = np.arange(QPW)[None, :] * n_w + np.arange(n_w)[:, None]
    else:
        idx = np.arange(n_w * QPW).reshape(n_w, QPW)
    return np.where(idx < n, idx, -1)


def rounds(c):
    return (c + PER_ROUND - 1) // PER_ROUND


def stage3(q, b, mn, n, cs, rs9):
    """stage 3 of the queries q from the bound b (metres): per query (row iterations per lane, lockstep rounds) today and on tiles"""
    nx, ny, nz = n
    f = (q - mn) / CELL
    ic = np.floor(f).astype(np.int64)
    u = f - ic
    ix, iy, iz = ic[:, 0], ic[:, 1], ic[:, 2]
    b2 = (b / CELL) ** 2 * (1 + 1e-4) + 1e-6
    today, tiles = [], []
    for dz in range(-K, K + 1):  # 81 rows x 2 halves
        for dy in range(-K, K + 1):
            y, z = iy + dy, iz + dz
            ok, xa, xb = extent(b2, slab(dy, u[:, 1]) ** 2 + slab(dz, u[:, 2]) ** 2, u[:, 0])
            ok &= (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
            xa, xb = np.maximum(ix + xa, ix - K), np.minimum(ix + xb, ix + K)
            inner = abs(dy) <= 2 and abs(dz) <= 2
            row = (np.clip(z, 0, nz - 1) * ny + np.clip(y, 0, ny - 1)) * nx
            for a_, b_ in ((xa, np.minimum(xb, ix - 3 if inner else ix)), (np.maximum(xa, ix + 3 if inner else ix + 1), xb)):
                a_, b_ = np.maximum(a_, 0), np.minimum(b_, nx - 1)
                k = ok & (a_ <= b_)
                today.append(np.where(k, cs[np.where(k, row + b_ + 1, 0)] - cs[np.where(k, row + a_, 0)], 0))
    for tz in (-1, 0, 1):  # 9 tiles of 3x3 super-rows x 2 halves, trimmed by the tile's nearest row
        for ty in (-1, 0, 1):
            Y, Z = iy + 3 * ty, iz + 3 * tz
            ok, xa, xb = extent(b2, slab(2 * ty, u[:, 1]) ** 2 + slab(2 * tz, u[:, 2]) ** 2, u[:, 0])
            ok &= (Y >= -1) & (Y <= ny) & (Z >= -1) & (Z <= nz)
            xa, xb = np.maximum(ix + xa, ix - K), np.minimum(ix + xb, ix + K)
            centre = ty == 0 and tz == 0
            srow = ((np.clip(Z, -1, nz) + 1) * (ny + 2) + (np.clip(Y, -1, ny) + 1)) * nx
            for a_, b_ in ((xa, np.minimum(xb, ix - 3 if centre else ix)), (np.maximum(xa, ix + 3 if centre else ix + 1), xb)):
                a_, b_ = np.maximum(a_, 0), np.minimum(b_, nx - 1)
                k = ok & (a_ <= b_)
                tiles.append(np.where(k, rs9[np.where(k, srow + b_ + 1, 0)] - rs9[np.where(k, srow + a_, 0)], 0))
    today, tiles = np.stack(today, 1), np.stack(tiles, 1)
    # geometry: 162 half-rows over 64 lanes, four per lane in one batch; 18 half-tiles, one per lane
    return [far_wave(today[i], 4) for i in range(len(q))], [far_wave(tiles[i], 1) for i in range(len(q))], today.sum(1), tiles.sum(1)


def model_pass(q, bound, nn_d, d5, mn, n, cs, rs9, rs3, pass_no):
    nx, ny, nz = n
    f = (q - mn) / CELL
    ic = np.floor(f).astype(np.int64)
    u = f - ic
    mf = np.minimum(np.minimum(u, 1 - u).min(1), 1.0)
    ix, iy, iz = ic[:, 0], ic[:, 1], ic[:, 2]
    b2 = (bound / CELL) ** 2 * (1 + 1e-4) + 1e-6
    xlo, xhi = np.maximum(ix - 1, 0), np.minimum(ix + 1, nx - 1)
    nq = len(q)
    # today: nine rows
    seg = np.zeros((nq, 9), np.int64)
    for r in range(9):
        dy, dz = r % 3 - 1, r // 3 - 1
        y, z = iy + dy, iz + dz
        valid = (xlo <= xhi) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        ok, xa, xb = extent(b2, slab(dy, u[:, 1]) ** 2 + slab(dz, u[:, 2]) ** 2, u[:, 0])
        xa, xb = np.maximum(ix + xa, xlo), np.minimum(ix + xb, xhi)
        ok &= valid & (xa <= xb)
        row = np.where(ok, (np.clip(z, 0, nz - 1) * ny + np.clip(y, 0, ny - 1)) * nx, 0)
        seg[:, r] = np.where(ok, cs[np.where(ok, row + xb + 1, 0)] - cs[np.where(ok, row + xa, 0)], 0)
    # the LDS list order: lane gl's rows gl, gl + 4, gl + 8, lanes in order; empty segments compacted away
    order = [0, 4, 8, 1, 5, 2, 6, 3, 7]
    lst = seg[:, order]
    nseg = (lst > 0).sum(1)
    comp = np.zeros_like(lst)
    for i in range(nq):  # (compaction; 65 k x 9)
        v = lst[i][lst[i] > 0]
        comp[i, : v.size] = v
    # replicas: trimmed by the widest row (distance 0)
    ok, xa, xb = extent(b2, np.zeros(nq), u[:, 0])
    xa, xb = np.maximum(ix + xa, xlo), np.minimum(ix + xb, xhi)
    sv = ok & (xlo <= xhi) & (iy >= -1) & (iy <= ny) & (iz >= -1) & (iz <= nz) & (xa <= xb)
    srow = np.where(sv, ((iz + 1) * (ny + 2) + (iy + 1)) * nx, 0)
    c9 = np.where(sv, rs9[np.where(sv, srow + xb + 1, 0)] - rs9[np.where(sv, srow + xa, 0)], 0)
    c3 = np.zeros((nq, 3), np.int64)  # 3x: super-row (y, z) = rows (y, z - 1 .. z + 1); three ranges, dy = -1, 0, 1
    for k, dy in enumerate((-1, 0, 1)):
        y = iy + dy
        ok3, xa3, xb3 = extent(b2, slab(dy, u[:, 1]) ** 2, u[:, 0])
        xa3, xb3 = np.maximum(ix + xa3, xlo), np.minimum(ix + xb3, xhi)
        ok3 &= (xlo <= xhi) & (y >= 0) & (y < ny) & (iz >= -1) & (iz <= nz) & (xa3 <= xb3)
        r3 = np.where(ok3, ((iz + 1) * ny + np.clip(y, 0, ny - 1)) * nx, 0)
        c3[:, k] = np.where(ok3, rs3[np.where(ok3, r3 + xb3 + 1, 0)] - rs3[np.where(ok3, r3 + xa3, 0)], 0)
    stage2 = nn_d > CELL * (1 + mf)  # not proven inside the 3x3x3 block
    best2 = np.minimum(bound, d5)     # the bound stage 3 starts from
    far = best2 > CELL * (2 + mf)     # not proven inside the 5x5x5 block
    s3_today, s3_tiles, c3_today, c3_tiles = stage3(q[far], np.minimum(best2[far], R), mn, n, cs, rs9) if far.any() else ([], [], np.zeros(0), np.zeros(0))
    n_waves = (nq + QPW - 1) // QPW
    cyc3_today = sum(r * C_ROW + k * C_ROUND for r, k in s3_today) / n_waves  # far queries are pooled: per wavefront of the launch
    cyc3_tiles = sum(r * C_ROW + k * C_ROUND for r, k in s3_tiles) / n_waves
    waves = wave_order(nq, pass_no)
    live = waves >= 0
    wv = np.where(live, waves, 0)

    def wmax(a):  # per wavefront, max over its live queries of a per-query [.., k] quantity
        return np.where(live[..., None] if a.ndim == 2 else live, a[wv], 0).max(1)

    today = wmax(rounds(comp)).sum(1)            # slot t: max over the queries of the rounds of their t-th segment
    today_slots = wmax((comp > 0).astype(np.int64)).sum(1)  # loop iterations (segments) the wavefront runs
    r9 = wmax(rounds(c9))
    c3r = rounds(c3)
    c3c = np.zeros_like(c3r)
    for i in range(nq):
        v = c3r[i][c3r[i] > 0]
        c3c[i, : v.size] = v
    r3 = wmax(c3c).sum(1)
    r3_slots = wmax((c3c > 0).astype(np.int64)).sum(1)
    return dict(pass_no=pass_no, bound_cells=float(np.median(bound) / CELL), seg=float(nseg.mean()), cand=float(seg.sum(1).mean()),
                cand9=float(c9.mean()), cand3=float(c3.sum(1).mean()), stage2=int(stage2.sum()),
                w_today=float(today.mean()), w_slots=float(today_slots.mean()), w9=float(r9.mean()), w3=float(r3.mean()),
                w3_slots=float(r3_slots.mean()), far=int(far.sum()), cand_far=float(c3_today.mean()) if far.any() else 0.0,
                cand_far9=float(c3_tiles.mean()) if far.any() else 0.0,
                cyc1_today=float(3 * C_ROW + today.mean() * C_ROUND), cyc1_9=float(C_ROW + r9.mean() * C_ROUND),
                cyc3_today=float(cyc3_today), cyc3_9=float(cyc3_tiles))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_work_model.txt"))
    ap.add_argument("--passes", type=int, default=11)
    args = ap.parse_args()
    from oracle import pyoracle as po
    from open3d_slam_amd import synthetic as syn

    scene = syn.make_scene()
    src = syn.vlp16_scan(scene, syn.ground_truth_pose())
    tgt, nrm = syn.sample_map(scene, 1_000_000)
    mn, n, cid = grid_of(tgt)
    nx, ny, nz = (int(v) for v in n)
    cell_lin = (cid[:, 2] * ny + cid[:, 1]) * nx + cid[:, 0]
    cs = starts(np.bincount(cell_lin, minlength=nx * ny * nz))
    tsorted = tgt[np.argsort(cell_lin, kind="stable")]  # the cell-sorted target cs indexes
    x, y, z = cid[:, 0], cid[:, 1], cid[:, 2]
    img9 = np.concatenate([((z + 1 - dz) * (ny + 2) + (y + 1 - dy)) * nx + x for dz in (-1, 0, 1) for dy in (-1, 0, 1)])
    rs9 = starts(np.bincount(img9, minlength=nx * (ny + 2) * (nz + 2)))
    img3 = np.concatenate([((z + 1 - dz) * ny + y) * nx + x for dz in (-1, 0, 1)])
    rs3 = starts(np.bincount(img3, minlength=nx * ny * (nz + 2)))
    rows = []
    prev_match = None
    for k in range(args.passes):
        T = np.eye(4) if k == 0 else po.icp_point_to_plane(src, tgt, nrm, R, max_iter=k, rel_fitness=0.0, rel_rmse=0.0)["transformation"]
        q = src @ T[:3, :3].T + T[:3, 3]
        d, j, d5 = nearest(q, tsorted, mn, (nx, ny, nz), cs)
        if prev_match is None:
            bound = np.full(len(q), R)
        else:
            bound = np.where(prev_match >= 0, np.linalg.norm(q - tsorted[np.maximum(prev_match, 0)], axis=1), R)
            bound = np.minimum(bound, R)
        rows.append(model_pass(q, bound, np.where(np.isfinite(d), d, R * 2), d5, mn, n, cs, rs9, rs3, k))
        prev_match = np.where(np.isfinite(d), j, -1)
        print(rows[-1], flush=True)
    lines = [
        "CPU model of the searching work per pass (scripts/search_work_model.py): configs[1], 65 536 queries vs the 1 M-pt map, cell 0.25 m,",
        f"grid {nx} x {ny} x {nz} = {nx * ny * nz} cells; super-row table 9x: {nx * (ny + 2) * (nz + 2)} entries, 3x: {nx * ny * (nz + 2)}.",
        "Per query (mean): segments and candidates of stage 1 today, candidates of the one 9x range and of the three 3x ranges; queries that",
        "go on to stage 2.  Per wavefront of 16 queries (mean): stage-1 scan rounds in lockstep (16 candidates per round and query) and the",
        "segment slots (loop iterations, each with its own per-segment set-up) today, with the 9x replica (one range, one slot) and the 3x one.",
        "Stage 3: queries, candidates per query today (half-rows) and on 9x tiles (duplicates of the inner cells included); cycles per",
        f"wavefront of stage 1 and stage 3 (row iteration {C_ROW:.0f} cycles per lane, lockstep round {C_ROUND:.0f} cycles), today -> 9x.",
        "",
        f"{'pass':>4} {'bound':>6} {'segs':>5} {'cand':>6} {'cand9':>6} {'cand3':>6} {'stage2':>7} | {'rounds':>6} {'slots':>5} | {'9x':>5} {'3x':>5} {'3x slots':>8}"
        f" | {'far':>6} {'cand':>6} {'cand9':>6} | {'stage-1 cyc':>13} {'stage-3 cyc':>13}",
    ]
    for r in rows:
        lines.append(f"{r['pass_no']:>4} {r['bound_cells']:>6.2f} {r['seg']:>5.2f} {r['cand']:>6.1f} {r['cand9']:>6.1f} {r['cand3']:>6.1f} {r['stage2']:>7} | "
                     f"{r['w_today']:>6.2f} {r['w_slots']:>5.2f} | {r['w9']:>5.2f} {r['w3']:>5.2f} {r['w3_slots']:>8.2f}"
                     f" | {r['far']:>6} {r['cand_far']:>6.0f} {r['cand_far9']:>6.0f} | {r['cyc1_today']:>6.0f}>{r['cyc1_9']:>6.0f} {r['cyc3_today']:>6.0f}>{r['cyc3_9']:>6.0f}")
    s = lambda key, a, b: sum(r[key] for r in rows[a:b])  # noqa: E731
    lines += ["",
              f"passes 0-4, per wavefront: stage-1 rounds today {s('w_today', 0, 5):.1f} in {s('w_slots', 0, 5):.1f} segment slots (9 row geometries per "
              f"query per pass); 9x {s('w9', 0, 5):.1f} rounds in 5 ranges (one geometry); 3x {s('w3', 0, 5):.1f} rounds in {s('w3_slots', 0, 5):.1f} slots (three).",
              f"cut of the lockstep rounds: 9x {100 * (1 - s('w9', 0, 5) / s('w_today', 0, 5)):.0f} %, 3x {100 * (1 - s('w3', 0, 5) / s('w_today', 0, 5)):.0f} %; "
              f"of the loop iterations (slots): 9x {100 * (1 - 5 / s('w_slots', 0, 5)):.0f} %, 3x {100 * (1 - s('w3_slots', 0, 5) / s('w_slots', 0, 5)):.0f} %.",
              "GATE (stage-1 + stage-3 rounds plus row work, passes 0-4, cycles per wavefront): today "
              f"{s('cyc1_today', 0, 5) + s('cyc3_today', 0, 5):.0f}, stage 1 on the replica {s('cyc1_9', 0, 5) + s('cyc3_today', 0, 5):.0f} "
              f"({100 * (1 - (s('cyc1_9', 0, 5) + s('cyc3_today', 0, 5)) / (s('cyc1_today', 0, 5) + s('cyc3_today', 0, 5))):.0f} % cut), "
              f"stages 1 and 3 on the replica {s('cyc1_9', 0, 5) + s('cyc3_9', 0, 5):.0f} "
              f"({100 * (1 - (s('cyc1_9', 0, 5) + s('cyc3_9', 0, 5)) / (s('cyc1_today', 0, 5) + s('cyc3_today', 0, 5))):.0f} % cut)."]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
