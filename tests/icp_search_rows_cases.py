"""Inputs for the row geometry of the ICP search's shell and far stages (icp_kernels.hpp: row_extent, nn_search_group's 5x5x5 shell,
nn_search_wave_far): which rows of the (2K+1)^2 cross-section a lane owns, where a row splits into its two halves, which half wins a
tie, that the trim by the hardware square root keeps every cell the ball reaches, and how rows and x-ranges are clipped at the grid.
tests/test_icp_search_rows_cpu.py proves the premises of these inputs with the brute force of tests/icp_search_restatement.py;
tests/test_icp_search_rows_gpu.py runs them on the device.

Every lattice input is built from ISLANDS: a query and the target points meant for it, the islands in a line along x and more than
2 r + 3 cells apart, so that no query sees another island's points -- in particular the rows of one query's cross-section hold that
island's points and nothing else.  Coordinates are small multiples of cell / 4096 with cell = 0.25: exact in f32 and f64, so the two
storages search the same numbers, and the grid's origin (the minimum over the target) is the anchor point at 0.
"""
from __future__ import annotations

import math

import numpy as np

import icp_search_restatement as rs

CELL = 0.25
ROW_KS = (3, 4, 5, 6, 8)  # 49, 81, 121 rows: one round of 128; 169, 289: the loop over rounds


def _assemble(name, islands, K, r, exact, seed):
    """islands: [(query offset in cells from the island's own cell corner, [target offsets in cells from the same corner])]; the own cell
    of island i is (K + 2 + i * (2 K + 3), K + 2, K + 2).  Anchors at 0 and beyond the last island fix the grid."""
    pitch = 2 * K + 3
    src, tgt = [], []
    for i, (q, ts) in enumerate(islands):
        corner = np.array([K + 2 + i * pitch, K + 2, K + 2], dtype=np.float64)
        src.append((corner + np.asarray(q, dtype=np.float64)) * CELL)
        for t in ts:
            tgt.append((corner + np.asarray(t, dtype=np.float64)) * CELL)
    hi = np.array([K + 2 + len(islands) * pitch, 2 * K + 5, 2 * K + 5], dtype=np.float64) * CELL
    tgt = np.array([np.zeros(3)] + tgt + [hi])
    src = np.array(src)
    assert (tgt.astype(np.float32).astype(np.float64) == tgt).all() and (src.astype(np.float32).astype(np.float64) == src).all()
    nrm = rs.unit_normals(np.random.default_rng(seed), len(tgt))
    return rs.Case(name, src, tgt, nrm, r, CELL, np.eye(4), exact)


def registration_normals(c) -> np.ndarray:
    """the normals the three-iteration REGISTRATION of an island case runs with (the searches and pass records keep c.nrm): c.nrm turned
    into the plane across the line from each target point to its island's query (the nearest one).  A point-to-plane residual is
    n . (p - q): across that line the residuals of a registration from the identity are rounding residue, its updates are next to
    nothing, and every pass finds the matches of the first again -- correspondence count, fitness and rmse of the record then say
    what the searches of ALL passes found, and passes 1 to 3 run with candidate lists on.  (With free normals an island's point is a
    plane its query slides along: the first update threw most of these inputs out of reach.  For the per-query record checks, though,
    a residual of rounding residue has no relative bound: they keep the free normals.)  Other cases: c.nrm as it is."""
    if c.name in ("clipping", "lists-far"):
        return c.nrm
    near = ((c.tgt[:, None, :] - c.src[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
    d = c.src[near] - c.tgt
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = c.nrm - (c.nrm * d).sum(axis=1, keepdims=True) * d
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _facing(d):
    """(query's position in its cell, target's position in its cell) along an axis on which the target's cell is d cells away: as
    close to each other as 0.1 cells from the faces allow"""
    return (0.5, 0.5) if d == 0 else ((0.875, 0.125) if d > 0 else (0.125, 0.875))


def row_case(K) -> rs.Case:
    """one island per row (dy, dz) of the cross-section, |dy|, |dz| <= K, r = (K - 1/4) cells: the target point lies in that row, in the
    query's own x-column (three columns to the left in the rows stage 1 and 2 cover, so that it is found by the far stage), as near as
    the cells allow.  Rows the ball does not reach (the corners) hold a point all the same: no match."""
    islands = []
    for dz in range(-K, K + 1):
        for dy in range(-K, K + 1):
            (qy, ty), (qz, tz) = _facing(dy), _facing(dz)
            inner = abs(dy) <= 2 and abs(dz) <= 2
            qx, tx = (0.125, -3 + 0.875) if inner else (0.5, 0.5)
            islands.append(((qx, qy, qz), [(tx, dy + ty, dz + tz)]))
    return _assemble(f"rows-K{K}", islands, K, (K - 0.25) * CELL, False, 100 + K)


XSPLIT_ROWS = ((0, 0), (1, -1), (2, 0), (-2, 2), (3, 0), (0, -3), (3, -1))  # four inner rows (|dy|, |dz| <= 2), three outer ones
XSPLIT_DX = (0, 1, -1, 2, -2, 3, -3)


def xsplit_case() -> rs.Case:
    """K = 4: the only point of an island in cell ix + dx of an inner and of an outer row -- either side of the split between a row's two
    halves, and either side of the five cells an inner row leaves to stages 1 and 2"""
    K = 4
    islands = []
    for dy, dz in XSPLIT_ROWS:
        for dx in XSPLIT_DX:
            (qx, tx), (qy, ty), (qz, tz) = _facing(dx), _facing(dy), _facing(dz)
            tx = 0.625 if dx == 0 else tx  # (never ON the query: a zero distance has no relative bound)
            islands.append(((qx, qy, qz), [(dx + tx, dy + ty, dz + tz)]))
    return _assemble("x-split", islands, K, (K - 0.25) * CELL, False, 201)


TIE_PAIRS = (((-0.5, 3.5, 0.5), (1.5, 3.5, 0.5)),       # the two halves of the outer row (3, 0): cells ix - 1 and ix + 1
             ((-2.5, 1.5, 0.5), (3.5, 1.5, 0.5)),       # the two halves of the inner row (1, 0): cells ix - 3 and ix + 3
             ((0.5, 3.5, 0.5), (0.5, -2.5, 0.5)),       # rows (3, 0) and (-3, 0): two lanes
             ((0.5, 3.5, 0.5), (0.5, 0.5, 3.5)),        # rows (3, 0) and (0, 3)
             ((0.5, 0.5, -3.125), (2.0, 1.875, 3.5)))   # rows (0, -4) and (1, 3): numbers 4 and 68 of the 81, the two rows of lane 4
                                                        # (29/8 cells away both: 29^2 = 12^2 + 11^2 + 24^2)


def ties_case() -> rs.Case:
    """K = 4, exact arithmetic: two target points at exactly the same distance from the query at the centre of its cell, in the two
    halves of one row (an outer row, split beside the own cell; an inner row, split around the five cells of stages 1 and 2) and in two
    different rows (of two lanes, and of one).  Every pair comes in both orders: the smaller original index must win."""
    K = 4
    islands = []
    for a, b in TIE_PAIRS:
        islands.append(((0.5, 0.5, 0.5), [a, b]))
        islands.append(((0.5, 0.5, 0.5), [b, a]))
    return _assemble("ties", islands, K, (K - 0.25) * CELL, True, 202)


SUPERSET_BOUNDS = (2.0, 2.5, 4.0)  # r in cells: the bound of pass 0
ULP_STEPS = (0, 1, -1)             # on the radius, one f32 ulp inside, one outside
BORDER_INSET = 1.0 / 16384.0       # cells: below the trim's additive margin of 1e-4


def superset_case(bound) -> rs.Case:
    """r = bound cells, K = ceil(bound).  The target point lies exactly at the x-extreme of the ball at its row, and that extreme is a cell
    border (query on a border, or in the middle of its cell for the half-width 2.5) or BORDER_INSET beyond one (the border lies INSIDE the ball by less than the trim's margin): on the radius
    (no match: strict), one f32 ulp nearer (a match), one farther (none), to the left and to the right.  Rows: the own one (half-width =
    bound), and for 2.5 the row two cells up at distance 1.5 (half-width 2, the 3-4-5 triangle)."""
    K = int(math.ceil(bound))
    rows = [(0.5, bound)] + ([(2.0, 2.0)] if bound == 2.5 else [])  # (target's y in cells from the query's cell corner, half-width)
    islands, steps = [], []
    for ty, w in rows:
        for ux in ((-w) % 1.0, (-w) % 1.0 + BORDER_INSET):  # (ux +- w is a whole number of cells)
            for side in (-1.0, 1.0):
                for step in ULP_STEPS:
                    islands.append(((ux, 0.5, 0.5), [(ux + side * w, ty, 0.5)]))
                    steps.append((step, side))
    case = _assemble(f"superset-{bound}", islands, K, bound * CELL, False, 300 + int(10 * bound))
    tgt = case.tgt.copy()
    for i, (step, side) in enumerate(steps):  # the ulp steps are taken on the assembled coordinate, in f32
        if step:
            inward = np.float32(-np.inf) if side > 0 else np.float32(np.inf)
            tgt[1 + i, 0] = float(np.nextafter(np.float32(tgt[1 + i, 0]), inward if step > 0 else -inward))
    return case._replace(tgt=tgt)


CLIP_R, CLIP_BOX, CLIP_TARGETS = 1.0, 2.5, 25


def clipping_case() -> rs.Case:
    """K = 4 on a sparse random target (25 points in a 2.5 m box: the nearest neighbour is cells away): queries in the boundary cell of
    every face, edge and corner of the grid, and 0.5 r and 0.97 r outside the bounding box in each of the 26 directions -- rows and
    x-ranges are clipped at the grid, and most of the cross-section of an outside query does not exist"""
    rng = np.random.default_rng(404)
    tgt = rng.uniform(0.0, CLIP_BOX, size=(CLIP_TARGETS, 3))
    tgt[0], tgt[1] = 0.0, CLIP_BOX  # the box is exactly [0, 2.5]^3: ten cells a side
    src = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                d = np.array([dx, dy, dz], dtype=np.float64)
                if not d.any():
                    continue
                inside = np.where(d < 0, 0.1, np.where(d > 0, CLIP_BOX - 0.1, rng.uniform(0.5, 2.0, size=3)))  # in the boundary cell
                src.append(inside)
                for f in (0.5, 0.97):
                    src.append(np.where(d < 0, 0.0, np.where(d > 0, CLIP_BOX, inside)) + d / np.linalg.norm(d) * f * CLIP_R)
    src = np.array(src) + rng.uniform(-1e-3, 1e-3, size=(len(src), 3))
    return rs.Case("clipping", src, tgt, rs.unit_normals(rng, len(tgt)), CLIP_R, CELL, np.eye(4), False)


def lattice_cases():
    return [row_case(K) for K in ROW_KS] + [xsplit_case(), ties_case()] + [superset_case(b) for b in SUPERSET_BOUNDS] + [clipping_case()]


# the registration whose far queries leave candidate sets: a 2 048-point scan of the synthetic scene against a map of 8 000 points,
# sparse enough that hundreds of queries find their neighbour more than three cells away (beyond the 5x5x5 cells of stages 1 and 2 wherever
# the query lies in its cell).  A pass lists candidates only after an update small enough for a margin under the cap (4 cm by default,
# twice the motion of the farthest scan point, 43 m out), and pass 0 follows no update: so the registration starts millimetres from the
# truth, update 0 is millimetres, pass 1 searches with lists on -- its far queries list -- and passes 2 and 3 verify inside those lists
LISTS_FAR_CELLS = 3.0
LISTS_MAP, LISTS_START = 8_000, ([0.002, -0.0015, 0.001], [0.004, -0.003, 0.005])  # (metres, degrees of roll / pitch / yaw) off the truth


def lists_case() -> rs.Case:
    from open3d_slam_amd import synthetic as syn

    src, tgt, nrm, truth = syn.config2_inputs(n_map=LISTS_MAP, n_az=128)
    return rs.Case("lists-far", src, tgt, nrm, 1.0, CELL, truth @ syn.make_pose(*LISTS_START), False)


def all_cases():
    return lattice_cases() + [lists_case()]
