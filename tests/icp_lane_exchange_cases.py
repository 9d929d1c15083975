"""Inputs for the lane exchanges of the ICP search (icp_kernels.hpp: lanes_min over the four lanes of a group and over the 64 lanes of a
wavefront, group_exclusive_sum) and for the order a pass deals its queries out in (query_index, QueryPrefetch::qi).
tests/test_icp_lane_exchange_cpu.py proves the premises with numpy alone; tests/test_icp_lane_exchange_gpu.py runs the inputs on the
device against the brute force of tests/icp_search_restatement.py.

The inputs are islands on the lattice of tests/icp_scan_loop_cases.py (exact in both storages, ties ARE ties on the device).  The order of
the points INSIDE a cell of the index is the order the build's atomics were served in, so no input can place a point in a lane by itself.
Instead every island of n points exists n times, the nearest point being its first, second, ... n-th point in turn: whatever
permutation the build leaves (the GPU test reads it back from the winners' positions), the winner is scanned by every lane.
"""
from __future__ import annotations

import numpy as np

import icp_scan_loop_cases as sc
import icp_search_restatement as rs

U = 1.0 / 4096                 # the lattice unit, in cells
QUERY = (132 * U, 196 * U, 100 * U)   # as in sc.segments_case: a little off the own cell's corner
QUAD_COUNTS = tuple(range(4, 17))      # candidates in the query's cell: one to four per lane of the group
WAVE = 64


def _sixteenths(rng, n, corner, y_from=0):
    """n distinct points of the cell at `corner` on its lattice of sixteenths, none in the y-layers below y_from"""
    pick = rng.choice(16 * (16 - y_from) * 16, size=n, replace=False)
    return [(corner[0] + (p % 16) / 16.0, corner[1] + (p // 16 % (16 - y_from) + y_from) / 16.0, corner[2] + (p // (16 * (16 - y_from))) / 16.0)
            for p in pick]


# ---- 1. the four lanes of a group ------------------------------------------------------------------------------------------------------
NEAR = (QUERY[0] + 4 * U, QUERY[1], QUERY[2])                                     # 4 units from the query: nearer than any lattice point
TIED = ((QUERY[0] - 8 * U, QUERY[1], QUERY[2]), (QUERY[0] + 8 * U, QUERY[1], QUERY[2]))  # 8 units to either side: an exact tie


def quad_case():
    """(case, owner, want): want[i] = the island-local number of the point that must win island i (-1: none).
      * n = 4 ... 16 candidates in the own cell, the nearest being point j of the island, j = 0 ... n - 1;
      * four candidates in the own cell, two of them tied nearest, at the places (a, b) of the island for every a != b: the one of the
        smaller original index wins, which is the first of the two in one order and the second in the other;
      * nothing in reach: every lane of the group ends with the empty bound it started from (one island's only point lies a cell beyond
        the radius, another's exactly ON it: d2 == r^2 stays out)."""
    rng = np.random.default_rng(601)
    islands, want = [], []
    for n in QUAD_COUNTS:
        for j in range(n):
            pts = _sixteenths(rng, n, (0.0, 0.0, 0.0))
            pts[j] = NEAR
            islands.append((QUERY, pts)), want.append(j)
    for a in range(4):
        for b in range(4):
            if a != b:
                pts = _sixteenths(rng, 4, (0.0, 0.0, 0.0))
                pts[a], pts[b] = TIED
                islands.append((QUERY, pts)), want.append(min(a, b))
    c = sc.C
    islands.append(((c, c, c), [(c + sc.K + 0.75, c, c)])), want.append(-1)    # beyond the radius (r = K - 0.25 cells)
    islands.append(((c, c, c), [(c + sc.K - 0.25, c, c)])), want.append(-1)    # ON the radius
    case, owner = sc._assemble("quad", islands, True, 602)
    return case, owner, np.array(want)


QUAD_R = 2 * sc.CELL  # two cells: a point on this radius lies in the 5x5x5 shell, which the GROUP scans (stage 2)


def quad_radius_case():
    """the radius under the group's exchange: island 0's only candidate at d2 == r^2 (none); island 1 the same and a nearer point behind it
    in the array (that one); island 2 two candidates ON the radius, in different rows of the shell (none)"""
    c = sc.C
    on, on2, near = (c + 2.0, c, c), (c, c - 2.0, c), (c, c + 1.0, c)
    islands = [((c, c, c), [on]), ((c, c, c), [on, near]), ((c, c, c), [on, on2])]
    case, owner = sc._assemble("quad-radius", islands, True, 603, r=QUAD_R)
    return case, owner, np.array([-1, 1, -1])


# ---- 2. the 64 lanes of a wavefront ----------------------------------------------------------------------------------------------------
FAR_QUERY = (sc.C + U, sc.C, sc.C + 3 * U)           # as in sc.half_rows_case
FAR_CORNER = (0.0, 3.0, 0.0)                          # the cell three rows up: beyond the shell, a half-row of the far stage
FAR_NEAR = (FAR_QUERY[0], 3.0, FAR_QUERY[2])          # on the cell's lower face, straight above the query
FAR_TIED = ((FAR_QUERY[0] - 8 * U, 3.0, FAR_QUERY[2]), (FAR_QUERY[0] + 8 * U, 3.0, FAR_QUERY[2]))


def wave_case():
    """(case, owner, want): 64 islands whose only points are 64 candidates of ONE far half-row (each lane of the wavefront scans one), the
    nearest being point k of the island, k = 0 ... 63; and 64 more with a tie between points k and 63 - k (the smaller original index
    wins: k for k < 32, 63 - k above).  Every other point keeps a sixteenth of a cell above the face the near ones lie on."""
    rng = np.random.default_rng(604)
    islands, want = [], []
    for k in range(WAVE):
        pts = _sixteenths(rng, WAVE, FAR_CORNER, y_from=1)
        pts[k] = FAR_NEAR
        islands.append((FAR_QUERY, pts)), want.append(k)
    for k in range(WAVE):
        pts = _sixteenths(rng, WAVE, FAR_CORNER, y_from=1)
        pts[k], pts[WAVE - 1 - k] = FAR_TIED
        islands.append((FAR_QUERY, pts)), want.append(min(k, WAVE - 1 - k))
    case, owner = sc._assemble("wave", islands, True, 605)
    return case, owner, np.array(want)


def builders():
    return {"quad": quad_case, "quad-radius": quad_radius_case, "wave": wave_case}


def winners(case, owner, want):
    """the original index of the point that must win each island (-1: none)"""
    out = np.full(len(want), -1, dtype=np.int64)
    for i, w in enumerate(want):
        if w >= 0:
            out[i] = np.flatnonzero(owner == i)[w]
    return out


def segment_start(owner, i):
    """where island i's points start in the cell-sorted target: the islands' cells lie on one row, in island order, behind the origin
    anchor; the far anchor comes last (sc._assemble)"""
    return 1 + int((np.asarray(owner)[owner >= 0] < i).sum())


# ---- 3. the order the queries are dealt out in ------------------------------------------------------------------------------------------
ORDER_COUNTS = (1, 15, 16, 17, 127, 128, 129, 4099)  # around a wavefront's 16 queries and a workgroup's 128, and 33 workgroups
ORDER_ITERS = 2      # passes 0 and 1 deal in the two spread orders (pass_order), the pass after them in scan order
ORDER_VOID = 0.3


def order_inputs(n_src):
    """(src, tgt, nrm, T0): the stage cloud with n_src queries, started at the later-pass pose so that the first update is a real one"""
    src, tgt, nrm = rs.void_cloud(ORDER_VOID, n_src=n_src)
    return src, tgt, nrm, rs.LATER_INIT


# ---- 4. the end of the array, now that the scan loop loads beyond the end of a range -------------------------------------------------
END_LENGTHS = tuple(range(1, 18))  # points in the LAST cell of the cell-sorted array: every residue of a group's 16-candidate round, plus one
END_FILL = 16                      # queries that coincide with a target point (random normals): they give J^T J its rank
END_BOX = 2.2                      # the target's box is [0, END_BOX]^3: its last cell, (8, 8, 8) at cell 0.25, is [2, 2.25)^3
END_PLANE = 2.125                  # the corner queries and the last cell's points share this x; every target normal there is e_x
SCAN_SLACK_BYTES = 4096            # icp_kernels.hpp: kScanSlackBytes
POINT_BYTES = {rs.F32: 16, rs.F64: 32}
IN_FLIGHT = {rs.F32: 4, rs.F64: 2}  # scan_strided: loads issued before the first is consumed


def array_end_case(n_last):
    """(case, stale): sc.array_end_case with a last cell of exactly n_last points, as a registration that stands still.  The 64 corner
    queries stand beyond the far corner in y and z, one cell outside the grid (iy = ny, iz = nz), in the plane x = END_PLANE; the n_last
    points of the last cell lie in that plane and carry the normal e_x, so every residual (p - q) . n is zero; END_FILL more queries
    coincide with target points of random normals.  J^T r = 0: every update is the identity, every pass searches where the first did,
    and from pass 1 on the searches run with candidate lists (margin = its minimum).
    Two arrays END with these n_last points: the cell-sorted points (the last cell of the last row) and the replica, whose last
    super-row -- the one of the padded row (ny + 1, nz + 1), which only queries at iy = ny, iz = nz search -- holds the cells of the
    grid's last row alone; the queries' range of it (cells ix - 1 ... nx - 1) runs to its end (last_super_row).
    `stale`, uploaded, indexed, registered against and freed first, lies around the corner queries, nearer to each than any target
    point: whatever a scan takes from behind the last element of either array in a reused block wins or is listed."""
    rng = np.random.default_rng(620 + n_last)
    tgt = rng.uniform(0.0, 1.99, size=(sc.END_TARGETS, 3))
    last = np.column_stack([np.full(n_last, END_PLANE), rng.uniform(2.0, END_BOX, size=(n_last, 2))])
    last[0, 1:] = END_BOX                                # the far corner of the box in y and z: the last cell is (8, 8, 8) whatever the seed gives
    tgt[0], tgt[1:1 + n_last] = 0.0, last
    nrm = rs.unit_normals(rng, len(tgt))
    nrm[1:1 + n_last] = (1.0, 0.0, 0.0)
    corner = np.column_stack([np.full(64, END_PLANE), END_BOX + rng.uniform(0.15, 0.3, size=(64, 2))])
    fill = tgt[100:100 + END_FILL]
    src = np.vstack([corner, fill])
    stale = np.column_stack([END_PLANE + rng.uniform(-0.05, 0.05, size=sc.END_STALE), END_BOX + rng.uniform(0.1, 0.35, size=(sc.END_STALE, 2))])
    return rs.Case(f"array-end-{n_last}", src, tgt, nrm, 1.0, sc.CELL, np.eye(4), False), stale


def _cells(tgt, pts, cell):
    """(cell coordinates of pts in the grid of tgt, the grid's (nx, ny, nz)): origin at the box's minimum, as build_grid_t"""
    t = np.asarray(tgt)
    n = np.floor((t.max(axis=0) - t.min(axis=0)) / cell).astype(np.int64) + 1
    return np.floor((np.asarray(pts) - t.min(axis=0)) / cell).astype(np.int64), n


def last_super_row(tgt, queries, cell=sc.CELL):
    """(points in the LAST range of the replica, whether every query's stage-1 range is that range).  The replica (icp_kernels.hpp:
    replica_scatter_kernel) puts a point of cell (x, y, z) into the super-rows (y - dy, z - dz), dy, dz in {-1, 0, 1}, super-row (Y, Z)
    standing at ((Z + 1) * (ny + 2) + (Y + 1)) * nx in rstart; a query at (ix, iy, iz) scans cells max(ix - 1, 0) ... min(ix + 1, nx - 1)
    of super-row (iy, iz).  The last super-row is (ny, nz); a range that ends with its cell nx - 1 ends the array."""
    ijk, n = _cells(tgt, tgt, cell)
    q, _ = _cells(tgt, queries, cell)
    in_last = (ijk[:, 1] == n[1] - 1) & (ijk[:, 2] == n[2] - 1)          # the only row with y + 1 == ny and z + 1 == nz
    xlo = max(int(q[:, 0].min()) - 1, 0)
    count = int((in_last & (ijk[:, 0] >= xlo)).sum())
    at_end = bool((q[:, 1] == n[1]).all() and (q[:, 2] == n[2]).all() and (q[:, 0] + 1 >= n[0] - 1).all() and (q[:, 0] == q[0, 0]).all())
    return count, at_end


def last_cell_count(tgt, cell=sc.CELL):
    """points in the cell that comes last in the cell-sorted order (the largest cell number holds the far corner)"""
    t = np.asarray(tgt)
    ijk = np.floor((t - t.min(axis=0)) / cell).astype(np.int64)
    n = ijk.max(axis=0) + 1
    cid = (ijk[:, 2] * n[1] + ijk[:, 1]) * n[0] + ijk[:, 0]
    return int((cid == cid.max()).sum())
