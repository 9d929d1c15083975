"""Inputs for the scan loop of the ICP search (icp_kernels.hpp: scan_strided, consider, nn_before, lanes_min): the candidate test as one
unsigned compare of (float bits of d2, original index), ties and the radius under it, and the loop's addressing at the end of a segment,
of a half-row and of the array.  tests/test_icp_scan_loop_cpu.py proves the premises of these inputs with numpy alone;
tests/test_icp_scan_loop_gpu.py runs them on the device against the brute force of tests/icp_search_restatement.py.

Lattice inputs are built from ISLANDS as in tests/icp_search_rows_cases.py: a query and the target points meant for it, the islands in a
line along x and more than 2 r + 3 cells apart.  Coordinates are multiples of cell / 4096 with cell = 0.25: exact in f32 and f64, and so
is every squared distance formed from them (by products and sums or by fused steps alike), so ties ARE ties on the device.
"""
from __future__ import annotations

import numpy as np

import icp_search_restatement as rs

CELL = 0.25
K = 4                     # r = 3.75 cells: 81 rows in the far stage's cross-section
R = (K - 0.25) * CELL
PITCH = 2 * K + 3


# ---- 1. the key order --------------------------------------------------------------------------------------------------------------
def key(d2, idx):
    """the 64-bit key of nn_before with f32 storage: float bits of d2 in the high word, the original index in the low word"""
    d2 = np.asarray(d2, dtype=np.float32)
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.int64).astype(np.uint32).astype(np.uint64)


NO_IDX = 0                # NNBest<P4f>::kNoIdx: the low word of the empty bound {r^2, -1, kNoIdx}
KEY_D2 = np.array([0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 1e-20, 0.0625, 0.99999994, 1.0, 1.0000001, 14.0625, 3.4028235e38, np.inf],
                  dtype=np.float32)  # +0, the smallest and the largest denormal, the smallest normal, ..., the largest finite value, +inf
KEY_NANS = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
KEY_IDX = np.array([0, 1, 2, 12345, 2 ** 31 - 2], dtype=np.int64)


# ---- islands -----------------------------------------------------------------------------------------------------------------------
def _assemble(name, islands, exact, seed, first=None, last=None, r=R):
    """islands: [(query offset in cells from the island's own cell corner, [target offsets in cells from the same corner])]; the own
    cell of island i is (K + 2 + i * PITCH, K + 2, K + 2).  The anchors that fix the grid (the origin and the far corner) stand in the
    MIDDLE of the target array, so that index 0 and the largest index belong to island points: `first` / `last` name the island whose
    points open / close the array (default: the first / the last island)."""
    order = list(range(len(islands)))
    if first is not None:
        order.remove(first), order.insert(0, first)
    if last is not None:
        order.remove(last), order.append(last)
    src, blocks = [], {}
    for i, (q, ts) in enumerate(islands):
        corner = np.array([K + 2 + i * PITCH, K + 2, K + 2], dtype=np.float64)
        src.append((corner + np.asarray(q, dtype=np.float64)) * CELL)
        blocks[i] = [(corner + np.asarray(t, dtype=np.float64)) * CELL for t in ts]
    hi = np.array([K + 2 + len(islands) * PITCH, 2 * K + 5, 2 * K + 5], dtype=np.float64) * CELL
    half = max(len(order) // 2, 1)
    tgt, owner = [], []
    for n, i in enumerate(order):
        if n == half:
            tgt += [np.zeros(3), hi]
            owner += [-1, -1]
        tgt += blocks[i]
        owner += [i] * len(blocks[i])
    assert len(order) > 1 and owner[0] >= 0 and owner[-1] >= 0
    tgt, src = np.array(tgt), np.array(src)
    assert (tgt.astype(np.float32).astype(np.float64) == tgt).all() and (src.astype(np.float32).astype(np.float64) == src).all()
    nrm = rs.unit_normals(np.random.default_rng(seed), len(tgt))
    return rs.Case(name, src, tgt, nrm, r, CELL, np.eye(4), exact), np.array(owner)


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------------
# (a, b): two points at exactly the same distance from the query at the centre (0.5, 0.5, 0.5) of its cell, offsets in cells
C = 0.5
TIE_PAIRS = (
    ("same cell, neighbours in a group's lanes", (C - 0.25, C, C), (C + 0.25, C, C)),                # d = 1/4
    ("two rows of the 3x3x3 block", (C, C + 1.0, C), (C, C, C - 1.0)),                               # d = 1
    ("stage 1 against stage 2", (C + 0.5, C + 1.0, C + 1.0), (C + 1.5, C, C)),                       # d = 3/2: cells (1,1,1) and (2,0,0)
    ("two rows of the 5x5x5 shell", (C, C + 1.75, C), (C, C, C - 1.75)),                             # d = 7/4: cells (0,2,0) and (0,0,-2)
    ("stage 2 against stage 3", (C + 1.5, C + 2.0, C), (C + 2.5, C, C)),                             # d = 5/2: cells (2,2,0) and (3,0,0)
    ("two half-rows of the far stage", (C - 3.0, C, C), (C + 3.0, C, C)),                            # d = 3
)
TIE_SPHERE = [(C + s * 0.25 * (a == 0), C + s * 0.25 * (a == 1), C + s * 0.25 * (a == 2)) for a in range(3) for s in (-1, 1)]  # six in one cell


def ties_case():
    """every pair in both orders, and six points of one cell on a sphere around the query (more tied points than a group has lanes).
    The array opens with a tied point (index 0) and closes with one (the largest index): the island of the first pair comes first,
    the sphere's island last."""
    islands = []
    for _, a, b in TIE_PAIRS:
        islands.append(((C, C, C), [a, b]))
        islands.append(((C, C, C), [b, a]))
    islands.append(((C, C, C), TIE_SPHERE))
    return _assemble("ties", islands, True, 501, first=0, last=len(islands) - 1)


# ---- 3. the radius -------------------------------------------------------------------------------------------------------------------
RADIUS_R = 5 * CELL  # r^2 = 25/16: exact; the candidate at (3, 4, 0) quarter-metres from the query


def d2_f32_fused(q, t):
    """(d2, exact): dist2 of icp_kernels.hpp with f32 storage, fmaf(dz, dz, fmaf(dy, dy, dx * dx)), every step rounded once -- emulated
    in f64, whose sum of an f32 square and an f32 holds all bits where `exact` says so (it then converts back to f32 without loss, or
    the rounding to f32 is the fused step's one rounding: an f64 sum of two such terms is exact unless they are 2^29 apart)"""
    d = (np.asarray(t, np.float64).astype(np.float32) - np.asarray(q, np.float64).astype(np.float32)).astype(np.float64)
    a = np.float32(d[..., 0] * d[..., 0]).astype(np.float64)
    b64 = d[..., 1] * d[..., 1] + a
    b = np.float32(b64).astype(np.float64)
    c64 = d[..., 2] * d[..., 2] + b
    return np.float32(c64), (np.float32(b64).astype(np.float64) == b64) & (np.float32(c64).astype(np.float64) == c64)


def d2_storage(q, t, storage):
    """the squared distance as the device forms it in a storage (f64: three products and two sums, as the brute force does)"""
    if storage == rs.F32:
        return d2_f32_fused(q, t)[0].astype(np.float64)
    d = np.asarray(t, np.float64) - np.asarray(q, np.float64)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _one_below(q, on, r2, storage):
    """the point `on` (at d2 == r2 from q) moved so that d2, as the device forms it, is the storage's number just below r2: y one ulp
    towards the query (that alone takes d2 several numbers down, the coordinate's ulp being the coarser), then z away from the query's
    plane by the multiple of its ulp that brings d2 back up to exactly one below -- found by trying them"""
    one = np.float32 if storage == rs.F32 else np.float64
    want = float(np.nextafter(one(r2), one(0.0)))
    t = np.array(on, dtype=np.float64)
    t[1] = float(np.nextafter(one(t[1]), one(0.0)))
    need = want - float(d2_storage(q, t, storage))
    assert need > 0.0
    uz = float(np.nextafter(one(t[2]), one(np.inf))) - t[2]
    k = int(np.sqrt(need) / uz) + np.arange(-50_000, 50_000)
    cand = np.repeat(t[None, :], len(k), axis=0)
    cand[:, 2] = t[2] + k * uz
    hit = np.flatnonzero(d2_storage(q, cand, storage) == want)
    assert hit.size, "no multiple of the z-ulp lands on the number below r^2"
    return cand[hit[0]]


def radius_case(storage):
    """island 0: the only candidate at d2 == r^2 exactly (no match: strict); island 1: the only candidate at the storage's number just
    below r^2, as the device forms d2 (a match); island 2: a candidate at d2 == r^2 and a nearer one behind it in the array (the bound
    r^2 is replaced, the point on the radius stays out); island 3: two candidates on the radius (a tie ON the radius: none wins)."""
    on = (C + 3.0, C + 4.0, C)
    islands = [((C, C, C), [on]), ((C, C, C), [on]), ((C, C, C), [on, (C, C + 2.0, C)]), ((C, C, C), [on, (C - 4.0, C - 3.0, C)])]
    (case, owner) = _assemble(f"radius-{storage}", islands, True, 502, r=RADIUS_R)
    tgt = case.tgt.copy()
    k = int(np.flatnonzero(owner == 1)[0])
    tgt[k] = _one_below(case.src[1], tgt[k], RADIUS_R * RADIUS_R, storage)
    return case._replace(tgt=tgt, storages=(storage,)), owner


# ---- 4. segment ends -----------------------------------------------------------------------------------------------------------------
SEGMENT_COUNTS = tuple(range(1, 34))  # points in the query's cell: a group of 4 lanes with four loads in flight takes 16 per iteration
HALF_ROW_COUNTS = (255, 256, 257)     # points of one far half-row: 64 lanes with four loads in flight take 256 per iteration


def _cell_points(rng, n, corner):
    """n distinct points of the cell at `corner` (offsets in cells) on its lattice of sixteenths, in random order"""
    pick = rng.choice(16 ** 3, size=n, replace=False)
    return [(corner[0] + (p % 16) / 16.0, corner[1] + (p // 16 % 16) / 16.0, corner[2] + (p // 256) / 16.0) for p in pick]


def segments_case():
    """islands whose own cell holds 1 ... 33 points and nothing else near: the segment of the group scan (the own row, or the replica's
    range of the block) is exactly that long.  The query stands a little off the cell's corner, off the lattice, so distances differ;
    which of the n points is nearest is left to the seed -- over 33 islands the winner falls on first, last and inner elements."""
    rng = np.random.default_rng(503)
    islands = [((132.0 / 4096, 196.0 / 4096, 100.0 / 4096), _cell_points(rng, n, (0.0, 0.0, 0.0))) for n in SEGMENT_COUNTS]
    return _assemble("segments", islands, True, 504)


def half_rows_case():
    """islands whose only points lie in ONE cell three rows up (row (3, 0), the own x-column: the left half-row of an outer row): a
    far-stage half-row of 255, 256 and 257 points, scanned by all 64 lanes"""
    rng = np.random.default_rng(505)
    islands = [((C + 1.0 / 4096, C, C + 3.0 / 4096), _cell_points(rng, n, (0.0, 3.0, 0.0))) for n in HALF_ROW_COUNTS]
    return _assemble("half-rows", islands, True, 506)


# ---- 5. the end of the array, with stale points behind it ---------------------------------------------------------------------------
END_TARGETS, END_STALE = 5000, 6000  # one pool class: see pool_block


def pool_block(nbytes):
    """the block dev_alloc hands out for a request (backend.hip): rounded up to an eighth of the next power of two, at least 256"""
    nbytes = max(nbytes, 256)
    gran = 256
    while gran * 8 < nbytes:
        gran <<= 1
    return (nbytes + gran - 1) // gran * gran


def pool_reuses(have, nbytes):
    """dev_alloc takes a cached block of `have` bytes for a request if it is large enough and at most a quarter larger"""
    want = pool_block(nbytes)
    return want <= have <= want + want // 4


def array_end_case():
    """a target of END_TARGETS points in the box [0, 2]^3 whose LAST cell in the cell-sorted order (the far corner) holds the nearest
    neighbours of the queries, which stand beyond that corner, outside the box.  END_STALE points of `stale`, uploaded, indexed and freed
    before the target is built, lie nearer to every query than any target point: whatever a scan reads behind the target's last
    element in a reused block would win or be listed."""
    rng = np.random.default_rng(507)
    tgt = rng.uniform(0.0, 2.0, size=(END_TARGETS, 3))
    tgt[0], tgt[1] = 0.0, 2.0                                     # the box is exactly [0, 2]^3; tgt[1] is the far corner itself
    tgt[2:40] = 2.0 - rng.uniform(0.0, 0.2, size=(38, 3))         # the corner cell is well filled
    src = 2.0 + rng.uniform(0.15, 0.3, size=(64, 3))              # beyond the corner: 0.26 to 0.52 m from it
    stale = 2.0 + rng.uniform(0.1, 0.35, size=(END_STALE, 3))     # around the queries, dense
    nrm = rs.unit_normals(rng, len(tgt))
    return rs.Case("array-end", src, tgt, nrm, 1.0, CELL, np.eye(4), False), stale


def lists_case():
    """the registration of tests/icp_search_rows_cases.py that starts millimetres from the truth, so that its passes after the first run
    with candidate lists on and the passes after those verify inside them: the counters of its passes show what the scans listed"""
    import icp_search_rows_cases as rc

    return rc.lists_case()._replace(name="lists")


# ---- later passes: the bound a search starts from ------------------------------------------------------------------------------------
# A search of pass > 0 starts from the match the previous search of the session cached (icp_kernels.hpp: prefetch_query, use_cache) or,
# in the fused kernel, from the best of the points the previous search listed.  The step-wise ABI takes the record of an update from the
# caller (o3ds_icp_update), so a hand-written one advances the pass with a pose the test chooses:
#   * ZERO_RECORD (no correspondences): the identity update.  The second search runs at the pose of the first, from what it cached.
#   * step_back_record(t): the update is the translation -t, exactly.  A session begun at the translation +t and searched there caches
#     the matches of THAT pose; after the update the pose is the identity and the search starts from them: stale points, a tied point
#     of the larger index, the point that now lies ON the radius -- or, begun out of everything's reach (OUT_OF_REACH), from `none`.
ONE_CELL = (CELL, 0.0, 0.0)
OUT_OF_REACH = (0.0, 0.0, 100 * CELL)
STARTS = {"stale": ONE_CELL, "none": OUT_OF_REACH}
ZERO_RECORD = np.zeros(32)


def translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def step_back_record(t):
    """the record (common.hpp: 21 entries of J^T J, 6 of J^T r, r^2 sum, count, d^2 sum) whose update is the translation -t exactly:
    J^T J the identity, J^T r = (0, 0, 0, t) -- x = -(J^T r) / 1, three zero angles -- and one correspondence, so that the step is taken"""
    rec = np.zeros(32)
    rec[[0, 6, 11, 15, 18, 20]] = 1.0
    rec[21:24] = -0.0
    rec[24:27] = t
    rec[28] = 1.0
    return rec


STILL_FILL = 8  # islands of the still case whose query coincides with a target point


def radius_still_case(storage):
    """the radius case for the FUSED kernel, whose bound of pass 2 onwards comes from the candidate sets: a registration whose every
    update is the identity, so that all its passes search at the pose the points were placed for.  A correspondence contributes J r to
    J^T r, and every residual here is exactly zero: island 1's point one below r^2 lies in the query's plane x = const and carries the
    normal e_x, so does island 2's nearer point, and STILL_FILL more islands hold one point AT the query (random normals: they give J^T J
    its rank).  Islands 0 and 3 are those of radius_case: one candidate, and two, exactly ON the radius, never a match -- but listed
    (the margin of a set is at least a millimetre), so that pass 2 forms its bound from points at d2 == r^2."""
    on, on_x = (C + 3.0, C + 4.0, C), (C, C + 5.0, C)
    islands = [((C, C, C), [on]), ((C, C, C), [on_x]), ((C, C, C), [on, (C, C + 2.0, C)]), ((C, C, C), [on, (C - 4.0, C - 3.0, C)])]
    islands += [((C, C, C), [(C, C, C)])] * STILL_FILL
    (case, owner) = _assemble(f"radius-still-{storage}", islands, True, 508, r=RADIUS_R)
    tgt, nrm = case.tgt.copy(), case.nrm.copy()
    k = int(np.flatnonzero(owner == 1)[0])
    tgt[k] = _one_below(case.src[1], tgt[k], RADIUS_R * RADIUS_R, storage)
    nrm[k] = nrm[int(np.flatnonzero(owner == 2)[1])] = (1.0, 0.0, 0.0)
    return case._replace(tgt=tgt, nrm=nrm, storages=(storage,)), owner


def lattice_cases():
    return [ties_case()[0], segments_case()[0], half_rows_case()[0]] + [radius_case(s)[0] for s in rs.STORAGES]


def all_cases():
    return lattice_cases() + [array_end_case()[0], lists_case()]
