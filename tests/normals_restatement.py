"""The neighbour selection of estimate_normals (csrc/normals_kernel.hpp) restated as brute force in numpy, and the clouds the exact normals
tests share.  Nothing here uses a search structure, a grid or the device.

What the kernel is specified to compute, and what this file therefore does:
  * the coordinates are rounded to the storage type (f32 or f64) when they are uploaded;
  * d2 of a pair is (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own;
  * a candidate is accepted iff d2 < storage(radius * radius), strictly, the product formed in f64;
  * a point's list is the first max_nn accepted candidates in the order (d2, original index), the point itself included;
  * everything after the selection is the oracle's f64 arithmetic on the stored values, in list order (orc_normals_from_neighbours);
    with f32 storage the normal is rounded to f32 when it is stored.

tests/test_normals_restatement_cpu.py proves `normals(..., F64)` against the oracle's own k-d tree search and asserts the premises of the
cases below; tests/test_normals_exact_gpu.py holds the device to `normals` per point.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

F32, F64 = "f32", "f64"
STORAGES = (F32, F64)


def to_storage(a, storage) -> np.ndarray:
    """the values as the device holds them, widened back to f64"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    return a.astype(np.float32).astype(np.float64) if storage == F32 else a.copy()


class Lists(NamedTuple):
    idx: np.ndarray       # (n, max_nn) int32: row i holds point i's neighbours in the order (d2, index); entries past cnt[i] are 0
    cnt: np.ndarray       # (n,) int32
    tie: np.ndarray       # (n,) bool: the list is full and the first candidate left out has the d2 of the last one kept
    last: np.ndarray      # (n,) int32: index of the last neighbour kept (-1: none)
    runner_up: np.ndarray  # (n,) int32: index of the first accepted candidate left out (-1: none)


def search(pts, radius, max_nn, storage, block=256) -> Lists:
    dt = np.float32 if storage == F32 else np.float64
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3).astype(dt)
    n = len(p)
    r2 = dt(float(radius) * float(radius))
    k = int(max_nn)
    idx = np.zeros((n, k), np.int32)
    cnt = np.zeros(n, np.int32)
    tie = np.zeros(n, bool)
    last = np.full(n, -1, np.int32)
    runner_up = np.full(n, -1, np.int32)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        dx = x[None, :] - x[b0:b1, None]
        dy = y[None, :] - y[b0:b1, None]
        dz = z[None, :] - z[b0:b1, None]
        xx, yy, zz = dx * dx, dy * dy, dz * dz
        s = xx + yy
        d2 = s + zz
        assert d2.dtype == dt
        ok = d2 < r2
        key = np.where(ok, d2, dt(np.inf))
        order = np.argsort(key, axis=1, kind="stable")  # columns are in index order: a stable sort orders by (d2, index)
        m = ok.sum(axis=1)
        take = min(k + 1, n)
        head = order[:, :take]
        c = np.minimum(m, k)
        cnt[b0:b1] = c
        w = min(k, n)
        idx[b0:b1, :w] = np.where(np.arange(w)[None, :] < c[:, None], head[:, :w], 0)
        rows = np.arange(b1 - b0)
        has = c > 0
        last[b0:b1] = np.where(has, head[rows, np.maximum(c - 1, 0)], -1)
        more = m > k  # (then n > k and column k of head exists)
        if more.any():
            ru = head[rows, min(k, take - 1)]
            runner_up[b0:b1] = np.where(more, ru, -1)
            tie[b0:b1] = more & (key[rows, ru] == key[rows, np.where(has, last[b0:b1], 0)])
    return Lists(idx, cnt, tie, last, runner_up)


def neighbours(pts, radius, max_nn, storage):
    """(idx, cnt): the ordered neighbour list of every point"""
    L = search(pts, radius, max_nn, storage)
    return L.idx, L.cnt


def normals_from(pts, lists: Lists, storage, raw=False) -> np.ndarray:
    from oracle import pyoracle

    out = pyoracle.normals_from_neighbours(to_storage(pts, storage), lists.idx, lists.cnt, raw)
    return out.astype(np.float32).astype(np.float64) if storage == F32 else out


def normals(pts, radius, max_nn, storage) -> np.ndarray:
    return normals_from(pts, search(pts, radius, max_nn, storage), storage)


def f32_only_ties(pts, lists: Lists) -> np.ndarray:
    """(n,) bool: of the points whose F32 list ties at the last place, those where the two candidates' d2 differ in f64 (on the stored
    f32 coordinates): the places where f32 storage must go by the index and f64 arithmetic would go by the distance"""
    s = to_storage(pts, F32)
    out = np.zeros(len(s), bool)
    i = np.flatnonzero(lists.tie)
    if len(i):
        d = lambda j: (((s[j] - s[i]) ** 2).sum(axis=1))  # noqa: E731
        out[i] = d(lists.last[i]) != d(lists.runner_up[i])
    return out


def expected_cell(stored, radius, max_nn) -> float:
    """The cell normals_t chooses for a cloud it has no remembered cell for (backend.hip): a pilot grid at radius / 8 anchored at the cloud's
    minimum, the mean number of points per occupied pilot cell, cell = pilot * sqrt(max_nn / (pi * mean)) clamped to [radius / 64, radius].
    Only the premises of the cases are asserted with it; it is never a reference for a normal."""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    pilot = radius / 8.0
    c = np.floor((stored - stored.min(axis=0)) * (1.0 / pilot)).astype(np.int64)
    occ = len(np.unique(c, axis=0))
    avg = len(stored) / occ
    cell = pilot * np.sqrt(max(1.0, float(max_nn)) / (3.14159265358979 * avg))
    return float(min(max(cell, radius / 64.0), radius))


def cells_of(stored, cell) -> np.ndarray:
    """integer cell coordinates on a grid of that cell anchored at the cloud's minimum"""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    return np.floor((stored - stored.min(axis=0)) * (1.0 / cell)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- clouds
def _surface(rng, n, extent, z0=1.5, origin=(0.0, 0.0)):
    """n points on a gently waved sheet extent x extent m, with a little noise: what a neighbourhood of a lidar scan looks like"""
    xy = rng.uniform(0.0, extent, (n, 2)) + np.asarray(origin)
    z = z0 + 0.3 * np.sin(0.7 * xy[:, 0]) * np.cos(0.5 * xy[:, 1]) + rng.normal(0.0, 0.01, n)
    return np.column_stack([xy, z])


@functools.lru_cache(maxsize=None)
def scan_thin() -> np.ndarray:
    """the 32 768-point synthetic OS-128 scan of the other pre-processing tests, VoxelDownSample(0.1), every 10th point: ~3100 points"""
    from open3d_slam_amd import synthetic as syn
    from oracle import pyoracle

    scan = syn.os128_scan(syn.make_scene(), np.eye(4), n_az=256)
    out = pyoracle.voxel_down_sample(scan, 0.1)[::10].copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lattice() -> np.ndarray:
    """12 x 12 x 3 points 0.25 m apart (coordinates exact in f32): whole shells of equidistant neighbours"""
    g = np.stack(np.meshgrid(np.arange(12) * 0.25, np.arange(12) * 0.25, np.arange(3) * 0.25, indexing="ij"), -1).reshape(-1, 3) + [3.0, -2.0, 1.0]
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def shuffled_duplicates() -> np.ndarray:
    """the lattice with exact duplicates (some three times), with points that differ from a lattice point by 1e-9 -- distinct in f64,
    equal to it in f32 --, shuffled"""
    g = lattice()
    rng = np.random.default_rng(3)
    near = g[rng.choice(len(g), 30, replace=False)] + rng.choice([-1e-9, 1e-9], (30, 3))
    dup = np.vstack([g, g[rng.choice(len(g), 40, replace=False)], g[:5], g[:5], near])
    out = dup[rng.permutation(len(dup))]
    assert len(np.unique(out, axis=0)) > len(np.unique(out.astype(np.float32), axis=0))
    out.setflags(write=False)
    return out


OFFSET = (1e5, -2e5, 50.0)


@functools.lru_cache(maxsize=None)
def offset_cloud() -> np.ndarray:
    """40 x 40 points 0.125 m apart in x and y, 1e5 / 2e5 m from the origin (where f32 holds x and y to 8 and 16 mm: the lattice is exact),
    z = 50 +- 0.2 mm of jitter.  dx*dx + dy*dy is exact in f32 and the same for a whole shell; dz*dz (< 2e-7) falls below the last bit of
    the sum for all but the nearest shells, so the members of a shell TIE in f32 and do not in f64: the place goes to the smaller index
    where f64 arithmetic would give it to the smaller dz"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(40) * 0.125, np.arange(40) * 0.125, indexing="ij"), -1).reshape(-1, 2)
    out = np.column_stack([g, rng.uniform(-2e-4, 2e-4, len(g))])[rng.permutation(len(g))] + np.asarray(OFFSET)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ragged_cloud() -> np.ndarray:
    """4097 points of a sheet 12 m across; its prefixes are the clouds of ragged size"""
    out = _surface(np.random.default_rng(5), 4097, 12.0, origin=(-6.0, 2.0))
    out.setflags(write=False)
    return out


RAGGED_SIZES = (1, 2, 3, 5, 15, 17, 63, 65, 4097)
RAGGED_PARAMS = (3.0, 20)

REUSE_PARAMS = (3.0, 20)


@functools.lru_cache(maxsize=None)
def clump_cloud() -> np.ndarray:
    """3000 points in a cube 0.18 m across: one pilot cell, so a fresh cell clamps to radius / 64 and every 3x3x3 block is crowded"""
    out = np.random.default_rng(21).uniform(0.0, 0.18, (3000, 3)) + [4.0, -3.0, 1.0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def spread_cloud() -> np.ndarray:
    """3100 points of a sheet 20 x 20 x 1 m: on the clump's cell its neighbourhoods are some twenty cells deep"""
    rng = np.random.default_rng(22)
    out = np.column_stack([rng.uniform(-10.0, 10.0, (3100, 2)), rng.uniform(0.0, 1.0, 3100)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lonely_cloud() -> np.ndarray:
    """2900 points over 400 x 400 x 20 m, each alone in its pilot cell: a fresh cell is as large as the heuristic makes one,
    radius / 8 * sqrt(max_nn / pi) -- 0.95 m at (3.0, 20); the clamp to `radius` itself needs max_nn > 64 pi"""
    rng = np.random.default_rng(23)
    out = np.column_stack([rng.uniform(-200.0, 200.0, (2900, 2)), rng.uniform(0.0, 20.0, 2900)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixed_cloud() -> np.ndarray:
    """half of the points in a 5 cm clump, half on a sheet 30 m across, interleaved"""
    rng = np.random.default_rng(31)
    a = rng.uniform(0.0, 0.05, (1500, 3)) + [12.0, 17.0, 1.4]
    b = _surface(rng, 1500, 30.0)
    out = np.vstack([a, b])[rng.permutation(3000)]
    out.setflags(write=False)
    return out


MIXED_PARAMS = (3.0, 20)


def beyond_radius(stored) -> float:
    """the radius the k-NN route of the generalized estimator sets (normals_t, knn_raw): no pair of points exceeds it"""
    d = stored.max(axis=0) - stored.min(axis=0)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * 1.001 + 1e-3)


@functools.lru_cache(maxsize=None)
def planar_cloud() -> np.ndarray:
    """1600 points with one z: a grid one cell high"""
    rng = np.random.default_rng(41)
    out = np.column_stack([rng.uniform(0.0, 10.0, (1600, 2)) + [2.0, -5.0], np.full(1600, 1.25)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def collinear_cloud() -> np.ndarray:
    """400 points on a line along x: a grid one cell high and one cell deep, and a covariance of rank one"""
    rng = np.random.default_rng(42)
    out = np.column_stack([np.sort(rng.uniform(-8.0, 8.0, 400)), np.full(400, 2.5), np.full(400, 0.75)])
    out.setflags(write=False)
    return out


FACE_PARAMS = ((4.0, 20), (4.0, 3))  # radius / 64 = 1 / 16, the lattice's spacing


@functools.lru_cache(maxsize=None)
def face_cloud() -> np.ndarray:
    """16 x 16 x 16 points 1/16 m apart from (1, 2, 0.5), all exact in f32.  A pilot cell (0.5 m) holds 512 of them, so the cell clamps to
    radius / 64 = 1/16 and EVERY point sits on the corner of eight cells; the points with index 0 and 15 along an axis are in the grid's
    first and last cells"""
    g = np.stack(np.meshgrid(np.arange(16) / 16.0, np.arange(16) / 16.0, np.arange(16) / 16.0, indexing="ij"), -1).reshape(-1, 3) + [1.0, 2.0, 0.5]
    out = g[np.random.default_rng(43).permutation(len(g))]
    out.setflags(write=False)
    return out


class Case(NamedTuple):
    name: str
    cloud: object  # () -> (n, 3) f64
    params: tuple  # ((radius, max_nn), ...); radius None: beyond_radius of the stored cloud
    storages: tuple = STORAGES


# max_nn: 1, 2, 3 (identity covariance below three), 20, 32 | 33 (the two instantiations), 48, 128, one beyond the cloud; the radii of
# test_estimate_normals_matches_oracle (3.0, 1.0, 0.5; 2.0 with 48) on the scan, radii that cut lattice shells on the lattices
# (on the lattices (0.5, 48) and (0.25, 20) give short lists with candidates at d2 == r^2 exactly, which the strict test leaves out)
PER_POINT = (
    Case("scan", scan_thin, ((3.0, 20), (1.0, 5), (0.5, 30), (2.0, 48), (3.0, 1), (1.0, 2), (0.5, 3), (3.0, 32), (3.0, 33), (3.0, 128), (1.0, 128), (0.5, 33)), (F32,)),
    Case("lattice", lattice, ((0.6, 7), (1.0, 20), (0.3, 30), (0.6, 1), (0.6, 2), (0.3, 3), (1.0, 32), (1.0, 33), (0.6, 48), (3.0, 128), (0.5, 48), (0.25, 20)), (F32,)),
    Case("lattice-prefix", lambda: lattice()[:7], ((5.0, 20),), (F32,)),  # max_nn beyond the cloud
    Case("duplicates", shuffled_duplicates, ((0.6, 7), (0.26, 5), (2.0, 40), (0.5, 3), (1.0, 32), (1.0, 33), (3.0, 128), (0.3, 2), (0.3, 1), (0.5, 48)), (F32,)),
    Case("offset", offset_cloud, ((3.0, 20), (1.0, 5), (0.5, 30), (2.0, 48), (3.0, 1), (3.0, 2), (1.0, 3), (3.0, 32), (3.0, 33), (3.0, 128)), (F32,)),
    # f64 storage beyond max_nn 48, against oracle.estimate_normals in the GPU test
    Case("scan-f64", scan_thin, ((3.0, 32), (3.0, 33), (3.0, 128)), (F64,)),
    Case("duplicates-f64", shuffled_duplicates, ((1.0, 32), (1.0, 33), (3.0, 128), (0.5, 48)), (F64,)),
)
SEEDED_F32 = ("offset", "duplicates")  # the cases that must hold ties that only f32 makes

RAGGED = tuple(Case(f"ragged-{n}", (lambda n=n: ragged_cloud()[:n]), (RAGGED_PARAMS,)) for n in RAGGED_SIZES)
REUSE = (  # (name, the cloud the handle sees first, the cloud estimated on the first one's cell)
    ("clump-then-spread", clump_cloud, spread_cloud),
    ("lonely-then-clump", lonely_cloud, clump_cloud),
)
MIXED = (Case("mixed", mixed_cloud, (MIXED_PARAMS,)),)
BEYOND = (Case("beyond", scan_thin, ((None, 20),)),)
DEGENERATE = (
    Case("planar", planar_cloud, ((1.0, 20), (3.0, 33))),
    Case("collinear", collinear_cloud, ((1.0, 20), (0.2, 5))),
    Case("faces", face_cloud, FACE_PARAMS),
)
ALL_CASES = PER_POINT + RAGGED + MIXED + BEYOND + DEGENERATE + tuple(
    Case(name, cloud, (REUSE_PARAMS,)) for name, cloud in (("clump", clump_cloud), ("spread", spread_cloud), ("lonely", lonely_cloud)))


def radius_of(case_radius, stored) -> float:
    return beyond_radius(stored) if case_radius is None else float(case_radius)


@functools.lru_cache(maxsize=None)
def reference(name: str, radius, max_nn: int, storage: str):
    """(lists, normals, radius used) of a case of ALL_CASES, computed once per process"""
    case = next(c for c in ALL_CASES if c.name == name)
    pts = case.cloud()
    r = radius_of(radius, to_storage(pts, storage))
    L = search(pts, r, max_nn, storage)
    nrm = normals_from(pts, L, storage)
    nrm.setflags(write=False)
    return L, nrm, r


def describe(differ, lists: Lists, limit=12) -> str:
    """what a failing comparison reports: the indices that differ, their neighbour counts, whether their lists tie at the last place"""
    differ = np.asarray(differ)
    d = differ[:limit]
    return f"{len(differ)} differ: idx {d.tolist()} cnt {lists.cnt[d].tolist()} tie-at-last {lists.tie[d].tolist()}"
