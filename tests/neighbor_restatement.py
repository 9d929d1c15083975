"""o3ds_neighbor_search and the two outlier filters restated as brute force in numpy over all pairs, and the cases the tests share.
Nothing here uses a search structure, a grid or the device.

What one query is specified to return (include/o3ds_backend.h), and what `search` therefore does:
  * target coordinates are the stored ones (f32 or f64 storage);
  * the query is the stored point, or storage(T s) with T s formed in f64 as icp_search_restatement.transform forms it;
  * d2 = (dx*dx + dy*dy) + dz*dz in the storage type, every operation rounded on its own;
  * a candidate is accepted iff d2 is finite and (radius <= 0 or d2 < storage(radius * radius), strictly, the product formed in f64);
  * the list is the first max_nn accepted candidates in the order (d2, original target index); total counts all accepted candidates;
  * a non-finite query has an empty list and total 0.

The filters ([O3D] RemoveStatisticalOutliers / RemoveRadiusOutliers, v0.15.1):
  * statistical: a_i = (sum of sqrt(d2) over point i's KNN list of nb_neighbors, self included, f64 in list order) / count; valid iff
    a_i > 0; mean and std (n_valid - 1 in the denominator) over the valid points; keep iff a_i > 0 and a_i < mean + std_ratio * std;
  * radius: keep iff total_i > nb_points, total_i the count of points with d2 < storage(radius^2), self included.
The two sums of the statistical rule are taken here in numpy's order and on the device in another: the cases leave a margin between
every a_i and the threshold (asserted in tests/test_neighbor_restatement_cpu.py) so that no verdict depends on it.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import icp_search_restatement as isr
import normals_restatement as nr

F32, F64 = nr.F32, nr.F64
STORAGES = nr.STORAGES
to_storage = nr.to_storage
transform = isr.transform


class Lists(NamedTuple):
    idx: np.ndarray    # (n, max_nn) uint32, entries past cnt are 0
    d2: np.ndarray     # (n, max_nn) f64: the storage-type d2 widened, entries past cnt are 0
    cnt: np.ndarray    # (n,) uint32
    total: np.ndarray  # (n,) uint32
    tie: np.ndarray    # (n,) bool: the list is full and the first accepted candidate left out has the d2 of the last one kept


def stored_queries(queries, storage, T=None, query_idx=None) -> np.ndarray:
    """the query points as the kernel sees them, widened to f64"""
    s = to_storage(queries, storage)
    if query_idx is not None:
        s = s[np.asarray(query_idx, dtype=np.int64)]
    if T is None:
        return s
    with np.errstate(invalid="ignore", over="ignore"):
        return to_storage(transform(T, s), storage)


def search(queries, target, max_nn, radius, storage, T=None, query_idx=None, block=256) -> Lists:
    dt = np.float32 if storage == F32 else np.float64
    q = stored_queries(queries, storage, T, query_idx).astype(dt)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3).astype(dt)
    n, nt, k = len(q), len(t), int(max_nn)
    idx = np.zeros((n, k), np.uint32)
    d2o = np.zeros((n, k), np.float64)
    cnt = np.zeros(n, np.uint32)
    total = np.zeros(n, np.uint32)
    tie = np.zeros(n, bool)
    if nt == 0 or n == 0:
        return Lists(idx, d2o, cnt, total, tie)
    bounded = float(radius) > 0.0
    r2 = dt(float(radius) * float(radius))
    tx, ty, tz = (np.ascontiguousarray(t[:, a]) for a in range(3))
    w = min(k, nt)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        with np.errstate(invalid="ignore", over="ignore"):
            dx = tx[None, :] - q[b0:b1, 0:1]
            dy = ty[None, :] - q[b0:b1, 1:2]
            dz = tz[None, :] - q[b0:b1, 2:3]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == dt
            ok = np.isfinite(d2)
            if bounded:
                ok &= d2 < r2
        key = np.where(ok, d2, dt(np.inf))
        order = np.argsort(key, axis=1, kind="stable")  # columns are in index order: a stable sort orders by (d2, index)
        m = ok.sum(axis=1)
        c = np.minimum(m, k)
        total[b0:b1] = m
        cnt[b0:b1] = c
        rows = np.arange(b1 - b0)
        if w:
            head = order[:, :w]
            valid = np.arange(w)[None, :] < c[:, None]
            idx[b0:b1, :w] = np.where(valid, head, 0)
            d2o[b0:b1, :w] = np.where(valid, key[rows[:, None], head].astype(np.float64), 0.0)
        more = m > k
        if k and more.any():  # (then nt > k: column k of the order exists)
            tie[b0:b1] = more & (key[rows, order[:, min(k, nt - 1)]] == key[rows, order[:, k - 1]])
    return Lists(idx, d2o, cnt, total, tie)


def average_distances(L: Lists) -> np.ndarray:
    """a_i of the statistical filter: square roots and their sum in f64, in list order; 0 for an empty list"""
    s = np.zeros(len(L.cnt))
    for j in range(L.d2.shape[1]):
        s = s + np.where(j < L.cnt, np.sqrt(L.d2[:, j]), 0.0)  # (+ 0.0 leaves a sum as it is)
    return np.where(L.cnt > 0, s / np.maximum(L.cnt, 1), 0.0)


class Verdict(NamedTuple):
    keep: np.ndarray       # (n,) bool
    a: np.ndarray          # (n,) a_i (statistical) or total_i as f64 (radius)
    threshold: float       # mean + std_ratio * std (NaN when n_valid < 2), or nb_points
    margin: float          # statistical: min |a_i - threshold| / threshold over the valid points (inf: none, or a NaN threshold)


def statistical(points, nb_neighbors, std_ratio, storage) -> Verdict:
    a = average_distances(search(points, points, nb_neighbors, 0.0, storage))
    valid = a > 0.0
    nv = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(a[valid].sum()) / np.float64(nv)
        std = np.sqrt(np.float64(((a[valid] - mean) ** 2).sum()) / np.float64(nv - 1))
        thr = float(mean + float(std_ratio) * std)
        keep = valid & (a < thr)
    margin = float(np.min(np.abs(a[valid] - thr) / thr)) if nv and np.isfinite(thr) and thr > 0 else float("inf")
    return Verdict(keep, a, thr, margin)


def radius_filter(points, nb_points, radius, storage) -> Verdict:
    tot = search(points, points, 0, radius, storage).total
    return Verdict(tot > int(nb_points), tot.astype(np.float64), float(nb_points), float("inf"))


def point_cloud_distance(reference, cloud, ids, storage):
    """helpers.cpp:185-218 by brute force: (distances, ids), both without the ids nothing was found for"""
    ids = np.asarray(ids, dtype=np.int64)
    L = search(reference, cloud, 1, 0.0, storage, query_idx=ids)
    found = L.cnt > 0
    return np.sqrt(L.d2[found, 0]), ids[found]


def describe(differ, L: Lists, limit=12) -> str:
    """what a failing comparison reports: the queries that differ, their counts, whether the restated list ties at its last place"""
    d = np.asarray(differ)[:limit]
    return f"{len(differ)} queries differ: {d.tolist()} cnt {L.cnt[d].tolist()} total {L.total[d].tolist()} tie-at-last {L.tie[d].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- clouds
def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def integer_lattice() -> np.ndarray:
    """6 x 6 x 6 points with integer coordinates, shuffled: whole shells at d2 = 1, 2, 3, 4, ... exactly, in both storages"""
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), np.arange(6.0), indexing="ij"), -1).reshape(-1, 3)
    return _frozen(g[np.random.default_rng(61).permutation(len(g))])


@functools.lru_cache(maxsize=None)
def other_sheet() -> np.ndarray:
    """4100 points of another sheet over the ground of normals_restatement.ragged_cloud: queries that are not target points"""
    return _frozen(nr._surface(np.random.default_rng(62), 4100, 12.0, z0=1.6, origin=(-6.0, 2.0)))


@functools.lru_cache(maxsize=None)
def void_target() -> np.ndarray:
    return _frozen(isr.void_cloud(0.9, n_tgt=5000, n_src=64)[1])


@functools.lru_cache(maxsize=None)
def void_queries() -> np.ndarray:
    """64 points within 0.12 m of the centre of a void 0.9 m in radius: the nearest target is rings of empty cells away"""
    return _frozen(isr.void_cloud(0.9, n_tgt=5000, n_src=64)[0])


@functools.lru_cache(maxsize=None)
def outside_queries() -> np.ndarray:
    """points 100 m and 1e4 m beyond the ragged sheet's box on every side, on its diagonals, and one in its middle"""
    c = np.array([0.0, 8.0, 1.5])
    d = [v for v in np.stack(np.meshgrid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], indexing="ij"), -1).reshape(-1, 3)]
    return _frozen(np.vstack([c + 100.0 * np.asarray(d), c + 1e4 * np.asarray(d)]))


@functools.lru_cache(maxsize=None)
def nan_target() -> np.ndarray:
    """300 points of the ragged sheet, six of them with a NaN coordinate (one, two or all three)"""
    t = np.array(nr.ragged_cloud()[:300])
    t[7, 0] = np.nan
    t[8, 1] = np.nan
    t[99, 2] = np.nan
    t[100, :2] = np.nan
    t[250, :] = np.nan
    t[299, 1:] = np.nan
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def odd_queries() -> np.ndarray:
    """20 points of the other sheet with NaN and infinite rows among them"""
    q = np.array(other_sheet()[:20])
    q[3] = [np.nan, 1.0, 1.0]
    q[4] = [1.0, 1.0, np.nan]
    q[9] = [np.inf, 1.0, 1.0]
    q[10] = [1.0, -np.inf, 1.0]
    q[15] = [np.nan, np.inf, -np.inf]
    return _frozen(q)


OFF_GRID_POSE = isr.rigid((10.0, 20.0, 30.0), (50.0, -40.0, 5.0))  # takes the queries tens of metres outside the target's box
NEAR_POSE = isr.rigid((1.0, -2.0, 3.0), (0.1, 0.05, -0.02))


@functools.lru_cache(maxsize=None)
def ragged_query_idx() -> np.ndarray:
    """4001 indices into the 4097-point ragged sheet, unordered, with repeats"""
    out = np.random.default_rng(63).integers(0, 4097, 4001).astype(np.uint32)
    out[:3] = out[3]
    out.setflags(write=False)
    return out


class Case(NamedTuple):
    name: str
    target: object                 # () -> (nt, 3)
    queries: object = None         # () -> (nq, 3); None: the target cloud itself (one device cloud)
    params: tuple = ()             # ((max_nn, radius), ...); radius 0: unbounded
    T: object = None
    query_idx: object = None       # () -> indices
    index_cell: float = 0.0        # > 0: the target is given an index of this cell first (o3ds_cloud_build_index)


K_ALL = (1, 5, 32, 33, 128)


def _prefix(cloud, n):
    return lambda: cloud()[:n]


def _tiny_cases():
    out = []
    for n in (0, 1, 2):
        out.append(Case(f"tiny-{n}", _prefix(nr.ragged_cloud, n), _prefix(other_sheet, 17), ((5, 0.0), (5, 3.0), (0, 3.0), (1, 0.0))))
    for k in K_ALL:
        for n in sorted({max(k - 1, 1), k, k + 1}):
            out.append(Case(f"fill-k{k}-n{n}", _prefix(nr.ragged_cloud, n), _prefix(other_sheet, 17), ((k, 0.0), (k, 4.0))))
            out.append(Case(f"fill-self-k{k}-n{n}", _prefix(nr.ragged_cloud, n), None, ((k, 0.0),)))
    return out


def _count_cases():
    return [Case(f"queries-{n}", _prefix(nr.ragged_cloud, 500), _prefix(other_sheet, n), ((5, 0.0), (20, 1.0))) for n in (1, 15, 16, 17, 63, 64, 65)]


LATTICE_STEP = 0.25  # of normals_restatement.lattice; 0.5 = two steps, 0.25 * sqrt(2) is not a float: the radii below sit ON shells

CASES = tuple(_tiny_cases() + _count_cases() + [
    Case("ragged-idx", nr.ragged_cloud, None, ((20, 0.0), (5, 0.5), (0, 0.5)), query_idx=ragged_query_idx),
    Case("ragged-other", nr.ragged_cloud, other_sheet, ((1, 0.0), (20, 0.0), (20, 3.0))),
    # ties at every place; radii exactly on a lattice distance (strictness); a radius beyond the whole cloud and one below the spacing
    Case("lattice", nr.lattice, None, tuple((k, 0.0) for k in K_ALL) + ((7, 0.5), (32, 0.5), (0, 0.5), (0, 0.25), (128, 100.0), (5, 0.1), (0, 0.1))),
    Case("lattice-other", nr.lattice, lambda: nr.lattice()[::7] + [0.125, 0.125, 0.125], ((8, 0.0), (9, 0.0), (5, 0.1), (0, 0.1), (20, 0.5))),
    Case("integers", integer_lattice, None, ((5, 0.0), (7, 0.0), (8, 0.0), (33, 0.0), (7, 1.0), (7, 2.0), (0, 2.0), (128, 3.0))),
    Case("offset", nr.offset_cloud, None, ((20, 0.0), (20, 3.0), (5, 0.125), (33, 1.0))),
    Case("duplicates", nr.shuffled_duplicates, None, ((5, 0.0), (7, 0.6), (1, 0.0), (3, 0.0), (0, 0.26))),
    Case("one-cell", _prefix(nr.clump_cloud, 300), None, ((5, 0.0), (33, 0.0), (5, 0.05)), index_cell=5.0),
    Case("sheet", nr.planar_cloud, None, ((20, 0.0), (20, 1.0))),
    Case("line", nr.collinear_cloud, None, ((5, 0.0), (5, 0.2))),
    Case("two-density", nr.mixed_cloud, None, ((20, 0.0), (20, 3.0))),
    Case("void", void_target, void_queries, ((1, 0.0), (20, 0.0), (5, 0.5), (5, 1.0))),
    Case("outside", _prefix(nr.ragged_cloud, 1000), outside_queries, ((5, 0.0), (1, 0.0), (5, 50.0), (0, 120.0))),
    Case("non-finite", nan_target, odd_queries, ((5, 0.0), (5, 1.0), (0, 1.0))),
    Case("non-finite-self", nan_target, None, ((5, 0.0), (0, 0.5))),
    Case("pose-off-grid", _prefix(nr.ragged_cloud, 1000), lambda: nr.ragged_cloud()[1000:1100], ((5, 0.0), (5, 3.0)), T=OFF_GRID_POSE),
    Case("pose-near", _prefix(nr.ragged_cloud, 1000), lambda: nr.ragged_cloud()[1000:1100], ((5, 0.0), (1, 0.3), (20, 1.0)), T=NEAR_POSE),
    Case("fine-index", nr.ragged_cloud, _prefix(other_sheet, 300), ((20, 0.0), (20, 1.0)), index_cell=0.05),
    Case("coarse-index", nr.ragged_cloud, _prefix(other_sheet, 300), ((20, 0.0), (20, 1.0)), index_cell=50.0),
])
TIE_CASES = ("lattice", "integers", "offset", "duplicates")  # must hold lists that tie at the last place kept
F32_TIE_CASES = ("offset", "duplicates")                       # ... some of which f32 storage alone makes


@functools.lru_cache(maxsize=None)
def reference(name: str, max_nn: int, radius: float, storage: str) -> Lists:
    """the restated lists of a case of CASES, computed once per process"""
    case = next(c for c in CASES if c.name == name)
    tgt = case.target()
    q = tgt if case.queries is None else case.queries()
    return search(q, tgt, max_nn, radius, storage, T=case.T, query_idx=None if case.query_idx is None else case.query_idx())


# ---------------------------------------------------------------------------------------------------------------- filter cases
@functools.lru_cache(maxsize=None)
def scan_with_outliers() -> np.ndarray:
    """a seeded sheet of 3000 points 12 m across with 30 planted points 5 to 9 m above it"""
    rng = np.random.default_rng(71)
    sheet = nr._surface(rng, 3000, 12.0)
    far = np.column_stack([rng.uniform(0.0, 12.0, (30, 2)), rng.uniform(6.0, 10.0, 30)])
    out = np.vstack([sheet, far])[rng.permutation(3030)]
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def unit_pairs() -> np.ndarray:
    """64 points in 32 pairs one metre apart, the pairs 100 m from each other: with nb_neighbors = 2 every a_i is (0 + 1) / 2, every
    partial sum of the a_i and of (a_i - mean)^2 is exact in any order, std = 0 and the threshold is a_i itself: nothing is kept"""
    base = np.column_stack([100.0 * np.arange(32), np.zeros(32), np.zeros(32)])
    return _frozen(np.vstack([base, base + [0.0, 1.0, 0.0]])[np.random.default_rng(72).permutation(64)])


@functools.lru_cache(maxsize=None)
def one_valid() -> np.ndarray:
    """a point, its exact duplicate and a third point: with nb_neighbors = 2 only the third has a_i > 0 -- n_valid = 1, a NaN threshold"""
    return _frozen([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [2.0, 2.0, 3.0]])


class FilterCase(NamedTuple):
    name: str
    cloud: object
    statistical: tuple  # ((nb_neighbors, std_ratio), ...)
    radius: tuple       # ((nb_points, radius), ...)
    exact_sums: bool = False  # the margin premise is replaced by sums that are exact in any order (unit_pairs)


FILTER_CASES = (
    FilterCase("scan", scan_with_outliers, ((20, 2.0), (5, 1.0), (33, 3.0)), ((5, 0.5), (16, 1.0), (1, 0.05))),
    FilterCase("pairs", unit_pairs, ((2, 1.0),), ((1, 1.5), (1, 1.0)), True),
    FilterCase("one-valid", one_valid, ((2, 1.0),), ((1, 2.0),)),
    FilterCase("single", lambda: one_valid()[:1], ((3, 1.0),), ((1, 1.0),)),
    FilterCase("small", _prefix(scan_with_outliers, 30), ((50, 1.0),), ((50, 100.0), (3, 3.0))),  # nb_neighbors beyond the cloud
)
MARGIN = 1e-9


def attributes(n):
    """unit normals and colours that name their point: what the filters must carry"""
    rng = np.random.default_rng(73)
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True), np.column_stack([(np.arange(n) % 256) / 256.0, (np.arange(n) // 256) / 256.0, np.full(n, 0.5)])
