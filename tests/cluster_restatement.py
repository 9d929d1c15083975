"""o3ds_cluster_dbscan and o3ds_remove_small_clusters restated as brute force in numpy over all pairs, and the cases the tests share.
Nothing here uses a search structure, a grid or the device.

What the labels are specified to be (include/o3ds_backend.h), with the arithmetic of neighbor_restatement.search:
  * coordinates are the stored ones (f32 or f64 storage); d2(i, j) = (dx*dx + dy*dy) + dz*dz in the storage type, every operation
    rounded on its own;
  * j is a neighbour of i iff d2 is finite and d2 < storage(eps * eps), strictly, the product formed in f64; N_i is the neighbour set of
    point i in its own cloud, self included; a point with a non-finite coordinate has an empty N_i;
  * i is a core point iff |N_i| >= min_points;
  * clusters are the connected components of the graph on the core points with an edge i - j iff j is in N_i, numbered in the order of
    each component's smallest core index;
  * a non-core point gets the smallest cluster id among the core points in N_i, or -1.
`closed_form` is that text.  `sequential` is [O3D] v0.15.1 PointCloud::ClusterDBSCAN transcribed as a procedure over the same adjacency:
seeds in index order, a breadth-first walk, a point first marked noise relabelled by the first cluster that reaches it.
tests/test_cluster_restatement_cpu.py holds the two equal on every case.

The filter: keep point i iff label_i >= 0 and sizes[label_i] >= min_cluster_size.
"""
from __future__ import annotations

import collections
import functools
from typing import NamedTuple

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

import neighbor_restatement as nb
import normals_restatement as nr

F32, F64 = nb.F32, nb.F64
STORAGES = nb.STORAGES


def adjacency(points, eps, storage, block=512):
    """(csr bool matrix a with a[i, j] iff j is in N_i -- columns ascending in every row --, the d2 of its entries widened to f64)"""
    dt = np.float32 if storage == F32 else np.float64
    p = nb.to_storage(points, storage).astype(dt)
    n = len(p)
    r2 = dt(float(eps) * float(eps))
    rows, cols, vals = [], [], []
    if n:
        tx, ty, tz = (np.ascontiguousarray(p[:, a]) for a in range(3))
        for b0 in range(0, n, block):
            b1 = min(n, b0 + block)
            with np.errstate(invalid="ignore", over="ignore"):
                dx = tx[None, :] - p[b0:b1, 0:1]
                dy = ty[None, :] - p[b0:b1, 1:2]
                dz = tz[None, :] - p[b0:b1, 2:3]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == dt
                ok = np.isfinite(d2) & (d2 < r2)
            r, c = np.nonzero(ok)  # (row-major: columns ascending within a row)
            rows.append(r + b0)
            cols.append(c)
            vals.append(d2[r, c].astype(np.float64))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0)
    a = scipy.sparse.csr_matrix((np.ones(len(rows), bool), (rows, cols)), shape=(n, n))
    return a, vals


class Clustering(NamedTuple):
    labels: np.ndarray   # (n,) int32
    n_clusters: int
    sizes: np.ndarray    # (n_clusters,) uint32: every point labelled c, core and border
    core: np.ndarray     # (n,) bool
    degree: np.ndarray   # (n,) |N_i|


def _finish(labels, n_clusters, core, degree) -> Clustering:
    labels = np.asarray(labels, dtype=np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=n_clusters).astype(np.uint32)
    return Clustering(labels, int(n_clusters), sizes, core, degree)


def closed_form(adj, min_points) -> Clustering:
    n = adj.shape[0]
    degree = np.diff(adj.indptr).astype(np.int64)
    core = degree >= int(min_points)
    labels = np.full(n, -1, np.int64)
    core_idx = np.flatnonzero(core)
    n_clusters = 0
    if len(core_idx):
        sub = adj[core_idx][:, core_idx]
        n_clusters, comp = scipy.sparse.csgraph.connected_components(sub, directed=False)
        _, first = np.unique(comp, return_index=True)   # position (in core order = index order) of each component's smallest core index
        rank = np.empty(n_clusters, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(n_clusters)
        labels[core_idx] = rank[comp]
    for i in np.flatnonzero(~core & (degree > 0)):
        nbrs = adj.indices[adj.indptr[i]:adj.indptr[i + 1]]
        ids = labels[nbrs[core[nbrs]]]
        if len(ids):
            labels[i] = ids.min()
    return _finish(labels, n_clusters, core, degree)


def sequential(adj, min_points) -> Clustering:
    """[O3D] v0.15.1 ClusterDBSCAN as a procedure: -2 undefined, -1 noise"""
    n = adj.shape[0]
    indptr, indices = adj.indptr, adj.indices
    degree = np.diff(indptr).astype(np.int64)
    labels = np.full(n, -2, np.int64)
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if degree[idx] < min_points:
            labels[idx] = -1
            continue
        todo = collections.deque(indices[indptr[idx]:indptr[idx + 1]].tolist())
        seen = set(todo)
        seen.add(idx)
        labels[idx] = cluster
        while todo:
            q = todo.popleft()
            if labels[q] == -1:
                labels[q] = cluster
            if labels[q] != -2:
                continue
            labels[q] = cluster
            if degree[q] >= min_points:
                for w in indices[indptr[q]:indptr[q + 1]].tolist():
                    if w not in seen:
                        seen.add(w)
                        todo.append(w)
        cluster += 1
    return _finish(labels, cluster, degree >= int(min_points), degree)


def discriminating(adj, c: Clustering) -> np.ndarray:
    """the border points whose lowest-index core neighbour lies in another cluster than the one they are given"""
    out = []
    for i in np.flatnonzero(~c.core & (c.labels >= 0)):
        nbrs = adj.indices[adj.indptr[i]:adj.indptr[i + 1]]
        cores = nbrs[c.core[nbrs]]
        if c.labels[cores[0]] != c.labels[i]:
            out.append(i)
    return np.asarray(out, dtype=np.int64)


def keep_mask(c: Clustering, min_cluster_size) -> np.ndarray:
    big = c.sizes >= int(min_cluster_size)
    return (c.labels >= 0) & big[np.maximum(c.labels, 0)] if c.n_clusters else np.zeros(len(c.labels), bool)


# ---------------------------------------------------------------------------------------------------------------- clouds
_frozen = nb._frozen
STEP = 0.09   # spacing of the chains; eps = 0.1 reaches the next point and not the one after


def _spiral(n, r0=2.0, arm=0.5):
    """n points STEP of arc apart along r = r0 + arm * theta / (2 pi): 370 m of line for n = 4096 on 14 x 14 m, the arms 0.5 m apart"""
    b = arm / (2.0 * np.pi)
    th = np.zeros(n)
    for k in range(1, n):
        r = r0 + b * th[k - 1]
        th[k] = th[k - 1] + STEP / np.sqrt(r * r + b * b)
    r = r0 + b * th
    return np.column_stack([r * np.cos(th), r * np.sin(th), 1.0 + 0.001 * np.arange(n) / n])


@functools.lru_cache(maxsize=None)
def chain() -> np.ndarray:
    """4096 points 0.09 m apart along a gently bent line (a spiral, so that a fine grid over it stays small), in order along the line"""
    return _frozen(_spiral(4096))


@functools.lru_cache(maxsize=None)
def chain_shuffled() -> np.ndarray:
    return _frozen(chain()[np.random.default_rng(81).permutation(4096)])


@functools.lru_cache(maxsize=None)
def chain_gap() -> np.ndarray:
    """the chain without two points next to each other: a gap of 0.27 m"""
    return _frozen(np.delete(chain(), [2000, 2001], axis=0))


@functools.lru_cache(maxsize=None)
def chain_gap_shuffled() -> np.ndarray:
    return _frozen(chain_gap()[np.random.default_rng(82).permutation(4094)])


@functools.lru_cache(maxsize=None)
def ring() -> np.ndarray:
    """2048 points on a circle whose chord between neighbours is 0.09 m, shuffled"""
    n = 2048
    r = STEP / (2.0 * np.sin(np.pi / n))
    a = 2.0 * np.pi * np.arange(n) / n
    return _frozen(np.column_stack([r * np.cos(a) + 3.0, r * np.sin(a) - 2.0, np.full(n, 0.5)])[np.random.default_rng(83).permutation(n)])


@functools.lru_cache(maxsize=None)
def bridge() -> np.ndarray:
    """27 points: two tight blobs of 12 at x = 0 (A) and x = 0.3 (B), an arm point at 0.09 (of A) and at 0.21 (of B), a bridge point at
    0.15 within eps of both arms and of no blob; index order [A0, arm_B, bridge, B..., arm_A, A1...]"""
    rng = np.random.default_rng(84)
    a = rng.uniform(-0.004, 0.004, (12, 3))
    b = rng.uniform(-0.004, 0.004, (12, 3)) + [0.3, 0.0, 0.0]
    arm_a, arm_b, mid = [0.09, 0.0, 0.0], [0.21, 0.0, 0.0], [0.15, 0.0, 0.0]
    return _frozen(np.vstack([a[:1], [arm_b], [mid], b, [arm_a], a[1:]]) + [1.0, 2.0, 3.0])


@functools.lru_cache(maxsize=None)
def dense_blobs() -> np.ndarray:
    """1500 points: three Gaussian blobs of 450 (sigma 0.25 m) 2.5 m apart and 150 points scattered over the box, shuffled"""
    rng = np.random.default_rng(85)
    centres = np.array([[0.0, 0.0, 0.0], [2.5, 0.0, 0.0], [0.0, 2.5, 0.5]])
    blobs = [rng.normal(0.0, 0.25, (450, 3)) + c for c in centres]
    far = rng.uniform(-1.5, 4.0, (150, 3))
    return _frozen(np.vstack(blobs + [far])[rng.permutation(1500)])


@functools.lru_cache(maxsize=None)
def duplicates() -> np.ndarray:
    """40 sites, 50 identical points on each, shuffled"""
    rng = np.random.default_rng(86)
    sites = rng.uniform(0.0, 10.0, (40, 3))
    return _frozen(np.repeat(sites, 50, axis=0)[rng.permutation(2000)])


@functools.lru_cache(maxsize=None)
def pairs() -> np.ndarray:
    """4096 pairs 0.25 m apart on a 64 x 64 grid of 2 m, shuffled: 8192 points, 4096 roots (the rank scan crosses its blocks)"""
    g = np.stack(np.meshgrid(2.0 * np.arange(64), 2.0 * np.arange(64), indexing="ij"), -1).reshape(-1, 2)
    base = np.column_stack([g, np.zeros(len(g))])
    return _frozen(np.vstack([base, base + [0.0, 0.25, 0.0]])[np.random.default_rng(87).permutation(8192)])


@functools.lru_cache(maxsize=None)
def inf_cloud() -> np.ndarray:
    t = np.array(nr.ragged_cloud()[:100])
    t[17, 1] = np.inf
    return _frozen(t)


LATTICE_STEP = 1.0                                                    # of neighbor_restatement.integer_lattice
STEP_PLUS_ULP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))  # one f32 ulp above it


class Case(NamedTuple):
    name: str
    cloud: object      # () -> (n, 3)
    params: tuple      # ((eps, min_points), ...)


def _prefix(cloud, n):
    return lambda: cloud()[:n]


CASES = tuple([Case(f"tiny-{n}", _prefix(nr.ragged_cloud, n), ((1.0, 1), (1.0, 2))) for n in (0, 1, 2, 63, 64, 65, 257)] + [
    Case("chain", chain, ((0.1, 3),)),
    Case("chain-shuffled", chain_shuffled, ((0.1, 3),)),
    Case("chain-gap", chain_gap, ((0.1, 3),)),
    Case("chain-gap-shuffled", chain_gap_shuffled, ((0.1, 3),)),
    Case("ring", ring, ((0.1, 3),)),
    Case("bridge", bridge, ((0.1, 10),)),
    Case("scan", nb.scan_with_outliers, ((0.5, 5), (0.3, 10))),
    Case("dense-blobs", dense_blobs, ((0.4, 150),)),
    Case("lattice", nb.integer_lattice, ((LATTICE_STEP, 1), (LATTICE_STEP, 2), (STEP_PLUS_ULP, 7))),
    Case("duplicates", duplicates, ((0.05, 50),)),
    Case("pairs", pairs, ((0.5, 2),)),
    Case("non-finite", nb.nan_target, ((1.0, 3), (0.5, 1))),
])
MIN_CLUSTER_SIZES = (1, 2, 51, 1000)  # of the filter, on every case: the noise only; singletons; the duplicates' 50; most clusters


def case(name) -> Case:
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def _adjacency(name: str, eps: float, storage: str):
    return adjacency(case(name).cloud(), eps, storage)


@functools.lru_cache(maxsize=None)
def reference(name: str, eps: float, min_points: int, storage: str) -> Clustering:
    """the restated clustering of a case of CASES, computed once per process and never written to"""
    c = closed_form(_adjacency(name, eps, storage)[0], min_points)
    for a in (c.labels, c.sizes, c.core, c.degree):
        a.setflags(write=False)
    return c
