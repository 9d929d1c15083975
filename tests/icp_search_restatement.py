"""The correspondence search of the ICP passes ("exact 1-NN within radius", icp_kernels.hpp) and the step record built from its matches
(o3ds_backend.h), restated as brute force in numpy: the checker of o3ds_icp_nn_keys / o3ds_icp_accumulate and of everything that rests on
the same device routine.  Nothing here calls the oracle's k-d tree or the device.

What the kernel is specified to compute, and what this file therefore does:
  * source and target are rounded to the storage type (f32 or f64) when they are uploaded;
  * p = T s in f64 (rigid 4x4), q = storage(p) is the query;
  * the match of a query is the target point t (of the ones a crop keeps) with the smallest d2 = |t - q|^2, if d2 < storage(r^2),
    strictly; equal d2 go to the smaller original index.  d2 is formed here in f64 from the coordinate differences, over ALL pairs;
  * the record of a pass sums, over the matched queries, the terms of o3ds_backend.h -- from the UNROUNDED p and the stored target
    point and normal, as write_record does.  The sums are math.fsum (correctly rounded), so the record carries the rounding of its
    addends only; `record` also returns the sum of |addends| per term, the scale a comparison is held against.

The second half builds the inputs the search tests share (tests/test_icp_search_restatement_cpu.py proves them against the oracle and
asserts their premises, tests/test_icp_search_exact_gpu.py runs them on the device): exact-arithmetic lattices, the radius itself, seeded
clouds with a central void, queries outside the grid, thin and tiny targets, a radius beyond 64 cells.
"""
from __future__ import annotations

import functools
import math
import sys
from typing import NamedTuple

import numpy as np

NO_KEY = 0x7FFFFFFFFFFFFFFF
F32, F64 = "f32", "f64"
STORAGES = (F32, F64)
METHOD_POINT_TO_PLANE, METHOD_GENERALIZED, METHOD_POINT_TO_POINT = 0, 1, 2  # o3ds_icp_method
GICP_EPSILON = 1e-3  # [O3D] TransformationEstimationForGeneralizedICP's default, and the handle's
LD = np.longdouble   # 64-bit mantissa on x86-64: the extended precision of the generalized record


def to_storage(a, storage) -> np.ndarray:
    """the values as the device holds them, widened back to f64"""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if storage == F32 else a.copy()


def r2_storage(r, storage) -> float:
    r2 = float(r) * float(r)
    return float(np.float32(r2)) if storage == F32 else r2


def transform(T, s) -> np.ndarray:
    """[O3D] PointCloud::Transform for a rigid pose: p = R s + t, f64"""
    T = np.asarray(T, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    return (T[0:3, 0] * s[:, 0:1] + T[0:3, 1] * s[:, 1:2]) + T[0:3, 2] * s[:, 2:3] + T[0:3, 3]


class Matches(NamedTuple):
    idx: np.ndarray     # winning original target index per query, -1 = nothing within r
    d2: np.ndarray      # f64 squared distance storage(p) -> winner (inf where idx == -1)
    gap: np.ndarray     # d2 of the runner-up (a point other than the winner, ties included) minus d2 of the best; inf if there is none
    best: np.ndarray    # d2 of the nearest kept point whether or not it lies within r (inf: no kept point, or a non-finite query)
    p: np.ndarray       # T s, unrounded
    q: np.ndarray       # storage(p)


def nearest_within(src, tgt, T, r, storage, keep=None, chunk=64) -> Matches:
    s = to_storage(np.asarray(src, dtype=np.float64).reshape(-1, 3), storage)
    t = to_storage(np.asarray(tgt, dtype=np.float64).reshape(-1, 3), storage)
    with np.errstate(invalid="ignore", over="ignore"):
        p = transform(T, s)
        q = to_storage(p, storage)
    r2 = r2_storage(r, storage)
    n, nt = len(q), len(t)
    kept = np.ones(nt, dtype=bool)
    if keep is not None:
        kept[:] = False
        kept[np.asarray(keep, dtype=np.int64)] = True
    idx = np.full(n, -1, dtype=np.int64)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    for a in range(0, n, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = t[None, :, :] - q[a:a + chunk, None, :]
            d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
        d2[~np.isfinite(d2)] = np.inf  # a NaN / inf query is farther than r from everything
        d2[:, ~kept] = np.inf
        if nt == 0:
            continue
        k = np.argmin(d2, axis=1)  # the first minimum: the smaller original index
        rows = np.arange(len(k))
        b = d2[rows, k]
        best[a:a + chunk] = b
        if nt > 1:
            d2[rows, k] = np.inf
            second[a:a + chunk] = d2.min(axis=1)
        idx[a:a + chunk] = np.where(b < r2, k, -1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), second - best, np.inf)
    return Matches(idx, np.where(idx >= 0, best, np.inf), gap, best, p, q)


PIVOT_STEP = 1024.0


def record_pivot(x) -> np.ndarray:
    """o3ds_backend.h, the point-to-point record: per axis the multiple of 1024 m nearest to x (rint), 0 where x is not finite or beyond
    2^30 m.  Zero for every point within 512 m of the origin."""
    with np.errstate(invalid="ignore"):
        k = np.rint(np.asarray(x, dtype=np.float64) / PIVOT_STEP)
        return np.where(np.abs(k) < 2.0 ** 20, k * PIVOT_STEP, 0.0)


def record(p, tgt, nrm, idx, storage, method=METHOD_POINT_TO_PLANE, src_nrm=None, T=None, eps=GICP_EPSILON):
    """(record[32], scale[32]): the step record of o3ds_backend.h over the matches idx (-1 = none) of the transformed, unrounded source
    points p, and per term the sum of |addends|.  Point-to-plane: [0..20] upper triangle of JtJ row-major, [21..26] Jtr, [27] sum r^2,
    [28] count, [29] sum d^2, J = [p x n ; n], r = (p - t) . n.  Point-to-point: [0..8] sum t_a p_b row-major, [9..11] sum p,
    [12..14] sum t, [28], [29], with p and t taken relative to the pivot of the pass (record_pivot of p[0]: p is the WHOLE transformed
    source, so p[0] is the pose applied to point 0 of the source cloud); d^2 is of the points themselves.  Generalized (needs src_nrm and the pose T): record_gicp, whose scale is its own."""
    if method == METHOD_GENERALIZED:
        return record_gicp(p, tgt, nrm, src_nrm, idx, T, eps, storage)
    t_all = to_storage(np.asarray(tgt, dtype=np.float64).reshape(-1, 3), storage)
    m = np.flatnonzero(np.asarray(idx) >= 0)
    P = np.asarray(p, dtype=np.float64)[m]
    Q = t_all[np.asarray(idx)[m]]
    D = P - Q
    d2 = D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2]
    terms = [None] * 32
    if method == METHOD_POINT_TO_POINT:
        c = record_pivot(np.asarray(p, dtype=np.float64)[0])
        P, Q = P - c, Q - c  # (one subtraction, as the device's fma(-c, 1, slot): exact for a point nearer to c than to the origin)
        for a in range(3):
            for b in range(3):
                terms[3 * a + b] = Q[:, a] * P[:, b]
        for a in range(3):
            terms[9 + a] = P[:, a]
            terms[12 + a] = Q[:, a]
    else:
        N = to_storage(np.asarray(nrm, dtype=np.float64).reshape(-1, 3), storage)[np.asarray(idx)[m]]
        J = np.empty((len(m), 6))
        J[:, 0] = P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1]
        J[:, 1] = P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2]
        J[:, 2] = P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]
        J[:, 3:6] = N
        res = D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1] + D[:, 2] * N[:, 2]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                terms[k] = J[:, a] * J[:, b]
                k += 1
        for a in range(6):
            terms[21 + a] = J[:, a] * res
        terms[27] = res * res
    terms[28] = np.ones(len(m))
    terms[29] = d2
    rec, scale = np.zeros(32), np.zeros(32)
    for k, v in enumerate(terms):
        if v is not None:
            rec[k] = math.fsum(v.tolist())
            scale[k] = math.fsum(np.abs(v).tolist())
    return rec, scale


# ---- the generalized estimator ([O3D] TransformationEstimationForGeneralizedICP), per matched pair, in extended precision
FORM_O3D, FORM_CLOSED = "o3d", "closed"


def _skew(v):
    """[v]x of n vectors: (n, 3) -> (n, 3, 3)"""
    K = np.zeros((len(v), 3, 3), dtype=v.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    return K


def rotation_from_e1(x):
    """[O3D] GetRotationFromE1ToX of n stored vectors (n, 3): v = e1 x X, c = e1 . X; the identity if c < -0.99 (decided on the value as
    it is stored), else I + [v]x + [v]x^2 / (1 + c).  The zero vector has c = 0 and v = 0: the identity, by the formula."""
    x = np.asarray(x, dtype=LD)
    v = np.zeros_like(x)
    v[:, 1], v[:, 2] = -x[:, 2], x[:, 1]
    K = _skew(v)
    special = x[:, 0] < -0.99
    f = LD(1) / np.where(special, LD(1), LD(1) + x[:, 0])
    Rx = np.eye(3, dtype=LD) + K + np.matmul(K, K) * f[:, None, None]
    Rx[special] = np.eye(3, dtype=LD)
    return Rx


def covariance_from_normals(x, eps):
    """[O3D] the covariance the generalized estimator gives a point with (stored) normal x: Rx diag(eps, 1, 1) Rx^T, (n, 3, 3)"""
    Rx = rotation_from_e1(x)
    return np.matmul(Rx * np.array([LD(eps), LD(1), LD(1)]), np.transpose(Rx, (0, 2, 1)))


def _inverse3(M):
    """inverses of n symmetric 3x3 matrices in extended precision: adjugate over determinant, then one Newton step B + B (I - M B)"""
    c = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            c[:, j, i] = (-1) ** (i + j) * (M[:, a[0], b[0]] * M[:, a[1], b[1]] - M[:, a[0], b[1]] * M[:, a[1], b[0]])
    det = M[:, 0, 0] * c[:, 0, 0] + M[:, 0, 1] * c[:, 1, 0] + M[:, 0, 2] * c[:, 2, 0]
    B = c / det[:, None, None]
    return B + np.matmul(B, np.eye(3, dtype=LD) - np.matmul(M, B))


def gicp_pairs(tgt_nrm, src_nrm, idx, T, eps, storage, form=FORM_O3D, zero_is_e1=True):
    """(m, B, w) of the matched pairs i -> idx[i] (m: their query indices): B = M^-1 (n, 3, 3) in extended precision and w = |B|_2 =
    1 / lambda_min(M).
      FORM_O3D     M = C(nt) + R C(ns) R^T with the covariances of covariance_from_normals, from the UNROTATED stored normals; R is the
                   3x3 block of the pose as it is.
      FORM_CLOSED  what the device documents (icp_kernels.hpp above gicp_record) for unit normals: M = 2I - k (a a^T + b b^T), k = 1 - eps
                   in f64, b = nt and a = R ns, where a stored normal with x < -0.99 -- and, with zero_is_e1, the zero vector -- counts as e1
                   (on the source side before the rotation)."""
    idx = np.asarray(idx)
    m = np.flatnonzero(idx >= 0)
    nt = to_storage(np.asarray(tgt_nrm, dtype=np.float64).reshape(-1, 3), storage)[idx[m]].astype(LD)
    ns = to_storage(np.asarray(src_nrm, dtype=np.float64).reshape(-1, 3), storage)[m].astype(LD)
    R = np.asarray(T, dtype=np.float64)[:3, :3].astype(LD)
    if form == FORM_O3D:
        M = covariance_from_normals(nt, eps) + np.matmul(np.matmul(R, covariance_from_normals(ns, eps)), R.T)
    else:
        def as_e1(x):
            x = x.copy()
            fire = x[:, 0] < -0.99
            if zero_is_e1:
                fire |= (x == 0).all(axis=1)
            x[fire] = np.array([1, 0, 0], dtype=LD)
            return x
        a, b = np.matmul(as_e1(ns), R.T), as_e1(nt)
        k = LD(1.0 - float(eps))
        M = 2 * np.eye(3, dtype=LD) - k * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])
    if len(m) == 0:
        return m, M, np.zeros(0)
    return m, _inverse3(M), 1.0 / np.linalg.eigvalsh(M.astype(np.float64))[:, 0]


def gicp_defect(tgt_nrm, src_nrm, idx, T, eps, storage, zero_is_e1=True) -> float:
    """the largest |B_closed - B_o3d| (entry-wise) over |B|_2 of a pair: how far the closed form stands from Open3D's own form on these
    stored normals (unit only to the storage's rounding) -- a term of the record built from one form differs from the other's by at most
    this times its scale.  One reference against the other; no device in it."""
    _, Bo, w = gicp_pairs(tgt_nrm, src_nrm, idx, T, eps, storage, FORM_O3D)
    _, Bc, _ = gicp_pairs(tgt_nrm, src_nrm, idx, T, eps, storage, FORM_CLOSED, zero_is_e1)
    if len(w) == 0:
        return 0.0
    return float((np.abs(Bc - Bo).max(axis=(1, 2)).astype(np.float64) / w).max())


def record_gicp(p, tgt, tgt_nrm, src_nrm, idx, T, eps, storage, form=FORM_O3D, zero_is_e1=True):
    """(record[32], scale[32]) of the generalized estimator over the matches idx of the transformed, unrounded source points p: per pair
    B = M^-1 (gicp_pairs), A = [-[p]x | I], d = p - q with q the stored target point; [0..20] upper triangle of sum A^T B A row-major,
    [21..26] sum A^T B d, [27] sum d^T B d, [28] count, [29] sum |d|^2.  The addends are formed in extended precision, rounded to f64 once
    and summed exactly.  Scale: with w = |B|_2, alpha_a = |column a of A|_1 (1 for a >= 3) and delta = |d|_1 of the pair,
    scale[(a, b)] = sum w alpha_a alpha_b, scale[21 + a] = sum w alpha_a delta, scale[27] = sum w delta^2 -- the device's inverse is
    accurate relative to |B|, not entry by entry, so the sum of |addends| would be too tight where B is 0.5 beside entries of 500."""
    m, B, w = gicp_pairs(tgt_nrm, src_nrm, idx, T, eps, storage, form, zero_is_e1)
    t_all = to_storage(np.asarray(tgt, dtype=np.float64).reshape(-1, 3), storage)
    P = np.asarray(p, dtype=np.float64)[m].astype(LD)
    D = P - t_all[np.asarray(idx)[m]].astype(LD)
    A = np.zeros((len(m), 3, 6), dtype=LD)
    A[:, :, :3] = -_skew(P)
    A[:, :, 3:] = np.eye(3, dtype=LD)
    BA = np.matmul(B, A)
    H = np.matmul(np.transpose(A, (0, 2, 1)), BA)                      # A^T B A
    g = np.matmul(np.transpose(BA, (0, 2, 1)), D[:, :, None])[:, :, 0]  # A^T B d  (B symmetric)
    e = (D[:, None, :] @ np.matmul(B, D[:, :, None]))[:, 0, 0]          # d^T B d
    alpha = np.abs(A).sum(axis=1).astype(np.float64)
    delta = np.abs(D).sum(axis=1).astype(np.float64)
    terms, scales = [None] * 32, [None] * 32
    k = 0
    for a in range(6):
        for b in range(a, 6):
            terms[k], scales[k] = H[:, a, b], w * alpha[:, a] * alpha[:, b]
            k += 1
    for a in range(6):
        terms[21 + a], scales[21 + a] = g[:, a], w * alpha[:, a] * delta
    terms[27], scales[27] = e, w * delta * delta
    terms[28] = scales[28] = np.ones(len(m))
    terms[29] = scales[29] = (D * D).sum(axis=1)
    rec, scale = np.zeros(32), np.zeros(32)
    for k in range(30):
        rec[k] = math.fsum(np.asarray(terms[k]).astype(np.float64).tolist())
        scale[k] = math.fsum(np.abs(np.asarray(scales[k]).astype(np.float64)).tolist())
    return rec, scale


def jtj_from_record(rec):
    """(JtJ 6x6, Jtr 6, sum r^2) of a point-to-plane (or generalized) record"""
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = rec[k]
            k += 1
    return A, np.asarray(rec[21:27]).copy(), float(rec[27])


def information(tgt, idx, storage) -> np.ndarray:
    """[O3D] GetInformationMatrixFromPointClouds over the matches: sum of G^T G, G = [-[t]x | I], t the matched target point"""
    t = to_storage(np.asarray(tgt, dtype=np.float64).reshape(-1, 3), storage)[np.asarray(idx)[np.asarray(idx) >= 0]]
    out = np.zeros((6, 6))
    for x, y, z in t:
        G = np.zeros((3, 6))
        G[0, 1], G[0, 2], G[1, 0], G[1, 2], G[2, 0], G[2, 1] = z, -y, -z, x, y, -x
        G[:, 3:] = np.eye(3)
        out += G.T @ G
    return out


# ---- keys (o3ds_icp_nn_keys): float bits of d2 << 32 | rank << 28 | position in the shard's index; NO_KEY = nothing within r
def decode_keys(keys):
    """(none mask, d2 as float32, rank, position) of an int64 / uint64 key array"""
    k = np.asarray(keys).astype(np.uint64)
    none = k == np.uint64(NO_KEY)
    d2 = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    rank = ((k >> np.uint64(28)) & np.uint64(0xF)).astype(np.int64)
    pos = (k & np.uint64(0x0FFFFFFF)).astype(np.int64)
    return none, d2, rank, pos


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


D2_F32_REL = 8.0 * 2.0 ** -24  # see tests/icp_search_harness.py


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    src: np.ndarray
    tgt: np.ndarray
    nrm: np.ndarray
    r: float
    cell: float
    T: np.ndarray
    exact: bool        # coordinates, pose and radius are such that every operation is exact in both storages: float bits must be equal
    storages: tuple = STORAGES


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def rigid(rpy_deg, t):
    a, b, c = np.deg2rad(rpy_deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


VOID_CENTRE = np.array([3.0, 3.0, 3.0])
VOID_SEEDS = {0.0: 7, 0.3: 11, 0.6: 2026, 0.9: 7}
VOID_QUERY_RADIUS = 0.12  # every query's nearest neighbour is about the void's radius away: a whole workgroup is served by one stage
VOID_QUERY_RADIUS_MIXED = 0.45


def void_cloud(void_radius, n_tgt=20_000, n_src=300, seed=None, query_radius=None):
    """(src, tgt, nrm): n_tgt targets uniform in the 6 m box [0, 6]^3 outside the ball of void_radius around its centre, random unit
    normals, n_src queries uniform in the ball of query_radius around the centre (default: VOID_QUERY_RADIUS around a void, the wider
    VOID_QUERY_RADIUS_MIXED in the cloud without one, where it spreads the nearest distances from millimetres to a cell).  Seeded: the
    same arrays at every call (the target does not depend on query_radius)."""
    if query_radius is None:
        query_radius = VOID_QUERY_RADIUS if void_radius > 0.0 else VOID_QUERY_RADIUS_MIXED
    rng = np.random.default_rng(VOID_SEEDS[void_radius] if seed is None else seed)
    tgt = np.empty((0, 3))
    while len(tgt) < n_tgt:
        c = rng.uniform(0.0, 6.0, size=(n_tgt, 3))
        tgt = np.concatenate([tgt, c[np.linalg.norm(c - VOID_CENTRE, axis=1) >= void_radius]])
    tgt = tgt[:n_tgt]
    nrm = unit_normals(rng, n_tgt)
    v = rng.normal(size=(n_src, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    src = VOID_CENTRE + v * (query_radius * rng.uniform(0.0, 1.0, size=(n_src, 1)) ** (1.0 / 3.0))
    return src, tgt, nrm


# a. lattice: cell 0.25, targets at k * 0.25, k = 0..7 per axis, each twice with different normals
LATTICE_CELL = 0.25
LATTICE_COUNTS = (1, 127, 128, 129, 300)
LATTICE_SUBRANGE = (37, 150)


def lattice_case(n_src) -> Case:
    rng = np.random.default_rng(5)
    k = np.arange(8)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * LATTICE_CELL
    order = rng.permutation(len(g))
    tgt = np.concatenate([g[order], g[order[::-1]]])  # every point twice, the copies far apart in the array
    nrm = unit_normals(rng, len(tgt))
    on = g[rng.integers(0, len(g), size=60)]                                                   # lattice points
    base = rng.integers(0, 7, size=(240, 3)) * LATTICE_CELL
    half = LATTICE_CELL / 2
    edge = base[:60] + np.eye(3)[rng.integers(0, 3, size=60)] * half                                 # 2-way ties
    face = base[60:120] + (1.0 - np.eye(3)[rng.integers(0, 3, size=60)]) * half                      # 4-way ties
    body = base[120:180] + half                                                                   # 8-way ties
    f = base[180:240].astype(np.float32)  # one f32 ulp to either side of a cell face (exact in both storages)
    ax = rng.integers(0, 3, size=60)
    side = np.where(rng.integers(0, 2, size=60) == 1, np.float32(np.inf), np.float32(-np.inf))
    f[np.arange(60), ax] = np.nextafter(f[np.arange(60), ax], side)
    src = np.concatenate([on, edge, face, body, f.astype(np.float64)])
    src = src[rng.permutation(len(src))][:n_src]
    # r = 0.5: two cells; r^2 = 0.25 is exact
    return Case(f"lattice-{n_src}", src, tgt, nrm, 0.5, LATTICE_CELL, np.eye(4), True)


# b. the radius itself: a target at (3c, 4c, 0) from the query with r = 5c is NOT a match (strict); one ulp inward it is
def radius_cases():
    c = 0.25
    out = []
    for storage in STORAGES:
        one = np.float32 if storage == F32 else np.float64
        q = np.array([[1.0, 1.0, 1.0]])
        on = q + np.array([[3 * c, 4 * c, 0.0]])
        inward = on.copy()
        inward[0, 1] = float(np.nextafter(one(on[0, 1]), one(0.0)))
        far = np.array([[40.0, 40.0, 40.0]])  # keeps the grid more than one cell wide; out of anyone's reach
        for name, t in (("on", on), ("inward", inward)):
            tgt = np.concatenate([t, far])
            out.append(Case(f"radius-{name}-{storage}", q, tgt, unit_normals(np.random.default_rng(3), 2), 5 * c, c, np.eye(4), True, (storage,)))
    # the same under an exact translation carried by the pose
    base = out[0]
    out.append(Case("radius-on-translated", base.src - np.array([8.0, -4.0, 2.0]), base.tgt, base.nrm, base.r, c, _translation([8.0, -4.0, 2.0]), True))
    return out


# c. stage boundaries
STAGE_CELLS = (1.3, 0.5, 0.25, 0.1)
STAGE_VOIDS = (0.0, 0.3, 0.6, 0.9)


def stage_case(void_radius, cell, r=1.0) -> Case:
    """r = 1: the queries next to the centre; a smaller r: queries out to VOID_QUERY_RADIUS_MIXED, matches and misses in one workgroup"""
    src, tgt, nrm = void_cloud(void_radius, query_radius=None if r == 1.0 else VOID_QUERY_RADIUS_MIXED)
    return Case(f"void{void_radius}-cell{cell}-r{r}", src, tgt, nrm, r, cell, np.eye(4), False)


# d. outside the grid
def outside_case() -> Case:
    rng = np.random.default_rng(13)
    r = 1.0
    k = np.arange(5) * 0.5
    tgt = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)  # the box [0, 2]^3, a point every 0.5 m
    nrm = unit_normals(rng, len(tgt))
    src = []
    for f in (0.2, 0.9, 1.1, 3.0):
        for ax in range(3):
            for sgn in (-1.0, 1.0):  # beyond a face, above a lattice point of that face (the nearest target point is that one)
                p = np.array([1.0, 1.0, 1.0])
                p[ax] = (2.0 if sgn > 0 else 0.0) + sgn * f * r
                src.append(p)
        for corner in ((0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0)):  # beyond a corner along the diagonal
            c = np.array(corner, dtype=np.float64)
            src.append(2.0 * c + (2.0 * c - 1.0) * (f * r / math.sqrt(3.0)))
    src = np.array(src)
    src = src + rng.uniform(-1e-3, 1e-3, size=src.shape)  # off the exact boundaries: these are no exact-arithmetic inputs
    away = np.array([[1e4, 1.0, 1.0], [1.0, -1e4, 1.0], [1.0, 1.0, 1e4], [-1e4, 1e4, -1e4]])
    bad = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf]])
    return Case("outside", np.concatenate([src, away, bad]), tgt, nrm, r, 0.25, np.eye(4), False)


# e. thin and tiny
def tiny_cases():
    out = []
    rng = np.random.default_rng(17)
    for n in (1, 2, 63, 64, 65):
        tgt = rng.uniform(0.0, 2.0, size=(n, 3))
        src = np.concatenate([tgt[rng.integers(0, n, size=40)] + rng.normal(scale=0.2, size=(40, 3)), rng.uniform(-1.0, 3.0, size=(40, 3))])
        out.append(Case(f"tiny-{n}", src, tgt, unit_normals(rng, n), 1.0, 0.25, np.eye(4), False))
    tgt = 1.0 + rng.uniform(0.0, 0.2, size=(5000, 3))  # one cell of 0.25 holds them all
    src = 1.1 + rng.normal(scale=0.15, size=(140, 3))
    out.append(Case("one-cell-5000", src, tgt, unit_normals(rng, 5000), 1.0, 0.25, np.eye(4), False))
    for ax, name in ((0, "x"), (2, "z")):
        tgt = np.zeros((100, 3))
        tgt[:, ax] = rng.uniform(0.0, 8.0, size=100)
        src = np.zeros((150, 3))
        src[:, ax] = rng.uniform(-1.0, 9.0, size=150)
        src += rng.normal(scale=0.03, size=src.shape)  # (near the line: off it by much, every pair of neighbours nearly ties)
        out.append(Case(f"line-{name}", src, tgt, unit_normals(rng, 100), 1.0, 0.25, np.eye(4), False))
    return out


# f. a radius beyond 64 cells: cell 0.05, r = 5 (K = 100), two targets 200 cells apart on the x axis
def far_radius_case() -> Case:
    c = 0.05
    tgt = np.array([[0.0, 0.0, 0.0], [200 * c, 0.0, 0.0]])
    src = np.array([[70 * c, 0.0, 0.0],    # 70 cells from the first, 130 from the second: a match at 3.5 m
                    [63 * c, 0.0, 0.0],    # 63 cells: a match at 3.15 m
                    [-101 * c, 0.0, 0.0],  # 5.05 m from the first: beyond r
                    [130 * c, 0.0, 0.0]])  # 70 cells from the SECOND, on its other side
    src = src + np.array([[0.003, 0.011, 0.007]])  # inside the one row of cells, off the cell faces and off exact ties
    return Case("far-radius", src, tgt, unit_normals(np.random.default_rng(19), 2), 5.0, c, np.eye(4), False)


# g. crops: the arguments of make_crop (kinds: 1 max radius, 2 min radius, 3 min-max radius, 4 cylinder); every kind, and `invert`.  The
# first one excludes everything within 0.6 m of the centre of the void-0 cloud: the nearest points of every query fail the predicate and
# the true match lies stages away.  All run on the void-0 cloud with r = 1 and the default cell.
CROP_VOID = 0.0
CROPS = [dict(kind=2, center=tuple(VOID_CENTRE), rmin=0.6),
         dict(kind=1, center=(3.0, 3.0, 3.0), rmax=0.7),
         dict(kind=3, center=(3.2, 3.0, 2.9), rmin=0.3, rmax=0.8),
         dict(kind=4, center=(3.0, 3.1, 3.0), rmax=0.6, zmin=2.5, zmax=3.4),
         dict(kind=1, center=(3.0, 3.0, 3.0), rmax=0.5, invert=True),
         dict(kind=4, center=(3.0, 3.0, 3.0), rmax=0.4, zmin=2.7, zmax=3.3, invert=True),
         dict(kind=0, invert=True)]


# h. large coordinates: the shift is carried by the pose
def large_cases():
    src, tgt, nrm = void_cloud(0.6)
    s64 = np.array([1e5, -2e5, 50.0])
    s32 = np.array([2000.0, 2000.0, 2000.0])
    return [Case("large-f64", src, tgt + s64, nrm, 1.0, 0.25, _translation(s64), False, (F64,)),
            Case("large-f32", src, tgt + s32, nrm, 1.0, 0.25, _translation(s32), False, (F32,))]


# i. later passes: an init that is off by (0.4, -0.3, 0.1) m and 3 degrees
LATER_INIT = rigid((1.5, -2.0, 1.7), (0.4, -0.3, 0.1))  # |rotation| ~ 3 degrees


# j. the generalized estimator: per-point source normals (generators of their own: the arrays above do not depend on them), poses, epsilons
# and the edge values of the normals
SOURCE_NORMAL_SEED = 4  # (chosen so that the later passes' poses keep the gap premise: test_premises_of_the_generalized_later_passes)


def lattice_source_normals(n_src):
    return unit_normals(np.random.default_rng([SOURCE_NORMAL_SEED, 0]), 300)[:n_src]


def void_source_normals(void_radius, n_src=300):
    return unit_normals(np.random.default_rng([SOURCE_NORMAL_SEED, 1 + int(round(10 * void_radius))]), n_src)


def about(centre, T):
    """the rigid motion T carried out about `centre` instead of the origin (its translation added afterwards)"""
    out = np.array(T, dtype=np.float64)
    c = np.asarray(centre, dtype=np.float64)
    out[:3, 3] = c - out[:3, :3] @ c + out[:3, 3]
    return out


YAW170 = about(VOID_CENTRE, rigid((0.0, 0.0, 170.0), (0.03, -0.02, 0.04)))  # a 170 degree yaw about the void's centre plus a few centimetres
GICP_EPSILONS = (1.0, 1e-3, 1e-6)
X99 = -0.99
EDGE_X = (("x=-1", -1.0), ("x=-0.99", X99), ("x=-0.99-ulp", float(np.nextafter(X99, -1.0))), ("x=-0.99+ulp", float(np.nextafter(X99, 0.0))),
          ("x=f32(-0.99)", float(np.float32(X99))), ("x=+1", 1.0), ("zero", None))
EDGE_GROUP = 12       # matched pairs per group, at least
EDGE_DUPLICATES = 10


class GicpCase(NamedTuple):
    name: str
    src: np.ndarray
    src_nrm: np.ndarray
    tgt: np.ndarray
    nrm: np.ndarray
    r: float
    cell: float
    T: np.ndarray
    eps: float = GICP_EPSILON
    storages: tuple = STORAGES
    groups: tuple = ()     # (name, first query, count): contiguous query ranges with one kind of normal each (gicp_edge_case)
    n_plain: int = 0       # gicp_edge_case: the targets before the duplicates were appended


def _with_x(rng, x, n):
    """n vectors with first component x (exactly) and the rest on the circle that makes them unit"""
    if x is None:
        return np.zeros((n, 3))
    phi = rng.uniform(0.0, 2.0 * math.pi, size=n)
    s = math.sqrt(max(1.0 - x * x, 0.0))
    return np.stack([np.full(n, x), s * np.cos(phi), s * np.sin(phi)], axis=1)


def gicp_edge_case() -> GicpCase:
    """The void-0 cloud under YAW170, its normals overwritten in disjoint groups of at least EDGE_GROUP matched pairs.  Target side: the
    seven EDGE_X values on the matched target point (every query that matches such a point belongs to that group and keeps a random source
    normal).  Source side, on queries whose match keeps its random normal nt: the same seven values, ns = R^T nt (a = b), ns = -R^T nt,
    ns orthogonal to R^T nt, R ns = -e1 with a stored x > 0 (the special case must not fire after the rotation), stored ns = -e1 with
    (R ns).x > 0 (it must fire).  The queries are re-ordered so that every group is one contiguous range (`groups`); the rest stay
    random.  Ten matched target points outside the target-side groups are appended once more with other normals: the copy has the larger
    index and must lose."""
    src, tgt, nrm = void_cloud(0.0)
    rng = np.random.default_rng([SOURCE_NORMAL_SEED, 99])
    T, R = YAW170, YAW170[:3, :3]
    m = nearest_within(src, tgt, T, 1.0, F64)
    assert (m.idx >= 0).all()
    nrm = nrm.copy()
    free = np.ones(len(src), dtype=bool)   # queries not yet in a group
    order, groups = [], []

    def close_group(name, members):
        groups.append((name, len(order), len(members)))
        order.extend(int(i) for i in members)
        free[members] = False

    for name, x in EDGE_X:   # target side: whole targets, until the group holds EDGE_GROUP pairs
        members = []
        for i in np.flatnonzero(free):
            if len(members) >= EDGE_GROUP:
                break
            if not free[i]:
                continue
            same = np.flatnonzero(m.idx == m.idx[i])
            nrm[m.idx[i]] = _with_x(rng, x, 1)[0]
            members.extend(same.tolist())
            free[same] = False
        close_group("tgt " + name, np.array(members))
    touched = np.unique(m.idx[~free])
    src_nrm = void_source_normals(0.0).copy()
    rest = np.flatnonzero(free)
    k = 0

    def take():
        nonlocal k
        out = rest[k:k + EDGE_GROUP]
        k += EDGE_GROUP
        return out

    for name, x in EDGE_X:
        members = take()
        src_nrm[members] = _with_x(rng, x, len(members))
        close_group("src " + name, members)
    for name in ("a=b", "a=-b", "a orthogonal b"):
        members = take()
        back = nrm[m.idx[members]] @ R   # rows R^T nt
        if name == "a=-b":
            back = -back
        elif name != "a=b":
            o = np.cross(back, rng.normal(size=back.shape))
            back = o / np.linalg.norm(o, axis=1, keepdims=True)
        src_nrm[members] = back
        close_group("src " + name, members)
    members = take()
    src_nrm[members] = -R[0, :]                    # R^T (-e1): rotates onto -e1
    close_group("src rotates to -e1", members)
    members = take()
    src_nrm[members] = np.array([-1.0, 0.0, 0.0])  # R (-e1) has x = cos 10 deg
    close_group("src -e1 rotates away", members)
    order.extend(int(i) for i in rest[k:])
    order = np.array(order)
    assert len(order) == len(src) and len(np.unique(order)) == len(src)
    dup = np.setdiff1d(np.unique(m.idx), touched)[:EDGE_DUPLICATES]
    assert len(dup) == EDGE_DUPLICATES
    tgt2 = np.concatenate([tgt, tgt[dup]])
    nrm2 = np.concatenate([nrm, unit_normals(rng, EDGE_DUPLICATES)])
    return GicpCase("gicp-edge", src[order], src_nrm[order], tgt2, nrm2, 1.0, 0.25, T, groups=tuple(groups), n_plain=len(tgt))


def gicp_cases():
    """every input of the generalized-record tests that is a plain case (the crop, the later passes and the shards build theirs)"""
    out = []
    for n in LATTICE_COUNTS:
        c = lattice_case(n)
        out.append(GicpCase(c.name, c.src, lattice_source_normals(n), c.tgt, c.nrm, c.r, c.cell, c.T))
    for c, v in ((stage_case(0.0, 0.25), 0.0), (stage_case(0.9, 0.25), 0.9), (stage_case(0.9, 0.25, r=0.5), 0.9)):
        out.append(GicpCase(c.name, c.src, void_source_normals(v), c.tgt, c.nrm, c.r, c.cell, c.T))
    c = stage_case(0.0, 0.25)
    for name, T in (("later-init", LATER_INIT), ("yaw170", YAW170)):
        out.append(GicpCase(f"void0.0-pose-{name}", c.src, void_source_normals(0.0), c.tgt, c.nrm, c.r, c.cell, T))
    for eps in GICP_EPSILONS:
        if eps != GICP_EPSILON:
            out.append(GicpCase(f"void0.0-eps{eps:g}", c.src, void_source_normals(0.0), c.tgt, c.nrm, c.r, c.cell, c.T, eps))
    for c in large_cases():
        out.append(GicpCase(c.name, c.src, void_source_normals(0.6), c.tgt, c.nrm, c.r, c.cell, c.T, GICP_EPSILON, c.storages))
    out.append(gicp_edge_case())
    return out


def all_cases():
    """every input of the search tests that is a plain (src, tgt, T, r, cell) case"""
    out = [lattice_case(n) for n in LATTICE_COUNTS] + radius_cases()
    out += [stage_case(v, c) for v in STAGE_VOIDS for c in STAGE_CELLS] + [stage_case(0.9, 0.25, r=0.5)]
    out += [outside_case()] + tiny_cases() + [far_radius_case()] + large_cases()
    return out


# ---- the generalized cases by name, their brute-force matches and the DEFECT table: shared by tests/test_icp_search_restatement_cpu.py,
# which proves them, and tests/test_icp_search_exact_gpu.py, which runs them on the device (computed once per process, left unchanged)
rs = sys.modules[__name__]  # (the three helpers below name this module as their users do)
GICP_CASES = gicp_cases()
DEFECT = {}          # (case name, storage) -> rs.gicp_defect of the whole case, filled by defect()


@functools.lru_cache(maxsize=None)
def _gicp_case(name):
    return {c.name: c for c in GICP_CASES}[name]


@functools.lru_cache(maxsize=None)
def gicp_matches(name, storage):
    c = _gicp_case(name)
    return rs.nearest_within(c.src, c.tgt, c.T, c.r, storage)


def defect(name, storage) -> float:
    """DEFECT[name, storage], computed on first use"""
    if (name, storage) not in DEFECT:
        c = _gicp_case(name)
        DEFECT[name, storage] = rs.gicp_defect(c.nrm, c.src_nrm, gicp_matches(name, storage).idx, c.T, c.eps, storage)
    return DEFECT[name, storage]
