"""Coloured ICP ([O3D] RegistrationColoredICP, Open3D v0.15.1) restated in numpy from the text of include/o3ds_backend.h: the colour
gradients of a cloud, the record of one joint step, and the registration loop -- and the cases the CPU and GPU tests share.  Nothing
here uses a search structure or the device; the neighbour lists and the correspondences are neighbor_restatement.search, which also
does the storage rounding.

Arithmetic: f64 on the stored values widened, every operation on its own (numpy never fuses), in the header's order:
  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;  cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);
  intensity = ((r + g) + b) / 3.0.
Sums: the gradient's M and v row by row in list order onto +0.0; the record's terms over blocks of 256 queries, a halving tree inside a
block (v[t] = v[t] + v[t + s], s = 128 .. 1), the block sums in ascending order onto +0.0.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import icp_search_restatement as isr
import neighbor_restatement as nbr

F32, F64 = nbr.F32, nbr.F64
STORAGES = nbr.STORAGES
to_storage = nbr.to_storage
rigid = isr.rigid

LAMBDA_DEFAULT = 0.968  # [O3D] TransformationEstimationForColoredICP
GRADIENT_MAX_NN = 30    # [O3D] RegistrationColoredICP: KDTreeSearchParamHybrid(2 r, 30)
BLOCK = 256


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def intensity(colors, storage) -> np.ndarray:
    c = to_storage(colors, storage)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0


# ---------------------------------------------------------------------------------------------------------------- gradients
def gradient_rows(points, normals, colors, radius, max_nn, storage):
    """per point: the rows (a, b) of the header in list order, the last row included, and how many there are (0: fewer than 4 entries)"""
    P, N, I = to_storage(points, storage), to_storage(normals, storage), intensity(colors, storage)
    L = nbr.search(points, points, max_nn, radius, storage)
    n = len(P)
    A = np.zeros((n, max_nn, 3))
    B = np.zeros((n, max_nn))
    cnt = L.cnt.astype(np.int64)
    rows = np.where(cnt >= 4, cnt, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, max_nn):
            j = L.idx[:, k].astype(np.int64)
            q = P[j]
            e = dot(q - P, N)
            A[:, k - 1] = (q - e[:, None] * N) - P
            B[:, k - 1] = I[j] - I
        last = np.maximum(rows - 1, 0)
        for i in np.flatnonzero(rows):
            A[i, last[i]] = float(last[i]) * N[i]
            B[i, last[i]] = 0.0
    return A, B, rows


def gradients(points, normals, colors, radius, max_nn, storage) -> np.ndarray:
    A, B, rows = gradient_rows(points, normals, colors, radius, max_nn, storage)
    n = len(rows)
    M = np.zeros((n, 3, 3))
    v = np.zeros((n, 3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(max_nn):
            on = k < rows
            a, b = A[:, k], B[:, k]
            for r in range(3):
                for c in range(r + 1):
                    M[:, r, c] = np.where(on, M[:, r, c] + a[:, r] * a[:, c], M[:, r, c])
                v[:, r] = np.where(on, v[:, r] + a[:, r] * b, v[:, r])
        d0 = M[:, 0, 0]
        l10, l20 = M[:, 1, 0] / d0, M[:, 2, 0] / d0
        d1 = M[:, 1, 1] - l10 * M[:, 1, 0]
        w = M[:, 2, 1] - l20 * M[:, 1, 0]
        l21 = w / d1
        d2 = (M[:, 2, 2] - l20 * M[:, 2, 0]) - l21 * w
        y0 = v[:, 0]
        y1 = v[:, 1] - l10 * y0
        y2 = (v[:, 2] - l20 * y0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (y0 / d0 - l10 * x1) - l20 * x2
        ok = (rows > 0) & np.isfinite(d0) & (d0 > 0) & np.isfinite(d1) & (d1 > 0) & np.isfinite(d2) & (d2 > 0)
    return np.where(ok[:, None], np.stack([x0, x1, x2], axis=1), 0.0)


def gradients_lstsq(points, normals, colors, radius, max_nn, storage) -> np.ndarray:
    """the independent formulation: the least-squares solution of the same rows by np.linalg.lstsq (SVD), zero where there are no rows"""
    A, B, rows = gradient_rows(points, normals, colors, radius, max_nn, storage)
    out = np.zeros((len(rows), 3))
    for i in np.flatnonzero(rows):
        if np.isfinite(A[i, :rows[i]]).all() and np.isfinite(B[i, :rows[i]]).all():
            out[i] = np.linalg.lstsq(A[i, :rows[i]], B[i, :rows[i]], rcond=None)[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- the step
class Pairs(NamedTuple):
    have: np.ndarray  # (n,) bool
    JG: np.ndarray    # (n, 6)
    rG: np.ndarray
    JI: np.ndarray
    rI: np.ndarray
    d2: np.ndarray


def pairs(src, src_col, tgt, tgt_nrm, tgt_col, tgt_grad, T, r, lam, storage) -> Pairs:
    L = nbr.search(src, tgt, 1, r, storage, T=T)
    p = nbr.stored_queries(src, storage, T)
    have = L.cnt > 0
    j = L.idx[:, 0].astype(np.int64)
    q, n = to_storage(tgt, storage)[j], to_storage(tgt_nrm, storage)[j]
    g = np.asarray(tgt_grad, dtype=np.float64).reshape(-1, 3)[j]
    Is, It = intensity(src_col, storage), intensity(tgt_col, storage)[j]
    sg, sp = math.sqrt(lam), math.sqrt(1.0 - lam)
    with np.errstate(invalid="ignore", over="ignore"):
        dn = dot(p - q, n)
        JG = np.concatenate([sg * cross(p, n), sg * n], axis=1)
        rG = sg * dn
        pp = p - dn[:, None] * n
        I0 = dot(g, pp - q) + It
        gn = dot(g, n)
        gM = gn[:, None] * n - g
        JI = np.concatenate([sp * cross(p, gM), sp * gM], axis=1)
        rI = sp * (Is - I0)
    return Pairs(have, JG, rG, JI, rI, L.d2[:, 0])


def block_tree_sum(terms) -> np.ndarray:
    """(n, k) terms -> (k,) sums in the header's order"""
    terms = np.asarray(terms, dtype=np.float64)
    n, k = terms.shape
    nb = (n + BLOCK - 1) // BLOCK
    v = np.zeros((nb * BLOCK, k))
    v[:n] = terms
    v = v.reshape(nb, BLOCK, k)
    s = BLOCK // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while s >= 1:
            v[:, :s] = v[:, :s] + v[:, s:2 * s]
            s //= 2
        out = np.zeros(k)
        for b in range(nb):
            out = out + v[b, 0]
    return out


def record_from_pairs(P: Pairs) -> np.ndarray:
    n = len(P.have)
    t = np.zeros((n, 32))
    with np.errstate(invalid="ignore", over="ignore"):
        k = 0
        for r in range(6):
            for c in range(r, 6):
                t[:, k] = P.JG[:, r] * P.JG[:, c] + P.JI[:, r] * P.JI[:, c]
                k += 1
        for r in range(6):
            t[:, 21 + r] = P.JG[:, r] * P.rG + P.JI[:, r] * P.rI
        t[:, 27] = P.rG * P.rG + P.rI * P.rI
    t[:, 28] = 1.0
    t[:, 29] = P.d2
    t[~P.have] = 0.0
    return block_tree_sum(t)


def step_record(src, src_col, tgt, tgt_nrm, tgt_col, tgt_grad, T, r, lam, storage) -> np.ndarray:
    if len(np.asarray(src).reshape(-1, 3)) == 0:
        return np.zeros(32)
    return record_from_pairs(pairs(src, src_col, tgt, tgt_nrm, tgt_col, tgt_grad, T, r, lam, storage))


def geometric_record(src, tgt, tgt_nrm, T, r, storage) -> np.ndarray:
    """the pure point-to-plane record over the same correspondences, queries and sum order: J = [p x n ; n], res = (p - q) . n"""
    L = nbr.search(src, tgt, 1, r, storage, T=T)
    p = nbr.stored_queries(src, storage, T)
    j = L.idx[:, 0].astype(np.int64)
    q, n = to_storage(tgt, storage)[j], to_storage(tgt_nrm, storage)[j]
    J = np.concatenate([cross(p, n), n], axis=1)
    res = dot(p - q, n)
    t = np.zeros((len(p), 32))
    k = 0
    for r_ in range(6):
        for c in range(r_, 6):
            t[:, k] = J[:, r_] * J[:, c]
            k += 1
    for r_ in range(6):
        t[:, 21 + r_] = J[:, r_] * res
    t[:, 27] = res * res
    t[:, 28] = 1.0
    t[:, 29] = L.d2[:, 0]
    t[L.cnt == 0] = 0.0
    return block_tree_sum(t)


def record_dense_longdouble(P: Pairs):
    """the independent formulation: J^T J, J^T r and r^T r of the stacked 2m x 6 Jacobian in np.longdouble; (record[30], scale[30]) with
    scale the sum of |addends| per term"""
    LD = np.longdouble
    m = P.have
    J = np.concatenate([P.JG[m], P.JI[m]], axis=0).astype(LD)
    res = np.concatenate([P.rG[m], P.rI[m]]).astype(LD)
    JtJ, Jtr = J.T @ J, J.T @ res
    aJtJ, aJtr = np.abs(J).T @ np.abs(J), np.abs(J).T @ np.abs(res)
    iu = np.triu_indices(6)
    rec = np.concatenate([JtJ[iu], Jtr, [res @ res, LD(m.sum()), P.d2[m].astype(LD).sum()]])
    scale = np.concatenate([aJtJ[iu], aJtr, [res @ res, LD(m.sum()), P.d2[m].astype(LD).sum()]])
    return rec.astype(np.float64), scale.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the loop
def jtj_from_record(rec):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = rec[:21]
    return A + np.triu(A, 1).T


def vector6_to_matrix4(x):
    """[O3D] TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6]"""
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    U = np.eye(4)
    U[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:6]
    return U


def register(src, src_col, tgt, tgt_nrm, tgt_col, r, storage, init=None, lam=LAMBDA_DEFAULT, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
             tgt_grad=None) -> dict:
    """[O3D] RegistrationICP's loop around step_record, as the header states it; the target's gradients are those of (2 r, 30)"""
    if tgt_grad is None:
        tgt_grad = gradients(tgt, tgt_nrm, tgt_col, 2.0 * r, GRADIENT_MAX_NN, storage)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = len(np.asarray(src).reshape(-1, 3))
    fitness = rmse = 0.0
    iterations, converged, n_corr, passes = 0, False, 0, 0
    if n == 0:
        return dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, converged=False, n_corr=0)
    while True:
        rec = step_record(src, src_col, tgt, tgt_nrm, tgt_col, tgt_grad, T, r, lam, storage)
        count = rec[28]
        f = count / n if count > 0 else 0.0
        e = math.sqrt(rec[29] / count) if count > 0 else 0.0
        conv = passes > 0 and abs(fitness - f) < rel_fitness and abs(rmse - e) < rel_rmse
        fitness, rmse, n_corr = f, e, int(count + 0.5)
        passes += 1
        converged = converged or conv
        if conv or iterations >= max_iter:
            break
        x = np.linalg.solve(jtj_from_record(rec), -rec[21:27]) if count > 0 else np.zeros(6)
        T = vector6_to_matrix4(x) @ T
        iterations += 1
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged, n_corr=n_corr)


# ---------------------------------------------------------------------------------------------------------------- clouds
def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def texture(p) -> np.ndarray:
    """the grey value of the sliding case at a point of the scene, on all three channels"""
    p = np.asarray(p, dtype=np.float64)
    v = 0.5 + 0.2 * np.sin(2.0 * np.pi * p[:, 1]) + 0.1 * np.cos(2.0 * np.pi * (p[:, 0] + p[:, 2]) / 1.5)
    return np.repeat(v[:, None], 3, axis=1)


def texture_gradient(p) -> np.ndarray:
    p = np.asarray(p, dtype=np.float64)
    k = -0.1 * np.sin(2.0 * np.pi * (p[:, 0] + p[:, 2]) / 1.5) * (2.0 * np.pi / 1.5)
    return np.stack([k, 0.2 * np.cos(2.0 * np.pi * p[:, 1]) * 2.0 * np.pi, k], axis=1)


def draw_surfaces(rng, n_floor, n_wall):
    """(points, analytic normals): n_floor points uniform on [0, 4]^2 at z = 0, then n_wall points at x = 0 with y in [0, 4], z in [0, 2]"""
    f = rng.uniform(0.0, 4.0, (n_floor, 2))
    wy, wz = rng.uniform(0.0, 4.0, n_wall), rng.uniform(0.0, 2.0, n_wall)
    pts = np.vstack([np.column_stack([f, np.zeros(n_floor)]), np.column_stack([np.zeros(n_wall), wy, wz])])
    nrm = np.vstack([np.tile([0.0, 0.0, 1.0], (n_floor, 1)), np.tile([1.0, 0.0, 0.0], (n_wall, 1))])
    return pts, nrm


SLIDE_GT = rigid((0.0, 0.0, 0.5), (0.01, 0.05, -0.01))  # the pose the registration must find; 0.05 m of it slide along the edge
SLIDE = 0.05


class Scene(NamedTuple):
    tgt: np.ndarray
    tgt_nrm: np.ndarray
    tgt_col: np.ndarray
    src: np.ndarray
    src_col: np.ndarray


@functools.lru_cache(maxsize=None)
def sliding_scene() -> Scene:
    """floor and wall from default_rng(7): the target, then a second draw of the same surfaces moved by the inverse of SLIDE_GT"""
    rng = np.random.default_rng(7)
    tgt, nrm = draw_surfaces(rng, 1024, 1024)
    second, _ = draw_surfaces(rng, 1024, 1024)
    inv = np.linalg.inv(SLIDE_GT)
    src = second @ inv[:3, :3].T + inv[:3, 3]
    return Scene(_frozen(tgt), _frozen(nrm), _frozen(texture(tgt)), _frozen(src), _frozen(texture(second)))


def translation_error(T) -> float:
    return float(np.linalg.norm(np.asarray(T)[:3, 3] - SLIDE_GT[:3, 3]))


SLIDING_PARAMS = ((0.15, LAMBDA_DEFAULT), (0.3, 0.5))  # (r, lambda): the issue's setting and the one it says holds equally


@functools.lru_cache(maxsize=None)
def sliding_result(r, lam, storage, max_iter=10, rel=0.0) -> dict:
    s = sliding_scene()
    return register(s.src, s.src_col, s.tgt, s.tgt_nrm, s.tgt_col, r, storage, lam=lam, max_iter=max_iter, rel_fitness=rel, rel_rmse=rel)


CONVERGING = dict(r=0.15, lam=LAMBDA_DEFAULT, max_iter=60)  # the sliding case with Open3D's default thresholds (1e-6)


# ---- gradient cases
class GradCase(NamedTuple):
    name: str
    cloud: object  # () -> (points, normals, colours)
    radius: float
    max_nn: int


EDGE_RADIUS = 0.3
EDGE = dict(three=(0, 3), four=(3, 7), dense=(7, 57), duplicates=(57, 65), zero_normal=(65, 74), nan=(74, 83), line=(83, 89))


@functools.lru_cache(maxsize=None)
def edge_cloud():
    """clusters 5 m apart, each a patch of the plane z = const with normal (0, 0, 1) unless said otherwise, radius EDGE_RADIUS:
    three / four points (lists of exactly 3 and 4 entries); 50 points within 0.1 m (lists truncated at 30); four points each with an
    exact duplicate (for the copy with the higher index the skipped first entry is the other one); nine points, one with a zero normal;
    nine points, one of them with a NaN coordinate; six points on a line (a collinear neighbourhood)"""
    rng = np.random.default_rng(17)
    parts, normals = [], []

    def patch(k, m, half, origin):
        xy = rng.uniform(-half, half, (m, 2))
        parts.append(np.column_stack([xy + origin, np.full(m, 0.25 * k)]))
        normals.append(np.tile([0.0, 0.0, 1.0], (m, 1)))

    patch(0, 3, 0.1, (0.0, 0.0))
    patch(1, 4, 0.1, (5.0, 0.0))
    patch(2, 50, 0.07, (10.0, 0.0))
    patch(3, 4, 0.1, (15.0, 0.0))
    parts.append(parts[-1].copy())
    normals.append(normals[-1].copy())
    patch(4, 9, 0.1, (20.0, 0.0))
    normals[-1][4] = 0.0
    patch(5, 9, 0.1, (25.0, 0.0))
    parts[-1][2, 1] = np.nan
    parts.append(np.column_stack([30.0 + 0.04 * np.arange(6), np.zeros(6), np.full(6, 1.5)]))
    normals.append(np.tile([0.0, 0.0, 1.0], (6, 1)))
    pts, nrm = np.vstack(parts), np.vstack(normals)
    col = rng.uniform(0.0, 1.0, (len(pts), 3))
    assert len(pts) == EDGE["line"][1]
    return _frozen(pts), _frozen(nrm), _frozen(col)


def _scene_target():
    s = sliding_scene()
    return s.tgt, s.tgt_nrm, s.tgt_col


def _uniform_target():
    s = sliding_scene()
    return s.tgt, s.tgt_nrm, _frozen(np.full(s.tgt.shape, 0.375))


GRAD_CASES = (
    GradCase("scene", _scene_target, 0.3, GRADIENT_MAX_NN),
    GradCase("edges", edge_cloud, EDGE_RADIUS, GRADIENT_MAX_NN),
    GradCase("uniform", _uniform_target, 0.3, GRADIENT_MAX_NN),
)


@functools.lru_cache(maxsize=None)
def reference_gradients(name, storage) -> np.ndarray:
    c = next(g for g in GRAD_CASES if g.name == name)
    out = gradients(*c.cloud(), c.radius, c.max_nn, storage)
    out.setflags(write=False)
    return out


# ---- step cases: sources of n points drawn on the scene's surfaces, against the scene's target
STEP_R = 0.15
STEP_GRADIENT = (0.3, GRADIENT_MAX_NN)  # the target's gradients: those the registration at STEP_R would make
STEP_SIZES = (100, 256, 257, 2125)
NEAR_POSE = rigid((0.2, -0.3, 0.5), (0.01, 0.05, -0.01))
FAR_POSE = rigid((0.0, 0.0, 0.0), (100.0, 0.0, 0.0))  # leaves no correspondence
STEP_POSES = (("near", NEAR_POSE), ("identity", np.eye(4)))
STEP_LAMBDAS = (LAMBDA_DEFAULT, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def step_source(n):
    """(points, colours): n points of the scene's surfaces (half floor, half wall), a few centimetres off them, textured; every fifth one
    is lifted 0.6 m off its surface and finds no correspondence"""
    rng = np.random.default_rng(100 + n)
    pts, nrm = draw_surfaces(rng, (n + 1) // 2, n // 2)
    off = rng.normal(scale=0.02, size=pts.shape)
    off[3::5] = 0.6 * nrm[3::5]
    return _frozen(pts + off), _frozen(texture(pts))


@functools.lru_cache(maxsize=None)
def reference_step(n, pose_name, lam, storage, zero_gradients=False) -> np.ndarray:
    s = sliding_scene()
    T = dict(STEP_POSES + (("far", FAR_POSE),))[pose_name]
    src, col = step_source(n)
    if zero_gradients:
        tgt_col = _uniform_target()[2]
        grad = np.zeros(s.tgt.shape)
    else:
        tgt_col, grad = s.tgt_col, reference_gradients("scene", storage)
    out = step_record(src, col, s.tgt, s.tgt_nrm, tgt_col, grad, T, STEP_R, lam, storage)
    out.setflags(write=False)
    return out
