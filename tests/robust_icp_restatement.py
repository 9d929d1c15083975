"""Robust loss kernels ([O3D] RobustKernel, Open3D v0.15.1) on the point-to-plane and the coloured estimator, restated in numpy from the
text of include/o3ds_backend.h (o3ds_robust_icp_step, o3ds_icp_robust_dev) -- and the cases the CPU and GPU tests share.  Arithmetic,
correspondences, sum order and the loop are colored_icp_restatement's; what is new is the weight of a residual and where it multiplies.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import colored_icp_restatement as cr
import neighbor_restatement as nbr

F32, F64 = cr.F32, cr.F64
STORAGES = cr.STORAGES
to_storage = cr.to_storage

L2, L1, HUBER, CAUCHY, GM, TUKEY = range(6)  # o3ds_loss_kind
LOSS_NAMES = ("l2", "l1", "huber", "cauchy", "gm", "tukey")
POINT_TO_PLANE, COLORED = 0, 1               # o3ds_robust_estimator
ESTIMATORS = ((POINT_TO_PLANE, "point_to_plane"), (COLORED, "colored"))


# ---------------------------------------------------------------------------------------------------------------- the losses
def weight(kind, k, r) -> np.ndarray:
    """[O3D] <Loss>::Weight(r), every operation on its own, the comparisons as written (a NaN residual takes what they give)"""
    r = np.asarray(r, dtype=np.float64)
    e = np.abs(r)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if kind == L2:
            return np.ones_like(r)
        if kind == L1:
            return np.where(r == 0.0, 1.0, 1.0 / np.where(r == 0.0, 1.0, e))  # DEPARTURE: r == 0 gives 1
        if kind == HUBER:
            return np.where(e > k, k / e, 1.0)
        if kind == CAUCHY:
            u = r / k
            return 1.0 / (1.0 + u * u)
        if kind == GM:
            d = k + r * r
            return k / (d * d)
        if kind == TUKEY:
            q = e / k
            u = np.where(q < 1.0, q, 1.0)
            v = 1.0 - u * u
            return v * v
    raise ValueError(kind)


def rho(kind, k, r) -> np.ndarray:
    """the loss itself, in Open3D's forms (RobustKernel.h): Weight(r) r is its derivative"""
    r = np.asarray(r, dtype=np.float64)
    e = np.abs(r)
    if kind == L2:
        return r * r / 2.0
    if kind == L1:
        return e
    if kind == HUBER:
        return np.where(e <= k, r * r / 2.0, k * (e - k / 2.0))
    if kind == CAUCHY:
        return k * k / 2.0 * np.log(1.0 + (r / k) ** 2)
    if kind == GM:
        return (r * r / 2.0) / (k + r * r)
    if kind == TUKEY:
        return np.where(e <= k, k * k / 6.0 * (1.0 - (1.0 - (r / k) ** 2) ** 3), k * k / 6.0)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- the step
class PlanePairs(NamedTuple):
    have: np.ndarray  # (n,) bool
    J: np.ndarray     # (n, 6)
    r: np.ndarray
    d2: np.ndarray


def plane_pairs(src, tgt, tgt_nrm, T, r, storage) -> PlanePairs:
    """POINT_TO_PLANE: the search's pairs, J = (cross(p, n) ; n), r = dot(p - q, n)"""
    L = nbr.search(src, tgt, 1, r, storage, T=T)
    p = nbr.stored_queries(src, storage, T)
    j = L.idx[:, 0].astype(np.int64)
    q, n = to_storage(tgt, storage)[j], to_storage(tgt_nrm, storage)[j]
    with np.errstate(invalid="ignore", over="ignore"):
        return PlanePairs(L.cnt > 0, np.concatenate([cr.cross(p, n), n], axis=1), cr.dot(p - q, n), L.d2[:, 0])


def plane_terms(P: PlanePairs, kind, k) -> np.ndarray:
    t = np.zeros((len(P.have), 32))
    with np.errstate(invalid="ignore", over="ignore"):
        w = weight(kind, k, P.r)
        i = 0
        for r in range(6):
            for c in range(r, 6):
                t[:, i] = w * (P.J[:, r] * P.J[:, c])
                i += 1
        for r in range(6):
            t[:, 21 + r] = w * (P.J[:, r] * P.r)
        t[:, 27] = P.r * P.r
    t[:, 28] = 1.0
    t[:, 29] = P.d2
    t[~P.have] = 0.0
    return t


def colored_terms(P: cr.Pairs, kind, k) -> np.ndarray:
    t = np.zeros((len(P.have), 32))
    with np.errstate(invalid="ignore", over="ignore"):
        wG, wI = weight(kind, k, P.rG), weight(kind, k, P.rI)
        i = 0
        for r in range(6):
            for c in range(r, 6):
                t[:, i] = wG * (P.JG[:, r] * P.JG[:, c]) + wI * (P.JI[:, r] * P.JI[:, c])
                i += 1
        for r in range(6):
            t[:, 21 + r] = wG * (P.JG[:, r] * P.rG) + wI * (P.JI[:, r] * P.rI)
        t[:, 27] = P.rG * P.rG + P.rI * P.rI  # unweighted
    t[:, 28] = 1.0
    t[:, 29] = P.d2
    t[~P.have] = 0.0
    return t


def step_record(estimator, kind, k, src, tgt, tgt_nrm, T, r, storage, src_col=None, tgt_col=None, tgt_grad=None, lam=cr.LAMBDA_DEFAULT) -> np.ndarray:
    if len(np.asarray(src).reshape(-1, 3)) == 0:
        return np.zeros(32)
    if estimator == COLORED:
        return cr.block_tree_sum(colored_terms(cr.pairs(src, src_col, tgt, tgt_nrm, tgt_col, tgt_grad, T, r, lam, storage), kind, k))
    return cr.block_tree_sum(plane_terms(plane_pairs(src, tgt, tgt_nrm, T, r, storage), kind, k))


def dense_longdouble(J, res, w, have, d2):
    """the independent formulation: J^T W J, J^T W r of the stacked rows in np.longdouble and the unweighted r^T r; (record[30], scale[30])
    with scale the sum of |addends| per term, as colored_icp_restatement.record_dense_longdouble"""
    LD = np.longdouble
    J, res, w = np.asarray(J, dtype=LD), np.asarray(res, dtype=LD), np.asarray(w, dtype=LD)
    WJ = w[:, None] * J
    iu = np.triu_indices(6)
    tail = [res @ res, LD(have.sum()), d2[have].astype(LD).sum()]
    rec = np.concatenate([(J.T @ WJ)[iu], WJ.T @ res, tail])
    scale = np.concatenate([(np.abs(J).T @ np.abs(WJ))[iu], np.abs(WJ).T @ np.abs(res), tail])
    return rec.astype(np.float64), scale.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the loop
def register(estimator, kind, k, src, tgt, tgt_nrm, r, storage, src_col=None, tgt_col=None, init=None, lam=cr.LAMBDA_DEFAULT, max_iter=30,
             rel_fitness=1e-6, rel_rmse=1e-6) -> dict:
    """colored_icp_restatement.register's loop around step_record; a system whose weights are all zero gives the identity update"""
    tgt_grad = cr.gradients(tgt, tgt_nrm, tgt_col, 2.0 * r, cr.GRADIENT_MAX_NN, storage) if estimator == COLORED else None
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = len(np.asarray(src).reshape(-1, 3))
    fitness = rmse = 0.0
    iterations, converged, n_corr, passes = 0, False, 0, 0
    if n == 0:
        return dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, converged=False, n_corr=0)
    while True:
        rec = step_record(estimator, kind, k, src, tgt, tgt_nrm, T, r, storage, src_col, tgt_col, tgt_grad, lam)
        count = rec[28]
        f = count / n if count > 0 else 0.0
        e = math.sqrt(rec[29] / count) if count > 0 else 0.0
        conv = passes > 0 and abs(fitness - f) < rel_fitness and abs(rmse - e) < rel_rmse
        fitness, rmse, n_corr = f, e, int(count + 0.5)
        passes += 1
        converged = converged or conv
        if conv or iterations >= max_iter:
            break
        x = np.linalg.solve(cr.jtj_from_record(rec), -rec[21:27]) if count > 0 and rec[:27].any() else np.zeros(6)
        T = cr.vector6_to_matrix4(x) @ T
        iterations += 1
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged, n_corr=n_corr)


# ---------------------------------------------------------------------------------------------------------------- step cases
# the coloured tests' own source, target and pose; 4200 queries are 17 blocks, one more than the block-sum fold takes at a time
STEP_SIZES = (100, 256, 257, 4200)
STEP_K = 0.02
STEP_LOSSES = tuple((kind, STEP_K) for kind in range(6))
STEP_R = cr.STEP_R


@functools.lru_cache(maxsize=None)
def _step_pairs(n, pose_name, estimator, storage):
    s = cr.sliding_scene()
    T = dict(cr.STEP_POSES + (("far", cr.FAR_POSE),))[pose_name]
    src, col = cr.step_source(n)
    if estimator == COLORED:
        return cr.pairs(src, col, s.tgt, s.tgt_nrm, s.tgt_col, cr.reference_gradients("scene", storage), T, STEP_R, cr.LAMBDA_DEFAULT, storage)
    return plane_pairs(src, s.tgt, s.tgt_nrm, T, STEP_R, storage)


@functools.lru_cache(maxsize=None)
def reference_step(n, pose_name, estimator, kind, k, storage) -> np.ndarray:
    P = _step_pairs(n, pose_name, estimator, storage)
    out = cr.block_tree_sum(colored_terms(P, kind, k) if estimator == COLORED else plane_terms(P, kind, k))
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- edge pairs
EDGE_K = 0.0625
EDGE_HEIGHTS = (0.0, 0.03125, 0.0625, 0.125)  # 0, k / 2, k, 2 k: exact in f32
EDGE_R = 0.15
EDGE_GRADIENT = (0.3, cr.GRADIENT_MAX_NN)
EDGE_LAMBDAS = (1.0, cr.LAMBDA_DEFAULT)       # at 1 the coloured estimator's r_G is the plain residual and r_I is a zero


class EdgeScene(NamedTuple):
    tgt: np.ndarray
    tgt_nrm: np.ndarray
    tgt_col: np.ndarray
    src: np.ndarray      # sixteen points, four at each height in turn
    src_col: np.ndarray
    heights: np.ndarray
    beyond: np.ndarray   # indices of the source points at k and 2 k


@functools.lru_cache(maxsize=None)
def edge_scene() -> EdgeScene:
    """a floor at z = 0 on the lattice of 0.25 m over [0, 2]^2 (81 points, every coordinate exact in f32), normals (0, 0, 1), textured;
    sixteen source points exactly above interior lattice points, at the heights 0, k / 2, k, 2 k in turn"""
    g = 0.25 * np.arange(9)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    tgt = np.column_stack([xy, np.zeros(len(xy))])
    nrm = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    ij = np.array([(1 + a, 1 + b) for a in range(4) for b in range(4)], dtype=np.float64)
    heights = np.tile(EDGE_HEIGHTS, 4)
    src = np.column_stack([0.25 * ij, heights])
    base = np.column_stack([0.25 * ij, np.zeros(16)])
    beyond = np.flatnonzero(heights >= EDGE_K)
    f = cr._frozen
    return EdgeScene(f(tgt), f(nrm), f(cr.texture(tgt)), f(src), f(cr.texture(base) + 0.03125), f(heights), beyond)


@functools.lru_cache(maxsize=None)
def edge_gradients(storage) -> np.ndarray:
    s = edge_scene()
    out = cr.gradients(s.tgt, s.tgt_nrm, s.tgt_col, *EDGE_GRADIENT, storage)
    out.setflags(write=False)
    return out


EDGE_LOSSES = ((L1, 0.0), (HUBER, EDGE_K), (TUKEY, EDGE_K), (CAUCHY, EDGE_K), (GM, EDGE_K), (L2, 0.0))


@functools.lru_cache(maxsize=None)
def reference_edge(estimator, kind, k, lam, storage, beyond_only=False) -> np.ndarray:
    s = edge_scene()
    sel = s.beyond if beyond_only else np.arange(len(s.src))
    out = step_record(estimator, kind, k, s.src[sel], s.tgt, s.tgt_nrm, np.eye(4), EDGE_R, storage, s.src_col[sel], s.tgt_col,
                      edge_gradients(storage), lam)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the outlier case
RAISED = 0.08
OUTLIER = dict(r=0.15, max_iter=15)
OUTLIER_LOSSES = ((L2, 0.0), (HUBER, 0.02), (CAUCHY, 0.02), (TUKEY, 0.05), (GM, 0.01), (L1, 0.0))
HALVING = (TUKEY, CAUCHY, HUBER, L1)  # at most half the L2 error; GM: below it


def _corner_draw(rng):
    """draw_surfaces(rng, 1024, 512) followed by a second wall at y = 0 with 512 points"""
    pts, nrm = cr.draw_surfaces(rng, 1024, 512)
    x = rng.uniform(0.0, 4.0, 512)
    z = rng.uniform(0.0, 2.0, 512)
    return (np.vstack([pts, np.column_stack([x, np.zeros(512), z])]), np.vstack([nrm, np.tile([0.0, 1.0, 0.0], (512, 1))]))


@functools.lru_cache(maxsize=None)
def outlier_scene() -> cr.Scene:
    """"corner with a raised patch": a floor and two walls from default_rng(7); the source is a second draw of them with 300 of its 1024
    floor points raised by 0.08 m (something lying on the floor that the map does not have), moved by the inverse of SLIDE_GT"""
    rng = np.random.default_rng(7)
    tgt, nrm = _corner_draw(rng)
    second, _ = _corner_draw(rng)
    raised = second.copy()
    raised[np.random.default_rng(11).choice(1024, 300, replace=False), 2] += RAISED
    inv = np.linalg.inv(cr.SLIDE_GT)
    f = cr._frozen
    return cr.Scene(f(tgt), f(nrm), f(cr.texture(tgt)), f(raised @ inv[:3, :3].T + inv[:3, 3]), f(cr.texture(second)))


@functools.lru_cache(maxsize=None)
def outlier_result(estimator, kind, k, storage) -> dict:
    s = outlier_scene()
    return register(estimator, kind, k, s.src, s.tgt, s.tgt_nrm, OUTLIER["r"], storage, s.src_col, s.tgt_col, max_iter=OUTLIER["max_iter"],
                    rel_fitness=0.0, rel_rmse=0.0)


def outlier_conditions(errors: dict) -> None:
    """the conditions of the outlier case on {kind: translation error}: asserted on the restatement and on the device's own results"""
    l2 = errors[L2]
    assert l2 > 0.010, l2
    for kind in HALVING:
        assert errors[kind] <= 0.5 * l2, (LOSS_NAMES[kind], errors[kind], l2)
    assert errors[GM] < l2, (errors[GM], l2)
