"""Search-free registration against voxel Gaussians (the normal-distributions transform) restated in numpy from the text of
include/o3ds_backend.h (the voxel-Gaussian section), operation for operation: the Gaussians of a cloud, the record of one step, the
registration loop -- and the scenes the CPU and GPU tests share.  The eigen-decomposition, the solve and the composition of an update are
degeneracy_restatement's, the loss weights robust_icp_restatement's, the sum order colored_icp_restatement's.

Arithmetic: numpy float64, every operation on its own; sums that the header orders are taken in that order.

Scenes: degeneracy_restatement's `room` and `corridor`, the target translated by SHIFT (and the ground truth with it) so that no surface lies
on a voxel face: on the unshifted noise-free room every surface sits on one, and which side a point falls on is decided by rounding.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import colored_icp_restatement as cr
import degeneracy_restatement as dr
import robust_icp_restatement as rr

F32, F64 = cr.F32, cr.F64
STORAGES = cr.STORAGES
to_storage = cr.to_storage
L2, L1, HUBER, CAUCHY, GM, TUKEY = rr.L2, rr.L1, rr.HUBER, rr.CAUCHY, rr.GM, rr.TUKEY

KEY_LIMIT = float(1 << 20)
OFFSETS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.int64)
TRIU = tuple((a, b) for a in range(3) for b in range(a, 3))  # 00 01 02 11 12 22


# ---------------------------------------------------------------------------------------------------------------- the Gaussians
class Gaussians(NamedTuple):
    voxel_size: float
    keys: np.ndarray         # (n, 3) int32, ascending packed-key order (kz major, then ky, then kx)
    counts: np.ndarray       # (n,) uint32
    mean: np.ndarray         # (n, 3)
    cov: np.ndarray          # (n, 6) upper triangle, row-major
    information: np.ndarray  # (n, 6)
    valid: np.ndarray        # (n,) uint8
    info: dict               # n_voxels, n_valid, n_skipped_points, n_flat
    packed: np.ndarray       # (n,) int64: the sort key


def pack(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.int64) + (1 << 20)
    return (k[..., 2] << 42) | (k[..., 1] << 21) | k[..., 0]


def voxel_coords(p, voxel_size):
    """(k (n, 3) int64, in a voxel (n,) bool): k_a = floor(x_a * inv); not finite, or some |k_a| >= 2^20: no voxel"""
    inv = 1.0 / float(voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(p, dtype=np.float64) * inv)
        ok = (np.abs(f) < KEY_LIMIT).all(axis=1)  # (a NaN compares false)
    return np.where(ok[:, None], f, 0.0).astype(np.int64), ok


def sym3(u) -> np.ndarray:
    return np.array([[u[0], u[1], u[2]], [u[1], u[3], u[4]], [u[2], u[4], u[5]]])


def voxel_gaussians(points, voxel_size, min_points, ratio, storage) -> Gaussians:
    P = to_storage(np.asarray(points, dtype=np.float64).reshape(-1, 3), storage)
    k, ok = voxel_coords(P, voxel_size)
    idx = np.flatnonzero(ok)
    pk = pack(k[idx])
    order = np.argsort(pk, kind="stable")  # members in ascending original index
    idx, pk = idx[order], pk[order]
    starts = np.flatnonzero(np.r_[True, pk[1:] != pk[:-1]]) if len(pk) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(pk)]
    n = len(starts)
    keys, counts = np.zeros((n, 3), np.int32), np.zeros(n, np.uint32)
    mean, cov, info, valid = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 6)), np.zeros(n, np.uint8)
    n_flat = 0
    for v, (lo, hi) in enumerate(zip(starts, ends)):
        members = P[idx[lo:hi]]
        nv = hi - lo
        s = np.zeros(3)
        for p in members:
            s = s + p
        mu = s / float(nv)
        S = np.zeros(6)
        with np.errstate(over="ignore", invalid="ignore"):
            for p in members:
                r = p - mu
                S = S + np.array([r[0] * r[0], r[0] * r[1], r[0] * r[2], r[1] * r[1], r[1] * r[2], r[2] * r[2]])
        C = S / float(nv - 1) if nv > 1 else S
        keys[v], counts[v], mean[v], cov[v] = k[idx[lo]], nv, mu, C
        if nv < min_points:
            continue
        lam, V = dr.eigen3(sym3(C))
        if not (math.isfinite(lam[2]) and lam[2] > 0.0):
            n_flat += 1
            continue
        f = ratio * lam[2]
        l = [f if lam[i] < f else lam[i] for i in range(3)]
        info[v] = [((V[a][0] * V[b][0]) / l[0] + (V[a][1] * V[b][1]) / l[1]) + (V[a][2] * V[b][2]) / l[2] for a, b in TRIU]
        valid[v] = 1
    counters = dict(n_voxels=n, n_valid=int(valid.sum()), n_skipped_points=int(len(P) - len(idx)), n_flat=n_flat)
    return Gaussians(float(voxel_size), keys, counts, mean, cov, info, valid, counters, pk[starts] if n else np.zeros(0, np.int64))


# ---------------------------------------------------------------------------------------------------------------- the step
def queries(src, T, storage) -> np.ndarray:
    S = to_storage(np.asarray(src, dtype=np.float64).reshape(-1, 3), storage)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[a, 0] * S[:, 0] + T[a, 1] * S[:, 1]) + T[a, 2] * S[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def jacobian(p) -> np.ndarray:
    """(n, 3, 6): columns e_c x p, then the unit vectors"""
    J = np.zeros((len(p), 3, 6))
    J[:, 1, 0], J[:, 2, 0] = -p[:, 2], p[:, 1]
    J[:, 0, 1], J[:, 2, 1] = p[:, 2], -p[:, 0]
    J[:, 0, 2], J[:, 1, 2] = -p[:, 1], p[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return J


def lookup(G: Gaussians, k, ok):
    """(index (n,), found-and-valid (n,)) of the voxels with coordinates k; no result depends on how"""
    nv = len(G.packed)
    if nv == 0:
        return np.zeros(len(k), np.int64), np.zeros(len(k), bool)
    inr = ok & (np.abs(k) < (1 << 20)).all(axis=1)
    pk = pack(np.where(inr[:, None], k, 0))
    at = np.minimum(np.searchsorted(G.packed, pk), nv - 1)
    return at, inr & (G.packed[at] == pk) & (G.valid[at] != 0)


def step_terms(src, G: Gaussians, T, neighbourhood, kind, k, storage) -> np.ndarray:
    """the (n, 32) terms of the queries"""
    p = queries(src, T, storage)
    n = len(p)
    t = np.zeros((n, 32))
    kq, ok = voxel_coords(p, G.voxel_size)
    J = jacobian(p)
    found, best = np.zeros(n, bool), np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for off in OFFSETS[:neighbourhood]:
            at, hit = lookup(G, kq + off, ok)
            if not hit.any():
                continue
            mu, Bu = G.mean[at], G.information[at]
            B = np.empty((n, 3, 3))
            for i, (a, b) in enumerate(TRIU):
                B[:, a, b] = B[:, b, a] = Bu[:, i]
            e = p - mu
            u = np.stack([(B[:, a, 0] * e[:, 0] + B[:, a, 1] * e[:, 1]) + B[:, a, 2] * e[:, 2] for a in range(3)], axis=1)
            m = cr.dot(e, u)
            r = np.where(m > 0.0, np.sqrt(np.where(m > 0.0, m, 0.0)), 0.0)
            w = rr.weight(kind, k, r)
            Gm = np.stack([np.stack([(B[:, a, 0] * J[:, 0, c] + B[:, a, 1] * J[:, 1, c]) + B[:, a, 2] * J[:, 2, c] for c in range(6)], axis=1)
                           for a in range(3)], axis=1)  # (n, 3, 6)
            i = 0
            for rw in range(6):
                for c in range(rw, 6):
                    h = w * ((J[:, 0, rw] * Gm[:, 0, c] + J[:, 1, rw] * Gm[:, 1, c]) + J[:, 2, rw] * Gm[:, 2, c])
                    t[:, i] = np.where(hit, t[:, i] + h, t[:, i])
                    i += 1
            for rw in range(6):
                g = w * ((J[:, 0, rw] * u[:, 0] + J[:, 1, rw] * u[:, 1]) + J[:, 2, rw] * u[:, 2])
                t[:, 21 + rw] = np.where(hit, t[:, 21 + rw] + g, t[:, 21 + rw])
            t[:, 27] = np.where(hit, t[:, 27] + m, t[:, 27])
            ee = cr.dot(e, e)
            best = np.where(hit & (~found | (ee < best)), ee, best)  # the first of equals stays
            found |= hit
    t[:, 28] = found.astype(np.float64)
    t[:, 29] = np.where(found, best, 0.0)
    return t


def step_record(src, G: Gaussians, T, neighbourhood, kind, k, storage) -> np.ndarray:
    if len(np.asarray(src).reshape(-1, 3)) == 0 or G.info["n_valid"] == 0:
        return np.zeros(32)
    return cr.block_tree_sum(step_terms(src, G, T, neighbourhood, kind, k, storage))


def dense_longdouble(src, G: Gaussians, T, neighbourhood, kind, k, storage):
    """the independent formulation: per query and voxel the matrices J (3x6) and B (3x3), H += w J^T B J and g += w J^T B e as matrix products
    in np.longdouble; (record[30], scale[30]) with scale the same sums over the absolute values, as robust_icp_restatement.dense_longdouble"""
    LD = np.longdouble
    p = queries(src, T, storage)
    kq, ok = voxel_coords(p, G.voxel_size)
    H, g, Hs, gs = np.zeros((6, 6), LD), np.zeros(6, LD), np.zeros((6, 6), LD), np.zeros(6, LD)
    m_sum, count, d2 = LD(0), 0, LD(0)
    for i in range(len(p)):
        x, y, z = p[i]
        J = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], dtype=LD)
        ees = []
        for off in OFFSETS[:neighbourhood]:
            at, hit = lookup(G, (kq[i] + off)[None, :], ok[i:i + 1])
            if not hit[0]:
                continue
            B = sym3(G.information[at[0]]).astype(LD)
            e = (p[i] - G.mean[at[0]]).astype(LD)
            m = e @ B @ e
            w = LD(rr.weight(kind, k, math.sqrt(float(m)) if m > 0 else 0.0))
            H += w * (J.T @ B @ J)
            g += w * (J.T @ (B @ e))
            Hs += w * (np.abs(J).T @ np.abs(B) @ np.abs(J))
            gs += w * (np.abs(J).T @ (np.abs(B) @ np.abs(e)))
            m_sum += m
            ees.append(e @ e)
        if ees:
            count += 1
            d2 += min(ees)
    iu = np.triu_indices(6)
    tail = [m_sum, LD(count), d2]
    return (np.concatenate([H[iu], g, tail]).astype(np.float64), np.concatenate([Hs[iu], gs, tail]).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------- the loop
def register(src, G: Gaussians, neighbourhood, kind, k, storage, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6) -> dict:
    """robust_icp_restatement.register's loop around step_record, with the solve and the composition of degeneracy_restatement (the LDL^T
    every step loop runs)"""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = len(np.asarray(src).reshape(-1, 3))
    fitness = rmse = 0.0
    iterations, converged, n_corr, passes = 0, False, 0, 0
    if n == 0:
        return dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, converged=False, n_corr=0)
    while True:
        rec = step_record(src, G, T, neighbourhood, kind, k, storage)
        count = rec[28]
        f = count / n if count > 0 else 0.0
        e = math.sqrt(rec[29] / count) if count > 0 else 0.0
        conv = passes > 0 and abs(fitness - f) < rel_fitness and abs(rmse - e) < rel_rmse
        fitness, rmse, n_corr = f, e, int(count + 0.5)
        passes += 1
        converged = converged or conv
        if conv or iterations >= max_iter:
            break
        T = dr.compose(dr.ordinary_x(rec), T)
        iterations += 1
    return dict(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged, n_corr=n_corr)


# ---------------------------------------------------------------------------------------------------------------- scenes
SHIFT = np.array([0.13, 0.21, 0.17])
FAR_SHIFT = dr.FAR_SHIFT  # (512, -256, 32) m, powers of two
VOXEL, MIN_POINTS, RATIO = 0.5, 6, 0.01
SCENES = ("room", "corridor")
STEP_SIZES = (1, 255, 256, 257, 2125)
LOOP_N = 2125
NEIGHBOURHOODS = (1, 7)
STEP_LOSSES = ((L2, 0.0), (CAUCHY, 1.0), (TUKEY, 3.0))
LOSS_NAMES = rr.LOSS_NAMES
INIT_OFFSET = np.array([0.12, -0.10, 0.08])  # the registration starts 0.20 m from the truth
LOOP_ITER = 30
POSE_TOL = (5e-3, 5e-3)  # metres, radians: about 3x the 0.6-1.7 mm and 0.4-1.7 mrad a float64 prototype of the header's text ended at


def translation(t) -> np.ndarray:
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _moved(far) -> np.ndarray:
    return SHIFT + FAR_SHIFT if far else SHIFT


@functools.lru_cache(maxsize=None)
def target(name, noisy, far=False) -> np.ndarray:
    return cr._frozen(dr.scene(name, noisy).tgt + _moved(far))


def source(name, noisy, n) -> np.ndarray:
    return dr.source(name, noisy, n)


def ground_truth(name, far=False) -> np.ndarray:
    return translation(_moved(far)) @ dr.ground_truth(name)


def initial_pose(far=False) -> np.ndarray:
    return translation(_moved(far) + INIT_OFFSET)


# the pose of the step cases: near the truth, not at it (a residual of exactly zero says little)
def step_pose(name, far=False) -> np.ndarray:
    return translation((0.012, -0.008, 0.010)) @ ground_truth(name, far)


@functools.lru_cache(maxsize=None)
def reference_gaussians(name, noisy, storage, far=False) -> Gaussians:
    return voxel_gaussians(target(name, noisy, far), VOXEL, MIN_POINTS, RATIO, storage)


@functools.lru_cache(maxsize=None)
def reference_step(name, noisy, n, neighbourhood, kind, k, storage, far=False) -> np.ndarray:
    out = step_record(source(name, noisy, n), reference_gaussians(name, noisy, storage, far), step_pose(name, far), neighbourhood, kind, k, storage)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_registration(name, noisy, neighbourhood, kind, k, storage) -> dict:
    return register(source(name, noisy, LOOP_N), reference_gaussians(name, noisy, storage), neighbourhood, kind, k, storage, init=initial_pose(),
                    max_iter=LOOP_ITER, rel_fitness=0.0, rel_rmse=0.0)


def pose_error(T, name, src, far=False):
    """(metres, radians) of T against the scene's ground truth, the translation taken at the scan's centre"""
    G = ground_truth(name, far)
    c0 = np.asarray(src).reshape(-1, 3).mean(axis=0)
    d = dr.centre_motion(T, G, c0)
    Rd = np.asarray(T)[:3, :3] @ G[:3, :3].T
    return float(np.linalg.norm(d)), math.acos(min(1.0, max(-1.0, (np.trace(Rd) - 1.0) / 2.0)))


# ---------------------------------------------------------------------------------------------------------------- the edge cloud
EDGE_FAR_VOXELS = 100


@functools.lru_cache(maxsize=None)
def edge_cloud() -> np.ndarray:
    """every case of the build rule in one cloud, voxel size 0.5, min_points 6; the voxels are named by their coordinates"""
    rng = np.random.default_rng(2026)

    def inside(k, n):  # n points well inside voxel k
        return (np.asarray(k, dtype=np.float64) + rng.uniform(0.1, 0.9, (n, 3))) * VOXEL

    parts = [
        inside((0, 0, 0), MIN_POINTS - 1),                                   # one member short: not valid, not flat
        inside((2, 0, 0), MIN_POINTS),                                       # exactly enough
        np.tile([[2.25, 1.25, 0.125]], (MIN_POINTS + 1, 1)),                 # identical points, every partial sum exact: n_flat
        np.array([1.05, 2.05, 3.05]) + np.outer(np.linspace(0.0, 0.3, 8), [1.0, 0.5, 0.25]),  # collinear: two clamped values
        np.array([[k * 0.5, 3.2, 0.3 + 0.01 * k] for k in range(-3, 5)]),    # exactly on faces x = k * 0.5
        np.array([[1.5, 3.5, 0.5], [1.5, 3.5, 0.75], [1.625, 3.625, 0.625], [1.75, 3.75, 0.875], [1.875, 3.5, 0.5], [1.5, 3.875, 0.75]]),  # corner + exact values
        np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [0.5 * (1 << 20), 0.1, 0.1], [0.1, -0.5 * (1 << 20) - 0.1, 0.1]]),  # skipped
        np.array([[0.5 * ((1 << 20) - 1) + 0.1, 0.1, 0.1]]),                 # the last voxel that exists
        inside((-3, -2, -1), 9), inside((-1, -1, -1), 7), -inside((4, 4, 4), 6),  # negative coordinates
        np.array([[0.3, 0.3, 5.2]]),                                         # a voxel of one point
    ]
    pts = np.vstack(parts)
    return cr._frozen(pts[rng.permutation(len(pts))])


def far_voxels(n_voxels=EDGE_FAR_VOXELS, per_voxel=5) -> np.ndarray:
    """per_voxel points in each of n_voxels voxels far from every scene (the lookup-independence case)"""
    rng = np.random.default_rng(77)
    k = np.array([(400 + 3 * (i % 10), -300 + 3 * (i // 10), 200 + (i % 7)) for i in range(n_voxels)], dtype=np.float64)
    return cr._frozen((np.repeat(k, per_voxel, axis=0) + rng.uniform(0.1, 0.9, (n_voxels * per_voxel, 3))) * VOXEL)


# ---------------------------------------------------------------------------------------------------------------- recorded premises
# measured by tests/test_ndt_restatement_cpu.py (printed there) on the shifted noisy room, f64 storage:
#   Gaussians against np.cov / np.linalg.eigh / np.linalg.inv on the valid voxels: the largest relative difference (of a matrix: the
#   largest |difference| over the largest |entry|) of mean, covariance and information; the bound is 16x
#   the record against dense_longdouble: the largest |difference| / scale over the terms; the bound is 16x
GAUSSIAN_REL_MEASURED = 3.27e-15  # measured 3.266e-15
GAUSSIAN_REL_TOL = 16 * GAUSSIAN_REL_MEASURED
RECORD_REL_MEASURED = 3.76e-16    # measured 3.754e-16 (neighbourhood 7)
RECORD_REL_TOL = 16 * RECORD_REL_MEASURED
