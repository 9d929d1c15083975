"""numpy restatement of the place-recognition front half (the checker of tests/test_place_recognition_*.py): Open3D v0.15.1's
ComputePairFeatures / ComputeSPFHFeature / ComputeFPFHFeature, the feature correspondences of RegistrationRANSACBasedOnFeatureMatching,
the hypothesis draws, the two correspondence checkers, validation and the serial stopping rule, as include/o3ds_backend.h states them."""
from __future__ import annotations

import math

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z: int) -> int:  # splitmix64 finaliser
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed: int, n: int, t: int, m: int) -> list:
    return [mix(seed + (n * t + j + 1) * GOLDEN) % m for j in range(n)]


def d2_rows(P, q):
    d = P - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def neighbours(P, radius, max_nn, tree=None):
    """per point: (indices, d2) -- the max_nn smallest (d2, index) with d2 < radius^2, sorted"""
    r2 = radius * radius
    out = []
    cand = tree.query_ball_point(P, radius * (1 + 1e-9)) if tree is not None else None
    for i in range(len(P)):
        idx = np.arange(len(P)) if cand is None else np.asarray(sorted(cand[i]), dtype=np.int64)
        d2 = d2_rows(P[idx], P[i])
        keep = d2 < r2
        idx, d2 = idx[keep], d2[keep]
        o = np.lexsort((idx, d2))[:max_nn]
        out.append((idx[o], d2[o]))
    return out


def pair_feature(p1, n1, p2, n2):
    """ComputePairFeatures -> (f0, f1, f2) (Python floats, one rounding per operation)"""
    dx, dy, dz = p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]
    dn = math.sqrt(dx * dx + dy * dy + dz * dz)
    if dn == 0.0:
        return 0.0, 0.0, 0.0
    a1 = (n1[0] * dx + n1[1] * dy + n1[2] * dz) / dn
    a2 = (n2[0] * dx + n2[1] * dy + n2[2] * dz) / dn
    a, b = n1, n2
    if math.acos(abs(a1)) > math.acos(abs(a2)):
        a, b = n2, n1
        dx, dy, dz = -dx, -dy, -dz
        f2 = -a2
    else:
        f2 = a1
    vx, vy, vz = dy * a[2] - dz * a[1], dz * a[0] - dx * a[2], dx * a[1] - dy * a[0]
    vn = math.sqrt(vx * vx + vy * vy + vz * vz)
    if vn == 0.0:
        return 0.0, 0.0, 0.0
    vx, vy, vz = vx / vn, vy / vn, vz / vn
    wx, wy, wz = a[1] * vz - a[2] * vy, a[2] * vx - a[0] * vz, a[0] * vy - a[1] * vx
    f1 = vx * b[0] + vy * b[1] + vz * b[2]
    f0 = math.atan2(wx * b[0] + wy * b[1] + wz * b[2], a[0] * b[0] + a[1] * b[1] + a[2] * b[2])
    return f0, f1, f2


def clamp_bin(v):
    b = math.floor(v)
    return 0 if b < 0 else (10 if b >= 11 else b)


def bins(f0, f1, f2):
    return (clamp_bin(11.0 * (f0 + math.pi) / (2.0 * math.pi)), 11 + clamp_bin(11.0 * (f1 + 1.0) * 0.5),
            22 + clamp_bin(11.0 * (f2 + 1.0) * 0.5))


def spfh(P, N, nbrs):
    S = np.zeros((len(P), 33))
    for i, (idx, _) in enumerate(nbrs):
        if len(idx) <= 1:
            continue
        incr = 100.0 / (len(idx) - 1)
        p, n = P[i].tolist(), N[i].tolist()
        for k in idx[1:]:
            for b in bins(*pair_feature(p, n, P[k].tolist(), N[k].tolist())):
                S[i, b] += incr
    return S


def fpfh(P, N, radius, max_nn, tree=None):
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    nbrs = neighbours(P, radius, max_nn, tree)
    S = spfh(P, N, nbrs)
    F = np.zeros_like(S)
    for i, (idx, d2) in enumerate(nbrs):
        if len(idx) <= 1:
            continue
        f = [0.0] * 33
        s = [0.0, 0.0, 0.0]
        for k, dk in zip(idx[1:], d2[1:]):
            if dk == 0.0:
                continue
            row = S[k]
            for j in range(33):
                v = row[j] / dk
                s[j // 11] += v
                f[j] += v
        s = [100.0 / x if x != 0.0 else x for x in s]
        F[i] = [f[j] * s[j // 11] + S[i, j] for j in range(33)]
    return F


def umeyama(p, q):
    """rigid (no scaling) least-squares T with q ~ T p"""
    mp, mq = p.mean(0), q.mean(0)
    S = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(S)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T


def edge_check(ps, qs, s):
    """(passed, margin): margin = distance of the closest comparison to its threshold (for the near-threshold exemption)"""
    ok, margin = True, np.inf
    for i in range(len(ps)):
        for j in range(i + 1, len(ps)):
            ds, dt = np.linalg.norm(ps[i] - ps[j]), np.linalg.norm(qs[i] - qs[j])
            margin = min(margin, abs(ds - dt * s), abs(dt - ds * s))
            if ds < dt * s or dt < ds * s:
                ok = False
    return ok, margin


def distance_check(ps, qs, T, tau):
    d = np.linalg.norm(qs - (ps @ T[:3, :3].T + T[:3, 3]), axis=1)
    return bool(np.all(d <= tau)), float(np.min(np.abs(d - tau)))


def stopping_rule(max_iteration, confidence, ransac_n, n_src, validated):
    """Open3D's loop read in index order.  validated: {t: (pairs, rmse)} of the hypotheses that passed the checkers.  Returns
    (iterations_run, best_t, validations)."""
    conf = min(1.0, max(0.0, confidence))
    est_k, best, best_t, vals, t_last = max_iteration, (0, 0.0), -1, 0, -1
    for t in sorted(validated):
        if t >= est_k:
            break
        vals += 1
        pairs, rmse = validated[t]
        if pairs > best[0] or (pairs == best[0] and rmse < best[1]):
            best, best_t, t_last = (pairs, rmse), t, t
            fitness = pairs / n_src
            with np.errstate(divide="ignore", invalid="ignore"):
                est = np.log(1.0 - conf) / np.log(1.0 - fitness ** ransac_n)
            if est < est_k:
                est_k = int(math.ceil(est))
    return max(min(est_k, max_iteration), t_last + 1), best_t, vals
