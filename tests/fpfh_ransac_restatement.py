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


def pair_feature(p1, n1, p2, n2, tags=None):
    """ComputePairFeatures -> (f0, f1, f2) (Python floats, one rounding per operation).  tags: a set that collects the branches taken
    ("zero_d", "zero_cross", "swap", "equal_no_swap", "atan2_+pi", "atan2_-pi", "f1_+1", "f1_-1")."""
    dx, dy, dz = p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]
    dn = math.sqrt(dx * dx + dy * dy + dz * dz)
    if dn == 0.0:
        if tags is not None:
            tags.add("zero_d")
        return 0.0, 0.0, 0.0
    a1 = (n1[0] * dx + n1[1] * dy + n1[2] * dz) / dn
    a2 = (n2[0] * dx + n2[1] * dy + n2[2] * dz) / dn
    a, b = n1, n2
    if math.acos(abs(a1)) > math.acos(abs(a2)):
        a, b = n2, n1
        dx, dy, dz = -dx, -dy, -dz
        f2 = -a2
        if tags is not None:
            tags.add("swap")
    else:
        f2 = a1
        if tags is not None and abs(a1) == abs(a2):
            tags.add("equal_no_swap")
    vx, vy, vz = dy * a[2] - dz * a[1], dz * a[0] - dx * a[2], dx * a[1] - dy * a[0]
    vn = math.sqrt(vx * vx + vy * vy + vz * vz)
    if vn == 0.0:
        if tags is not None:
            tags.add("zero_cross")
        return 0.0, 0.0, 0.0
    vx, vy, vz = vx / vn, vy / vn, vz / vn
    wx, wy, wz = a[1] * vz - a[2] * vy, a[2] * vx - a[0] * vz, a[0] * vy - a[1] * vx
    f1 = vx * b[0] + vy * b[1] + vz * b[2]
    f0 = math.atan2(wx * b[0] + wy * b[1] + wz * b[2], a[0] * b[0] + a[1] * b[1] + a[2] * b[2])
    if tags is not None:
        if abs(f0) == math.pi:
            tags.add("atan2_+pi" if f0 > 0 else "atan2_-pi")
        if abs(f1) == 1.0:
            tags.add("f1_+1" if f1 > 0 else "f1_-1")
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


def pair_feature_tags(P, N, nbrs):
    """the branches of pair_feature that the SPFH of (P, N, nbrs) takes (a set of tags)"""
    tags = set()
    for i, (idx, _) in enumerate(nbrs):
        p, n = P[i].tolist(), N[i].tolist()
        for k in idx[1:]:
            pair_feature(p, n, P[k].tolist(), N[k].tolist(), tags)
    return tags


# ---- feature nearest neighbour, exactly as feature_nn_kernel ---------------------------------------------------------------------
def feature_nn(A, B, chunk=256):
    """out[i] = argmin_j d(A[i], B[j]) with d = 0; d = d + (a_b - b_b)^2 for b = 0..32 in order (f64, one rounding per operation), ties
    to the lower j; -1 when B is empty"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.full(len(A), -1, np.int64)
    if len(B) == 0:
        return out
    Bt = np.ascontiguousarray(B.T)
    for i0 in range(0, len(A), chunk):
        a = A[i0:i0 + chunk]
        d = np.zeros((len(a), len(B)))
        t = np.empty_like(d)
        for b in range(A.shape[1]):
            np.subtract(a[:, b:b + 1], Bt[b][None, :], out=t)
            np.multiply(t, t, out=t)
            d += t
        out[i0:i0 + chunk] = np.argmin(d, axis=1)  # (the first minimum: the lower index)
    return out


def feature_correspondences(A, B, mutual, ransac_n, ab=None, ba=None):
    """RegistrationRANSACBasedOnFeatureMatching's pairs as o3ds_feature_correspondences states them: ((k, 2) int64, fell_back).
    ab / ba: feature_nn(A, B) / feature_nn(B, A) when already known."""
    ab = feature_nn(A, B) if ab is None else ab
    one = np.column_stack([np.arange(len(A)), ab]).astype(np.int64)
    if len(A) == 0 or len(B) == 0:
        return np.zeros((0, 2), np.int64), False
    if not mutual:
        return one, False
    ba = feature_nn(B, A) if ba is None else ba
    keep = ba[ab] == np.arange(len(A))
    if keep.sum() >= 3 * max(ransac_n, 0):
        return one[keep], False
    return one, True


def ls_cost(T, p, q):
    """sum_k |q_k - T p_k|^2 (the least-squares cost Umeyama minimises over rigid T)"""
    r = q - (p @ T[:3, :3].T + T[:3, 3])
    return float(np.sum(r * r))


# ---- structured clouds (every coordinate and normal exact in f32) ---------------------------------------------------------------
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])


def lattice(side, spacing=0.125, seed=0, dups=()):
    """a side^3 cubic lattice (index order x fastest) with normals drawn from {+-x, +-y, +-z}; dups: indices of points appended a
    second time (same position, another axis normal), for |d| = 0 pairs"""
    g = np.arange(side) * spacing
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    P = np.column_stack([x.ravel(), y.ravel(), z.ravel()])
    rng = np.random.default_rng(seed)
    N = AXES[rng.integers(0, 6, len(P))]
    if len(dups):
        P = np.vstack([P, P[list(dups)]])
        N = np.vstack([N, AXES[rng.integers(0, 6, len(dups))]])
    return P, N


def dyadic_cloud(n, seed, half=(7.0, 7.0, 7.0), q=2.0 ** -10):
    """n points with coordinates on the 2^-10 grid, |x_a| < half_a < 8, and unit normals rounded to f32 (so f32 storage holds both
    exactly)"""
    rng = np.random.default_rng(seed)
    P = np.round(rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(half) / q) * q
    N = rng.normal(size=(n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    return P, N


def tile(P, N, offsets):
    """copies of (P, N) at the given offsets, copy-major (copy c holds points c * len(P) ...)"""
    offsets = np.asarray(offsets, np.float64)
    return (np.vstack([P + o for o in offsets]), np.tile(N, (len(offsets), 1)))
