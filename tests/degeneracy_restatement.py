"""Degeneracy-aware ICP restated in numpy from the text of include/o3ds_backend.h (the degeneracy section), operation for operation: the
centre of a cloud as o3ds_cloud_center forms it, the re-centring of a pass's 6x6 system, the two 3x3 Jacobi eigen-decompositions, the
rule that marks directions, the LDL^T solve every step loop runs (with its fused multiply-adds, which are exact here), the constrained
update and the registration loop -- and the scenes the CPU and GPU tests share.  The record of a pass is robust_icp_restatement's.

Arithmetic: Python floats (IEEE f64, every operation on its own); fma(a, b, c) is one rounding of the exact a b + c.  sin and cos are
the platform's; the poses of the cases keep every angle of an update below 0.02 rad, where sin x and cos x are one or two terms of their
series away from x and 1 and a correctly rounded result is what every library returns.

Scenes (corridor axis = x):
  room          floor, the walls y = 0 and x = 0 at right angles, the end wall x = 4: nothing degenerate
  corridor      floor and the parallel walls y = 0 and y = 2: translation along x degenerate
  plane         the floor alone: translations along x and y and the rotation about z degenerate
  far_corridor  the corridor moved by (512, -256, 32) m, powers of two
each noise-free (analytic normals: the dropped values are exactly 0) and noisy (seeded): sigma = 1 cm on every point, and normals tilted
by sigma_n = 0.01 rad -- what a fit over a metre of such points leaves -- so that a dropped direction carries the small, real information
(lambda^ about sigma_n^2 = 1e-4) that a recorded scan gives it, and the ordinary solve a pivot that is noise.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np

import colored_icp_restatement as cr
import icp_search_restatement as isr
import robust_icp_restatement as rr

F32, F64 = cr.F32, cr.F64
STORAGES = cr.STORAGES
to_storage = cr.to_storage
SWEEPS = 8
TINY = 2.2250738585072014e-308


def fma(a, b, c) -> float:
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    if a == 0.0 or b == 0.0:
        return a * b + c  # (keeps the sign of a zero sum)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---------------------------------------------------------------------------------------------------------------- the centre
def cloud_center(points, storage) -> np.ndarray:
    """o3ds_cloud_center: 256 chunks of ceil(n / 256) points, thread t of a chunk adds its points lo + t, lo + t + 256, ... one after the
    other, a halving tree over the 256 threads, the same tree over the chunks, the sums divided by n"""
    P = to_storage(points, storage)
    n = len(P)
    if n == 0:
        return np.zeros(3)
    ln = (n + 255) // 256
    lo = np.arange(256) * ln
    hi = np.minimum(lo + ln, n)
    acc = np.zeros((256, 256, 3))
    for m in range((ln + 255) // 256):
        i = lo[:, None] + np.arange(256)[None, :] + 256 * m
        ok = i < hi[:, None]
        acc = np.where(ok[..., None], acc + P[np.minimum(i, n - 1)], acc)

    def tree(a):
        s = 128
        while s >= 1:
            a[:s] = a[:s] + a[s:2 * s]
            s //= 2
        return a[0]

    chunks = np.stack([tree(acc[c].copy()) for c in range(256)])
    return tree(chunks) / float(n)


# ---------------------------------------------------------------------------------------------------------------- 6x6 pieces
def dense(P, Q) -> np.ndarray:
    """entry (i, j) = P[i][0] Q[0][j], then + P[i][k] Q[k][j] for k = 1 .. 5; Q may be a vector"""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    vec = Q.ndim == 1
    if vec:
        Q = Q[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        s = P[:, 0:1] * Q[0:1, :]
        for k in range(1, P.shape[1]):
            s = s + P[:, k:k + 1] * Q[k:k + 1, :]
    return s[:, 0] if vec else s


def upper_symmetric(A) -> np.ndarray:
    A = np.asarray(A, dtype=np.float64)
    return np.triu(A) + np.triu(A, 1).T


def recentre_matrix(c) -> np.ndarray:
    M = np.eye(6)
    M[3:, :3] = [[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]]
    return M


def _rotate(a, V, p, q, r):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    a[p][p] = a[p][p] - h
    a[q][q] = a[q][q] + h
    a[p][q] = a[q][p] = 0.0
    x, y = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * x - s * y
    a[r][q] = a[q][r] = s * x + c * y
    for k in range(3):
        x, y = V[k][p], V[k][q]
        V[k][p] = c * x - s * y
        V[k][q] = s * x + c * y


def eigen3(S):
    """(values ascending, vectors as columns) of the symmetric 3x3 given by the UPPER triangle of S: cyclic Jacobi, SWEEPS sweeps"""
    a = [[float(S[min(i, j)][max(i, j)]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        _rotate(a, V, 0, 1, 2)
        _rotate(a, V, 0, 2, 1)
        _rotate(a, V, 1, 2, 0)
    lam = [a[0][0], a[1][1], a[2][2]]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if lam[i] > lam[j]:
            lam[i], lam[j] = lam[j], lam[i]
            for k in range(3):
                V[k][i], V[k][j] = V[k][j], V[k][i]
    for j in range(3):
        big = V[0][j]
        if abs(V[1][j]) > abs(big):
            big = V[1][j]
        if abs(V[2][j]) > abs(big):
            big = V[2][j]
        if big < 0.0:
            for k in range(3):
                V[k][j] = -V[k][j]
    return np.array(lam), np.array(V)


def solve6(A, b) -> np.ndarray:
    """the LDL^T of the step loops' tail on (the upper triangle of A, b): symmetric pivoting on the largest |diagonal| (the first of equals),
    multipliers a (1 / d), eliminations and back substitution by fma, components of pivots not above the smallest normal double zeroed"""
    a = [[float(A[min(i, j)][max(i, j)]) for j in range(6)] for i in range(6)]
    b = [float(v) for v in b]
    perm = list(range(6))
    rd = [0.0] * 6
    for s in range(6):
        piv, best = s, abs(a[s][s])
        for j in range(s + 1, 6):
            if abs(a[j][j]) > best:
                best, piv = abs(a[j][j]), j
        if piv != s:
            a[s], a[piv] = a[piv], a[s]
            b[s], b[piv] = b[piv], b[s]
            perm[s], perm[piv] = perm[piv], perm[s]
            for row in a:
                row[s], row[piv] = row[piv], row[s]
        d, bs = a[s][s], b[s]
        rd[s] = 1.0 / d if abs(d) > TINY else 0.0
        for i in range(s + 1, 6):
            l = a[i][s] * (1.0 / d) if d != 0.0 else a[i][s]
            for j in range(s + 1, 6):
                a[i][j] = fma(-l, a[s][j], a[i][j])
            b[i] = fma(-l, bs, b[i])
    xs = [0.0] * 6
    for i in range(5, -1, -1):
        num = b[i]
        for j in range(i + 1, 6):
            num = fma(-a[i][j], xs[j], num)
        xs[i] = num * rd[i] if rd[i] != 0.0 else num - b[i]
    x = np.zeros(6)
    for i in range(6):
        x[perm[i]] = xs[i]
    return x


# ---------------------------------------------------------------------------------------------------------------- the analysis
class Analysis(NamedTuple):
    centre: np.ndarray        # c = T c0
    eigenvalues: np.ndarray   # (6,) normalised
    eigenvectors: np.ndarray  # (6, 6) V
    degenerate: np.ndarray    # (6,) int32
    x: np.ndarray             # the update of the pass
    M: np.ndarray
    Hc: np.ndarray            # M^T H M as computed (its upper triangle is what was read)
    gc: np.ndarray
    raw: np.ndarray           # eigenvalues before the division by n_corr

    @property
    def n_degenerate(self) -> int:
        return int(self.degenerate.sum())


def ordinary_x(rec) -> np.ndarray:
    return solve6(cr.jtj_from_record(rec), -rec[21:27]) if rec[28] > 0.0 else np.zeros(6)


def analyse(rec, T, c0, min_rot, min_trans, recentre=True) -> Analysis:
    rec, T = np.asarray(rec, dtype=np.float64), np.asarray(T, dtype=np.float64)
    H, g = cr.jtj_from_record(rec), -rec[21:27]
    c = np.array([((T[i, 0] * c0[0] + T[i, 1] * c0[1]) + T[i, 2] * c0[2]) + T[i, 3] for i in range(3)])
    M = recentre_matrix(c if recentre else np.zeros(3))
    W = dense(H, M)
    Hc = dense(M.T, W)
    gc = dense(M.T, g)
    lr, Vr = eigen3(Hc[0:3, 0:3])
    lt, Vt = eigen3(Hc[3:6, 3:6])
    raw = np.concatenate([lr, lt])
    V = np.zeros((6, 6))
    V[0:3, 0:3], V[3:6, 3:6] = Vr, Vt
    n = float(rec[28])
    if n > 0.0:
        with np.errstate(invalid="ignore", over="ignore"):
            lh = raw / n
        thr = np.array([min_rot] * 3 + [min_trans] * 3)
        deg = (lh < thr).astype(np.int32)
    else:
        lh, deg = np.zeros(6), np.ones(6, np.int32)
    if deg.sum() == 0:
        x = ordinary_x(rec)
    else:
        A = dense(V.T, dense(upper_symmetric(Hc), V))
        b = dense(V.T, gc)
        for i in np.flatnonzero(deg):
            A[i, :] = 0.0
            A[:, i] = 0.0
            A[i, i] = 1.0
            b[i] = 0.0
        y = solve6(A, b)
        x = dense(M, dense(V, y)) + 0.0
    return Analysis(c, lh, V, deg, x, M, Hc, gc, raw)


def compose(x, T) -> np.ndarray:
    """T <- U T with U of [O3D] TransformVector6dToMatrix4d; every entry of the product is fma(U_r3, T_3c, ... fma(U_r0, T_0c, 0))"""
    U = cr.vector6_to_matrix4(x)
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            s = 0.0
            for k in range(4):
                s = fma(U[r, k], T[k, c], s)
            out[r, c] = s
    return out


def register(src, tgt, tgt_nrm, r, storage, min_rot, min_trans, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, kind=rr.L2, k=0.0,
             estimator=rr.POINT_TO_PLANE, src_col=None, tgt_col=None, lam=cr.LAMBDA_DEFAULT) -> dict:
    """o3ds_icp_degeneracy_aware_dev: robust_icp_restatement.register's loop with the analysis in the place of its solve; the report's
    fields beside the result's"""
    tgt_grad = cr.gradients(tgt, tgt_nrm, tgt_col, 2.0 * r, cr.GRADIENT_MAX_NN, storage) if estimator == rr.COLORED else None
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    n = len(np.asarray(src).reshape(-1, 3))
    out = dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, converged=False, n_corr=0, centre=np.zeros(3),
               eigenvalues=np.zeros(6), eigenvectors=np.zeros((6, 6)), degenerate=np.zeros(6, np.int32), n_degenerate=0,
               ever_degenerate=np.zeros(6, np.int32), n_passes_constrained=0)
    if n == 0:
        return out
    c0 = cloud_center(src, storage)
    fitness = rmse = 0.0
    iterations, converged, passes = 0, False, 0
    ever, constrained = np.zeros(6, np.int32), 0
    while True:
        rec = rr.step_record(estimator, kind, k, src, tgt, tgt_nrm, T, r, storage, src_col, tgt_col, tgt_grad, lam)
        an = analyse(rec, T, c0, min_rot, min_trans)
        count = rec[28]
        f = count / n if count > 0 else 0.0
        e = math.sqrt(rec[29] / count) if count > 0 else 0.0
        conv = passes > 0 and abs(fitness - f) < rel_fitness and abs(rmse - e) < rel_rmse
        fitness, rmse = f, e
        passes += 1
        converged = converged or conv
        if conv or iterations >= max_iter:
            break
        T = compose(an.x, T)
        iterations += 1
        ever |= an.degenerate
        constrained += int(an.n_degenerate > 0)
    out.update(transformation=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged, n_corr=int(count + 0.5),
               centre=an.centre, eigenvalues=an.eigenvalues, eigenvectors=an.eigenvectors, degenerate=an.degenerate,
               n_degenerate=an.n_degenerate, ever_degenerate=ever, n_passes_constrained=constrained)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
# a surface: (origin, edge u, edge v, normal); a point is origin + a u + b v with a, b uniform in [0, 1)
FLOOR_ROOM = ((0, 0, 0), (4, 0, 0), (0, 3, 0), (0, 0, 1))
SURFACES = {
    "room": (FLOOR_ROOM, ((0, 0, 0), (4, 0, 0), (0, 0, 2), (0, 1, 0)), ((0, 0, 0), (0, 3, 0), (0, 0, 2), (1, 0, 0)),
             ((4, 0, 0), (0, 3, 0), (0, 0, 2), (-1, 0, 0))),
    "corridor": (((0, 0, 0), (8, 0, 0), (0, 2, 0), (0, 0, 1)), ((0, 0, 0), (8, 0, 0), (0, 0, 2), (0, 1, 0)),
                 ((0, 2, 0), (8, 0, 0), (0, 0, 2), (0, -1, 0))),
    "plane": (((0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 1)),),
}
SURFACES["far_corridor"] = SURFACES["corridor"]
FAR_SHIFT = np.array([512.0, -256.0, 32.0])
SCENES = ("room", "corridor", "plane", "far_corridor")
AXIS = np.array([1.0, 0.0, 0.0])  # of both corridors
VARIANTS = (False, True)          # noisy?
SIGMA, SIGMA_N = 0.01, 0.01       # metres on the points, radians on the normals
N_TARGET = 3000
SEEDS = {"room": 11, "corridor": 12, "plane": 13, "far_corridor": 12}  # the far corridor IS the corridor, moved
R = 0.25                          # max_correspondence_distance of every case
# the pose a registration must find, carried out about the scene's middle: no motion of that middle along the corridor
GT_LOCAL = isr.rigid((0.2, -0.3, 0.4), (0.0, 0.03, -0.02))
STEP_SIZES = tuple(sorted(set(rr.STEP_SIZES) | {1, 255, 256, 257}))
# what the expected verdicts are, as indices into eigenvalues: translation values ascend, so dropped ones come first
EXPECTED = {"room": (), "corridor": (3,), "plane": (0, 3, 4), "far_corridor": (3,)}


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def _draw(rng, surfaces, n, noisy):
    """n points dealt to the surfaces in turn, their normals, both perturbed when noisy"""
    ab = rng.uniform(0.0, 1.0, (n, 2))
    which = np.arange(n) % len(surfaces)
    S = np.array(surfaces, dtype=np.float64)[which]  # (n, 4, 3)
    pts = S[:, 0] + ab[:, 0:1] * S[:, 1] + ab[:, 1:2] * S[:, 2]
    nrm = S[:, 3].copy()
    noise, tilt = rng.normal(0.0, SIGMA, (n, 3)), rng.normal(0.0, SIGMA_N, (n, 3))
    if noisy:
        pts = pts + noise
        nrm = nrm + np.cross(tilt, nrm)
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts, nrm


def scene_middle(name) -> np.ndarray:
    S = np.array(SURFACES[name], dtype=np.float64)
    corners = np.concatenate([S[:, 0], S[:, 0] + S[:, 1] + S[:, 2]])
    mid = 0.5 * (corners.min(axis=0) + corners.max(axis=0))
    return mid + FAR_SHIFT if name == "far_corridor" else mid


def ground_truth(name) -> np.ndarray:
    return isr.about(scene_middle(name), GT_LOCAL)


class Scene(NamedTuple):
    tgt: np.ndarray
    tgt_nrm: np.ndarray
    second: np.ndarray  # a second draw of the same surfaces (4200 points): sources are its prefixes moved by the inverse of the ground truth


@functools.lru_cache(maxsize=None)
def scene(name, noisy) -> Scene:
    rng = np.random.default_rng(SEEDS[name] + (1000 if noisy else 0))
    tgt, nrm = _draw(rng, SURFACES[name], N_TARGET, noisy)
    second, _ = _draw(rng, SURFACES[name], max(STEP_SIZES), noisy)
    if name == "far_corridor":
        tgt, second = tgt + FAR_SHIFT, second + FAR_SHIFT
    return Scene(_frozen(tgt), _frozen(nrm), _frozen(second))


@functools.lru_cache(maxsize=None)
def source(name, noisy, n) -> np.ndarray:
    inv = np.linalg.inv(ground_truth(name))
    return _frozen(scene(name, noisy).second[:n] @ inv[:3, :3].T + inv[:3, 3])


LOOP_N = 2125  # the source of the registration cases


@functools.lru_cache(maxsize=None)
def step_record(name, noisy, n, storage) -> np.ndarray:
    s = scene(name, noisy)
    rec = rr.step_record(rr.POINT_TO_PLANE, rr.L2, 0.0, source(name, noisy, n), s.tgt, s.tgt_nrm, np.eye(4), R, storage)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def reference_analysis(name, noisy, n, storage, min_rot, min_trans) -> Analysis:
    c0 = cloud_center(source(name, noisy, n), storage)
    return analyse(step_record(name, noisy, n, storage), np.eye(4), c0, min_rot, min_trans)


@functools.lru_cache(maxsize=None)
def reference_registration(name, noisy, storage, min_rot, min_trans, max_iter=12) -> dict:
    s = scene(name, noisy)
    return register(source(name, noisy, LOOP_N), s.tgt, s.tgt_nrm, R, storage, min_rot, min_trans, max_iter=max_iter, rel_fitness=0.0, rel_rmse=0.0)


def centre_motion(T, T0, c0) -> np.ndarray:
    """how far the scan's centre has moved between the poses T0 and T"""
    return (np.asarray(T)[:3, :3] @ c0 + np.asarray(T)[:3, 3]) - (np.asarray(T0)[:3, :3] @ c0 + np.asarray(T0)[:3, 3])


def pose_error(T, name, c0):
    """(along the axis, across it, angle) of T against the scene's ground truth, the translation taken at the scan's centre"""
    G = ground_truth(name)
    d = centre_motion(T, G, c0)
    along = float(d @ AXIS)
    across = float(np.linalg.norm(d - along * AXIS))
    Rd = np.asarray(T)[:3, :3] @ G[:3, :3].T
    angle = math.acos(min(1.0, max(-1.0, (np.trace(Rd) - 1.0) / 2.0)))
    return along, across, angle


# ---------------------------------------------------------------------------------------------------------------- recorded premises
# measured by tests/test_degeneracy_restatement_cpu.py over every scene, variant and storage at LOOP_N points (printed there):
#   rotation (m^2):  largest value of a direction that must be dropped DROP_ROT, smallest of one that must be kept KEEP_ROT
#   translation:     DROP_TRANS, KEEP_TRANS
# The thresholds of every test are the geometric means; the CPU test asserts at least 10x on either side.
DROP_ROT, KEEP_ROT = 2.74e-4, 0.311      # measured 2.7357e-04 (noisy plane, about its normal) and 0.31120 (noisy room)
DROP_TRANS, KEEP_TRANS = 1.08e-4, 0.239  # measured 1.0750e-04 (noisy plane) and 0.23907 (noisy room)
MIN_ROT = math.sqrt(DROP_ROT * KEEP_ROT)        # 9.23e-3 m^2
MIN_TRANS = math.sqrt(DROP_TRANS * KEEP_TRANS)  # 5.08e-3
# the eigen-decomposition against numpy.linalg.eigh over every block of every scene: |lambda - eigh| and |A V - V Lambda|_F are at most
# EIGEN_K eps |A|_F; measured worst 1.94, times 4
EIGEN_K_MEASURED, EIGEN_K = 1.94, 7.76
# corridor against far corridor, normalised eigenvalues after re-centring: measured 1.97e-6 (f32 storage: the far scene's coordinates
# carry 2^-14 m) and 5.8e-11 (f64), times 4
SHIFT_TOL = {F32: 8e-6, F64: 2.4e-10}
# the noisy corridor, 12 updates from the identity: the ordinary loop carries the scan's centre 42.6 mm along the axis (recorded: more
# than 20 mm); the constrained loop 0.2 mm -- the dropped eigenvector is the axis up to the normals' noise -- measured 2.0e-4 m, times 4
SLIDE_MIN, ALONG_TOL = 0.02, 8e-4
# ... and leaves the pose within the parity tolerance of SURVEY.md 8c for f32 storage of the ground truth across the axis and in angle
# (measured 1.0e-4 m, 4.2e-4 rad; the scans' own noise, sigma / sqrt(n), is what is left in either storage)
TRUTH_TOL = 1e-3
