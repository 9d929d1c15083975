"""o3ds_segment_plane restated in numpy, and the cases the tests share.  Nothing here uses the device or a search structure.

What the result is specified to be (include/o3ds_backend.h), all of it in f64 on the stored coordinates, every operation rounded on its
own (numpy fuses nothing):
  * SUM ORDER (`ordered_sum`): m terms in 256 chunks of len = max(1, ceil(m / 256)) consecutive terms, each chunk added up one term after
    the other from +0.0, then a halving tree over the 256 chunk sums (v[t] += v[t + s] for t < s; s = 128, 64, ..., 1).  A term of a point
    that is no inlier is +0.0;
  * SAMPLE t: the points mix(seed + (ransac_n t + j + 1) golden) mod n, j < ransac_n (`draw`; with replacement);
  * HYPOTHESIS: ransac_n == 3 the triangle's plane (`triangle_planes`), else `fit_plane` over the sample in sample order; skipped iff all
    four coefficients are exactly 0;
  * EVALUATION: dist = |((a x + b y) + c z) + d|, inlier iff dist < threshold; count, error = sum of dist; fitness = count / n,
    inlier_rmse = error / sqrt(count) or 0 (`evaluate`, by blocks of hypotheses);
  * WINNER: read in index order from (fitness 0, rmse 0); t replaces the best iff its fitness is greater, or equal and its rmse strictly
    smaller (`winner`);
  * the inliers of the winning plane in cloud order, and `fit_plane` of them: centroid, six moments about it, the largest of the three
    determinants picks the axis (ties x, then y), the normal is normalised, d = -n . centroid;
  * no winner: zeros, best_t -1, no inliers.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import neighbor_restatement as nb
import normals_restatement as nr

F32, F64 = nb.F32, nb.F64
STORAGES = nb.STORAGES
to_storage = nb.to_storage

CHUNKS = 256
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BATCH = 1024  # hypotheses per device batch (no result depends on it; the cases cross it)


def mix(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, ransac_n, num_iterations, n) -> np.ndarray:
    """(num_iterations, ransac_n) point indices"""
    t = np.arange(num_iterations, dtype=np.uint64)[:, None]
    j = np.arange(ransac_n, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        arg = np.uint64(seed % (1 << 64)) + (np.uint64(ransac_n) * t + j + np.uint64(1)) * GOLDEN
    return (mix(arg) % np.uint64(n)).astype(np.int64)


def chunk_len(m) -> int:
    return max(1, -(-int(m) // CHUNKS))


def ordered_sum(v) -> np.ndarray:
    """the sum over the last axis in the documented order"""
    v = np.asarray(v, dtype=np.float64)
    m = v.shape[-1]
    ln = chunk_len(m)
    pad = np.zeros(v.shape[:-1] + (CHUNKS * ln,))
    pad[..., :m] = v
    pad = pad.reshape(v.shape[:-1] + (CHUNKS, ln))
    acc = np.zeros(v.shape[:-1] + (CHUNKS,))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(ln):
            acc = acc + pad[..., k]
        s = CHUNKS // 2
        while s >= 1:
            acc = acc[..., :s] + acc[..., s:2 * s]
            s //= 2
    return acc[..., 0]


def _normalised(a, b, c, cx, cy, cz):
    """(a, b, c) / norm and d = -((a cx + b cy) + c cz); the zero plane where norm == 0"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = np.sqrt((a * a + b * b) + c * c)
        zero = norm == 0.0
        safe = np.where(zero, 1.0, norm)
        a, b, c = a / safe, b / safe, c / safe
        d = -((a * cx + b * cy) + c * cz)
    out = np.stack([a, b, c, d], axis=-1)
    out[zero] = 0.0
    return out


def triangle_planes(p0, p1, p2) -> np.ndarray:
    """[O3D] ComputeTrianglePlane for (T, 3) arrays of points: (T, 4)"""
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = p1 - p0, p2 - p0
        a = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        b = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        c = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return _normalised(a, b, c, p0[:, 0], p0[:, 1], p0[:, 2])


def fit_plane(x, y, z, inl, k) -> np.ndarray:
    """[O3D] GetPlaneFromPoints of the points flagged by inl among the m = x.shape[-1] terms; k = their number.  Leading axes batch."""
    k = np.asarray(k, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cx = ordered_sum(np.where(inl, x, 0.0)) / k
        cy = ordered_sum(np.where(inl, y, 0.0)) / k
        cz = ordered_sum(np.where(inl, z, 0.0)) / k
        rx, ry, rz = x - cx[..., None], y - cy[..., None], z - cz[..., None]
        xx, xy, xz = (ordered_sum(np.where(inl, rx * q, 0.0)) for q in (rx, ry, rz))
        yy, yz = (ordered_sum(np.where(inl, ry * q, 0.0)) for q in (ry, rz))
        zz = ordered_sum(np.where(inl, rz * rz, 0.0))
        det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
        ax = (det_x >= det_y) & (det_x >= det_z)
        ay = ~ax & (det_y >= det_z)
        t_xy, t_xz, t_yz = xz * yz - xy * zz, xy * yz - xz * yy, xy * xz - yz * xx
        a = np.where(ax, det_x, np.where(ay, t_xy, t_xz))
        b = np.where(ax, t_xy, np.where(ay, det_y, t_yz))
        c = np.where(ax, t_xz, np.where(ay, t_yz, det_z))
    return _normalised(a, b, c, cx, cy, cz)


def fit_axis(x, y, z) -> str:
    """which determinant the fit of all the given points picks"""
    cx, cy, cz = (ordered_sum(q) / len(q) for q in (x, y, z))
    rx, ry, rz = x - cx, y - cy, z - cz
    xx, xy, xz, yy, yz, zz = (ordered_sum(p * q) for p, q in ((rx, rx), (rx, ry), (rx, rz), (ry, ry), (ry, rz), (rz, rz)))
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    return "x" if det_x >= det_y and det_x >= det_z else "y" if det_y >= det_z else "z"


def hypotheses(p, ransac_n, num_iterations, seed) -> np.ndarray:
    """(num_iterations, 4) planes of the stored points p (n, 3)"""
    if num_iterations == 0:
        return np.zeros((0, 4))
    s = p[draw(seed, ransac_n, num_iterations, len(p))]  # (T, ransac_n, 3)
    if ransac_n == 3:
        return triangle_planes(s[:, 0], s[:, 1], s[:, 2])
    return fit_plane(s[..., 0], s[..., 1], s[..., 2], np.ones(s.shape[:2], bool), float(ransac_n))


def distances(planes, p) -> np.ndarray:
    """(T, n)"""
    a, b, c, d = (planes[:, k:k + 1] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((a * p[None, :, 0] + b * p[None, :, 1]) + c * p[None, :, 2]) + d)


def evaluate(planes, p, thr, block=64):
    """(count (T,) int64, error (T,)) of every plane, by blocks of hypotheses"""
    T = len(planes)
    count, error = np.zeros(T, np.int64), np.zeros(T)
    for b0 in range(0, T, block):
        dist = distances(planes[b0:b0 + block], p)
        with np.errstate(invalid="ignore"):
            inl = dist < thr
        count[b0:b0 + block] = inl.sum(axis=1)
        error[b0:b0 + block] = ordered_sum(np.where(inl, dist, 0.0))
    return count, error


def score(count, error, n):
    """(fitness, inlier_rmse) of one hypothesis"""
    return float(count) / float(n), (float(error) / float(np.sqrt(np.float64(count))) if count > 0 else 0.0)


def winner(planes, count, error, n):
    """the serial rule: (best_t or -1, fitness, inlier_rmse, n_degenerate)"""
    best_t, best_f, best_r, n_deg = -1, 0.0, 0.0, 0
    for t in range(len(planes)):
        if not planes[t].any():  # all four exactly 0 (a NaN is not)
            n_deg += 1
            continue
        f, r = score(count[t], error[t], n)
        if f > best_f or (f == best_f and r < best_r):
            best_t, best_f, best_r = t, f, r
    return best_t, best_f, best_r, n_deg


class Result(NamedTuple):
    plane: np.ndarray        # (4,) the refit
    best_plane: np.ndarray   # (4,)
    fitness: float
    inlier_rmse: float
    n_inliers: int
    best_t: int
    n_degenerate: int
    inliers: np.ndarray      # (n_inliers,) int64, ascending
    planes: np.ndarray       # (T, 4) every hypothesis
    count: np.ndarray        # (T,)
    error: np.ndarray        # (T,)


def segment(points, thr, ransac_n, num_iterations, seed, storage) -> Result:
    p = to_storage(points, storage)
    n = len(p)
    assert 3 <= ransac_n <= 8 and n >= ransac_n
    planes = hypotheses(p, ransac_n, num_iterations, seed)
    count, error = evaluate(planes, p, thr)
    best_t, f, r, n_deg = winner(planes, count, error, n)
    if best_t < 0:
        return Result(np.zeros(4), np.zeros(4), 0.0, 0.0, 0, -1, n_deg, np.zeros(0, np.int64), planes, count, error)
    best = planes[best_t]
    with np.errstate(invalid="ignore"):
        inl = distances(best[None], p)[0] < thr
    plane = fit_plane(p[:, 0], p[:, 1], p[:, 2], inl, float(inl.sum()))
    return Result(plane, best.copy(), f, r, int(inl.sum()), best_t, n_deg, np.flatnonzero(inl), planes, count, error)


# ---------------------------------------------------------------------------------------------------------------- clouds
_frozen = nb._frozen


@functools.lru_cache(maxsize=None)
def sheets() -> np.ndarray:
    """two parallel 8 x 8 sheets of integer points one unit apart (z = 0 and z = 1) and eight integer points above them, shuffled: every
    coordinate, cross product and distance is exact in both storages"""
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    lo, hi = np.column_stack([g, np.zeros(64)]), np.column_stack([g, np.ones(64)])
    top = np.column_stack([np.arange(8.0), np.arange(8.0)[::-1], 3.0 + np.arange(8.0) % 3])
    return _frozen(np.vstack([lo, hi, top])[np.random.default_rng(91).permutation(136)])


SHEET_SPACING = 1.0


def _rot(axis):
    """the rotation that takes z to `axis`, after a tilt of a few degrees"""
    from open3d_slam_amd import synthetic as syn

    tilt = syn.rpy_to_R(np.deg2rad(4.0), np.deg2rad(-6.0), np.deg2rad(20.0))
    perm = {"z": np.eye(3), "x": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
            "y": np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])}[axis]
    return perm @ tilt


@functools.lru_cache(maxsize=None)
def scan(n_az=64) -> np.ndarray:
    """the synthetic VLP-16 scan (16 x n_az points, sensor frame): the floor 1.5 m below the sensor, the room's walls, the cylinders;
    range noise 0.01 m"""
    from open3d_slam_amd import synthetic as syn

    return _frozen(syn.vlp16_scan(syn.make_scene(), np.eye(4), n_az=n_az))


@functools.lru_cache(maxsize=None)
def ground(axis) -> np.ndarray:
    """the 1024-point scan turned so that its floor's normal lies near `axis`, a few degrees off"""
    return _frozen(scan() @ _rot(axis).T)


@functools.lru_cache(maxsize=None)
def tilted_plane() -> np.ndarray:
    """2000 points of the plane z = 0.2 x - 0.1 y with 0.02 m of noise"""
    rng = np.random.default_rng(92)
    xy = rng.uniform(-6.0, 6.0, (2000, 2))
    return _frozen(np.column_stack([xy, 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + rng.normal(0.0, 0.02, 2000)]))


@functools.lru_cache(maxsize=None)
def offset_plane() -> np.ndarray:
    """the same 1e3 m from the origin on every axis: an f32 ulp there is 6e-5 m, and the threshold 0.02 m cuts through the noise"""
    return _frozen(tilted_plane() + 1.0e3)


@functools.lru_cache(maxsize=None)
def collinear() -> np.ndarray:
    """100 integer points of the line (t, 2 t, 3 t), shuffled: every cross product is exactly zero in both storages"""
    t = np.arange(100.0)
    return _frozen(np.column_stack([t, 2.0 * t, 3.0 * t])[np.random.default_rng(93).permutation(100)])


@functools.lru_cache(maxsize=None)
def duplicates() -> np.ndarray:
    return _frozen(np.tile([[1.25, -2.5, 3.0]], (70, 1)))


@functools.lru_cache(maxsize=None)
def non_finite() -> np.ndarray:
    """300 points of the ragged sheet, six with a NaN coordinate and four with an infinite one"""
    t = np.array(nb.nan_target())
    t[40, 0] = np.inf
    t[41, 2] = -np.inf
    t[42] = [np.inf, -np.inf, 1.0]
    t[150, 1] = -np.inf
    return _frozen(t)


class Case(NamedTuple):
    name: str
    cloud: object     # () -> (n, 3)
    params: tuple     # ((distance_threshold, ransac_n, num_iterations, seed), ...)


def _prefix(cloud, n):
    return lambda: cloud()[:n]


SECOND_TERM = (256, 257, 258)  # around the n that first gives a chunk of the sum order a second term
CASES = tuple(
    [Case(f"size-{n}", _prefix(nr.ragged_cloud, n), ((0.1, 3, 64, 1),)) for n in (3, 63, 64, 65) + SECOND_TERM] +
    [Case("size-4097", nr.ragged_cloud, ((0.1, 3, 65, 2),)),
     Case("iterations", _prefix(nr.ragged_cloud, 257), tuple((0.1, 3, T, 3) for T in (1, 63, 64, 65, BATCH + 1))),
     Case("sample-size", _prefix(nr.ragged_cloud, 257), ((0.1, 4, 65, 4), (0.1, 8, 65, 5), (0.1, 8, BATCH + 1, 6))),
     Case("sheets", sheets, ((SHEET_SPACING, 3, 192, 7), (1.5, 3, 192, 7), (SHEET_SPACING, 4, 65, 8))),
     Case("ground-x", functools.partial(ground, "x"), ((0.05, 3, 128, 9), (0.05, 4, 64, 9))),
     Case("ground-y", functools.partial(ground, "y"), ((0.05, 3, 128, 10), (0.05, 8, 64, 10))),
     Case("ground-z", functools.partial(ground, "z"), ((0.05, 3, 128, 11), (0.05, 3, 128, 12))),
     Case("collinear", collinear, ((0.5, 3, 65, 13),)),
     Case("duplicates", duplicates, ((0.5, 3, 65, 14), (0.5, 4, 65, 14))),
     Case("non-finite", non_finite, ((0.1, 3, 200, 15), (float("inf"), 3, 64, 15))),
     Case("offset", offset_plane, ((0.02, 3, 100, 16),)),
     Case("no-winner", _prefix(nr.ragged_cloud, 65), ((0.0, 3, 64, 17), (-1.0, 3, 64, 17), (float("nan"), 3, 64, 17), (0.1, 3, 0, 17)))])
TIE_PARAMS = CASES[[c.name for c in CASES].index("sheets")].params[:2]


def case(name) -> Case:
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name: str, storage: str, params: tuple) -> Result:
    """the restated result of a case of CASES, computed once per process and never written to"""
    r = segment(case(name).cloud(), *params, storage)
    for a in (r.plane, r.best_plane, r.inliers, r.planes, r.count, r.error):
        a.setflags(write=False)
    return r


# the split through neighbors.SplitByPlane and the clustering of the rest: the 8192-point scan, the floor 1.5 m below the sensor
SPLIT_N_AZ = 512
SPLIT_PARAMS = (0.05, 3, 100, 0)  # distance_threshold (five times the range noise), ransac_n, num_iterations, seed
SPLIT_DBSCAN = (7.0, 5)           # eps, min_points: the rings on the floor lie up to 4.9 m apart, so only a large eps joins the whole scan
SPLIT_REST_CLUSTERS = 8           # of the rest at those (test_plane_restatement_cpu.py confirms both counts by brute force)
