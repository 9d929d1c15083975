"""Inputs for the operations that place a cloud with a pose and then bin it into voxels (cloud_kernels.hpp: transform_kernel,
carve_rays_kernel, dense_insert_kernel, dense_probe_kernel, dense_carve_kernel, the overlap; map_kernels.hpp: pm_place_kernel,
pm_carve_rays_kernel), and the placement itself restated in numpy.

The device and the oracle place a point as ((m0 * x + m1 * y) + m2 * z) + m3, one rounding per operation.  A placement that fuses a
multiply-add, sums a row in another order or rounds once differs from that by an ulp or two -- which shows in a voxel key only when the
placed point lies within an ulp of a voxel face.  The clouds here are AIMED at faces: a target position q with one coordinate on a face
k * v is taken back through the inverse pose, p = place(inv(T), q), so that place(T, p) lands within a few ulp of the face, on either
side.  tests/test_placed_binning_cpu.py proves on the CPU that these inputs tell the placements apart (the oracle's own results change
when a once-rounded placement is substituted); tests/test_placed_binning_gpu.py holds the device to the oracle on them, exactly.

numpy only: nothing here needs a GPU or the oracle.
"""
from __future__ import annotations

import functools
import math

import numpy as np

VOXELS = (0.1, 0.25)


# ---- the placement -------------------------------------------------------------------------------------------------------------------
def place(T, P):
    """T (p, 1) for every row of P in the order of place_point (cloud_kernels.hpp) and orc_transform_points: one rounding per operation"""
    T = np.asarray(T, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.column_stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)])


def rotate(T, N):
    """T (n, 0) for every row of N in the order of rotate_normal and orc_transform_normals"""
    T = np.asarray(T, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.column_stack([(T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z for r in range(3)])


def place_rounded_once(T, P):
    """the same placement with the row summed in extended precision and rounded to double once: what a fused multiply-add chain is like"""
    L = np.longdouble
    T = np.asarray(T, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    x, y, z = P[:, 0].astype(L), P[:, 1].astype(L), P[:, 2].astype(L)
    return np.column_stack([(L(T[r, 0]) * x + L(T[r, 1]) * y + L(T[r, 2]) * z + L(T[r, 3])).astype(np.float64) for r in range(3)])


def storage(x, prec):
    """what a cloud of the given storage holds of the doubles handed to it"""
    if x is None:
        return None
    x = np.asarray(x, dtype=np.float64)
    return x if prec == "f64" else x.astype(np.float32).astype(np.float64)


def keys(P, voxel):
    """getVoxelIdx(p, 1 / v) (VoxelHashMap.hpp:47-50): floor of the product with the rounded reciprocal, per axis"""
    return np.floor(np.asarray(P, dtype=np.float64) * (1.0 / voxel)).astype(np.int64)


def make_pose(t, rpy_deg):
    """translation o Rz(yaw) Ry(pitch) Rx(roll), angles in degrees (open3d_slam_amd.synthetic.make_pose, restated to keep this numpy only)"""
    a, b, g = (math.radians(v) for v in rpy_deg)
    sa, ca, sb, cb, sg, cg = math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g)
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = t
    return T


def inverse(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


# a general pose: all nine rotation entries are non-zero
POSE = make_pose((1.5, -0.7, 0.2), (2.0, -1.0, 30.0))
# the carving's pose: the same rotation, the sensor on a corner of both grids (multiples of 0.5, exact in binary), so that a ray in one of
# the sensor's coordinate planes runs ALONG a voxel face and the side it samples hangs on the last bits of the placed return
CARVE_POSE = make_pose((1.5, -0.5, 0.5), (2.0, -1.0, 30.0))
CARVE_RMAX = 6.5      # the builder's cropping volume around the sensor: map points beyond it are not carved
CARVE_PARAMS = (dict(), dict(max_length=3.0, truncation=0.3, min_dot=0.8))  # default and non-default (the voxel comes on top)
DENSE_CARVE_PARAMS = (dict(), dict(radius=0.03, max_length=6.0, truncation=0.3))  # of dense_map_carve, likewise
INSERT_RMAX = 7.0     # the cropping volume of map_insert_scan around POSE's translation: placed points beyond it pass through


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _clusters(rng, n_anchor, voxel, sizes):
    """target positions in clusters that share one voxel face: per anchor a face coordinate k * voxel on a random axis and 1 ... `sizes`
    members spread over the interior of one voxel in the two other axes.  Returns (positions, anchor of every position, axis of every anchor)."""
    base = np.floor(rng.uniform(-8.0, 8.0, (n_anchor, 3)) / voxel)  # voxel indices
    axis = rng.integers(0, 3, n_anchor)
    cnt = rng.integers(1, sizes + 1, n_anchor)
    owner = np.repeat(np.arange(n_anchor), cnt)
    q = (base[owner] + rng.uniform(0.1, 0.9, (len(owner), 3))) * voxel
    q[np.arange(len(owner)), axis[owner]] = base[owner, axis[owner]] * voxel  # on the face, as the double product k * v
    return q, owner, axis


@functools.lru_cache(maxsize=None)
def face_aimed(voxel, seed=1, n_anchor=1350, sizes=5):
    """(source points p, unit normals, aimed positions q, anchor of every point, face axis of every anchor): about 4000 points with
    place(POSE, p) within a few ulp of q, each q on a face of the `voxel` grid, in clusters of 1 ... 5 per voxel (so that min_points = 3
    has voxels to find)"""
    rng = np.random.default_rng([seed, int(round(voxel * 1000))])
    q, owner, axis = _clusters(rng, n_anchor, voxel, sizes)
    p = place(inverse(POSE), q)
    return p, _unit(rng.normal(size=p.shape)), q, owner, axis


@functools.lru_cache(maxsize=None)
def overlap_target(voxel):
    """about 4000 target points for the overlap with face_aimed(voxel) placed by POSE: per anchor of two thirds of the source's clusters
    0 ... 4 points ON the cluster's face (lattice) and 0 ... 2 just below it (near-lattice: the voxel under the face), the other two
    coordinates inside the cluster's voxel; and a block far away that shares no voxel with anything."""
    rng = np.random.default_rng([7, int(round(voxel * 1000))])
    _, _, q, owner, axis = face_aimed(voxel)
    n_anchor = len(axis)
    first = np.searchsorted(owner, np.arange(n_anchor))  # a member of every cluster
    out = []
    for a in rng.permutation(n_anchor)[: 2 * n_anchor // 3]:
        ax = int(axis[a])
        lo = np.floor(q[first[a]] / voxel + 1e-6)  # the voxel on the upper side of the face
        for below, cnt in ((False, rng.integers(0, 5)), (True, rng.integers(0, 3))):
            t = (lo + rng.uniform(0.1, 0.9, (cnt, 3))) * voxel
            t[:, ax] = q[first[a], ax] - (1e-9 if below else 0.0)
            out.append(t)
    out.append(rng.uniform(100.0, 104.0, (600, 3)))
    t = np.vstack(out)
    return t[rng.permutation(len(t))]


@functools.lru_cache(maxsize=None)
def dense_scene(voxel):
    """(points, normals) of about 3000 points aimed at faces as face_aimed, of another seed: what the dense map takes with POSE"""
    p, n = face_aimed(voxel, seed=2, n_anchor=1000)[:2]
    return p, n


@functools.lru_cache(maxsize=None)
def carve_scene():
    """(map points, map normals, raw scan in the sensor frame) of the carving with CARVE_POSE: about 2000 returns at 0.25 ... 7.5 m (1 ... 75
    samples at voxel 0.1, 1 ... 30 at 0.25: whole and partial batches of 8), most of them in one of the sensor's coordinate planes or on an axis
    through it; a map of 6000 points, half of them around the returns and half anywhere, and 400 clutter points in free space hugging, on
    either side, the planes the rays run in."""
    rng = np.random.default_rng(23)
    s = CARVE_POSE[:3, 3]
    n = 2000
    d = rng.normal(size=(n, 3))
    kind = rng.uniform(size=n)
    ax = rng.integers(0, 3, n)
    in_plane, on_axis = kind < 0.6, (kind >= 0.6) & (kind < 0.7)
    d[in_plane, ax[in_plane]] = 0.0
    d[on_axis] = 0.0
    d[on_axis, ax[on_axis]] = rng.choice([-1.0, 1.0], int(on_axis.sum()))
    d = _unit(d)
    r = rng.uniform(0.25, 7.5, n)
    q = s + r[:, None] * d  # (a zero component of d leaves the sensor's coordinate as it is, bit for bit)
    scan = place(inverse(CARVE_POSE), q)
    near = q[rng.integers(0, n, 3000)] + rng.normal(scale=0.03, size=(3000, 3))
    anywhere = s + rng.uniform(-8.0, 8.0, (3000, 3))
    k = rng.choice(np.flatnonzero(in_plane), 400)
    clutter = s + (rng.uniform(0.1, 0.9, 400) * r[k])[:, None] * d[k] + rng.uniform(-0.02, 0.02, (400, 3))
    clutter[np.arange(400), ax[k]] = s[ax[k]] + rng.uniform(-0.04, 0.04, 400)
    mp = np.vstack([near, anywhere, clutter])
    mp = mp[rng.permutation(len(mp))]
    return mp, _unit(rng.normal(size=mp.shape)), scan


def insert_scans(voxel):
    """two clouds with normals for two insertions into one map with POSE: face-aimed ones, the second with the carving scene's map taken
    into POSE's sensor frame on top (so that the map the insertions build has something where the carving scene's rays run)"""
    (a, an), (b, bn) = (face_aimed(voxel, seed=s, n_anchor=1000)[:2] for s in (3, 4))
    mp, mn, _ = carve_scene()
    return [(a, an), (np.vstack([b, place(inverse(POSE), mp)]), np.vstack([bn, mn]))]


def dense_voxels(W, N, voxel):
    """VoxelizedPointCloud of the placed points W (normals N or None), restated: (packed keys ascending -- the order of
    dense_map_to_cloud --, point counts, mean positions, mean normals or None, position of every voxel in first-occurrence order --
    the order of the oracle's dense_fuse)"""
    k = keys(W, voxel) + (1 << 20)
    packed = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    uniq, first, inv, cnt = np.unique(packed, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    mean = lambda X: None if X is None else _group_sum(X, inv, len(uniq)) / cnt[:, None]
    return uniq, cnt, mean(W), mean(N), np.argsort(first, kind="stable")


def _group_sum(X, inv, m):
    out = np.zeros((m, 3))
    np.add.at(out, inv, X)
    return out
