"""The step that turns a point-to-point record into a pose (icp_kernels.hpp umeyama_from_record / svd3_jacobi, which every ICP form and
every RANSAC hypothesis goes through), restated in numpy with no device and nothing of the oracle's SVD.

  umeyama_reference  Eigen::umeyama(with_scaling = false) as Eigen forms it -- means, DEMEANED covariance, SVD with descending singular
                     values, the diag(1, 1, -1) rule, t = mu_q - R mu_p -- in np.longdouble, with a one-sided Jacobi SVD written out here.
  record_of          the 32-double point-to-point record of include/o3ds_backend.h from the pairs, every sum through math.fsum, in the frame
                     the device forms it in (coordinates relative to `pivot`).
  device_form        the header's documented formula (Sigma = rec / m - mu_q mu_p^T, then an SVD) in plain f64: a MODEL of the device
                     text that the CPU test uses to show which cases can tell the two forms apart.  No GPU test compares against it.
  check_update       the assertions a pose T is held to for one case (tests/test_point_to_point_update_gpu.py applies them to the
                     device's T, tests/test_point_to_point_restatement_cpu.py to device_form's).
  cases              the catalogue: pair sets (p, q) with the correspondence known by construction, on dyadic grids so that no input
                     depends on a machine's libm beyond a last place of a grid step.
"""
from __future__ import annotations

import functools
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
OFFSET = np.array([1.0e5, -2.0e5, 50.0])      # the offsets tests/test_icp_gpu.py::test_large_coordinates_and_exact_sums claims
OFFSET_NEAR = np.array([1.0e4, -2.0e4, 50.0])
PIVOT_STEP = 1024.0  # the device forms the record relative to the multiple of PIVOT_STEP nearest (per axis) to T applied to source point 0
# assertion 6: angle(R, R_ref) <= K 2^-53 (|mu_q| |mu_p| + |Sigma|_F) / g.  K = 3 x the largest ratio device_form shows on the near-origin
# cases, rounded up: measured 46.0 on generic_rot1deg_129, whose sigma_2 and sigma_3 lie 5 % apart (LAPACK's U and V each lose
# eps sigma / (sigma_2 - sigma_3), and not all of it cancels in U V^T); every other case stays below 3.
# tests/test_point_to_point_restatement_cpu.py asserts 3 x the maximum <= K.
K_BOUND = 140.0
TOL_UNIT = 1e-12   # |R^T R - I|, |det R - 1|: what tests/test_place_recognition_gpu.py holds hypotheses to
TOL_COST = 1e-9    # least-squares cost where R is not unique (same file)
TOL_PARITY = {"f64": 1e-6, "f32": 1e-3}  # SURVEY.md 8c, rad and m
UNIQUE_GAP = 1e-6  # R counts as unique iff g > UNIQUE_GAP sigma_1 (the exemption of tests/test_place_recognition_gpu.py)
ENVELOPE_EXTENT = 0.5  # m; parity is claimed for pair sets at least this large at coordinates up to 2.5e5 m


# ---- reference ------------------------------------------------------------------------------------------------------------------------
def _svd3_ld(A):
    """one-sided (Hestenes) Jacobi SVD of a 3x3 in longdouble: (column norms descending, the rotated columns, V).  A V = [a0 a1 a2],
    the a_k mutually orthogonal; nothing is normalised here (a vanishing column stays a vanishing column)."""
    a = np.array(A, dtype=LD).copy()
    v = np.eye(3, dtype=LD)
    tol = LD(4) * np.finfo(LD).eps
    for _ in range(200):  # (zeta may overflow to inf where gamma is all but zero: t = 0 then, as it should be)
        moved = False
        for i, j in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = a[:, i] @ a[:, i], a[:, j] @ a[:, j], a[:, i] @ a[:, j]
            if gamma == 0 or abs(gamma) <= tol * np.sqrt(alpha * beta):
                continue
            moved = True
            zeta = (beta - alpha) / (LD(2) * gamma)
            with np.errstate(over="ignore"):
                t = (LD(1) if zeta >= 0 else LD(-1)) / (abs(zeta) + np.sqrt(LD(1) + zeta * zeta))
            c = LD(1) / np.sqrt(LD(1) + t * t)
            s = c * t
            for m in (a, v):
                x, y = m[:, i].copy(), m[:, j].copy()
                m[:, i], m[:, j] = c * x - s * y, s * x + c * y
        if not moved:
            break
    n = np.sqrt(np.sum(a * a, axis=0))
    order = np.argsort(-n, kind="stable")
    return n[order], a[:, order], v[:, order]


def _unit_orthogonal_to(u):
    k = int(np.argmin(np.abs(u)))
    w = -u[k] * u
    w[k] += LD(1)
    return w / np.sqrt(w @ w)


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def umeyama_reference(p, q) -> dict:
    """Eigen::umeyama(p, q, false) in longdouble.  Returns R, t (longdouble), T (f64 4x4), sigma (descending), s = sign of det U det V, the
    gap g = sigma_2 + s sigma_3 (R is the unique minimiser iff g > 0), Sigma, mu_p, mu_q."""
    p, q = np.asarray(p, dtype=LD).reshape(-1, 3), np.asarray(q, dtype=LD).reshape(-1, 3)
    m = LD(len(p))
    mu_p, mu_q = p.sum(0) / m, q.sum(0) / m
    S = (q - mu_q).T @ (p - mu_p) / m
    sig, a, v = _svd3_ld(S)
    # U: the normalised columns where they carry anything at all (one-sided Jacobi keeps small columns orthogonal to RELATIVE accuracy),
    # completed otherwise.  R = u1 v1^T + u2 v2^T + s u3 v3^T with det R = +1 does not depend on which completion is taken when g > 0.
    floor = np.finfo(LD).eps * LD(8) * (sig[0] if sig[0] > 0 else LD(1))
    u = np.zeros((3, 3), dtype=LD)
    u[:, 0] = a[:, 0] / sig[0] if sig[0] > floor else np.array([1, 0, 0], dtype=LD)
    u[:, 1] = a[:, 1] / sig[1] if sig[1] > floor else _unit_orthogonal_to(u[:, 0])
    u[:, 2] = a[:, 2] / sig[2] if sig[2] > floor else np.cross(u[:, 0], u[:, 1])
    s = LD(-1) if _det3(u) * _det3(v) < 0 else LD(1)
    R = np.outer(u[:, 0], v[:, 0]) + np.outer(u[:, 1], v[:, 1]) + s * np.outer(u[:, 2], v[:, 2])
    t = mu_q - R @ mu_p
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.astype(np.float64), t.astype(np.float64)
    return dict(R=R, t=t, T=T, sigma=sig, s=float(s), g=sig[1] + s * sig[2], Sigma=S, mu_p=mu_p, mu_q=mu_q)


def is_unique(ref) -> bool:
    return bool(ref["g"] > UNIQUE_GAP * ref["sigma"][0])


# ---- the record and the model of the device's formula ----------------------------------------------------------------------------------
def pivot_of(x) -> np.ndarray:
    """the frame of the record: per axis the multiple of PIVOT_STEP nearest to x = T s_0 (ties to even, as rint), 0 where x is not finite or
    beyond 2^30 m (tests/icp_search_restatement.py record_pivot is the same rule, held against o3ds_icp_accumulate's records)"""
    with np.errstate(invalid="ignore"):
        k = np.rint(np.asarray(x, dtype=np.float64) / PIVOT_STEP)
        return np.where(np.abs(k) < 2.0 ** 20, k * PIVOT_STEP, 0.0)


def record_of(p, q, pivot=(0.0, 0.0, 0.0)) -> np.ndarray:
    """[0..8] sum q_a p_b (row a, column b), [9..11] sum p, [12..14] sum q, [28] the pair count, [29] sum |p - q|^2, the rest 0; p and q
    relative to `pivot` (an exact shift in f64 for the catalogue's inputs); one rounding per product, the sums exact (math.fsum)"""
    c = np.asarray(pivot, dtype=np.float64)
    p, q = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    d = p - q
    p, q = p - c, q - c
    rec = np.zeros(32)
    for a in range(3):
        for b in range(3):
            rec[3 * a + b] = math.fsum((q[:, a] * p[:, b]).tolist())
        rec[9 + a] = math.fsum(p[:, a].tolist())
        rec[12 + a] = math.fsum(q[:, a].tolist())
    rec[28] = float(len(p))
    rec[29] = math.fsum(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).tolist())
    return rec


def device_form(rec, pivot=(0.0, 0.0, 0.0)) -> np.ndarray:
    """the documented formula in f64: Sigma = rec / m - mu_q mu_p^T from the record's sums, SVD (LAPACK), the sign rule,
    t = mu_q - R mu_p, then back from the record's frame: t + c - R c"""
    rec = np.asarray(rec, dtype=np.float64)
    c = np.asarray(pivot, dtype=np.float64)
    inv = 1.0 / rec[28]
    ms, mt = rec[9:12] * inv, rec[12:15] * inv
    S = rec[0:9].reshape(3, 3) * inv - np.outer(mt, ms)
    U, _, Vt = np.linalg.svd(S)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (mt - R @ ms) + (c - R @ c)
    return T


# ---- comparisons -----------------------------------------------------------------------------------------------------------------------
def angle(Ra, Rb) -> float:
    """the rotation angle of Ra Rb^T (from the antisymmetric part below 0.1 rad, where acos of the trace has no digits)"""
    D = np.asarray(Ra, dtype=LD)[:3, :3] @ np.asarray(Rb, dtype=LD)[:3, :3].T
    w = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]], dtype=LD) / LD(2)
    sn, cs = np.sqrt(w @ w), (D[0, 0] + D[1, 1] + D[2, 2] - LD(1)) / LD(2)
    return float(np.arctan2(sn, cs))


def _place(T, p):
    T, p = np.asarray(T, dtype=LD), np.asarray(p, dtype=LD).reshape(-1, 3)
    return p @ T[:3, :3].T + T[:3, 3]


def placement(Ta, Tb, p) -> float:
    """max_i |Ta p_i - Tb p_i| (not the difference of the translation columns, which at a 2e5 m lever is angle x 2e5 and says nothing)"""
    d = _place(Ta, p) - _place(Tb, p)
    return float(np.max(np.sqrt(np.sum(d * d, axis=1))))


def ls_cost(T, p, q) -> float:
    r = np.asarray(q, dtype=LD).reshape(-1, 3) - _place(T, p)
    return float(np.sum(r * r))


def ulp(x) -> float:
    return float(np.spacing(np.float64(abs(float(x)))))


def extent(p) -> float:
    """the diagonal of the pair set's source box (>= the lever of any point about the mean)"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def angle_bound_unit(ref, pivot_p=(0.0, 0.0, 0.0), pivot_q=(0.0, 0.0, 0.0)) -> float:
    """B / K: the first-order perturbation bound of the documented formula, 2^-53 (|mu_q| |mu_p| + |Sigma|_F) / g, the means taken in the
    frame in which the record is formed (an ICP pass shifts p and q by one pivot, a RANSAC hypothesis each by its own)"""
    mq, mp = ref["mu_q"] - np.asarray(pivot_q, dtype=LD), ref["mu_p"] - np.asarray(pivot_p, dtype=LD)
    return float(EPS * (np.sqrt(mq @ mq) * np.sqrt(mp @ mp) + np.sqrt(np.sum(ref["Sigma"] ** 2))) / ref["g"])


def check_update(T, case, ref=None, pivot=(0.0, 0.0, 0.0), storage="f64", pivot_q=None) -> dict:
    """Assertions 1-8 of the point-to-point update for one case (and the parity of the claimed envelope); returns the figures.  T maps
    case.p onto case.q; ref = umeyama_reference(case.p, case.q)."""
    p, q = case["p"], case["q"]
    ref = ref or umeyama_reference(p, q)
    T = np.asarray(T, dtype=np.float64)
    out = dict(case=case["name"])
    assert np.all(np.isfinite(T)), (case["name"], T)                                                     # 1
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), (case["name"], T[3])                             # 2
    R = T[:3, :3].astype(LD)
    out["ortho"] = float(np.max(np.abs(R.T @ R - np.eye(3))))
    out["det"] = float(abs(_det3(R) - 1))
    assert out["ortho"] <= TOL_UNIT, out                                                                # 3
    assert out["det"] <= TOL_UNIT, out                                                                  # 4
    mq = ref["mu_q"]
    out["mean"] = float(np.max(np.abs(R @ ref["mu_p"] + T[:3, 3].astype(LD) - mq)))
    out["mean_limit"] = 4.0 * ulp(np.max(np.abs(mq)))
    assert out["mean"] <= out["mean_limit"], out                                                        # 5
    if is_unique(ref):
        unit = angle_bound_unit(ref, pivot, pivot if pivot_q is None else pivot_q)
        out["angle"], out["B"] = angle(T, ref["R"]), K_BOUND * unit
        out["ratio"] = out["angle"] / unit
        out["placement"] = placement(T, _T_ld(ref), p)
        out["placement_limit"] = out["B"] * extent(p) + out["mean_limit"]
        assert out["angle"] <= out["B"], out                                                            # 6
        assert out["placement"] <= out["placement_limit"], out                                          # 7
        if case["envelope"]:                                                                            # b
            assert out["angle"] <= TOL_PARITY[storage] and out["placement"] <= TOL_PARITY[storage], out
    else:
        out["cost"], out["cost_ref"] = ls_cost(T, p, q), ls_cost(_T_ld(ref), p, q)
        assert abs(out["cost"] - out["cost_ref"]) <= TOL_COST, out                                      # 8
    return out


def _T_ld(ref):
    T = np.eye(4, dtype=LD)
    T[:3, :3], T[:3, 3] = ref["R"], ref["t"]
    return T


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def _grid(a, bits=20):
    return np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits


def rotation(axis, ang) -> np.ndarray:
    """Rodrigues, longdouble"""
    n = np.asarray(axis, dtype=LD)
    n = n / np.sqrt(n @ n)
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]], dtype=LD)
    a = LD(ang)
    return np.eye(3, dtype=LD) + np.sin(a) * Kx + (LD(1) - np.cos(a)) * (Kx @ Kx)


AXIS = (1.0, 2.0, 3.0)
SHIFT = np.array([0.3125, -0.1875, 0.125])  # on the grid
CYCLE = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # 120 deg about (1, 1, 1): q = (z, x, y), exact
QUARTER_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # 90 deg about z, exact


def _moved(p, R, t=SHIFT, bits=20):
    return _grid((np.asarray(p, dtype=LD) @ np.asarray(R, dtype=LD).T + np.asarray(t, dtype=LD)).astype(np.float64), bits)


def _orbit(base, swap):
    """the images of the base points under the eight sign changes and the exchange of the two coordinates `swap`"""
    out = []
    for b in base:
        for k in range(8):
            v = b * np.array([1 - 2 * (k & 1), 1 - (k & 2), 1 - ((k & 4) >> 1)], dtype=np.float64)
            out.append(v)
            w = v.copy()
            w[list(swap)] = v[list(swap)[::-1]]
            out.append(w)
    return np.array(out)


def _spread(rng, n, half, dmin):
    """n grid points, uniform in the box +-half, no two closer than dmin (drawn one after the other, a draw too close to an earlier one
    drawn again): what lets a correspondence pass find the pairs of a set that moves by less than dmin / 2"""
    half = np.asarray(half, dtype=np.float64)
    out = []
    while len(out) < n:
        c = _grid(rng.uniform(-half, half))
        if all(np.linalg.norm(c - o) >= dmin for o in out):
            out.append(c)
    return np.array(out)


SLAB_TURN, SLAB_SHIFT = math.radians(0.5), (0.25 * SHIFT[0], 0.25 * SHIFT[1], 0.0)


def _thin(xy, ratio):
    """the planar set xy as a slab, z = +-h in turn, and its copy turned in the plane: sigma_3 / sigma_1 of the demeaned Sigma is about
    h^2 / var ~ ratio.  h is dyadic (2^-60 steps): the slab lies below the 2^-20 grid of the other cases"""
    n = len(xy)
    h = float(np.round(math.sqrt(ratio * float(max(np.var(xy[:, 0]), np.var(xy[:, 1])))) * 2.0 ** 60) / 2.0 ** 60)
    z = h * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    p = np.c_[xy, z]
    q = np.c_[_moved(np.c_[xy, np.zeros(n)], rotation((0, 0, 1), SLAB_TURN), SLAB_SHIFT)[:, :2], z]
    return p, q


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name -> dict(name, p, q, unique (by construction; the CPU test holds the reference to it), offset (None = near the origin: every
    coordinate within 512 m), envelope (unique and inside the envelope parity is claimed for), radius (None, or the correspondence
    distance at which an ICP pass from the identity finds exactly these pairs: the computed-record cases))"""
    out = {}

    def add(name, p, q, unique=True, offset=None, radius=None):
        p, q = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
        if offset is not None:
            p, q = p + offset, q + offset  # (exact: grid coordinates of a few metres and offsets that are integers)
        out[name] = dict(name=name, p=p, q=q, unique=unique, offset=offset, radius=radius,
                         envelope=bool(unique and extent(p) >= ENVELOPE_EXTENT))

    rng = np.random.default_rng(20)
    g300 = _spread(rng, 300, (7.0, 7.0, 7.0), 1.0)
    g129 = _spread(rng, 129, (2.5, 2.5, 2.5), 0.6)
    # generic full rank, by rotation angle about a direction that is no axis
    add("generic_rot0_300", g300, g300 + 0.5 * SHIFT, radius=0.4)
    add("generic_rot1e-8_300", g300, _moved(g300, rotation(AXIS, 1e-8), bits=44))
    add("generic_rot1deg_129", g129, _moved(g129, rotation(AXIS, math.radians(1.0)), 0.25 * SHIFT), radius=0.25)
    add("generic_rot3deg_4", g300[:4], _moved(g300[:4], rotation(AXIS, math.radians(3.0))), radius=1.0)
    add("generic_rot90_300", g300, _moved(g300, rotation(AXIS, math.radians(90.0))))
    add("generic_rot179.9_300", g300, _moved(g300, rotation(AXIS, math.radians(179.9))))
    g1 = _grid(rng.uniform(-0.75, 0.75, (300, 3)))  # p = 9 g: the half turn about (1, 2, 2) / 3, (2 n n^T - 9 I) / 9, keeps it on the grid
    add("generic_rot180_300", 9.0 * g1, 2.0 * np.outer(g1 @ [1.0, 2.0, 2.0], [1.0, 2.0, 2.0]) - 9.0 * g1 + SHIFT)
    # reflections: q the mirror image of p (det Sigma < 0); with sigma_2 = sigma_3 no rotation is singled out
    box = _grid(rng.uniform(-1.0, 1.0, (300, 3)) * [7.0, 5.0, 3.0])
    add("reflection_300", box, box * [1.0, 1.0, -1.0] + SHIFT)
    sym = _orbit(_grid(rng.uniform(0.25, 3.0, (8, 3)) * [2.0, 1.0, 1.0]), (1, 2))  # cov = diag(a, b, b), exactly
    add("reflection_equal_128", sym, sym * [1.0, 1.0, -1.0] + SHIFT, unique=False)
    # equal singular values
    cube = 0.5 * np.array([[1 - 2 * (k & 1), 1 - (k & 2), 1 - ((k & 4) >> 1)] for k in range(8)], dtype=np.float64)
    add("isotropic_cube_exact_8", cube, cube @ CYCLE.T + SHIFT)  # Sigma = CYCLE / 4: all gammas exactly zero
    add("isotropic_cube_3deg_8", cube, _moved(cube, rotation(AXIS, math.radians(3.0)), 0.25 * SHIFT), radius=0.25)  # equal up to the grid: the stopping rule never fires
    disc = _orbit(_grid(rng.uniform(0.25, 3.0, (8, 3)) * [1.0, 1.0, 0.25]), (0, 1))  # cov = diag(a, a, b), a > b
    add("isotropic_pair_128", disc, disc @ QUARTER_Z.T + SHIFT)
    # coplanar: sigma_3 = 0 exactly, U completed by a cross product
    flat = _spread(rng, 300, (8.0, 8.0, 0.0), 0.6)
    add("coplanar_axis_300", flat, _moved(flat, rotation((0, 0, 1), SLAB_TURN), SLAB_SHIFT), radius=0.25)
    ab = _grid(rng.uniform(-2.0, 2.0, (300, 2)))
    tilt = np.c_[ab, -ab[:, 0] - ab[:, 1]]  # the plane x + y + z = 0; CYCLE turns it in itself
    add("coplanar_tilted_300", tilt, tilt @ CYCLE.T)
    for tag, ratio in (("1e-13", 1e-13), ("1e-14", 1e-14), ("1e-15", 1e-15)):  # either side of svd3_jacobi's `tiny` switch
        p, q = _thin(flat[:200, :2], ratio)
        add("near_coplanar_%s_200" % tag, p, q, radius=0.25)
    # rank one and less
    s = _grid(rng.uniform(-2.0, 2.0, 20))
    line = np.c_[s, 2.0 * s, 2.0 * s]
    add("collinear_20", line, line @ CYCLE.T + SHIFT, unique=False)
    add("two_pairs", g300[:2], g300[:2] + 0.5 * SHIFT, unique=False, radius=0.4)
    add("one_pair", g300[:1], g300[:1] + 0.5 * SHIFT, unique=False, radius=0.4)
    add("identical_20", np.tile(g300[5], (20, 1)), np.tile(g300[5] + 0.5 * SHIFT, (20, 1)), unique=False, radius=0.4)
    # small pair sets: a 20-pair patch of +-0.3 m (a small overlap) and a 3-pair triangle of 0.5 m sides (a RANSAC draw)
    small = rotation(AXIS, math.radians(2.0))
    patch = _spread(rng, 20, (0.3, 0.3, 0.3), 0.15)
    tri = _grid(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.25, 0.4375, 0.0625]]) + [1.0, -2.0, 0.5])
    pq = {"generic_rot3deg_300": (g300, _moved(g300, rotation(AXIS, math.radians(3.0))), None),
          "coplanar_axis_300": (out["coplanar_axis_300"]["p"], out["coplanar_axis_300"]["q"], 0.25),
          "patch_20": (patch, _moved(patch, small, 0.03125 * SHIFT), 0.05),
          "triangle_3": (tri, _moved(tri, small, 0.03125 * SHIFT), 0.125)}
    add("generic_rot3deg_300", *pq["generic_rot3deg_300"][:2])
    add("patch_20", *pq["patch_20"][:2], radius=pq["patch_20"][2])
    add("triangle_3", *pq["triangle_3"][:2], radius=pq["triangle_3"][2])
    # the same sets at the claimed offsets, translated on both sides
    for name, (p, q, radius) in pq.items():
        add(name + "_offset", p, q, offset=OFFSET, radius=radius)
    add("patch_20_offset_near", *pq["patch_20"][:2], offset=OFFSET_NEAR, radius=pq["patch_20"][2])
    return out


def near_origin(case) -> bool:
    return case["offset"] is None


def decoys(case, count=40, seed=77) -> np.ndarray:
    """target points that are no query's partner: at least 4 radii (and at least 1 m) from every p and q of the case, on the 2^-10 grid
    around the pair set"""
    rng = np.random.default_rng(seed)
    pts = np.vstack([case["p"], case["q"]])
    off = np.zeros(3) if case["offset"] is None else case["offset"]
    clear = max(4.0 * case["radius"], 1.0)
    lo, hi = pts.min(0) - off - 3.0 * clear, pts.max(0) - off + 3.0 * clear
    out = []
    while len(out) < count:
        c = _grid(rng.uniform(lo, hi), 10) + off
        if np.min(np.linalg.norm(pts - c, axis=1)) > clear * 1.01:
            out.append(c)
    return np.array(out)


# ---- RANSAC hypotheses ------------------------------------------------------------------------------------------------------------------
RANSAC_SEED, RANSAC_N, RANSAC_ITER = 7, 3, 512


def ransac_clouds():
    """a 300-point cloud on the 2^-10 grid (exact in f32 storage too), unit normals, and its copy turned 25 deg about AXIS and shifted"""
    rng = np.random.default_rng(5)
    P = _grid(rng.uniform(-6.0, 6.0, (300, 3)), 10)
    N = rng.normal(size=(300, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    R = rotation(AXIS, math.radians(25.0))
    Q = _grid((P.astype(LD) @ R.T).astype(np.float64) + [1.5, -0.75, 0.25], 10)
    NQ = (N.astype(LD) @ R.T).astype(np.float32).astype(np.float64)
    return P, N, Q, NQ
