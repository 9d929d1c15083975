"""Open3D v0.15.1 GlobalOptimization with GlobalOptimizationLevenbergMarquardt (pipelines/registration/GlobalOptimization.cpp), restated
in numpy as plain serial code: the checker of o3ds_global_optimization.  Open3D is not on the machines this project is built on; the
restatement is written from knowledge of its source, so this row is UNPINNED.

Points that are not certain, and why each is harmless or where it would show:
  * The right-hand side.  Open3D forms b with JsT_Info = Js^T * Info * confidence and subtracts either JsT_Info * e or
    (e^T * Info * confidence) * Js; both are conf * Js^T Info e for a symmetric Info and differ only in rounding.  Here:
    q = (Js^T Info conf) e, b_s -= q, b_t -= -q (Jt = -Js exactly: the generators enter negated).
  * TransformVector6dToMatrix4d multiplies three Eigen AngleAxis objects, which Eigen composes through quaternions; here the rotation
    is the product of the three elementary matrices Rz(gamma) Ry(beta) Rx(alpha).  Same matrix up to rounding.
  * Eigen's 4x4 inverse (cofactors) versus numpy's LU inverse: rounding only.
  * colPivHouseholderQr versus numpy.linalg.solve (LU): the solve's rounding differs; H + lambda I is SPD, so both are accurate to
    cond * eps.  The device uses Cholesky.
  * The stop checks as remembered: CheckRightTerm reads max(b) (the signed maximum, not max |b|); CheckRelativeIncrement is
    |delta| < eps (|x| + eps) with x = TransformMatrix4dToVector6d of the current poses; CheckRelativeResidualIncrement is
    r_cur - r_new < eps r_cur and is evaluated only for an accepted step (rho > 0); CheckResidual / CheckMaxIteration run after each
    outer iteration, CheckMaxIterationLM after each inner one.  The outer counter starts at 0 and stops when iter >= max_iteration, so
    up to max_iteration + 1 outer iterations run.
  * The new residual of a trial step is ComputeResidual(pose_graph /* the OLD graph: old confidences */, zeta_new).
  * ValidatePoseGraph: connectivity over all edges is required; an edge whose node id is out of range invalidates the graph (the ABI
    reports that as an invalid argument instead, it must not read out of bounds); a certain edge with confidence != 1 invalidates it.
Stop reasons (o3ds_pose_graph_result.stop_reason): 0 none ran, 1 right term, 2 relative increment, 3 relative residual increment,
4 residual, 5 max iteration, 6 max LM iteration -- the first check that set `stop`.
"""
from __future__ import annotations

import dataclasses

import numpy as np

STOP_NONE, STOP_RIGHT_TERM, STOP_REL_INCREMENT, STOP_REL_RESIDUAL, STOP_RESIDUAL, STOP_MAX_ITER, STOP_MAX_ITER_LM = range(7)

# jacobian_operator: the six generators (alpha, beta, gamma, a, b, c), GlobalOptimization.cpp
JACOBIAN_OPERATOR = [np.zeros((4, 4)) for _ in range(6)]
JACOBIAN_OPERATOR[0][1, 2], JACOBIAN_OPERATOR[0][2, 1] = -1.0, 1.0
JACOBIAN_OPERATOR[1][0, 2], JACOBIAN_OPERATOR[1][2, 0] = 1.0, -1.0
JACOBIAN_OPERATOR[2][0, 1], JACOBIAN_OPERATOR[2][1, 0] = -1.0, 1.0
JACOBIAN_OPERATOR[3][0, 3] = 1.0
JACOBIAN_OPERATOR[4][1, 3] = 1.0
JACOBIAN_OPERATOR[5][2, 3] = 1.0


@dataclasses.dataclass
class Edge:  # PoseGraphEdge
    source: int
    target: int
    transformation: np.ndarray
    information: np.ndarray
    uncertain: bool = False
    confidence: float = 1.0


@dataclasses.dataclass
class Option:  # GlobalOptimizationOption
    max_correspondence_distance: float = 0.075
    edge_prune_threshold: float = 0.25
    preference_loop_closure: float = 1.0
    reference_node: int = -1


@dataclasses.dataclass
class Criteria:  # GlobalOptimizationConvergenceCriteria
    max_iteration: int = 100
    min_relative_increment: float = 1e-6
    min_relative_residual_increment: float = 1e-6
    min_right_term: float = 1e-6
    min_residual: float = 1e-6
    max_iteration_lm: int = 20
    upper_scale_factor: float = 2.0 / 3.0
    lower_scale_factor: float = 1.0 / 3.0


def lin6(M) -> np.ndarray:  # GetLinearized6DVector
    return np.array([(-M[1, 2] + M[2, 1]) / 2.0, (-M[2, 0] + M[0, 2]) / 2.0, (-M[0, 1] + M[1, 0]) / 2.0, M[0, 3], M[1, 3], M[2, 3]])


def relative_poses(nodes, e: Edge):  # GetRelativePoses
    return np.linalg.inv(e.transformation), nodes[e.source], np.linalg.inv(nodes[e.target])


def misalignment(X_inv, Ts, Tt_inv) -> np.ndarray:  # GetMisalignmentVector
    return lin6(X_inv @ Tt_inv @ Ts)


def jacobian(X_inv, Ts, Tt_inv):  # GetJacobian
    Js = np.stack([lin6(X_inv @ Tt_inv @ G @ Ts) for G in JACOBIAN_OPERATOR], axis=1)
    Jt = np.stack([lin6(X_inv @ Tt_inv @ -G @ Ts) for G in JACOBIAN_OPERATOR], axis=1)
    return Js, Jt


def vector6_to_matrix4(v) -> np.ndarray:  # utility::TransformVector6dToMatrix4d: Rz(v2) Ry(v1) Rx(v0), translation v3..5
    a, b, g = v[0], v[1], v[2]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = v[3:6]
    return T


def matrix4_to_vector6(T) -> np.ndarray:  # utility::TransformMatrix4dToVector6d
    R = T[:3, :3]
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if not sy < 1e-6:
        r = [np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])]
    else:
        r = [np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0]
    return np.array([*r, T[0, 3], T[1, 3], T[2, 3]])


def compute_line_process_weight(edges, option: Option) -> float:  # ComputeLineProcessWeight
    if not edges:
        return 0.0
    avg = 0.0
    for e in edges:
        avg += e.information[5, 5]
    avg /= float(len(edges))
    return option.preference_loop_closure * option.max_correspondence_distance ** 2 * avg


def compute_zeta(nodes, edges) -> np.ndarray:  # ComputeZeta
    out = np.zeros(6 * len(edges))
    for k, e in enumerate(edges):
        out[6 * k:6 * k + 6] = misalignment(*relative_poses(nodes, e))
    return out


def compute_residual(edges, zeta, lpw) -> float:  # ComputeResidual
    r = 0.0
    for k, e in enumerate(edges):
        z = zeta[6 * k:6 * k + 6]
        r += e.confidence * (z @ e.information @ z) + lpw * (np.sqrt(e.confidence) - 1.0) ** 2
    return r


def update_confidence(edges, zeta, lpw, option: Option) -> int:  # UpdateConfidence (in place), returns valid_edges_num
    valid = 0
    for k, e in enumerate(edges):
        if e.uncertain:
            z = zeta[6 * k:6 * k + 6]
            temp = lpw / (lpw + z @ e.information @ z)
            e.confidence = temp * temp
            if e.confidence > option.edge_prune_threshold:
                valid += 1
    return valid


def compute_linear_system(nodes, edges, zeta):  # ComputeLinearSystem
    n = len(nodes)
    H = np.zeros((6 * n, 6 * n))
    b = np.zeros(6 * n)
    for k, e in enumerate(edges):
        z = zeta[6 * k:6 * k + 6]
        Js, Jt = jacobian(*relative_poses(nodes, e))
        JsT_Info = Js.T @ e.information * e.confidence
        JtT_Info = Jt.T @ e.information * e.confidence
        i, j = 6 * e.source, 6 * e.target
        H[i:i + 6, i:i + 6] += JsT_Info @ Js
        H[i:i + 6, j:j + 6] += JsT_Info @ Jt
        H[j:j + 6, i:i + 6] += JtT_Info @ Js
        H[j:j + 6, j:j + 6] += JtT_Info @ Jt
        b[i:i + 6] -= JsT_Info @ z
        b[j:j + 6] -= JtT_Info @ z
    return H, b


def pose_vector(nodes) -> np.ndarray:  # UpdatePoseVector
    return np.concatenate([matrix4_to_vector6(T) for T in nodes]) if len(nodes) else np.zeros(0)


def update_pose_graph(nodes, delta):  # UpdatePoseGraph
    return [vector6_to_matrix4(delta[6 * i:6 * i + 6]) @ T for i, T in enumerate(nodes)]


def optimize_pose_graph(nodes, edges, criteria: Criteria, option: Option, solve=np.linalg.solve) -> dict:
    """GlobalOptimizationLevenbergMarquardt::OptimizePoseGraph on (nodes, edges) in place: `nodes` is a list of 4x4 poses, the edges'
    confidences are updated.  Returns the pass's statistics."""
    crit = criteria
    lpw = compute_line_process_weight(edges, option)
    zeta = compute_zeta(nodes, edges)
    current_residual = new_residual = compute_residual(edges, zeta, lpw)
    update_confidence(edges, zeta, lpw, option)
    x = pose_vector(nodes)
    H, b = compute_linear_system(nodes, edges, zeta)
    current_lambda = 1e-5 * (H.diagonal().max() if len(H) else 0.0)
    ni, rho = 2.0, 0.0
    out = dict(line_process_weight=lpw, iterations=0, lm_steps=0, stop_reason=STOP_NONE, residual=current_residual, trace=[], norms=[])
    if len(b) and b.max() < crit.min_right_term:  # CheckRightTerm
        out["stop_reason"] = STOP_RIGHT_TERM
        return out
    stop, reason, it = False, STOP_NONE, 0

    def set_stop(cond, why):
        nonlocal stop, reason
        if not stop and cond:
            stop, reason = True, why

    while not stop:
        lm_count = 0
        while True:
            delta = solve(H + current_lambda * np.eye(len(H)), b)
            out["lm_steps"] += 1
            out["norms"].append((np.linalg.norm(delta), np.linalg.norm(x)))  # what stop check 2 compares
            set_stop(np.linalg.norm(delta) < crit.min_relative_increment * (np.linalg.norm(x) + crit.min_relative_increment), STOP_REL_INCREMENT)
            if not stop:
                nodes_new = update_pose_graph(nodes, delta)
                zeta_new = compute_zeta(nodes_new, edges)
                new_residual = compute_residual(edges, zeta_new, lpw)  # the OLD graph's confidences
                rho = (current_residual - new_residual) / (delta @ (current_lambda * delta + b) + 1e-3)
                out["trace"].append((current_lambda, current_residual, new_residual, rho))
                if rho > 0:
                    set_stop(current_residual - new_residual < crit.min_relative_residual_increment * current_residual, STOP_REL_RESIDUAL)
                    alpha = 1.0 - (2.0 * rho - 1.0) ** 3
                    alpha = min(alpha, crit.upper_scale_factor)
                    current_lambda *= max(crit.lower_scale_factor, alpha)
                    ni = 2.0
                    current_residual = new_residual
                    zeta = zeta_new
                    nodes[:] = nodes_new
                    x = pose_vector(nodes)
                    update_confidence(edges, zeta, lpw, option)
                    H, b = compute_linear_system(nodes, edges, zeta)
                    set_stop(b.max() < crit.min_right_term, STOP_RIGHT_TERM)
                    if stop:
                        break
                else:
                    current_lambda *= ni
                    ni *= 2.0
            lm_count += 1
            set_stop(lm_count >= crit.max_iteration_lm, STOP_MAX_ITER_LM)
            if rho > 0 or stop:
                break
        set_stop(current_residual < crit.min_residual, STOP_RESIDUAL)
        set_stop(it >= crit.max_iteration, STOP_MAX_ITER)
        it += 1
    out.update(iterations=it, stop_reason=reason, residual=current_residual)
    return out


def first_system(nodes, edges, option: Option):
    """H, b and lambda of a pass's first LM step (the head of optimize_pose_graph); the confidences of `edges` are left as given"""
    nodes = [np.array(T, dtype=np.float64) for T in nodes]
    edges = [dataclasses.replace(e) for e in edges]
    lpw = compute_line_process_weight(edges, option)
    zeta = compute_zeta(nodes, edges)
    update_confidence(edges, zeta, lpw, option)
    H, b = compute_linear_system(nodes, edges, zeta)
    return H, b, 1e-5 * H.diagonal().max()


# ---- solvers for the solve= hook ------------------------------------------------------------------------------------------------------
class NotPositiveDefinite(np.linalg.LinAlgError):
    def __init__(self, row):
        super().__init__(f"pivot of row {row} is not positive")
        self.row = row


def cholesky_lower(A) -> np.ndarray:
    """plain LL^T, column by column; the first pivot that is not positive and finite raises NotPositiveDefinite(row)"""
    A = np.asarray(A, dtype=np.float64)
    m = len(A)
    L = np.zeros((m, m))
    for j in range(m):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0 or not np.isfinite(d):
            raise NotPositiveDefinite(j)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_cholesky(A, b) -> np.ndarray:
    """(L L^T) x = b by forward and back substitution: the device's method in serial order"""
    L = cholesky_lower(A)
    m = len(L)
    y = np.zeros(m)
    for j in range(m):
        y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros(m)
    for j in range(m - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


try:  # the residual of the refinement in 40 digits where mpmath is there and the system small enough for it; nothing depends on it
    import mpmath as _mp
except ImportError:
    _mp = None
MPMATH_MAX_ROWS = 130


def _residual(A, b, x) -> np.ndarray:
    """b - A x for a longdouble x, rounded to f64 once at the end"""
    if _mp is not None and len(b) <= MPMATH_MAX_ROWS:
        with _mp.workprec(140):
            xs = [_mp.mpf(float(v)) + _mp.mpf(float(v - np.longdouble(float(v)))) for v in x]
            return np.array([float(_mp.mpf(float(b[i])) - _mp.fdot(zip((float(a) for a in A[i]), xs))) for i in range(len(b))])
    return (b.astype(np.longdouble) - A.astype(np.longdouble) @ x).astype(np.float64)


def solve_refined(A, b, rounds=3) -> np.ndarray:
    """an f64 LU solve, then iterative refinement: the residual in extended precision (np.longdouble, 64 mantissa bits on x86; mpmath for
    small systems when it imports), the correction by the f64 solve, the sum kept in longdouble.  Accurate to f64 rounding of the true
    solution while cond(A) 2^-53 is well below 1."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if not len(b):
        return np.zeros(0)
    x = np.linalg.solve(A, b).astype(np.longdouble)
    for _ in range(rounds):
        x = x + np.linalg.solve(A, _residual(A, b, x)).astype(np.longdouble)
    return x.astype(np.float64)


def _connected(n_nodes, edges) -> bool:  # ValidatePoseGraphConnectivity(pose_graph, false)
    if n_nodes == 0:
        return True
    adj = [[] for _ in range(n_nodes)]
    for e in edges:
        adj[e.source].append(e.target)
        adj[e.target].append(e.source)
    seen, todo = {0}, [0]
    while todo:
        i = todo.pop()
        for j in adj[i]:
            if j not in seen:
                seen.add(j)
                todo.append(j)
    return len(seen) == n_nodes


def global_optimization(nodes, edges, criteria: Criteria | None = None, option: Option | None = None, solve=np.linalg.solve) -> dict:
    """GlobalOptimization(pose_graph, LM, criteria, option).  nodes: (n, 4, 4) poses, edges: list of Edge.  Returns poses, final
    confidences, the kept mask and per-pass statistics; valid = 0 leaves everything as it was (Open3D's warn-and-return)."""
    criteria = criteria or Criteria()
    option = option or Option()
    nodes = [np.array(T, dtype=np.float64) for T in nodes]
    n = len(nodes)
    edges = [dataclasses.replace(e, transformation=np.array(e.transformation, float), information=np.array(e.information, float)) for e in edges]
    conf0 = np.array([e.confidence for e in edges])
    res = dict(valid=0, poses=np.array(nodes).reshape(n, 4, 4), confidence=conf0, kept=np.ones(len(edges), bool), passes=[])
    for e in edges:
        if not (0 <= e.source < n and 0 <= e.target < n):
            raise ValueError("an edge references an invalid node")
    if not _connected(n, edges) or any((not e.uncertain) and e.confidence != 1.0 for e in edges):
        return res
    res["valid"] = 1
    if n <= 1:
        return res
    orig = [T.copy() for T in nodes]
    res["passes"].append(optimize_pose_graph(nodes, edges, criteria, option, solve))
    res["poses_pass1"] = np.array(nodes)
    conf = np.array([e.confidence for e in edges])
    kept = np.array([(not e.uncertain) or e.confidence > option.edge_prune_threshold for e in edges], bool)
    pruned = [e for e, k in zip(edges, kept) if k]
    res["passes"].append(optimize_pose_graph(nodes, pruned, criteria, option, solve))
    conf[kept] = [e.confidence for e in pruned]
    ref = option.reference_node
    if 0 <= ref < n:  # CompensateReferencePoseGraphNode
        comp = orig[ref] @ np.linalg.inv(nodes[ref])
        nodes = [comp @ T for T in nodes]
    res.update(poses=np.array(nodes), confidence=conf, kept=kept)
    return res


# ---- scenarios shared by the CPU and GPU tests --------------------------------------------------------------------------------------
def rz(a) -> np.ndarray:
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def information_from_points(P) -> np.ndarray:
    """[O3D] GetInformationMatrixFromPointClouds' sum over correspondences p: G^T G with G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0],
    [y, -x, 0, 0, 0, 1]]; (5, 5) is the correspondence count."""
    P = np.asarray(P, dtype=np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    o, l = np.zeros_like(x), np.ones_like(x)
    G = np.stack([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1), np.stack([y, -x, o, o, o, l], 1)], 1)  # (n, 3, 6)
    return np.einsum("nki,nkj->ij", G, G)


def figure_eight_graph(n_nodes=40, drift_yaw=0.004, drift_fwd=0.01, n_points=1500, seed=3):
    """A figure-eight trajectory (synthetic.figure_eight_poses) reduced to n_nodes submap nodes.  Odometry edges i -> i + 1 carry a drift
    bias (a yaw and a forward-scale error per edge) and the nodes start from the drifted chain; three true loop closures (source >
    target, exact ground-truth transforms) and one gross outlier.  Returns (ground truth, initial poses, edges)."""
    from open3d_slam_amd import synthetic

    G = synthetic.figure_eight_poses(n_frames=10 * n_nodes, step=0.5)[::10]
    rng = np.random.default_rng(seed)

    def info():
        P = rng.uniform(-10, 10, (n_points, 3)) * [1.0, 1.0, 0.2]
        return information_from_points(P)

    edges = []
    for i in range(n_nodes - 1):
        X = np.linalg.inv(G[i + 1]) @ G[i]  # e = lin(X^-1 Tt^-1 Ts) = 0 at the ground truth
        B = rz(drift_yaw)
        B[0, 3] = drift_fwd * np.linalg.norm(X[:3, 3])
        edges.append(Edge(i, i + 1, X @ B, info(), uncertain=False))
    T0 = [G[0].copy()]
    for i in range(n_nodes - 1):
        T0.append(T0[-1] @ np.linalg.inv(edges[i].transformation))
    h = n_nodes // 2
    for s, t in [(h, 0), (n_nodes - 1, 0), (min(h + 3, n_nodes - 1), 3)]:
        edges.append(Edge(s, t, np.linalg.inv(G[t]) @ G[s], info(), uncertain=True))
    bad = rz(1.0)
    bad[:3, 3] = [6.0, -4.0, 0.5]
    edges.append(Edge(h + n_nodes // 4, n_nodes // 4, bad, info(), uncertain=True))
    return np.array(G), np.array(T0), edges


def drift(poses, G) -> float:
    """mean translation error against ground truth after aligning node 0"""
    A = G[0] @ np.linalg.inv(poses[0])
    return float(np.mean([np.linalg.norm((A @ T)[:3, 3] - g[:3, 3]) for T, g in zip(poses, G)]))


# ---- scenarios for the branches the figure-eight never takes (tests/test_pose_graph_edges_*.py) ------------------------------------------
def scrambled_graph(n_nodes=30, seed=11, certain=False):
    """The figure-eight with every start pose left-multiplied by V6toM4(N(0, [1, 1, 1, 5, 5, 5])): far enough from the solution that LM
    rejects steps (rho <= 0), several in a row.  certain=True makes every edge certain, the gross outlier included."""
    G, T0, E = figure_eight_graph(n_nodes=n_nodes)
    rng = np.random.default_rng(seed)
    T0 = np.array([vector6_to_matrix4(rng.normal(size=6) * [1.0, 1.0, 1.0, 5.0, 5.0, 5.0]) @ T for T in T0])
    if certain:
        E = [dataclasses.replace(e, uncertain=False) for e in E]
    return G, T0, E


def _noisy_edge(rng, G, s, t, noise, uncertain, n_points):
    X = np.linalg.inv(G[t]) @ G[s] @ vector6_to_matrix4(rng.normal(size=6) * noise)
    return Edge(int(s), int(t), X, information_from_points(rng.uniform(-8, 8, (n_points, 3))), bool(uncertain))


def hub_graph(n, extra=None, seed=5, bundle=0, noise=0.01, n_points=60):
    """Node 0 tied to every node, the edge direction alternating (every third one uncertain), plus `extra` (default 3 n) random edges,
    half of them uncertain: H's first block column is dense, so the Cholesky factor fills in completely.  `bundle` further edges all lie
    on the pair (1, 2), in alternating directions: one block list of that length.  Returns (ground truth, start poses, edges)."""
    rng = np.random.default_rng(seed)
    extra = 3 * n if extra is None else extra
    G = [vector6_to_matrix4(rng.normal(size=6) * [0.3, 0.3, 1.0, 4.0, 4.0, 1.0]) for _ in range(n)]
    E = []
    for i in range(1, n):
        s, t = (0, i) if i % 2 else (i, 0)
        E.append(_noisy_edge(rng, G, s, t, noise, i % 3 == 0, n_points))
    for _ in range(extra):
        s, t = rng.integers(0, n, 2)
        if s == t:
            t = (s + 1) % n
        E.append(_noisy_edge(rng, G, s, t, noise, rng.random() < 0.5, n_points))
    for k in range(bundle):
        E.append(_noisy_edge(rng, G, 1 + k % 2, 2 - k % 2, noise, k % 3 == 0, n_points))
    T0 = np.array([T @ vector6_to_matrix4(rng.normal(size=6) * 2.0 * noise) for T in G])
    return np.array(G), T0, E


def _walk(rng, n):
    G = [np.eye(4)]
    for _ in range(n - 1):
        G.append(G[-1] @ vector6_to_matrix4(rng.normal(size=6) * [0.02, 0.02, 0.2, 2.0, 0.5, 0.1]))
    return G


def multi_edge_graph(n=8, seed=2):
    """A noisy odometry chain with a loop closure, three parallel edges on the pair (2, 5) -- 2 -> 5 certain, 5 -> 2 uncertain, 2 -> 5
    uncertain -- and one uncertain self-edge 3 -> 3: block lists of length >= 3 with both signs, and source == target."""
    rng = np.random.default_rng(seed)
    G = _walk(rng, n)
    E = [_noisy_edge(rng, G, i, i + 1, 0.01, False, 400) for i in range(n - 1)]
    E.append(_noisy_edge(rng, G, n - 1, 0, 0.0, True, 400))
    E.append(_noisy_edge(rng, G, 2, 5, 0.01, False, 400))
    E.append(_noisy_edge(rng, G, 5, 2, 0.01, True, 400))
    E.append(_noisy_edge(rng, G, 2, 5, 0.01, True, 400))
    E.append(_noisy_edge(rng, G, 3, 3, 0.01, True, 400))
    return np.array(G), np.array(G), E


def gimbal_graph(n=10, seed=4):
    """Nodes 1 and n - 2 stand at pitch +pi/2 and -pi/2 exactly (R00 = R10 = 0: TransformMatrix4dToVector6d's else branch), the others
    are yaw-only with yaws of a radian and more, and every translation is small: |x| is made of the angles, so which branch computed
    them decides stop check 2 (pose_graph_edge_cases.GIMBAL_INCREMENTS holds the min_relative_increment values that tell the branches apart)."""
    rng = np.random.default_rng(seed)
    G = []
    for i in range(n):
        T = rz(1.0 + 2.0 * rng.random())
        T[:3, 3] = rng.normal(size=3) * 0.05
        G.append(T)
    for i, sgn in ((1, 1.0), (n - 2, -1.0)):
        a = 0.3 + rng.random()
        ca, sa = np.cos(a), np.sin(a)
        G[i][:3, :3] = [[0.0, sgn * sa, sgn * ca], [0.0, ca, -sa], [-sgn, 0.0, 0.0]]  # Ry(sgn pi/2) Rx(a), its zeros exact
    E = [_noisy_edge(rng, G, i, i + 1, 0.01, False, 400) for i in range(n - 1)]
    E.append(_noisy_edge(rng, G, n - 1, 0, 0.0, True, 400))
    E.append(_noisy_edge(rng, G, n // 2, 1, 0.0, True, 400))
    return np.array(G), np.array(G), E


def all_outliers_graph(n=6, seed=6):
    """Every pair of nodes joined by an uncertain edge with a random transform kilometres and radians from the poses: every confidence
    is ~1e-11 and the residual sits at its saturation value, so the first accepted step gains less than the relative-residual bound, the
    pass ends there and pass 2 has no edges at all."""
    rng = np.random.default_rng(seed)
    G = _walk(rng, n)
    E = []
    for s in range(n):
        for t in range(s):
            X = vector6_to_matrix4(rng.normal(size=6) * [1.0, 1.0, 1.0, 2000.0, 2000.0, 2000.0])
            E.append(Edge(s, t, X, information_from_points(rng.uniform(-8, 8, (400, 3))), True))
    return np.array(G), np.array(G), E


def leaf_cut_graph(n=8, seed=7):
    """multi_edge_graph's chain and loop closure on nodes 0 .. n - 2; node n - 1 is a leaf held by one uncertain edge that is a kilometre
    off: its confidence is ~1e-12, it is pruned, and in pass 2 the leaf has no edge (its pivots are lambda alone, its delta 0)."""
    rng = np.random.default_rng(seed)
    G = _walk(rng, n)
    E = [_noisy_edge(rng, G, i, i + 1, 0.01, False, 400) for i in range(n - 2)]
    E.append(_noisy_edge(rng, G, n - 2, 0, 0.0, True, 400))
    leaf = _noisy_edge(rng, G, n - 1, n // 2, 0.0, True, 400)
    leaf.transformation[:3, 3] += [1000.0, -300.0, 50.0]
    E.append(leaf)
    return np.array(G), np.array(G), E


def all_uncertain(edges):
    return [dataclasses.replace(e, uncertain=True) for e in edges]


def recovered_delta(new, old) -> np.ndarray:
    """the step of one UpdatePoseGraph read back from the poses: delta_i = TransformMatrix4dToVector6d(new_i old_i^-1)"""
    return np.concatenate([matrix4_to_vector6(a @ np.linalg.inv(b)) for a, b in zip(new, old)])
