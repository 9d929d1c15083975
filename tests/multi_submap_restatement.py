"""Host restatement of o3ds_icp_register_multi on the CPU oracle (point-to-plane): the yardstick of tests/test_multi_submap_gpu.py, itself
checked in tests/test_multi_submap_cpu.py against the oracle's own one-target registration.

UNION  per pass every map is searched on its own (its own k-d tree); a query's correspondence is the nearest of the per-map matches,
       equal squared distances to the lower slot (np.argmin takes the first); the record is the one-target record over the winners.
JOINT  per pass every map contributes its own record; the records are summed, the fitness denominator is n_targets * n_src
       (tests/test_sharded_cpu.py, the "submap" partitioning, in one process)."""
import numpy as np


class HostIcpState:
    """The device-side step (icp_step_block) on the host: convergence test of the previous pass, solve, T <- U T."""

    def __init__(self, init, max_iter, rel_fit, rel_rmse):
        self.T = np.array(init, dtype=np.float64)
        self.max_iter, self.rel_fit, self.rel_rmse = max_iter, rel_fit, rel_rmse
        self.fitness = self.rmse = 0.0
        self.n_corr = 0
        self.passes = self.iterations = 0
        self.done = self.converged = False

    def step(self, rec, n_total, oracle):
        if self.done:
            return
        cnt = rec[28]
        fit = cnt / n_total if cnt > 0 else 0.0
        rmse = float(np.sqrt(rec[29] / cnt)) if cnt > 0 else 0.0
        conv = self.passes > 0 and abs(self.fitness - fit) < self.rel_fit and abs(self.rmse - rmse) < self.rel_rmse
        self.fitness, self.rmse, self.n_corr = fit, rmse, int(cnt + 0.5)
        self.passes += 1
        if conv:
            self.converged = self.done = True
            return
        if self.iterations >= self.max_iter:
            self.done = True
            return
        if cnt > 0:
            A = np.zeros((6, 6))
            A[np.triu_indices(6)] = rec[:21]
            A = A + A.T - np.diag(np.diag(A))
            U, _ = oracle.solve_update(A, rec[21:27])
        else:
            U = np.eye(4)
        self.T = U @ self.T
        self.iterations += 1

    def result(self):
        return dict(transformation=self.T, fitness=self.fitness, inlier_rmse=self.rmse, iterations=self.iterations,
                    converged=self.converged, n_corr=self.n_corr)


def _record_of(oracle, P, tgt, nrm, corr, d2):
    rec = np.zeros(32)
    JTJ, JTr, r2 = oracle.compute_jtj_jtr(P, tgt, nrm, corr)
    rec[:21] = JTJ[np.triu_indices(6)]
    rec[21:27] = JTr
    rec[27], rec[28], rec[29] = r2, int((corr >= 0).sum()), d2[corr >= 0].sum()
    return rec


def union_correspondences(oracle, trees, maps, P, max_corr):
    """(index into the concatenation of the maps in slot order or -1, squared distance) per query"""
    n = len(P)
    best = np.full(n, -1, dtype=np.int64)
    best_d2 = np.full(n, np.inf)
    off = 0
    for tree, (tgt, _) in zip(trees, maps):
        if len(tgt):
            corr, d2 = oracle.evaluate(tree, P, max_corr)[:2]
            corr = np.asarray(corr, dtype=np.int64)
            take = (corr >= 0) & (np.asarray(d2) < best_d2)  # strictly nearer: a tie stays with the lower slot
            best[take] = corr[take] + off
            best_d2[take] = np.asarray(d2)[take]
        off += len(tgt)
    return best, np.where(best >= 0, best_d2, 0.0)


def register_multi(oracle, form, src, maps, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """maps: [(points, normals)], slot order; form "union" or "joint"; point-to-plane"""
    src = np.ascontiguousarray(src, dtype=np.float64)
    trees = [oracle.KDTree(m[0]) if len(m[0]) else None for m in maps]
    cat_p = np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1, 3) for m in maps])
    cat_n = np.concatenate([np.asarray(m[1], dtype=np.float64).reshape(-1, 3) for m in maps])
    st = HostIcpState(np.eye(4) if init is None else init, max_iter, rel_fitness, rel_rmse)
    while not st.done:
        P = src @ st.T[:3, :3].T + st.T[:3, 3]
        if form == "union":
            corr, d2 = union_correspondences(oracle, trees, maps, P, max_corr)
            st.step(_record_of(oracle, P, cat_p, cat_n, corr.astype(np.int32), d2), len(src), oracle)
        else:
            rec = np.zeros(32)
            for tree, (tgt, nrm) in zip(trees, maps):
                if len(tgt):
                    corr, d2 = oracle.evaluate(tree, P, max_corr)[:2]
                    rec += _record_of(oracle, P, tgt, nrm, np.asarray(corr), np.asarray(d2))
            st.step(rec, len(maps) * len(src), oracle)
    return st.result()
