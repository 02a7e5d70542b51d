"""Point-to-point ICP with Open3D's semantics in fp64, independent of the oracle: scipy cKDTree correspondences, numpy SVD update.

The contract (lidarreg.h lr_icp, oracle.c orc_icp): the source point p = T x (fp64, ((T0 x + T1 y) + T2 z) + T3 per row) is matched
to the target point j minimising d2 = ((q_x - p_x)^2 + (q_y - p_y)^2) + (q_z - p_z)^2, with q the fp32 target promoted to fp64,
among those with d2 < max_dist^2 (strict); ties go to the lowest target index.  The update is the least-squares rigid fit of the
matched pairs applied on the left of T; at most max_iter updates; the run stops after an evaluation whose fitness and inlier RMSE
both changed by less than rel_fitness / rel_rmse since the previous one, or with fewer than 3 correspondences.

The k-d tree only proposes candidates: every proposal is re-scored with the contract's d2, and every point whose tree distance
lies within 1e-9 (relative) of the nearest one is proposed, so exact and near ties are decided by the contract's rule.
"""
import numpy as np
from scipy.spatial import cKDTree

NEAR = 1e-9          # relative slack of the candidate search around the tree's nearest distance and around max_dist


def transform(T, src):
    x = np.asarray(src, np.float32).astype(np.float64)
    return np.stack([((T[a, 0] * x[:, 0] + T[a, 1] * x[:, 1]) + T[a, 2] * x[:, 2]) + T[a, 3] for a in range(3)], axis=1)


class Target:
    """The finite rows of a target cloud in a k-d tree, with their original indices."""

    def __init__(self, tgt):
        q = np.asarray(tgt, np.float32).astype(np.float64)
        self.q = q
        self.rows = np.nonzero(np.all(np.isfinite(q), axis=1))[0]
        self.tree = cKDTree(q[self.rows])

    def d2(self, p, j):
        d = self.q[j] - p
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    def match(self, p, max_dist, k=8):
        """Contract correspondence of every row of p (fp64 [n,3]): (index or -1, d2)."""
        n = p.shape[0]
        ub = max_dist * (1 + NEAR) + 1e-300
        dist, idx = self.tree.query(p, k=k, distance_upper_bound=ub)
        found = np.isfinite(dist[:, 0])
        best_j = np.full(n, -1, np.int64)
        best_d2 = np.full(n, np.inf)
        max_d2 = max_dist * max_dist
        # rows whose k-th proposal is still within NEAR of the nearest: ask the tree for the whole ball
        crowded = found & np.isfinite(dist[:, -1]) & (dist[:, -1] <= dist[:, 0] * (1 + NEAR) + 1e-300)
        simple = found & ~crowded
        if simple.any():
            d, ix = dist[simple], idx[simple]
            keep = np.isfinite(d) & (d <= d[:, :1] * (1 + NEAR) + 1e-300)
            rows = np.where(keep, self.rows[np.minimum(ix, len(self.rows) - 1)], np.iinfo(np.int64).max)
            cand_d2 = np.where(keep, self.d2(p[simple][:, None, :], np.minimum(rows, len(self.q) - 1)), np.inf)
            ok = cand_d2 < max_d2
            cand_d2 = np.where(ok, cand_d2, np.inf)
            # nearest by the contract's d2, then the lowest index
            m = cand_d2.min(axis=1)
            tie = (cand_d2 == m[:, None]) & np.isfinite(cand_d2)
            j = np.where(tie, rows, np.iinfo(np.int64).max).min(axis=1)
            hit = np.isfinite(m)
            sel = np.nonzero(simple)[0]
            best_j[sel[hit]] = j[hit]
            best_d2[sel[hit]] = m[hit]
        for i in np.nonzero(crowded)[0]:
            ball = np.asarray(self.tree.query_ball_point(p[i], dist[i, 0] * (1 + NEAR) + 1e-300), np.int64)
            rows = self.rows[ball]
            d2 = self.d2(p[i][None, :], rows)
            ok = d2 < max_d2
            if ok.any():
                m = d2[ok].min()
                best_j[i] = rows[ok][d2[ok] == m].min()
                best_d2[i] = m
        return best_j, best_d2


def svd_update(P, Q):
    """Least-squares rigid fit Q ~ R P + t of fp64 pairs (centred SVD) -> 4x4."""
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - cp).T @ (Q - cq)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = cq - R @ cp
    return T


def icp(src, tgt, T_init, max_dist=0.6, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, target=None):
    """Returns (T, info) with info = dict(fitness, inlier_rmse, n_corr, iterations, margin): margin is the smallest distance of a
    convergence test to its 1e-6 decision, over the evaluations that were tested (how close the stop decision came to flipping)."""
    tg = Target(tgt) if target is None else target
    n0 = np.asarray(src).shape[0]
    T = np.asarray(T_init, np.float64).copy()
    prev = None
    margin = np.inf
    k = 0
    while True:
        p = transform(T, src)
        j, d2 = tg.match(p, max_dist)
        hit = j >= 0
        n = int(hit.sum())
        fit = n / n0
        rmse = float(np.sqrt(d2[hit].sum() / n)) if n > 0 else 0.0
        done = False
        if k > 0:
            df, dr = abs(prev[0] - fit), abs(prev[1] - rmse)
            margin = min(margin, abs(df - rel_fitness), abs(dr - rel_rmse))
            done = df < rel_fitness and dr < rel_rmse
        if k >= max_iter or n < 3:
            done = True
        if done:
            break
        U = svd_update(p[hit], tg.q[j[hit]])
        T = U @ T
        T[3] = [0, 0, 0, 1]
        prev = (fit, rmse)
        k += 1
    return T, dict(fitness=fit, inlier_rmse=rmse, n_corr=n, iterations=k, margin=margin)
