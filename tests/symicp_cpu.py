"""numpy restatement of contract Y (lr_symicp) of include/lidarreg.h / DESIGN.md §23, independent of the library, and of the neighbour
count of lr_normals2.  The per-point arithmetic is numpy's element-wise float64 (IEEE, no fused multiply-add), the scalar arithmetic of
the solve and the step is numpy's float64 scalar (the same; a division by zero or an overflow yields what IEEE says, no exception), the
nearest neighbour is that of tests/refine_z_cpu.py, the products and the transform those of tests/bbrf_cpu.py."""
import math

import numpy as np

from tests import bbrf_cpu, refine_z_cpu
from tests.bbrf_cpu import dot3, mat3, rot3

RUN = 1024          # Y4: indices per run
SEG = 16            # Y4: consecutive terms per lane
LANES = RUN // SEG
NSUM = 28           # 21 entries of H (a <= b), 6 of g, b b
MAX_ITER = 1000
DEFAULTS = dict(n_iter=30, max_dist=0.6, min_cos=0.7, eps_rot=1e-5, eps_trans=1e-4, piv_eps=1e-9)
NORMAL_DEFAULTS = dict(normal_radius=1.0, max_nn=32, min_nb=5)
F = np.float64


def cross3(U, V):
    """(u x v)_x = u_y v_z - u_z v_y, cyclically; every product rounded."""
    with np.errstate(all="ignore"):
        return np.stack([U[:, 1] * V[:, 2] - U[:, 2] * V[:, 1], U[:, 2] * V[:, 0] - U[:, 0] * V[:, 2], U[:, 0] * V[:, 1] - U[:, 1] * V[:, 0]], axis=1)


def move(B, nB, W, t):
    """Y1: B'_j = (W.B_j) + t, nB'_j = W.nB_j."""
    with np.errstate(all="ignore"):
        return rot3(W, B) + np.array(t, F)[None, :], rot3(W, nB)


def candidates(A, Bp, search=None):
    """Y2: (f, r, fwd, bwd): f = N(A, B'), r = N(B', A); fwd[i] iff f_i >= 0; bwd[j] iff r_j >= 0 and f[r_j] != j."""
    search = refine_z_cpu.nn if search is None else search
    n0, n1 = len(A), len(Bp)
    if n0 == 0 or n1 == 0:
        return np.full(n0, -1, np.int64), np.full(n1, -1, np.int64), np.zeros(n0, bool), np.zeros(n1, bool)
    f = search(A, Bp)[1]
    r = search(Bp, A)[1]
    fwd = f >= 0
    bwd = (r >= 0) & (f[np.where(r >= 0, r, 0)] != np.arange(n1))
    return f, r, fwd, bwd


def rows(A, nA, Bp, nBp, i, j, max_dist, min_cos):
    """Y3 on the candidates (i[k], j[k]): (terms [len, 28], accepted [len] bool); a rejected candidate's terms are +0.0."""
    out = np.zeros((len(i), NSUM))
    if not len(i):
        return out, np.zeros(0, bool)
    p, q, na, nb = Bp[j], A[i], nA[i], nBp[j]
    with np.errstate(all="ignore"):
        d = p - q
        dot = dot3(na, nb)
        ok = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(na).all(axis=1) & np.isfinite(nb).all(axis=1)
        ok &= dot3(d, d) <= max_dist * max_dist
        ok &= np.abs(dot) >= min_cos
        s = np.where(dot < 0.0, -1.0, 1.0)
        n = na + s[:, None] * nb
        c = np.concatenate([cross3(p + q, n), n], axis=1)
        b = -dot3(d, n)
        k = 0
        for a in range(6):
            for e in range(a, 6):
                out[:, k] = c[:, a] * c[:, e]; k += 1
        for a in range(6):
            out[:, k] = c[:, a] * b; k += 1
        out[:, k] = b * b
    out[~ok] = 0.0
    return out, ok


def tree_sum(t):
    """Y4's order over the rows of t [n, m]: runs of 1024; in a run lane l adds its 16 consecutive terms in order from +0.0; the lanes
    fold v[l] = v[l] + v[l + h] for h = 32 .. 1; the run sums are added in run order from +0.0.  Returns [m]."""
    t = np.ascontiguousarray(t, F)
    if t.ndim == 1:
        return tree_sum(t[:, None])[0]
    n, m = t.shape
    runs = -(-n // RUN)
    pad = np.zeros((runs * RUN, m)); pad[:n] = t
    pad = pad.reshape(runs, LANES, SEG, m)
    with np.errstate(all="ignore"):
        v = np.zeros((runs, LANES, m))
        for k in range(SEG):
            v = v + pad[:, :, k]
        h = LANES // 2
        while h >= 1:
            v = v[:, :h] + v[:, h:2 * h]
            h //= 2
        total = np.zeros(m)
        for r_ in range(runs):
            total = total + v[r_, 0]
    return total


def cholesky_solve(H, g, piv_eps):
    """Y5 on H [6][6] (its upper triangle is read) and g [6]: (status 0 / 2, x or None, pivots d_j computed so far)."""
    n = len(g)
    H = [[F(H[min(a, b)][max(a, b)]) for b in range(n)] for a in range(n)]
    L = [[F(0.0)] * n for _ in range(n)]
    piv = []
    with np.errstate(all="ignore"):
        for j in range(n):
            d = H[j][j]
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            piv.append(float(d))
            if not d > F(piv_eps) * H[j][j]:
                return 2, None, piv
            L[j][j] = np.sqrt(d)
            for i in range(j + 1, n):
                s = H[i][j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / L[j][j]
        y = [F(0.0)] * n
        for i in range(n):
            s = F(g[i])
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        x = [F(0.0)] * n
        for i in range(n - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, n):
                s = s - L[k][i] * x[k]
            x[i] = s / L[i][i]
    return 0, x, piv


def half_rotation(at):
    """Y6: (c, R) with c = 1 / sqrt(1 + a.a), R = c I + c [a]x + (c c / (1 + c)) a a^T, as R[a][b] = (D_ab + c S_ab) + k2 (a_a a_b)."""
    a0, a1, a2 = (F(v) for v in at)
    with np.errstate(all="ignore"):
        aa = (a0 * a0 + a1 * a1) + a2 * a2
        c = F(1.0) / np.sqrt(F(1.0) + aa)
        k2 = (c * c) / (F(1.0) + c)
        z = F(0.0)
        S = [[z, -a2, a1], [a2, z, -a0], [-a1, a0, z]]
        v = [a0, a1, a2]
        R = [[((c if a == b else z) + c * S[a][b]) + k2 * (v[a] * v[b]) for b in range(3)] for a in range(3)]
    return c, R, aa


def matvec(M, v):
    with np.errstate(all="ignore"):
        return [(M[a][0] * v[0] + M[a][1] * v[1]) + M[a][2] * v[2] for a in range(3)]


def pose(W, t):
    """(B_to_A, T): [W t; 0 1] and its rigid inverse [W^T, -(W^T.t); 0 1] (B8's form)."""
    M = np.eye(4); T = np.eye(4)
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                M[a, b] = W[a][b]; T[a, b] = W[b][a]
            M[a, 3] = t[a]
            T[a, 3] = -((W[0][a] * t[0] + W[1][a] * t[1]) + W[2][a] * t[2])
    return M, T


def sums_of(A, nA, Bp, nBp, f, r, fwd, bwd, max_dist, min_cos):
    """Y3 + Y4: (28 sums, n_pairs)."""
    i = np.flatnonzero(fwd); j = np.flatnonzero(bwd)
    tf = np.zeros((len(A), NSUM)); tb = np.zeros((len(Bp), NSUM))
    rf, okf = rows(A, nA, Bp, nBp, i, f[i], max_dist, min_cos)
    rb, okb = rows(A, nA, Bp, nBp, r[j], j, max_dist, min_cos)
    tf[i] = rf; tb[j] = rb
    with np.errstate(all="ignore"):
        total = (tree_sum(tf) if len(A) else np.zeros(NSUM)) + (tree_sum(tb) if len(Bp) else np.zeros(NSUM))
    return total, int(okf.sum()) + int(okb.sum())


def symicp(A, nA, B, nB, n_iter=30, max_dist=0.6, min_cos=0.7, eps_rot=1e-5, eps_trans=1e-4, piv_eps=1e-9, T_init=None, search=None,
           trace=None):
    """Contract Y.  Returns (result dict, log [n_iter, 8]); rows past iters_run stay +0.0.  trace: a list that receives per iteration
    dict(f, r, n_pairs, piv, x)."""
    f64 = lambda X: np.ascontiguousarray(X, F).reshape(-1, 3)
    A, nA, B, nB = f64(A), f64(nA), f64(B), f64(nB)
    log = np.zeros((n_iter, 8))
    if T_init is None:
        W = [[F(1.0 if a == b else 0.0) for b in range(3)] for a in range(3)]; t = [F(0.0)] * 3
    else:
        Ti = np.asarray(T_init, F).reshape(4, 4)
        W = [[Ti[a, b] for b in range(3)] for a in range(3)]; t = [Ti[a, 3] for a in range(3)]
    status = converged = iters_run = n_pairs = 0
    msq = F(0.0)
    with np.errstate(all="ignore"):
        for k in range(n_iter):
            Bp, nBp = move(B, nB, W, t)
            f, r, fwd, bwd = candidates(A, Bp, search)
            S, n_pairs = sums_of(A, nA, Bp, nBp, f, r, fwd, bwd, max_dist, min_cos)
            msq = S[27] / F(n_pairs) if n_pairs > 0 else F(0.0)
            log[k, 0] = n_pairs; log[k, 1] = msq
            iters_run = k + 1
            rec = dict(f=f, r=r, n_pairs=n_pairs, piv=None, x=None)
            if trace is not None:
                trace.append(rec)
            if n_pairs < 6:
                status = 1
                break
            H = [[F(0.0)] * 6 for _ in range(6)]
            q = 0
            for a in range(6):
                for e in range(a, 6):
                    H[a][e] = S[q]; q += 1
            st, x, piv = cholesky_solve(H, [S[21 + a] for a in range(6)], piv_eps)
            rec["piv"] = piv; rec["x"] = x
            if st:
                status = 2
                break
            if not all(np.isfinite(v) for v in x):
                status = 3
                break
            c, R, aa = half_rotation(x[:3])
            dW = mat3(R, R)
            dt = matvec(R, [c * x[3], c * x[4], c * x[5]])
            W = mat3(dW, W)
            wt = matvec(dW, t)
            t = [wt[a] + dt[a] for a in range(3)]
            tt = (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]
            log[k, 2] = aa; log[k, 3] = tt
            if aa <= F(eps_rot) * F(eps_rot) and tt <= F(eps_trans) * F(eps_trans):
                converged = 1
                break
    M, T = pose(W, t)
    return dict(T=T, B_to_A=M, status=status, iters_run=iters_run, converged=converged, n_pairs=n_pairs, mean_sq=float(msq)), log


def icp_p2p(A, B, n_iter=30, max_dist=0.6, eps_rot=1e-5, eps_trans=1e-4, search=None):
    """A point-to-point ICP on the same clouds and distance, for the accuracy comparison only (not a contract): B moves onto A, pairs
    (f_j = N(B', A), within max_dist), Kabsch by numpy's SVD per iteration, stopped when the step's angle is at most eps_rot and its
    translation at most eps_trans.  Returns B_to_A."""
    search = refine_z_cpu.nn if search is None else search
    M = np.eye(4)
    for _ in range(n_iter):
        Bp = B @ M[:3, :3].T + M[:3, 3]
        d, idx, _ = search(Bp, A)
        ok = (idx >= 0) & (d <= max_dist)
        if ok.sum() < 3:
            break
        P, Q = Bp[ok], A[idx[ok]]
        pc, qc = P.mean(axis=0), Q.mean(axis=0)
        U, _, Vt = np.linalg.svd((P - pc).T @ (Q - qc))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        R = Vt.T @ D @ U.T
        step = np.eye(4); step[:3, :3] = R; step[:3, 3] = qc - R @ pc
        M = step @ M
        ang = math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0)))
        if ang <= eps_rot and np.linalg.norm(step[:3, 3]) <= eps_trans:
            break
    return M


def normals_counted(X, radius, max_nn, nbrs=None):
    """lr_normals2: (normals [n,3], counts int32 [n]) -- the normals of bbrf_cpu.normals and the number of neighbours each point took
    (0 .. max_nn, the point itself included; 0 for a non-finite point)."""
    X = np.ascontiguousarray(X, F).reshape(-1, 3)
    nbrs = bbrf_cpu.neighbours(X, radius, max_nn) if nbrs is None else nbrs
    nrm, _ = bbrf_cpu.normals(X, radius, max_nn, nbrs=nbrs)
    return nrm, np.array([len(nb) for nb in nbrs], np.int32).reshape(len(X))
