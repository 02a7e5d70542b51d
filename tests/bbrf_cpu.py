"""numpy restatement of contract B (lr_bbrf) and of the normals contract (lr_normals) of include/lidarreg.h / DESIGN.md §14, independent
of the library.  The per-point arithmetic is numpy's element-wise float64 (IEEE, no fused multiply-add), the scalar arithmetic of the
step is Python's float (the same), the nearest neighbour and the two-level sum are those of tests/refine_z_cpu.py."""
import math

import numpy as np

from tests import refine_z_cpu

RUN = refine_z_cpu.RUN
FACT = [float(math.factorial(k)) for k in range(18)]
SIN_C = [(-1.0 if (k // 2) & 1 else 1.0) / FACT[k] for k in (17, 15, 13, 11, 9, 7, 5, 3)]      # x^17 .. x^3
COS_C = [(-1.0 if (k // 2) & 1 else 1.0) / FACT[k] for k in (16, 14, 12, 10, 8, 6, 4, 2)]      # x^16 .. x^2
ANGLE_MAX = 0.5
DEFAULTS = dict(n_iter=100, angles_lr=2e-4, trans_lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def sin_poly(x):
    """B2: z = x x; q = c17; q = q z + c_k for k = 15 .. 3; sin = x + (x z) q."""
    z = x * x
    q = SIN_C[0]
    for c in SIN_C[1:]:
        q = q * z + c
    return x + (x * z) * q


def cos_poly(x):
    """B2: z = x x; q = c16; q = q z + c_k for k = 14 .. 2; cos = 1 + z q."""
    z = x * x
    q = COS_C[0]
    for c in COS_C[1:]:
        q = q * z + c
    return 1.0 + z * q


def mat3(P, Q):
    """(P Q)[a][b] = (P[a][0] Q[0][b] + P[a][1] Q[1][b]) + P[a][2] Q[2][b], every product rounded."""
    return [[(P[a][0] * Q[0][b] + P[a][1] * Q[1][b]) + P[a][2] * Q[2][b] for b in range(3)] for a in range(3)]


def rotation(theta, phi, psi):
    """B2: W = Rz (Ry Rx) and dW/dtheta = Rz (Ry dRx), dW/dphi = Rz (dRy Rx), dW/dpsi = dRz (Ry Rx), as lists of lists of floats."""
    s1, c1, s2, c2, s3, c3 = sin_poly(theta), cos_poly(theta), sin_poly(phi), cos_poly(phi), sin_poly(psi), cos_poly(psi)
    Rx = [[1.0, 0.0, 0.0], [0.0, c1, -s1], [0.0, s1, c1]]
    Ry = [[c2, 0.0, s2], [0.0, 1.0, 0.0], [-s2, 0.0, c2]]
    Rz = [[c3, -s3, 0.0], [s3, c3, 0.0], [0.0, 0.0, 1.0]]
    dRx = [[0.0, 0.0, 0.0], [0.0, -s1, -c1], [0.0, c1, -s1]]
    dRy = [[-s2, 0.0, c2], [0.0, 0.0, 0.0], [-c2, 0.0, -s2]]
    dRz = [[-s3, -c3, 0.0], [c3, -s3, 0.0], [0.0, 0.0, 0.0]]
    YX = mat3(Ry, Rx)
    return mat3(Rz, YX), [mat3(Rz, mat3(Ry, dRx)), mat3(Rz, mat3(dRy, Rx)), mat3(dRz, YX)]


def rot3(M, X):
    """rows ((M[a][0] x + M[a][1] y) + M[a][2] z) of X [n,3]"""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([(M[a][0] * x + M[a][1] * y) + M[a][2] * z for a in range(3)], axis=1)


def dot3(U, V):
    with np.errstate(all="ignore"):
        return (U[:, 0] * V[:, 0] + U[:, 1] * V[:, 1]) + U[:, 2] * V[:, 2]


def move(B, nB, p):
    """B3: (B', nB', W, dW) at the parameters p = (theta, phi, psi, tx, ty, tz)."""
    W, dW = rotation(p[0], p[1], p[2])
    with np.errstate(all="ignore"):
        Bp = rot3(W, B) + np.array([p[3], p[4], p[5]])[None, :]
    return Bp, rot3(W, nB), W, dW


def best_buddies(A, Bp, search=None):
    """B4: (f, keep): f = N(A, B'), keep[i] iff f_i >= 0 and N(B', A)[f_i] == i.  search: refine_z_cpu.nn (the default) or nn_tree."""
    search = refine_z_cpu.nn if search is None else search
    if len(A) == 0 or len(Bp) == 0:
        return np.full(len(A), -1, np.int64), np.zeros(len(A), bool)
    f = search(A, Bp)[1]
    r = search(Bp, A)[1]
    keep = (f >= 0) & (r[np.where(f >= 0, f, 0)] == np.arange(len(A)))
    return f, keep


def pair_terms(A, nA, B, nB, Bp, nBp, dW, f, keep):
    """B5 / B6 per source index: [n0, 7] = the loss term and sign(dot) d dot / d(theta, phi, psi, tx, ty, tz); +0.0 where not a pair."""
    n0 = len(A)
    out = np.zeros((n0, 7))
    i = np.flatnonzero(keep)
    if not len(i):
        return out, np.zeros(0)
    j = f[i]
    a, na, b, nb, bp, nbp = A[i], nA[i], B[j], nB[j], Bp[j], nBp[j]
    with np.errstate(all="ignore"):
        s = np.where(dot3(na, nbp) < 0.0, -1.0, 1.0)
        m = na + s[:, None] * nbp
        d = a - bp
        dot = dot3(d, m)
        ad = np.abs(dot)
        out[i, 0] = np.where(ad > 1e-15, ad, 1e-15)
        live = ~(dot * dot < 1e-30)
        sg = np.where(live, np.where(dot < 0.0, -1.0, 1.0), 0.0)
        for q in range(3):
            u, w = rot3(dW[q], b), rot3(dW[q], nb)
            e = dot3(d, s[:, None] * w) - dot3(u, m)
            out[i, 1 + q] = np.where(live, sg * e, 0.0)
        for c in range(3):
            out[i, 4 + c] = np.where(live, sg * (-m[:, c]), 0.0)
    return out, dot


def loss_and_grad(A, nA, B, nB, p, f=None, keep=None, search=None):
    """(loss, grad[6], n_pairs, f, keep) at p; f / keep given: the pair set held fixed."""
    Bp, nBp, W, dW = move(B, nB, p)
    if f is None:
        f, keep = best_buddies(A, Bp, search)
    n_pairs = int(keep.sum())
    terms, _ = pair_terms(A, nA, B, nB, Bp, nBp, dW, f, keep)
    if n_pairs == 0:
        return math.inf, [0.0] * 6, 0, f, keep
    sums = [float(refine_z_cpu.two_level_sum(terms[:, c])) for c in range(7)]
    with np.errstate(all="ignore"):
        return sums[0] / n_pairs, [sums[1 + q] / n_pairs for q in range(6)], n_pairs, f, keep


class Adam:
    """B7: torch's rule on six scalars, lr per parameter, the powers of beta as running products."""

    def __init__(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps = list(lr), beta1, beta2, eps
        self.m, self.v, self.p1, self.p2 = [0.0] * len(lr), [0.0] * len(lr), 1.0, 1.0

    def step(self, p, g):
        self.p1 = self.p1 * self.b1
        self.p2 = self.p2 * self.b2
        c1, c2 = 1.0 - self.p1, math.sqrt(1.0 - self.p2)
        out = []
        for k in range(len(p)):
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * g[k]
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * (g[k] * g[k])
            den = _sqrt(self.v[k]) / c2 + self.eps
            out.append(p[k] - (self.lr[k] / c1) * _div(self.m[k], den))
        return out


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 and x != math.inf else float(np.sqrt(np.float64(x)))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def pose(p):
    """B8: (B_to_A, T) as 4x4 arrays from the parameters p."""
    W, _ = rotation(p[0], p[1], p[2])
    M = np.eye(4); T = np.eye(4)
    for a in range(3):
        for b in range(3):
            M[a, b] = W[a][b]; T[a, b] = W[b][a]
        M[a, 3] = p[3 + a]
    for a in range(3):
        T[a, 3] = -((W[0][a] * p[3] + W[1][a] * p[4]) + W[2][a] * p[5])
    return M, T


def bbrf(A, nA, B, nB, n_iter=100, angles_lr=2e-4, trans_lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, trace=None, search=None):
    """Contract B.  Returns (result dict, log [n_iter, 8]); rows past iters_run stay +0.0.  trace: a list that receives per iteration
    dict(f, keep, grad).  search: the nearest-neighbour restatement, refine_z_cpu.nn (the default) or nn_tree."""
    f64 = lambda X: np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    A, nA, B, nB = f64(A), f64(nA), f64(B), f64(nB)
    log = np.zeros((n_iter, 8))
    p = [0.0] * 6
    adam = Adam([angles_lr] * 3 + [trans_lr] * 3, beta1, beta2, eps)
    status, best_iter, best_loss, n_best, best_p, iters_run = 0, -1, math.inf, 0, [0.0] * 6, 0
    for k in range(n_iter):
        loss, g, n_pairs, f, keep = loss_and_grad(A, nA, B, nB, p, search=search)
        log[k, :6] = p; log[k, 6] = loss; log[k, 7] = n_pairs
        iters_run = k + 1
        if trace is not None:
            trace.append(dict(f=f, keep=keep, grad=g))
        if n_pairs == 0:
            status = 1
            break
        if loss < best_loss:
            best_iter, best_loss, n_best, best_p = k, loss, n_pairs, list(p)
        p = adam.step(p, g)
        if not all(abs(x) <= ANGLE_MAX for x in p[:3]):
            status = 3
            break
    M, T = pose(best_p)
    return dict(T=T, B_to_A=M, status=status, best_iter=best_iter, best_loss=best_loss, n_pairs_best=n_best, iters_run=iters_run), log


# ---- the normals contract ---------------------------------------------------------------------------------------------------------------
SWEEPS = 8


def neighbours(X, radius, max_nn):
    """Per point the indices of its at most max_nn finite points of least (d2, index) with d2 <= fl(radius radius), in that order (a
    non-finite point: none)."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    ok = np.isfinite(X).all(axis=1)
    live = np.flatnonzero(ok)
    r2 = radius * radius
    out = [np.zeros(0, np.int64)] * len(X)
    for s in range(0, len(live), 256):
        q = live[s:s + 256]
        M = refine_z_cpu.d2_matrix(X[q], X[live])
        for a, i in enumerate(q):
            c = np.flatnonzero(M[a] <= r2)
            c = c[np.lexsort((live[c], M[a, c]))][:max_nn]
            out[i] = live[c]
    return out


def jacobi(C):
    """The contract's eigen-solver on C [n,3,3] (symmetric): (A after the sweeps, V), element-wise over n."""
    A = np.array(C, np.float64, copy=True); V = np.zeros_like(A)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = A[:, p, q].copy()
                on = apq != 0.0
                safe = np.where(on, apq, 1.0)
                th = (A[:, q, q] - A[:, p, p]) / (2.0 * safe)
                t = np.where(th < 0.0, -1.0, 1.0) / (np.abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0); s = t * c
                new = A.copy(); newV = V.copy()
                new[:, p, p] = A[:, p, p] - t * apq
                new[:, q, q] = A[:, q, q] + t * apq
                new[:, p, q] = new[:, q, p] = 0.0
                arp, arq = A[:, r, p], A[:, r, q]
                new[:, r, p] = new[:, p, r] = c * arp - s * arq
                new[:, r, q] = new[:, q, r] = s * arp + c * arq
                for k in range(3):
                    newV[:, k, p] = c * V[:, k, p] - s * V[:, k, q]
                    newV[:, k, q] = s * V[:, k, p] + c * V[:, k, q]
                A = np.where(on[:, None, None], new, A); V = np.where(on[:, None, None], newV, V)
    return A, V


def covariances(X, nbrs):
    """[n,3,3] by the cumulant form over each point's neighbours in their order (zeros where fewer than 3)."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    C = np.zeros((len(X), 3, 3))
    for i, nb in enumerate(nbrs):
        if len(nb) < 3:
            continue
        P = X[nb]
        S = [0.0] * 9
        for x, y, z in P.tolist():
            S[0] += x; S[1] += y; S[2] += z
            S[3] += x * x; S[4] += x * y; S[5] += x * z; S[6] += y * y; S[7] += y * z; S[8] += z * z
        k = float(len(nb))
        E = [v / k for v in S]
        C[i] = [[E[3] - E[0] * E[0], E[4] - E[0] * E[1], E[5] - E[0] * E[2]],
                [E[4] - E[0] * E[1], E[6] - E[1] * E[1], E[7] - E[1] * E[2]],
                [E[5] - E[0] * E[2], E[7] - E[1] * E[2], E[8] - E[2] * E[2]]]
    return C


def normals(X, radius=0.01, max_nn=13, nbrs=None):
    """(normals [n,3], info dict(status, n_dropped, n_default))."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    n = len(X)
    ok = np.isfinite(X).all(axis=1)
    nbrs = neighbours(X, radius, max_nn) if nbrs is None else nbrs
    full = np.array([len(nb) >= 3 for nb in nbrs], bool) if n else np.zeros(0, bool)
    out = np.zeros((n, 3)); out[:, 2] = 1.0
    if full.any():
        A, V = jacobi(covariances(X, nbrs)[full])
        d = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
        col = np.zeros(len(d), np.int64)
        lam = d[:, 0].copy()
        for k in (1, 2):
            less = d[:, k] < lam
            col = np.where(less, k, col); lam = np.where(less, d[:, k], lam)
        v = V[np.arange(len(d)), :, col]
        with np.errstate(all="ignore"):
            ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            unit = v / ln[:, None]
        good = ln > 0.0
        res = np.where(good[:, None], unit, np.array([0.0, 0.0, 1.0])[None, :])
        out[np.flatnonzero(full)] = res
    return out, dict(status=0 if ok.any() else 1, n_dropped=int((~ok).sum()), n_default=int((ok & ~full).sum()))
