"""numpy restatement of contracts N (lr_nn3) and Z (lr_refine_z) of include/lidarreg.h / DESIGN.md §13, independent of the library: the
nearest neighbour by brute force, the median from a sort of the bit patterns, the two-level sum as cumulative sums.  float64 throughout;
numpy's element-wise + - * / sqrt are IEEE operations without fused multiply-add, so every line here is the contract's arithmetic."""
import os

import numpy as np

RUN = 1024          # run length of the two-level sum (Z6)


def transform(X, T):
    """C1 of the overlap contract: ((T[a,0] x + T[a,1] y) + T[a,2] z) + T[a,3]; T None: the points as they are."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    if T is None:
        return X.copy()
    T = np.asarray(T, np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def d2_matrix(A, B):
    """N2 for every (i, j)."""
    with np.errstate(over="ignore", invalid="ignore"):
        M = A[:, None, 0] - B[None, :, 0]; M *= M
        t = A[:, None, 1] - B[None, :, 1]; t *= t; M += t
        t = A[:, None, 2] - B[None, :, 2]; t *= t; M += t
        return M


def nn(A, B, chunk=64, second=False):
    """N1-N5: (dist float64[n0], idx int64[n0], info dict).  Brute force over chunks of queries (on threads: numpy's loops release the
    lock); argmin returns the first minimum: the lowest-j rule.  second: also the second-smallest distance of every query (inf where there
    is none), for the conditions the golden inputs must meet."""
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
    n0 = len(A)
    okB = np.isfinite(B).all(axis=1); okA = np.isfinite(A).all(axis=1)
    live = np.flatnonzero(okB)
    Bl = np.ascontiguousarray(B[live])
    idx = np.full(n0, -1, np.int64); d2 = np.full(n0, np.inf); d2b = np.full(n0, np.inf)

    def work(s):
        q = np.flatnonzero(okA[s:s + chunk]) + s
        if not len(q):
            return
        M = d2_matrix(A[q], Bl)
        k = np.argmin(M, axis=1)
        r = np.arange(len(q))
        idx[q] = live[k]; d2[q] = M[r, k]
        if second and len(live) > 1:
            M[r, k] = np.inf
            d2b[q] = M.min(axis=1)

    if len(live) and n0:
        starts = range(0, n0, chunk)
        if n0 * len(live) < 1 << 22:
            for s in starts:
                work(s)
        else:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
                list(ex.map(work, starts))
    info = dict(status=0 if len(live) else 1, n0_dropped=int((~okA).sum()), n1_dropped=int((~okB).sum()))
    out = (np.sqrt(d2), idx, info)
    return out + (np.sqrt(d2b),) if second else out


TREE_K = 8          # candidates per query of nn_tree
TREE_CLEAR = 1e-9   # the k-th tree distance must exceed the best by this relative margin (the tree's own arithmetic is good to a few ulp)


def nn_tree(A, B, second=False, stats=None):
    """N1-N5 as nn returns them, in O(n log n): scipy's k-d tree proposes TREE_K candidates per finite query, the contract's d2 (N2) is
    re-evaluated on them and the minimum taken.  A target outside the candidates is at least the k-th tree distance d_k away, so the
    candidates hold the answer whenever d_k > d_1 (1 + 1e-9) (with `second`: d_2 in place of d_1) and d_k lies in 1e-150 .. 1e150, where
    squares neither underflow nor overflow.  Every other query -- and every query whose best d2 is attained by two candidates, so that
    the lowest-index rule is only ever applied by nn's argmin -- is resolved by nn itself, brute force over all targets; with fewer
    than TREE_K live targets all queries are.  stats: a dict that receives fallback = the number of queries resolved by brute force."""
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
    n0 = len(A)
    okB = np.isfinite(B).all(axis=1); okA = np.isfinite(A).all(axis=1)
    live, q = np.flatnonzero(okB), np.flatnonzero(okA)
    idx = np.full(n0, -1, np.int64); d = np.full(n0, np.inf); db = np.full(n0, np.inf)
    brute = q
    if len(live) >= TREE_K and len(q):
        from scipy.spatial import cKDTree
        Bl, Aq = B[live], A[q]
        dt, jt = cKDTree(Bl).query(Aq, k=TREE_K, workers=min(16, os.cpu_count() or 1))
        C = Bl[jt]                                                           # [nq, k, 3]
        with np.errstate(over="ignore", invalid="ignore"):
            M = Aq[:, None, 0] - C[:, :, 0]; M *= M
            t = Aq[:, None, 1] - C[:, :, 1]; t *= t; M += t
            t = Aq[:, None, 2] - C[:, :, 2]; t *= t; M += t
            near = dt[:, 1] if second else dt[:, 0]
            clear = (dt[:, -1] > near * (1.0 + TREE_CLEAR)) & (dt[:, -1] > 1e-150) & (dt[:, -1] < 1e150)
        best = M.min(axis=1)
        clear &= (M == best[:, None]).sum(axis=1) == 1
        r = np.flatnonzero(clear)
        idx[q[r]] = live[jt[r, np.argmin(M[r], axis=1)]]; d[q[r]] = np.sqrt(best[r])
        if second:
            db[q[r]] = np.sqrt(np.partition(M[r], 1, axis=1)[:, 1])
        brute = q[~clear]
    if len(brute) and len(live):
        out = nn(A[brute], B, second=second)
        d[brute], idx[brute] = out[0], out[1]
        if second:
            db[brute] = out[3]
    if stats is not None:
        stats["fallback"] = int(len(brute)) if len(live) else 0
    info = dict(status=0 if len(live) else 1, n0_dropped=int((~okA).sum()), n1_dropped=int((~okB).sum()))
    return (d, idx, info, db) if second else (d, idx, info)

def two_level_sum(t):
    """Z6's S: every run of 1024 consecutive terms summed left to right from +0, then the run sums left to right."""
    t = np.ascontiguousarray(t, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        runs = [np.cumsum(np.concatenate([[0.0], t[s:s + RUN]]))[-1] for s in range(0, len(t), RUN)]
        return np.cumsum(np.concatenate([[0.0], runs]))[-1]


def median(w):
    """Z4: numpy's median of non-negative doubles (+inf included), from the order of their bit patterns."""
    k = np.sort(np.ascontiguousarray(w, np.float64).view(np.uint64))
    n = len(k)
    lo, hi = k[(n - 1) >> 1:((n - 1) >> 1) + 1].view(np.float64)[0], k[n >> 1:(n >> 1) + 1].view(np.float64)[0]
    if n & 1:
        return lo
    with np.errstate(over="ignore"):
        return (lo + hi) / 2.0


def refine_z(A, B, T=None, xy_gate=0.3, max_repeats=10, min_change=1e-6, trace=None, search=None):
    """Contract Z.  Returns the result block as a dict.  trace: a list that receives, per repeat, dict(ind, valid, mean, xy, d, d_second).
    search: the nearest-neighbour restatement to use, nn (the default) or nn_tree."""
    search = nn if search is None else search
    A_ = transform(A, T)
    B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
    dz, status, repeats, n_valid, mean = 0.0, 0, 0, 0, 0.0
    n0_dropped = n1_dropped = 0
    for _ in range(max_repeats):
        if trace is None:
            d, ind, info = search(A_, B)
            d_second = None
        else:
            d, ind, info, d_second = search(A_, B, second=True)
        if repeats == 0:
            n0_dropped, n1_dropped = info["n0_dropped"], info["n1_dropped"]
        repeats += 1
        has = ind >= 0
        Bs = B[np.where(has, ind, 0)] if len(B) else np.zeros_like(A_)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            dx, dy = A_[:, 0] - Bs[:, 0], A_[:, 1] - Bs[:, 1]
            xy = np.sqrt(dx * dx + dy * dy)
            valid = has & (xy <= xy_gate)
            z = A_[:, 2] - Bs[:, 2]
            w = 1.0 / np.abs(z)
        n_valid = int(valid.sum())
        mean = 0.0
        if n_valid == 0:
            status = 1
        else:
            med = median(w[valid])
            if med == np.inf:
                status = 2
            else:
                with np.errstate(over="ignore", invalid="ignore"):
                    wc = np.where(valid, np.minimum(w, med), 0.0)
                    num = two_level_sum(np.where(valid, wc * np.where(valid, z, 0.0), 0.0)); den = two_level_sum(wc)
                    mean = num / den
        if trace is not None:
            trace.append(dict(ind=ind.copy(), valid=valid.copy(), mean=mean, xy=xy, d=d, d_second=d_second, z=z))
        with np.errstate(over="ignore", invalid="ignore"):
            A_[:, 2] = A_[:, 2] - mean
        dz = dz - mean
        if status != 0 or abs(mean) < min_change:
            break
    return dict(status=status, repeats=repeats, n_valid=n_valid, n0_dropped=n0_dropped, n1_dropped=n1_dropped, reserved=0, dz=float(dz), last_step=float(mean))
