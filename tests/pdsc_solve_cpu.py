"""Contract S1-S9 of lr_pdsc_solve (include/lidarreg.h) restated in numpy, stage by stage, so that a test can feed a stage
with the device's own upstream output.  Decisions (dead rows, the NMS predicate, orders, counts) are evaluated as the contract states
them -- the fp32 distance of S2 bit for bit; sums whose order the contract fixes for the device are evaluated in fp64 here (dtype =
float32 runs S3-S6 in numpy's fp32 instead: the yardstick of the device tests where no recording exists).  The last section
(solve_contract and its stages) evaluates S3-S9 in the contract's OWN order and arithmetic instead, to the bit: what
tests/test_gpu_pdsc_solve_exact.py holds the device to.  Nothing here is fast.
"""
import numpy as np
from scipy.spatial import cKDTree

C = 128
DEFAULTS = dict(num_iterations=10, k=40, refine_iters=20, ratio=0.1, nms_radius=0.6, inlier_threshold=0.6, refine_threshold=1.2, sigma_d=1.2, sigma=1.0)


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------
def live_rows(src, tgt, feat, conf):
    return np.isfinite(src).all(1) & np.isfinite(tgt).all(1) & np.isfinite(conf) & np.isfinite(feat).all(1)


# ---- S3 ---------------------------------------------------------------------------------------------------------------------------------
def normalize32(feat, live):
    """S3 in its own order, bit for bit what the contract states: float32 [m,128], zero on dead rows."""
    f = np.where(live[:, None], feat, 0).astype(np.float32)
    lane = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = f[:, 0::2] * f[:, 0::2] + f[:, 1::2] * f[:, 1::2]
        for d in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lane ^ d]
        den = np.maximum(np.sqrt(p[:, :1]), np.float32(1e-12))
        return np.where(live[:, None], f / den, np.float32(0)).astype(np.float32)


def normalize(feat, live, dtype=np.float64):
    if dtype == np.float32:
        return normalize32(feat, live)
    f = np.where(live[:, None], feat, 0).astype(np.float64)
    return f / np.maximum(np.linalg.norm(f, axis=1, keepdims=True), 1e-12)


# ---- S2 ---------------------------------------------------------------------------------------------------------------------------------
def dist32(a, b):
    """E3's fp32 distance of the rows of a and b (float32 [n,3])."""
    d = a.astype(np.float32) - b.astype(np.float32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def local_max(src, conf, live, R):
    """local_max(i) of S2 for every row (False on dead rows).  Candidate pairs come from a k-d tree with a widened radius; the
    predicate itself is the contract's fp32 one."""
    m = len(conf)
    lm = live.copy()
    idx = np.flatnonzero(live)
    if len(idx) < 2:
        return lm
    R32 = np.float32(R)
    pts = src[idx].astype(np.float64)
    pairs = cKDTree(pts).query_pairs(float(R32) * (1 + 1e-5) + 1e-4, output_type="ndarray")
    if len(pairs):
        i, j = idx[pairs[:, 0]], idx[pairs[:, 1]]
        near = dist32(src[i], src[j]) < R32
        i, j = i[near], j[near]
        lm[i[conf[i] < conf[j]]] = False
        lm[j[conf[j] < conf[i]]] = False
    return lm


def n_seeds(nlive, ratio):
    return int(nlive * ratio) if nlive >= 2 else 0


def seed_keys(conf, lm):
    return np.where(lm, conf, np.float32(0)).astype(np.float32)


def seed_order(key, live, n):
    """The first n live rows by descending key, ascending index on equal keys."""
    idx = np.flatnonzero(live)
    order = idx[np.argsort(-key[idx].astype(np.float64), kind="stable")]
    return order[:n].astype(np.int64)


def pick_seeds(src, conf, live, R, ratio):
    return seed_order(seed_keys(conf, local_max(src, conf, live, R)), live, n_seeds(int(live.sum()), ratio))


# ---- S4 ---------------------------------------------------------------------------------------------------------------------------------
def sims(fn, live, seeds):
    """fp64 similarities of the seeds to every row [len(seeds), m]: -inf on dead rows and on the seed itself."""
    s = fn[seeds].astype(np.float64) @ fn.astype(np.float64).T
    s[:, ~live] = -np.inf
    s[np.arange(len(seeds)), seeds] = -np.inf
    return s


def knn(fn, live, seeds, k, slab=256):
    """[n_seeds, k'] by descending similarity, ascending index on ties, and the similarities in that order."""
    kp = min(k, int(live.sum()) - 1)
    idx = np.zeros((len(seeds), kp), np.int64)
    val = np.zeros((len(seeds), kp))
    for lo in range(0, len(seeds), slab):
        s = sims(fn, live, seeds[lo:lo + slab])
        o = np.argsort(-s, axis=1, kind="stable")[:, :kp]
        idx[lo:lo + slab] = o
        val[lo:lo + slab] = np.take_along_axis(s, o, 1)
    return idx, val


# ---- S5, S6 ---------------------------------------------------------------------------------------------------------------------------------
def compat(s, t, sigma_d, dtype):
    """E3 over the rows of s, t [..., k, 3]: [..., k, k]."""
    s, t = s.astype(np.float32).astype(dtype), t.astype(np.float32).astype(dtype)
    ds, dt = s[..., :, None, :] - s[..., None, :, :], t[..., :, None, :] - t[..., None, :, :]
    la = np.sqrt((ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]) + ds[..., 2] * ds[..., 2])
    lb = np.sqrt((dt[..., 0] * dt[..., 0] + dt[..., 1] * dt[..., 1]) + dt[..., 2] * dt[..., 2])
    d = la - lb
    nk = dtype(np.float32(-1.0 / (sigma_d * sigma_d)))
    return np.maximum(dtype(0), d * d * nk + dtype(1))


def seed_weights(fn, src, tgt, nbr, sigma, sigma_d, num_iterations, dtype=np.float64, slab=512):
    """w [n_seeds, k'] of S6 for the neighbour lists nbr [n_seeds, k']."""
    ns, kp = nbr.shape
    w = np.zeros((ns, kp), dtype)
    nk = dtype(np.float32(-1.0 / (sigma * sigma)))
    eps = dtype(np.float32(1e-6))
    for lo in range(0, ns, slab):
        nb = nbr[lo:lo + slab]
        f = fn[nb].astype(dtype)
        M = np.maximum(dtype(0), (dtype(1) - f @ f.transpose(0, 2, 1)) * nk + dtype(1)) * compat(src[nb], tgt[nb], sigma_d, dtype)
        M[:, np.arange(kp), np.arange(kp)] = 0
        v = np.ones((len(nb), kp, 1), dtype)
        for _ in range(num_iterations):
            v = M @ v
            v = v / (np.sqrt((v * v).sum(1, keepdims=True)) + eps)
        v = v[:, :, 0]
        w[lo:lo + slab] = v / (v.sum(1, keepdims=True) + eps)
    return w


# ---- S7 ---------------------------------------------------------------------------------------------------------------------------------
def fit(A, B, w):
    """rigid_transform_3d (models/common.py:7-45) in fp64: A, B [n,3], w [n] -> T 4x4."""
    A, B, w = A.astype(np.float64), B.astype(np.float64), w.astype(np.float64)
    den = w.sum() + 1e-6
    ca, cb = (A * w[:, None]).sum(0) / den, (B * w[:, None]).sum(0) / den
    H = ((A - ca) * w[:, None]).T @ (B - cb)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, np.linalg.det(V @ U.T)])
    R = V @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T


def seed_transforms(src, tgt, nbr, w):
    return np.stack([fit(src[n], tgt[n], ww) for n, ww in zip(nbr, w)]) if len(nbr) else np.zeros((0, 4, 4))


# ---- S8 ---------------------------------------------------------------------------------------------------------------------------------
def residuals(T, src, tgt):
    """fp64 residuals of every row under T ([4,4] or [n,4,4] -> [m] or [n,m]); NaN rows stay NaN."""
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore"):
        p = np.einsum("...ij,mj->...mi", T[..., :3, :3], s) + T[..., None, :3, 3]
        return np.sqrt(((p - t) ** 2).sum(-1))


def counts(Ts, src, tgt, live, thr, slab=64):
    out = np.zeros(len(Ts), np.int64)
    for lo in range(0, len(Ts), slab):
        out[lo:lo + slab] = ((residuals(Ts[lo:lo + slab], src[live], tgt[live])) < thr).sum(1)
    return out


def labels(T, src, tgt, live, thr):
    with np.errstate(invalid="ignore"):
        return (live & (residuals(T, np.where(live[:, None], src, 0), np.where(live[:, None], tgt, 0)) < thr)).astype(np.uint8)


# ---- S9 ---------------------------------------------------------------------------------------------------------------------------------
def refine(T, src, tgt, live, thr, iters, last=None):
    """(T, fits run).  last: a list that receives (A, B, w) of the last fit."""
    s, t = src[live], tgt[live]
    prev, rounds = 0, 0
    for _ in range(iters):
        d = residuals(T, s, t)
        inl = d < thr
        if int(inl.sum()) == prev:
            break
        prev = int(inl.sum())
        T = fit(s[inl], t[inl], 1.0 / (1.0 + (d[inl] / thr) ** 2))
        if last is not None:
            last[:] = [s[inl].astype(np.float64), t[inl].astype(np.float64), 1.0 / (1.0 + (d[inl] / thr) ** 2)]
        rounds += 1
    return T, rounds


# ---- the whole tail -----------------------------------------------------------------------------------------------------------------------
def solve(src, tgt, feat, conf, dtype=np.float64, **kw):
    p = dict(DEFAULTS, **kw)
    m = len(conf)
    live = live_rows(src, tgt, feat, conf) if m else np.zeros(0, bool)
    out = dict(live=live, m=m, dead=int(m - live.sum()), T=np.eye(4), T_best=np.eye(4), labels=np.zeros(m, np.uint8), seeds=np.zeros(0, np.int64),
               best_rank=-1, best_index=-1, best_count=0, refine_rounds=0)
    if not live.any():
        return dict(out, status=1, n_seeds=0)
    seeds = pick_seeds(src, conf, live, p["nms_radius"], p["ratio"])
    if not len(seeds):
        return dict(out, status=2, n_seeds=0)
    fn = normalize(feat, live, dtype)
    nbr, _ = knn(fn, live, seeds, p["k"])
    w = seed_weights(fn, src, tgt, nbr, p["sigma"], p["sigma_d"], p["num_iterations"], dtype)
    Ts = seed_transforms(src, tgt, nbr, w)
    cnt = counts(Ts, src, tgt, live, p["inlier_threshold"])
    best = int(np.argmax(cnt))                       # (the first of the largest)
    T, rounds = refine(Ts[best], src, tgt, live, p["refine_threshold"], p["refine_iters"])
    return dict(out, status=0, n_seeds=len(seeds), seeds=seeds, fn=fn, knn=nbr, weights=w, seed_T=Ts, counts=cnt, best_rank=best,
                best_index=int(seeds[best]), best_count=int(cnt[best]), T_best=Ts[best], T=T, refine_rounds=rounds,
                labels=labels(Ts[best], src, tgt, live, p["inlier_threshold"]))


# ---- the contract's own arithmetic: S3 - S9 to the bit --------------------------------------------------------------------------------------
# What the fp64 functions above evaluate in numpy's order is evaluated here in the order §17.1 fixes for the device, so that the device
# has exactly one right answer: fmaf32 (tests/fcgf_cpu.py) wherever the contract says fmaf, numpy's float32 elementwise arithmetic (IEEE,
# unfused, subnormals kept) elsewhere in S5 / S6, fp64 elementwise arithmetic in the kernel's association in S7 - S9, lr_rt_from_cov through
# the oracle library.  fmaf32 forms a x b exactly in fp64, adds c with the error term (TwoSum), rounds that sum to odd and narrows once: 53
# bits rounded to odd narrow without a second rounding error to any grid of at most 51 bits, the fp32 subnormals' coarser grid included
# (tests/test_pdsc_solve_exact_cpu.py checks it against libm there).  Vectorised over the seeds; nothing here is fast.
from tests.dgr_cpu import tree_sum
from tests.fcgf_cpu import fmaf32

F32 = np.float32


def sims_chain(fn32, seeds, slab=64):
    """S4's similarity of the seeds to every row, float32 [len(seeds), m]: one fmaf chain per (seed, key), channels c and 64 + c per step."""
    fn32 = np.ascontiguousarray(fn32, F32)
    out = np.empty((len(seeds), len(fn32)), F32)
    cols = np.ascontiguousarray(fn32.T)
    for lo in range(0, len(seeds), slab):
        q = fn32[seeds[lo:lo + slab]]
        acc = np.zeros((len(q), len(fn32)), F32)
        for c in range(64):
            acc = fmaf32(cols[64 + c][None, :], q[:, 64 + c, None], fmaf32(cols[c][None, :], q[:, c, None], acc))
        out[lo:lo + slab] = acc
    return out


def sims_exact(fn32, seeds):
    """The same where every product and every partial sum is exact in fp32 (the lattice features of tests/pdsc_solve_exact_cases.py): any
    order gives the chain's value, so one matmul does."""
    return (fn32[seeds].astype(np.float64) @ fn32.astype(np.float64).T).astype(F32)


def knn_contract(sim, live, seeds, k, grid=None):
    """S4's lists [n_seeds, k'] from the similarities [n_seeds, m]: live rows other than the seed by descending similarity, ascending index
    on ties.  grid: the similarities are exact multiples of 1 / grid -- the top k' are then taken by a partition on the integer key
    round(grid sim) 2^15 + (32767 - index), which orders as S4 does."""
    kp = min(k, int(live.sum()) - 1)
    ns, m = sim.shape
    if grid is None:
        s = sim.astype(np.float64)
        s[:, ~live] = -np.inf
        s[np.arange(ns), seeds] = -np.inf
        return np.argsort(-s, axis=1, kind="stable")[:, :kp].astype(np.int64)
    assert m <= 32768
    key = np.rint(sim.astype(np.float64) * grid).astype(np.int64) * 32768 + (32767 - np.arange(m, dtype=np.int64))
    key[:, ~live] = -2 ** 62
    key[np.arange(ns), seeds] = -2 ** 62
    part = np.argpartition(-key, kp - 1, axis=1)[:, :kp]
    return np.take_along_axis(part, np.argsort(-np.take_along_axis(key, part, 1), axis=1), 1).astype(np.int64)


def knn_exact(fn32, live, seeds, k, grid, slab=512):
    """S4's lists where the similarities are exact multiples of 1 / grid: sims_exact and the integer partition, a slab of seeds at a time."""
    return np.concatenate([knn_contract(sims_exact(fn32, seeds[lo:lo + slab]), live, seeds[lo:lo + slab], k, grid) for lo in range(0, len(seeds), slab)])


def butterfly64(p):
    """The butterfly of S3 / S6 over 64 lanes, float32 [n, 64] -> [n]."""
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ d]
    return p[:, 0]


def _lanes(x):
    p = np.zeros((len(x), 64), F32)
    p[:, :x.shape[1]] = x
    return p


def matrix_chain(fn32, src, tgt, nbr, sigma, sigma_d, exact_dot=False):
    """S5: M float32 [n, k', k'] of the lists nbr.  exact_dot: the dot products are exact in fp32 in any order (lattice features)."""
    f = fn32[nbr]
    n, kp = nbr.shape
    if exact_dot:
        dot = (f.astype(np.float64) @ f.astype(np.float64).transpose(0, 2, 1)).astype(F32)
    else:
        dot = np.zeros((n, kp, kp), F32)
        for c in range(C):
            dot = fmaf32(f[:, :, None, c], f[:, None, :, c], dot)
    nk_f, nk_d = F32(-1.0 / (sigma * sigma)), F32(-1.0 / (sigma_d * sigma_d))
    one = F32(1)
    fs = np.maximum(F32(0), fmaf32(one - dot, nk_f, one))
    s, t = src[nbr].astype(F32), tgt[nbr].astype(F32)
    ds, dt = s[:, :, None, :] - s[:, None, :, :], t[:, :, None, :] - t[:, None, :, :]
    la = np.sqrt((ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]) + ds[..., 2] * ds[..., 2])
    lb = np.sqrt((dt[..., 0] * dt[..., 0] + dt[..., 1] * dt[..., 1]) + dt[..., 2] * dt[..., 2])
    d = la - lb
    M = fs * np.maximum(F32(0), fmaf32(d * d, nk_d, one))
    M[:, np.arange(kp), np.arange(kp)] = 0
    assert M.dtype == F32
    return M


def power_chain(M, num_iterations):
    """S6 on S5's matrices: w float32 [n, k']."""
    n, kp, _ = M.shape
    eps = F32(1e-6)
    v = np.ones((n, kp), F32)
    with np.errstate(under="ignore"):
        for _ in range(num_iterations):
            u = np.zeros((n, kp), F32)
            for b in range(kp):
                u = fmaf32(M[:, :, b], v[:, b:b + 1], u)
            v = u / (np.sqrt(butterfly64(_lanes(u * u))) + eps)[:, None]
        w = v / (butterfly64(_lanes(v)) + eps)[:, None]
    assert w.dtype == F32
    return w


def weights_chain(fn32, src, tgt, nbr, sigma, sigma_d, num_iterations, exact_dot=False, slab=128):
    """S5 and S6: w float32 [n_seeds, k'] of the neighbour lists nbr."""
    w = np.zeros(nbr.shape, F32)
    for lo in range(0, len(nbr), slab):
        w[lo:lo + slab] = power_chain(matrix_chain(fn32, src, tgt, nbr[lo:lo + slab], sigma, sigma_d, exact_dot), num_iterations)
    return w


_ORACLE = []          # the oracle library, built (if stale) and loaded at the first fit


def rt_from_cov(H, ca, cb):
    """lr_rt_from_cov (csrc/lr_contract.h) through the oracle library: H [3,3], ca, cb [3] -> T [4,4]."""
    import ctypes
    from oracle import oracle as orc
    if not _ORACLE:
        orc.build()
        _ORACLE.append(orc.lib())
    f64 = ctypes.POINTER(ctypes.c_double)
    H, ca, cb, T = np.ascontiguousarray(H, np.float64).reshape(9), np.ascontiguousarray(ca, np.float64), np.ascontiguousarray(cb, np.float64), np.empty(16)
    _ORACLE[0].orc_rt_from_cov(H.ctypes.data_as(f64), ca.ctypes.data_as(f64), cb.ctypes.data_as(f64), T.ctypes.data_as(f64))
    return T.reshape(4, 4)


def fit_contract(src, tgt, nbr, w):
    """S7 as ps_seedfit_kernel associates it: seven sequential fp64 sums over the neighbours ascending, the centroids over W + 1e-6, nine
    sequential sums (w (a_x - ca_x)) (b_y - cb_y), lr_rt_from_cov.  [n_seeds, 4, 4]."""
    n, kp = nbr.shape
    A, B, w = src[nbr].astype(np.float64), tgt[nbr].astype(np.float64), w.astype(np.float64)
    P = np.concatenate([A, B], 2)
    s = np.zeros((n, 7))
    for b in range(kp):
        s[:, 0] = s[:, 0] + w[:, b]
        s[:, 1:] = s[:, 1:] + w[:, b, None] * P[:, b]
    den = s[:, 0] + 1e-6
    cen = s[:, 1:] / den[:, None]
    H = np.zeros((n, 3, 3))
    for b in range(kp):
        H = H + (w[:, b, None, None] * (A[:, b, :, None] - cen[:, :3, None])) * (B[:, b, None, :] - cen[:, None, 3:])
    return np.stack([rt_from_cov(H[i], cen[i, :3], cen[i, 3:]) for i in range(n)]) if n else np.zeros((0, 4, 4))


def resid_contract(T, src, tgt):
    """S8's residual in its association: T [4,4] or [n,4,4], src / tgt [m,3] -> [m] or [n,m] float64."""
    T = np.asarray(T, np.float64)
    Ts = T.reshape(-1, 4, 4)
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    sx, sy, sz = s[None, :, 0], s[None, :, 1], s[None, :, 2]
    with np.errstate(invalid="ignore"):
        d = [(((Ts[:, x, 0, None] * sx + Ts[:, x, 1, None] * sy) + Ts[:, x, 2, None] * sz) + Ts[:, x, 3, None]) - t[None, :, x] for x in range(3)]
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return r[0] if T.ndim == 2 else r


def _records(src, tgt, live):
    """The rows as the kernels' records hold them: zeros on dead rows."""
    return np.where(live[:, None], src, 0).astype(np.float64), np.where(live[:, None], tgt, 0).astype(np.float64)


def counts_contract(Ts, src, tgt, live, thr, slab=64):
    s, t = _records(src, tgt, live)
    out = np.zeros(len(Ts), np.int64)
    for lo in range(0, len(Ts), slab):
        out[lo:lo + slab] = (live[None, :] & (resid_contract(Ts[lo:lo + slab], s, t) < thr)).sum(1)
    return out


def labels_contract(T, src, tgt, live, thr):
    s, t = _records(src, tgt, live)
    return (live & (resid_contract(T, s, t) < thr)).astype(np.uint8)


def refine_contract(T, src, tgt, live, thr, iters):
    """S9: (T, fits run).  Every sum in E2's tree over ALL rows (dgr_cpu.tree_sum is lr_block_tree_sum<1024> behind the threads' ascending
    partials); a row that is dead or no inlier adds nothing to its thread's partial -- here +0.0, which changes no bit of a partial that
    started from +0.0."""
    s, t = _records(src, tgt, live)
    r = np.concatenate([s, t], 1)
    T = np.array(T, np.float64)
    prev, rounds = 0, 0
    for _ in range(iters):
        d = resid_contract(T, s, t)
        inl = live & (d < thr)
        n = int(inl.sum())
        if n == prev:
            break
        prev = n
        e = d / thr
        w = np.where(inl, 1.0 / (1.0 + e * e), 0.0)
        den = tree_sum(w)[0] + 1e-6
        cen = tree_sum(np.where(inl[:, None], w[:, None] * r, 0.0)) / den
        terms = (w[:, None, None] * (r[:, :3, None] - cen[None, :3, None])) * (r[:, None, 3:] - cen[None, None, 3:])
        H = tree_sum(np.where(inl[:, None], terms.reshape(-1, 9), 0.0)).reshape(3, 3)
        T = rt_from_cov(H, cen[:3], cen[3:])
        rounds += 1
    return T, rounds


def solve_contract(src, tgt, feat, conf, lattice=False, **kw):
    """The whole tail from the inputs alone, in the contract's own arithmetic: everything pointdsc.solve(..., trace=True) returns.
    lattice: the features are those of tests/pdsc_solve_exact_cases.py (S4 and S5's dot products exact multiples of 1/64: a matmul)."""
    p = dict(DEFAULTS, **kw)
    m = len(conf)
    live = live_rows(src, tgt, feat, conf) if m else np.zeros(0, bool)
    out = dict(live=live, m=m, dead=int(m - live.sum()), T=np.eye(4), T_best=np.eye(4), labels=np.zeros(m, np.uint8), seeds=np.zeros(0, np.int64),
               best_rank=-1, best_index=-1, best_count=0, n_labels=0, refine_rounds=0, n_seeds=0)
    if not live.any():
        return dict(out, status=1)
    seeds = pick_seeds(src, conf, live, p["nms_radius"], p["ratio"])
    if not len(seeds):
        return dict(out, status=2)
    fn = normalize32(feat, live)
    nbr = knn_exact(fn, live, seeds, p["k"], grid=64) if lattice else knn_contract(sims_chain(fn, seeds), live, seeds, p["k"])
    w = weights_chain(fn, src, tgt, nbr, p["sigma"], p["sigma_d"], p["num_iterations"], exact_dot=lattice)
    Ts = fit_contract(src, tgt, nbr, w)
    cnt = counts_contract(Ts, src, tgt, live, p["inlier_threshold"])
    best = int(np.argmax(cnt))
    T, rounds = refine_contract(Ts[best], src, tgt, live, p["refine_threshold"], p["refine_iters"])
    lab = labels_contract(Ts[best], src, tgt, live, p["inlier_threshold"])
    return dict(out, status=0, n_seeds=len(seeds), seeds=seeds, fn=fn, knn=nbr, weights=w, seed_T=Ts, counts=cnt, best_rank=best,
                best_index=int(seeds[best]), best_count=int(cnt[best]), T_best=Ts[best], T=T, refine_rounds=rounds, labels=lab, n_labels=int(lab.sum()))


# ---- the kNN kernel's plan (ps_make_plan, ps_max_blocks of csrc/lr_pdsc_solve.hip) -------------------------------------------------------------
def plan(n_seeds_, m):
    nsb = (n_seeds_ + 127) // 128 if n_seeds_ > 0 else 1
    ch = max(1, min(8, 512 // nsb))
    tiles = (m + 31) // 32 if m > 0 else 1
    ch = min(ch, tiles)
    tpc = (tiles + ch - 1) // ch
    return dict(nsb=nsb, chunks=(tiles + tpc - 1) // tpc, per=tpc * 32)


def max_blocks(smax):
    nsb = (smax + 127) // 128 if smax > 0 else 1
    return min(8 * nsb, max(512, nsb))
