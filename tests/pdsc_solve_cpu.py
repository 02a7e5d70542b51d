"""Contract S1-S9 of lr_pdsc_solve (include/lidarreg.h) restated in numpy, stage by stage, so that a test can feed a stage
with the device's own upstream output.  Decisions (dead rows, the NMS predicate, orders, counts) are evaluated as the contract states
them -- the fp32 distance of S2 bit for bit; sums whose order the contract fixes for the device are evaluated in fp64 here (dtype =
float32 runs S3-S6 in numpy's fp32 instead: the yardstick of the device tests where no recording exists).  Nothing here is fast.
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
