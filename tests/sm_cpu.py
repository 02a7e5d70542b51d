"""Spectral matching restated in numpy -- the yardstick of csrc/lr_sm.hip (contract: include/lidarreg.h).

Independent of the device code: the compatibility matrix is formed whole (in row slabs), the power iteration is a matrix product, the
selection a lexsort, the fit a weighted Kabsch by SVD (Experiments/models/common.py:7-45).  dtype float64 is the reference the GPU is
held to; dtype float32 measures what fp32 arithmetic alone costs on a case (the tolerance of the eigenvector test is a multiple of
THAT distance, never of the kernel's)."""
import functools

import numpy as np


def finite_rows(a, b):
    return np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)


def compat(a, b, thr, dtype=np.float64, slab=512):
    """C [M,M]: max(0, 4.5 - d^2 / (2 sigma^2)), d = |a_i - a_j| - |b_i - b_j| on direct differences; diagonal 0 by index; rows and
    columns of a non-finite correspondence 0."""
    M = len(a)
    ok = finite_rows(a, b)
    A = np.where(ok[:, None], a, 0).astype(dtype); B = np.where(ok[:, None], b, 0).astype(dtype)
    sigma = thr / 3.0
    C = np.empty((M, M), dtype)
    for i0 in range(0, M, slab):
        da = A[i0:i0 + slab, None, :] - A[None, :, :]
        db = B[i0:i0 + slab, None, :] - B[None, :, :]
        la = np.sqrt((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2])
        lb = np.sqrt((db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1]) + db[..., 2] * db[..., 2])
        d = la - lb
        if dtype == np.float32:
            c = np.maximum(np.float32(0), (d * d) * np.float32(-1.0 / (2.0 * sigma * sigma)) + np.float32(4.5))
        else:
            c = np.maximum(0.0, 4.5 - d * d / (2.0 * sigma * sigma))
        C[i0:i0 + slab] = c
    C[np.arange(M), np.arange(M)] = 0
    C[~ok, :] = 0; C[:, ~ok] = 0
    return C


def power(C, iterations=10):
    v = np.ones(len(C), C.dtype)
    for _ in range(iterations):
        v = C @ v
        v = v / (np.sqrt((v * v).sum(dtype=C.dtype)) + C.dtype.type(1e-6))
    return v


def top_k(M, ratio):
    return int(M * ratio)


def select(v, K):
    """Indices of the K largest under (value descending, index ascending), ascending."""
    order = np.lexsort((np.arange(len(v)), -np.asarray(v, np.float64)))
    return np.sort(order[:K])


def kabsch_weighted(a, b, w):
    """common.py:7-45 in fp64: centroids over (sum w + 1e-6), H = Am^T diag(w) Bm, R = V diag(1,1,det(V U^T)) U^T.  Entries of weight 0 are not read."""
    use = np.asarray(w) > 0
    A = np.asarray(a, np.float64)[use]; B = np.asarray(b, np.float64)[use]; W = np.asarray(w, np.float64)[use]
    den = W.sum() + 1e-6
    ca = (A * W[:, None]).sum(0) / den; cb = (B * W[:, None]).sum(0) / den
    H = (A - ca).T @ ((B - cb) * W[:, None])
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, np.linalg.det(V @ U.T)])
    R = V @ D @ U.T
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = cb - R @ ca
    return T


def sm(a, b, thr=0.6, ratio=0.05, iterations=10, dtype=np.float64, m=None):
    """The whole solver on the first m (default: all) correspondences: dict(v, K, sel, labels, w_sum, status, T)."""
    m = len(a) if m is None else int(m)
    a, b = np.asarray(a)[:m], np.asarray(b)[:m]
    v = power(compat(a, b, thr, dtype), iterations) if m else np.zeros(0, dtype)
    K = top_k(m, ratio)
    sel = select(v, K)
    labels = np.zeros(m, np.uint8); labels[sel] = 1
    w = np.asarray(v, np.float64) * labels
    status = 1 if (K < 3 or not w.sum() > 0) else 0
    T = np.eye(4) if status else kabsch_weighted(a, b, w)
    return dict(v=v, K=K, sel=sel, labels=labels, w_sum=float(w.sum()), status=status, T=T)


def planted_v(M, pairs, iterations=10):
    """The eigenvector of sm_cases.line(M) with disjoint planted partner pairs, in closed form: every planted entry has exactly one
    partner with c = 4.5 and every other c is 0, so the 2 len(pairs) non-zero entries stay equal to one scalar s: s0 = 1, u = 4.5 s,
    s <- u / (u sqrt(n) + 1e-6), `iterations` times.  fp64 [M]."""
    idx = np.array([i for pq in pairs for i in pq], np.int64)
    v = np.zeros(M, np.float64)
    if len(idx):
        s = 1.0
        for _ in range(iterations):
            u = 4.5 * s
            s = u / (u * np.sqrt(float(len(idx))) + 1e-6)
        v[idx] = s
    return v


def planted_distances(a, b, q):
    """d(q, j) = |a_q - a_j| - |b_q - b_j| for every j of an integer-valued set on the x axis, in exact integer arithmetic: int64 [M]."""
    assert not a[:, 1:].any() and not b[:, 1:].any()
    ax, bx = a[:, 0].astype(np.int64), b[:, 0].astype(np.int64)
    assert np.array_equal(ax, a[:, 0]) and np.array_equal(bx, b[:, 0])
    return np.abs(ax[q] - ax) - np.abs(bx[q] - bx)


def plan(m, cus=256):
    """The matvec's work plan restated from sm_make_plan (csrc/lr_sm.hip): (row blocks of 64, column chunks, columns per chunk) for a
    live count m on a device of `cus` compute units."""
    target = min(max(8 * cus, 64), 4096)
    rb = (m + 63) >> 6 if m > 0 else 1
    ch = max(1, min(target // rb, rb, 64))
    m4 = (m + 3) & ~3 if m > 0 else 4
    per = (((m4 + ch - 1) // ch) + 3) & ~3
    return rb, (m4 + per - 1) // per, per


def power_chunked32(C, per, iterations=10, slab=2048):
    """The power iteration on an fp32 C with the contract's order of summation: a row's sum runs in fp32 IN SEQUENCE over each chunk
    of `per` columns (np.cumsum: one running fp32 sum), the chunks of a row, the norm and the division in fp64, v rounded to fp32 once
    per iteration.  What the device's order of summation alone costs against numpy's blocked fp32 matvec."""
    M = len(C)
    v = np.ones(M, np.float32)
    for _ in range(iterations):
        s = np.zeros(M, np.float64)
        for i0 in range(0, M, slab):
            for j0 in range(0, M, per):
                s[i0:i0 + slab] += np.cumsum(C[i0:i0 + slab, j0:j0 + per] * v[j0:j0 + per], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        v = (s / (np.sqrt((s * s).sum()) + 1e-6)).astype(np.float32)
    return v


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name="float64"):
    """sm() of a case of tests/sm_cases.py, computed once per process and shared (read-only)."""
    from tests import sm_cases
    c = sm_cases.by_name(name)
    r = sm(c["a"], c["b"], c["thr"], c["ratio"], 10, np.dtype(dtype_name).type)
    for x in r.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return r


def rot_dist(T1, T2):
    return float(np.linalg.norm(np.asarray(T1)[:3, :3] - np.asarray(T2)[:3, :3]))


def rot_angle(T1, T2):
    """Angle between the rotations from |R1 - R2|_F = 2 sqrt(2) sin(angle / 2): well conditioned near 0, where arccos of the trace turns
    the 1e-7 rounding of a float32 matrix into 1e-3 rad."""
    return float(2.0 * np.arcsin(min(1.0, rot_dist(T1, T2) / (2.0 * np.sqrt(2.0)))))


def trans_dist(T1, T2):
    return float(np.linalg.norm(np.asarray(T1)[:3, 3] - np.asarray(T2)[:3, 3]))
