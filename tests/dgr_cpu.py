"""Contract G1-G9 of lr_dgr_refine (include/lidarreg.h d1) restated in numpy: the weighted Huber refinement of Deep Global
Registration over a 6-D rotation and a translation, with Adam.  fp64 throughout, only + - * / sqrt in the contract's association, the sums
in G2's tree, so the device equals this text bit for bit.  Per-correspondence arithmetic is vectorised (elementwise numpy is IEEE and
unfused); what one lane does on the device is written on Python floats.  The fit of G3 is lr_rt_from_moments of csrc/lr_contract.h, the one
text the oracle library compiles for the host.  Nothing here is fast.
"""
import ctypes
import math

import numpy as np

NB = 1024
EPS = float(np.finfo(np.float32).eps)      # 2^-23
CLAMP = 1e-8
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
LOSS_STOP = 1e-7
DEFAULTS = dict(max_iter=1000, max_break=20, quantization_size=1.0, lr=0.1, gamma=0.999, ratio=1e-5, clip=0.0, wsum_threshold=0.0)


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------
def live_rows(src, tgt, w, clip):
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(src).all(1) & np.isfinite(tgt).all(1) & np.isfinite(w) & (w > 0) & (w.astype(np.float64) >= clip)


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------
def tree_sum(v):
    """S over the columns of v [L] or [L,k]: thread t adds entries t, t + 1024, ... from +0.0 (a partial from +0.0 is never -0.0, so the +0.0
    padding changes no bit), then s[t] += s[t + h], h = 512 .. 1."""
    v = np.asarray(v, np.float64)
    v = v[:, None] if v.ndim == 1 else v
    rows = -(-len(v) // NB)
    pad = np.zeros((rows * NB, v.shape[1]))
    pad[:len(v)] = v
    s = np.zeros((NB, v.shape[1]))
    for r in range(rows):
        s = s + pad[r * NB:(r + 1) * NB]
    h = NB // 2
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------------
def rt_from_moments(mom):
    """lr_rt_from_moments (csrc/lr_contract.h) through the oracle library: mom = { n, sum p [3], sum q [3], sum p q^T [9] } -> T [16]."""
    from oracle import oracle as orc
    f64 = ctypes.POINTER(ctypes.c_double)
    mom = np.ascontiguousarray(mom, np.float64)
    sp, sq, spq, T = mom[1:4].copy(), mom[4:7].copy(), mom[7:16].copy(), np.empty(16)
    orc.lib().orc_kabsch_moments(ctypes.c_double(float(mom[0])), sp.ctypes.data_as(f64), sq.ctypes.data_as(f64), spq.ctypes.data_as(f64), T.ctypes.data_as(f64))
    return T


def moments(X, Y, w, w1):
    wn = w / (w1 + EPS)
    wx = wn[:, None] * X
    cols = [wn[:, None], wx, wn[:, None] * Y] + [wx[:, a:a + 1] * Y for a in range(3)]
    return tree_sum(np.concatenate(cols, 1))


def init_params(X, Y, w, w1, T_init=None):
    """p = (a, b, t): nine Python floats."""
    if T_init is not None:
        T = np.asarray(T_init, np.float64).reshape(16)
    else:
        T = rt_from_moments(moments(X, Y, w, w1))
        with np.errstate(over="ignore"):
            T[:12] = T[:12].astype(np.float32).astype(np.float64)
    return [float(T[4 * x]) for x in range(3)] + [float(T[4 * x + 1]) for x in range(3)] + [float(T[4 * x + 3]) for x in range(3)]


# ---- G4, on one lane ---------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _clamp(v):
    return CLAMP if v < CLAMP else v


def _sqrt(v):
    return float(np.sqrt(np.float64(v)))


def _div(a, b):
    """IEEE division on Python floats (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b))


def rotation(p):
    """G4: dict with the columns x, y, z and what the back-propagation reads."""
    with np.errstate(all="ignore"):
        a, b = list(p[:3]), list(p[3:6])
        na = _sqrt(_dot(a, a))
        da = _clamp(na)
        x = [_div(a[k], da) for k in range(3)]
        xx = _dot(x, x)
        n2 = _clamp(xx)
        xb = _dot(x, b)
        c = _div(xb, n2)
        u = [b[k] - c * x[k] for k in range(3)]
        nu = _sqrt(_dot(u, u))
        du = _clamp(nu)
        y = [_div(u[k], du) for k in range(3)]
        z = _cross(x, y)
    return dict(x=x, y=y, z=z, b=b, na=na, nu=nu, xx=xx, xb=xb, n2=n2, c=c)


def rotation_matrix(p):
    o = rotation(p)
    return np.array([o["x"], o["y"], o["z"]], np.float64).T


def rotation_back(o, G):
    """G6's one-lane part: G [3,3] = d loss / d R -> (da, db), six Python floats."""
    with np.errstate(all="ignore"):
        x, y, b, c, n2 = o["x"], o["y"], o["b"], o["c"], o["n2"]
        Gx, Gy, Gz = ([float(G[k][j]) for k in range(3)] for j in range(3))
        t = _cross(y, Gz)
        Gx = [Gx[k] + t[k] for k in range(3)]
        t = _cross(Gz, x)
        Gy = [Gy[k] + t[k] for k in range(3)]
        if o["nu"] < CLAMP:
            du = [_div(Gy[k], CLAMP) for k in range(3)]
        else:
            yg = _dot(y, Gy)
            du = [_div(Gy[k] - y[k] * yg, o["nu"]) for k in range(3)]
        dc = -_dot(du, x)
        Gx = [Gx[k] - c * du[k] for k in range(3)]
        t1 = _div(dc, n2)
        Gx = [Gx[k] + t1 * b[k] for k in range(3)]
        db = [du[k] + t1 * x[k] for k in range(3)]
        if not o["xx"] < CLAMP:
            dn2 = -_div(dc * o["xb"], n2 * n2)
            Gx = [Gx[k] + (2.0 * dn2) * x[k] for k in range(3)]
        if o["na"] < CLAMP:
            da = [_div(Gx[k], CLAMP) for k in range(3)]
        else:
            xg = _dot(x, Gx)
            da = [_div(Gx[k] - x[k] * xg, o["na"]) for k in range(3)]
    return da + db


# ---- G5, G6 -----------------------------------------------------------------------------------------------------------------------------
def loss_and_sums(X, Y, w, w1, q, R, t):
    """The thirteen sums of an iteration: loss, dt [3], G [3,3]; also s [L] (the test's premise: the least |s - 1|)."""
    with np.errstate(all="ignore"):
        r = np.stack([((((R[a][0] * X[:, 0] + R[a][1] * X[:, 1]) + R[a][2] * X[:, 2]) + t[a]) - Y[:, a]) / q for a in range(3)], 1)
        s = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        small = s < 1.0
        rt = np.sqrt(s + EPS)
        l = np.where(small, 0.5 * s, 0.5 * (rt - 0.5))
        k = np.where(small, 1.0, 0.5 / rt)
        cf = ((k * w) / w1) / q
        g = cf[:, None] * r
        cols = [(w * l)[:, None], g] + [g[:, a:a + 1] * X for a in range(3)]
        S = tree_sum(np.concatenate(cols, 1))
        loss = float(np.float64(S[0]) / np.float64(w1))
    return loss, [float(v) for v in S[1:4]], S[4:13].reshape(3, 3), s


# ---- G7, G8, G9 -------------------------------------------------------------------------------------------------------------------------
def refine(src, tgt, weights=None, T_init=None, m_dev=None, log=True, **kw):
    """lr_dgr_refine: dict(T, loss, w1, iterations, break_count, L, status, log [max_iter,10], margins, s_gap).  margins: per iteration with a
    break decision, |d - thr| / thr; s_gap: the least |s - 1| over all evaluations (the premises the tests assert)."""
    P = dict(DEFAULTS, **kw)
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    m = len(src) if m_dev is None else max(0, min(int(m_dev), len(src)))
    w32 = np.ones(m, np.float32) if weights is None else np.asarray(weights, np.float32)[:m]
    live = live_rows(src[:m], tgt[:m], w32, P["clip"])
    X, Y, w = src[:m][live].astype(np.float64), tgt[:m][live].astype(np.float64), w32[live].astype(np.float64)
    L = int(live.sum())
    w1 = float(tree_sum(w)[0])
    out = dict(T=np.eye(4), loss=0.0, w1=w1, iterations=0, break_count=0, L=L, status=0, log=np.zeros((P["max_iter"], 10)), margins=[], s_gap=np.inf)
    if L == 0 or w1 < P["wsum_threshold"]:
        out["status"] = 1 if L == 0 else 2
        return out
    q, ratio = float(P["quantization_size"]), float(P["ratio"])
    p0 = init_params(X, Y, w, w1, T_init)
    p, mom1, mom2 = list(p0), [0.0] * 9, [0.0] * 9
    lr, pw1, pw2 = float(P["lr"]), 1.0, 1.0
    prev, brk, status, its, loss = 0.0, 0, 0, P["max_iter"] - 1, 0.0
    for i in range(P["max_iter"]):
        o = rotation(p)
        R = [[o["x"][a], o["y"][a], o["z"][a]] for a in range(3)]
        loss, dt, G, s = loss_and_sums(X, Y, w, w1, q, R, p[6:9])
        out["log"][i, :9], out["log"][i, 9] = p, loss
        if np.isfinite(s).all():
            out["s_gap"] = min(out["s_gap"], float(np.abs(s - 1.0).min()))
        if i == 0:
            prev = loss
        if not math.isfinite(loss):
            status, its = 3, i
            break
        if loss < LOSS_STOP:
            its = i
            break
        grad = rotation_back(o, G) + dt
        pw1, pw2 = pw1 * BETA1, pw2 * BETA2
        with np.errstate(all="ignore"):
            for k in range(9):
                gk = grad[k]
                mom1[k] = BETA1 * mom1[k] + (1.0 - BETA1) * gk
                mom2[k] = BETA2 * mom2[k] + (1.0 - BETA2) * (gk * gk)
                p[k] = p[k] - _div(lr, 1.0 - pw1) * _div(mom1[k], _div(_sqrt(mom2[k]), _sqrt(1.0 - pw2)) + ADAM_EPS)
        lr = lr * float(P["gamma"])
        if not all(math.isfinite(v) for v in p):
            status, its = 3, i
            break
        d, thr = abs(prev - loss), prev * ratio
        if thr > 0:
            out["margins"].append(abs(d - thr) / thr)
        if d < thr:
            brk += 1
            if brk >= P["max_break"]:
                its = i
                break
        prev = loss
    pf = p0 if status == 3 else p
    T = np.eye(4)
    with np.errstate(all="ignore"):
        T[:3, :3], T[:3, 3] = rotation_matrix(pf), pf[6:9]
    out.update(T=T, loss=loss, iterations=its, break_count=brk, status=status, p0=p0)
    if not log:
        out.pop("log")
    return out
