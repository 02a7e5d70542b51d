"""Plain restatement of the stage after RANSAC (csrc/lr_refit.hip): which pairs are inliers of a model, the least-squares fit over
them, the gates that leave the model as it was, and the inlier mask.  It shares no text with the kernel or with oracle.c.

The inlier decision is exact.  The clouds are float32 up-cast and T is fp64, so every input is a dyadic rational: scaled by a power of
two they are integers, and |T p - q|^2 - thr2 is evaluated in Python integers (a `fractions` computation with one common power-of-two
denominator, vectorised over the pairs).  exact_d2_mp does the same in mpmath at rigid_hp.DPS digits; the CPU suite finds them equal.

The fit takes one of two routes, by the number of inliers n:
  n <= MP_MAX   rigid_hp.fit over the inlier pairs themselves, in mpmath (weighted for refit = 3);
  n >  MP_MAX   (unweighted only) the raw moments n, sum p, sum q, sum p q^T are formed exactly -- a product of two float32 values is
                exact in fp64, math.fsum of such terms is correctly rounded, and a second fsum of the terms and minus that sum
                recovers the remainder, i.e. about 106 bits -- and the 3x3 problem H = sum p q^T - (sum p)(sum q)^T / n goes to mpmath.
Both return the dict rigid_hp.check expects.  The CPU suite runs one set of pairs down both routes.

The weights of refit = 3 are 1 / max(sqrt(sum_k (F0[i][k] - F1[j][k])^2), clamp), clamp = 1e-12, where difference, square, running sum
over k = 0..31 and square root are float32 operations (the contract: DGR's feature distance is a float32 tensor); the quotient is fp64.
Descriptors narrower than 32 are zero-padded, which adds exact zeros to the sum.
"""
import math
from fractions import Fraction

import numpy as np
from mpmath import mp

from tests import rigid_hp as hp

MP_MAX = 1100              # inliers up to which the fit runs over the pairs in mpmath
CLAMP = 1e-12              # smallest feature distance of a weighted pair
SAFETY = 4.0               # a decision counts as settled when the exact gap exceeds SAFETY x the rounding bound
U64, U32 = 2.0 ** -53, 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ exact inlier decision
def _ints(a, S):
    """a * 2^S as Python integers (object array); exact, or an AssertionError."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a.ravel())
    mi = np.ldexp(m, 53).astype(np.int64)
    out = np.empty(a.size, object)
    for k, (v, s) in enumerate(zip(mi.tolist(), (e.astype(np.int64) - 53 + S).tolist())):
        if v == 0:
            out[k] = 0
        else:
            while s < 0 and v % 2 == 0:
                v //= 2; s += 1
            assert s >= 0, "scale too small for this value"
            out[k] = v << s
    return out.reshape(a.shape)


def _scale(a):
    """The smallest S >= 0 with a * 2^S integral for every entry of the fp64 array a."""
    a = np.asarray(a, np.float64).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    return int(max(0, 53 - np.frexp(a)[1].min()))


def exact_d2(P, Q, T, thr2):
    """Pairs P[c] <-> Q[c] ([m,3], float32 values), T 4x4 fp64, thr2 a float: (inlier [m] bool, gap [m] fp64, d2 [m] fp64) with
    inlier = |T p - q|^2 < thr2 decided exactly, gap = the correctly rounded |T p - q|^2 - thr2 and d2 the correctly rounded distance."""
    P = np.asarray(P, np.float64).reshape(-1, 3); Q = np.asarray(Q, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    m = P.shape[0]
    if m == 0:
        return np.zeros(0, bool), np.zeros(0), np.zeros(0)
    Sp, St = max(_scale(P), _scale(Q)), _scale(T[:3])
    Pi, Qi, Ti = _ints(P, Sp), _ints(Q, Sp), _ints(T[:3], St)
    one_p, one_t = 1 << Sp, 1 << St
    d2 = np.zeros(m, object)
    for a in range(3):
        r = Ti[a, 0] * Pi[:, 0] + Ti[a, 1] * Pi[:, 1] + Ti[a, 2] * Pi[:, 2] + Ti[a, 3] * one_p - Qi[:, a] * one_t
        d2 = d2 + r * r
    thr = Fraction(float(thr2))
    den = 1 << (2 * (Sp + St))
    D = d2 * thr.denominator - thr.numerator * den          # (|T p - q|^2 - thr2) * den * thr.denominator, an integer
    K = den * thr.denominator
    inl = np.array([v < 0 for v in D], bool)
    gap = np.array([v / K for v in D], np.float64)           # int / int is correctly rounded
    return inl, gap, np.array([v / den for v in d2], np.float64)


def exact_d2_mp(P, Q, T, thr2):
    """exact_d2's (inlier, gap) pair by pair in mpmath at rigid_hp.DPS digits."""
    P = np.asarray(P, np.float64).reshape(-1, 3); Q = np.asarray(Q, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    inl, gap = [], []
    with mp.workdps(hp.DPS):
        Tm = [[mp.mpf(float(v)) for v in row] for row in T[:3]]
        th = mp.mpf(float(thr2))
        for p, q in zip(P, Q):
            pm = [mp.mpf(float(v)) for v in p]
            d2 = mp.mpf(0)
            for a in range(3):
                r = Tm[a][0] * pm[0] + Tm[a][1] * pm[1] + Tm[a][2] * pm[2] + Tm[a][3] - mp.mpf(float(q[a]))
                d2 += r * r
            inl.append(bool(d2 < th)); gap.append(float(d2 - th))
    return np.array(inl, bool), np.array(gap, np.float64)


def magnitude(P, Q, T):
    """M: a bound on every intermediate of T p - q, sum_k |T_ak| |p_k| + |t_a| + |q_a| over the pairs and rows."""
    P = np.abs(np.asarray(P, np.float64).reshape(-1, 3)); Q = np.abs(np.asarray(Q, np.float64).reshape(-1, 3))
    T = np.abs(np.asarray(T, np.float64).reshape(4, 4))
    if P.shape[0] == 0:
        return 0.0
    return float((P @ T[:3, :3].T + T[:3, 3] + Q).max())


def d2_bound(d2, M, u, k):
    """How far a floating-point d2 can lie from the exact one.  Each residual component is the result of k roundings of quantities of
    magnitude <= M (fp64 refit: 3 products, 3 sums, 1 difference, k = 7, u = 2^-53; fp32 mask: T rounded to float32, 3 fma, 1
    difference, k = 5, u = 2^-24), so |dr_a| <= k u M (1 + k u); the squared norm moves by at most 2 sqrt(3) |r| |dr| + 3 |dr|^2, and
    its own 5 roundings (fp32 fma form: 3) add 5 u d2.  First order in u throughout, with 1.01 covering the higher orders."""
    dr = k * u * M
    return 1.01 * (2.0 * math.sqrt(3.0) * np.sqrt(np.asarray(d2, np.float64)) * dr + 3.0 * dr * dr + 5.0 * u * np.asarray(d2, np.float64))


# ------------------------------------------------------------------------------------------------------------ the fit
def _two_sum(terms):
    """The sum of fp64 terms to about 106 bits: the correctly rounded sum and the correctly rounded remainder."""
    terms = list(terms)
    s = math.fsum(terms)
    return mp.mpf(s) + mp.mpf(math.fsum(terms + [-s]))


def fit_moments(P, Q):
    """Unweighted Kabsch through the exact raw moments (see the module docstring); the dict of rigid_hp.fit."""
    P = np.asarray(P, np.float64).reshape(-1, 3); Q = np.asarray(Q, np.float64).reshape(-1, 3)
    assert np.array_equal(P, P.astype(np.float32)) and np.array_equal(Q, Q.astype(np.float32)), "products must be exact in fp64"
    n = P.shape[0]
    with mp.workdps(hp.DPS):
        sp = [_two_sum(P[:, a].tolist()) for a in range(3)]
        sq = [_two_sum(Q[:, a].tolist()) for a in range(3)]
        cp = [v / n for v in sp]; cq = [v / n for v in sq]
        H = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                H[a, b] = _two_sum((P[:, a] * Q[:, b]).tolist()) - sp[a] * sq[b] / n
        U, S, Vt = mp.svd_r(H)
        V = Vt.T
        d = mp.mpf(1) if hp._det3(V * U.T) >= 0 else mp.mpf(-1)
        R = V * mp.diag([1, 1, d]) * U.T
        t = [cq[a] - mp.fsum(R[a, b] * cp[b] for b in range(3)) for a in range(3)]
        s = [S[0], S[1], S[2]]
        den = s[1] + d * s[2]
        scale = float(np.sum(np.linalg.norm(P, axis=1) * np.linalg.norm(Q, axis=1)))
        kappa = float(s[0] / den) if den > 0 and s[0] != 0 else float("inf")
        kappa_raw = float(scale / den) if den > 0 else float("inf")
        return dict(R=hp._np(R), Rmp=R, t=np.array([float(v) for v in t]), cp=np.array([float(v) for v in cp]),
                    cq=np.array([float(v) for v in cq]), s=np.array([float(v) for v in s]), d=int(d), kappa=kappa, kappa_raw=kappa_raw,
                    fstar=s[0] + s[1] + d * s[2], scale=scale, Hmp=H, H=hp._np(H))


def fit(P, Q, w=None, route=None):
    """route None: by size (module docstring); "mp" / "moments" force one."""
    n = np.asarray(P).reshape(-1, 3).shape[0]
    if route is None:
        route = "mp" if (w is not None or n <= MP_MAX) else "moments"
    if route == "mp":
        return hp.fit(P, Q, w)
    assert w is None, "the exact-moment route is unweighted"
    return fit_moments(P, Q)


def weights(F0, F1, i0, i1, clamp=CLAMP):
    """The weights of refit = 3 for the pairs (i0[c], i1[c]); fp64 [m]."""
    F0 = np.asarray(F0, np.float32); F1 = np.asarray(F1, np.float32)
    e = F0[np.asarray(i0, np.int64)] - F1[np.asarray(i1, np.int64)]
    acc = np.zeros(e.shape[0], np.float32)
    for k in range(e.shape[1]):
        acc = acc + e[:, k] * e[:, k]
    dist = np.maximum(np.sqrt(acc), np.float32(clamp))
    with np.errstate(divide="ignore"):
        return 1.0 / dist.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the stage
def refit(xyz0, xyz1, idx1, T_in, thr2, idx0=None, m=None, F0=None, F1=None, have_model=True, clamp=CLAMP, route=None):
    """What lr_refit (idx0 = m = F0 = None), and the refit stage of lr_register_pair with refit = 1 (the same), 2 (idx0, idx1 = the
    filtered lists, m = their live length) and 3 (F0, F1) must produce from the model T_in.  Returns a dict:
      T         4x4 fp64: the restatement's own answer where a fit was made, else T_in
      ref       the dict for rigid_hp.check, or None where the gates leave T = T_in
      n_refit   the number of inlier pairs (0 without a model), status (1 without a model)
      rows      the list rows c the decision was made for, i0 / i1 their point indices, inlier / gap / d2 as exact_d2 returns them."""
    xyz0 = np.asarray(xyz0, np.float32).astype(np.float64); xyz1 = np.asarray(xyz1, np.float32).astype(np.float64)
    T_in = np.asarray(T_in, np.float64).reshape(4, 4)
    idx1 = np.asarray(idx1, np.int64)
    n = len(idx1) if idx0 is None else min(len(idx1), len(idx0))
    if m is not None:
        n = min(n, int(m))
    rows = np.arange(n)
    i1 = idx1[:n]
    i0 = rows if idx0 is None else np.asarray(idx0, np.int64)[:n]
    live = i1 >= 0                                      # a row with no partner is skipped
    rows, i0, i1 = rows[live], i0[live], i1[live]
    inl, gap, d2 = exact_d2(xyz0[i0], xyz1[i1], T_in, thr2)
    out = dict(rows=rows, i0=i0, i1=i1, inlier=inl, gap=gap, d2=d2, T=T_in.copy(), ref=None, n_refit=int(inl.sum()), status=0,
               M=magnitude(xyz0[i0], xyz1[i1], T_in))
    if not have_model:
        out.update(n_refit=0, status=1)
        return out
    weighted = F0 is not None
    w = weights(F0, F1, i0[inl], i1[inl], clamp) if weighted else None
    if out["n_refit"] == 0 or (not weighted and out["n_refit"] < 3):
        return out
    out["w"] = w
    out["ref"] = fit(xyz0[i0[inl]], xyz1[i1[inl]], w, route)
    T = np.eye(4); T[:3, :3] = out["ref"]["R"]; T[:3, 3] = out["ref"]["t"]
    out["T"] = T
    return out


def mask(src, tgt, T, thr2, m=None):
    """lr_inlier_mask's decision made exactly: dict(inlier, gap, d2 [m], bound [m]: how far the float32 d2 of lr_score_d2 may be off)."""
    src = np.asarray(src, np.float32).astype(np.float64); tgt = np.asarray(tgt, np.float32).astype(np.float64)
    n = src.shape[0] if m is None else min(src.shape[0], int(m))
    inl, gap, d2 = exact_d2(src[:n], tgt[:n], T, float(np.float32(thr2)))
    return dict(inlier=inl, gap=gap, d2=d2, bound=d2_bound(d2, magnitude(src[:n], tgt[:n], T), U32, 5))
