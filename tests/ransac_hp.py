"""Independent fp64 restatements of RANSAC scoring, selection and the uniform hypothesis stream (numpy only).

The oracle (oracle/oracle.c) shares its arithmetic text with the kernels: it evaluates the same fp32 fma chain, so a wrong
contract would be wrong in both.  The helpers here evaluate the same quantities in fp64 from the stated definitions and bound
how far the fp32 contract may stray from them:

* ``score_fp64`` -- inlier count, sum of d^2 and the *band* of correspondences whose fp32 decision may differ from the fp64 one;
* generators of near-threshold sets and of scenes scaled to the threshold, optionally far from the origin;
* ``philox4x32_10`` / ``hypotheses`` -- the uniform sampler (Philox4x32-10, ``(w * m) >> 32``), the edge-length check (ELC) and
  a centred SVD fit, vectorised over hypothesis ids.
"""
import numpy as np

U32 = 2.0 ** -24                 # unit roundoff of fp32
SCALE = 1048576.0                # the contract's fixed-point scale of d^2 (2^20)
M32 = np.uint64(0xFFFFFFFF)


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def d2_bound(T, src, tgt, t_err=0.0):
    """Per correspondence: fp64 d^2 of the model T (4x4) and delta_i, a bound on |d2_fp32 - d2| for the fp32 contract.

    The contract (oracle.c score_model, lr_ransac.hip lr_model_d2) evaluates, with Rt = (float)T,
        x_a  = fma(Rt[a,0], p0, fma(Rt[a,1], p1, fma(Rt[a,2], p2, Rt[a,3])))        (three roundings)
        e_a  = x_a - q_a                                                             (one rounding)
        d2   = fma(e_0, e_0, fma(e_1, e_1, e_2 * e_2))                               (at most three roundings per term)
    and decides d2 < thr2 with thr2 the fp32 threshold itself.  With u = 2^-24 and gamma_n = n u / (1 - n u):
      * |Rt - T| <= u |T| + t_err elementwise (t_err: how far the T given here may be from the one the kernel rounded);
      * so |x_a - (T p)_a| <= A_a (u + gamma_3 (1 + u)) + t_err S =: X_a,  A_a = sum_b |T_ab p_b| + |T_a3|,  S = 1 + sum_b |p_b|;
      * |e_a - r_a| <= X_a + u (|r_a| + X_a) =: E_a,  r_a = (T p)_a - q_a the fp64 residual;
      * |d2 - sum r_a^2| <= sum_a E_a (2 |r_a| + E_a) + gamma_3 sum_a (|r_a| + E_a)^2 =: delta.
    The fp64 evaluation of r and d^2 here carries errors of order 2^-53 of the same terms: delta is doubled to cover them (and any
    slack in the above).  The fixed-point truncation (uint32)(d2 * 2^20) does not enter the decision; it costs < 2^-20 per inlier
    in the error sum, see ``score_fp64``."""
    T = np.asarray(T, np.float64)
    p = np.asarray(src, np.float32).astype(np.float64)
    q = np.asarray(tgt, np.float32).astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    x = p @ R.T + t
    r = x - q
    d2 = np.sum(r * r, axis=1)
    A = np.abs(p) @ np.abs(R).T + np.abs(t)
    S = 1.0 + np.sum(np.abs(p), axis=1, keepdims=True)
    X = A * (U32 + _gamma(3) * (1 + U32)) + t_err * S
    E = X + U32 * (np.abs(r) + X)
    delta = np.sum(E * (2 * np.abs(r) + E), axis=1) + _gamma(3) * np.sum((np.abs(r) + E) ** 2, axis=1)
    return d2, 2.0 * delta


def score_fp64(src, tgt, T, thr2, t_err=0.0):
    """fp64 scoring of one model.  Returns dict(count, ssq = sum of d^2 over the fp64 inliers, inlier (bool), band (bool),
    d2, delta).  thr2 is the fp32 threshold the kernels compare against (rounded to float32 here).

    Outside the band (|d2 - thr2| > delta) the fp32 contract takes the same decision as the fp64 one, so for the fp32 result
    (count32, ssq32):  |count32 - count| <= #band  and
        |ssq32 * 2^-20 - ssq| <= count32 * 2^-20 + sum_{inliers} delta + #band * thr2
    (truncation of every term, rounding of the in-both terms, the terms of band members counted by one side only)."""
    thr2 = float(np.float32(thr2))
    d2, delta = d2_bound(T, src, tgt, t_err)
    with np.errstate(invalid="ignore"):
        inl = d2 < thr2
        band = np.abs(d2 - thr2) <= delta
    return dict(count=int(inl.sum()), ssq=float(d2[inl].sum()), inlier=inl, band=band, d2=d2, delta=delta,
                delta_in=float(delta[inl | band].sum()), thr2=thr2)


def ssq_tolerance(ref, count32):
    """The bound of ``score_fp64``'s docstring on |ssq32 * 2^-20 - ref['ssq']|."""
    return count32 / SCALE + ref["delta_in"] + int(ref["band"].sum()) * ref["thr2"]


# ----------------------------------------------------------------------------- generators

def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def motion(rng, t_scale=30.0):
    """A random proper rigid motion (fp64 4x4)."""
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3] = Q
    T[:3, 3] = rng.uniform(-t_scale, t_scale, 3)
    return T


def near_threshold_set(m, k, thr, eta=0.02, n_band=0, rng=None, T=None, extent=None, offset=0.0, below=None, shuffle=True):
    """m correspondences under a planted motion T: k exact inliers (tgt = T src, rounded to fp32); the others at residual
    thr (1 - eta) (below=True), thr (1 + eta) (below=False) or either at random (below=None), in random directions; n_band of
    them at residual thr itself (inside the decision band up to the fp32 rounding of tgt).  extent: side of the source box
    (default max(80, 40 thr)); offset: added to every coordinate of both clouds (m away from the origin).
    shuffle=False keeps the order: exact inliers first, then the band members, then the rest.
    Returns (src, tgt, T) with src/tgt float32 [m,3]."""
    rng = np.random.default_rng(0) if rng is None else rng
    extent = max(80.0, 40.0 * thr) if extent is None else extent
    T = motion(rng, t_scale=0.3 * extent) if T is None else T
    src = rng.uniform(-extent / 2, extent / 2, (m, 3)) + offset
    Tp = src @ T[:3, :3].T + T[:3, 3]
    if below is None:
        rad = np.where(rng.random(m) < 0.5, 1 - eta, 1 + eta)
    else:
        rad = np.full(m, (1 - eta) if below else (1 + eta))
    rad[:k] = 0.0
    band_idx = np.arange(k, min(m, k + n_band))
    rad[band_idx] = 1.0
    tgt = Tp + thr * rad[:, None] * _unit(rng, m)          # (T acts on the offset sources as they are)
    perm = rng.permutation(m) if shuffle else np.arange(m)
    return src[perm].astype(np.float32), tgt[perm].astype(np.float32), T


def scaled_scene(m, thr, inlier=0.4, rng=None, offset=0.0, extent_factor=40.0):
    """A scene whose extent (max(80, extent_factor thr)) is much larger than the threshold: inliers with noise thr / 4, outliers
    uniform in the box; offset moves both clouds away from the origin.  Returns (src, tgt, T)."""
    rng = np.random.default_rng(0) if rng is None else rng
    extent = max(80.0, extent_factor * thr)
    T = motion(rng, t_scale=0.2 * extent)
    src = rng.uniform(-extent / 2, extent / 2, (m, 3))
    src[:, 2] *= 0.2
    tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, thr / 4, (m, 3))
    bad = rng.random(m) > inlier
    tgt[bad] = rng.uniform(-extent / 2, extent / 2, (bad.sum(), 3)) + T[:3, 3]
    src, tgt = src + offset, tgt + offset
    Toff = T.copy()
    Toff[:3, 3] = T[:3, 3] + offset - T[:3, :3] @ np.full(3, offset)
    return src.astype(np.float32), tgt.astype(np.float32), Toff


# ----------------------------------------------------------------------------- the uniform hypothesis stream

PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: ctr [..., 4] and key [..., 2] of uint32 values -> [..., 4] uint32."""
    c = [np.asarray(ctr, np.uint64)[..., i] & M32 for i in range(4)]
    k0 = np.asarray(key, np.uint64)[..., 0] & M32
    k1 = np.asarray(key, np.uint64)[..., 1] & M32
    for _ in range(10):
        p0 = PHILOX_M0 * c[0]
        p1 = PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_words(seed, h):
    """The four words of hypothesis ids h (array): counter (h_lo, h_hi, 0, 0), key (seed_lo, seed_hi)."""
    h = np.asarray(h, np.uint64)
    ctr = np.stack([h & M32, h >> np.uint64(32), np.zeros_like(h), np.zeros_like(h)], axis=-1)
    s = np.uint64(seed)
    key = np.broadcast_to(np.array([s & M32, s >> np.uint64(32)], np.uint64), h.shape + (2,))
    return philox4x32_10(ctr, key)


def sample_indices(seed, h, m, ns):
    """Uniform draw with replacement: index k of hypothesis h = (w_k * m) >> 32."""
    w = philox_words(seed, h).astype(np.uint64)[..., :ns]
    return ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def elc_pass(src, tgt, s, sim=0.9):
    """Edge-length check of samples s [H, ns]: every pair of sample edges within the ratio 0.9 (fp64 lengths)."""
    P = np.asarray(src, np.float32).astype(np.float64)[s]
    Q = np.asarray(tgt, np.float32).astype(np.float64)[s]
    ok = np.ones(s.shape[0], bool)
    ns = s.shape[1]
    for i in range(ns):
        for j in range(i + 1, ns):
            a, b = P[:, j] - P[:, i], Q[:, j] - Q[:, i]
            ds = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            dt = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
            ok &= ~((ds < dt * sim) | (dt < ds * sim))
    return ok


def svd_fit(P, Q):
    """Centred least-squares rigid fit Q ~ R P + t by SVD, batched: P, Q [H, n, 3] fp64 -> (T [H,4,4], singular values [H,3])."""
    cp, cq = P.mean(axis=1), Q.mean(axis=1)
    H = np.einsum("hna,hnb->hab", P - cp[:, None], Q - cq[:, None])
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("hba,hcb->hac", Vt, U)))          # det(V U^T)
    d[d == 0] = 1.0
    D = np.zeros_like(H)
    D[:, 0, 0] = 1.0; D[:, 1, 1] = 1.0; D[:, 2, 2] = d
    R = np.einsum("hba,hbc,hdc->had", Vt, D, U)                           # V D U^T
    T = np.tile(np.eye(4), (P.shape[0], 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = cq - np.einsum("hab,hb->ha", R, cp)
    return T, S


def hypotheses(src, tgt, ids, ns=3, use_elc=True, seed=51):
    """The uniform sampler's hypotheses ids (array): dict(sample [H,ns], valid [H], T [H,4,4], sv [H,3]) -- T of every id
    (valid or not) from the centred SVD fit of its sample; sv: singular values of the sample's cross-covariance."""
    ids = np.asarray(ids, np.uint64)
    m = np.asarray(src).shape[0]
    s = sample_indices(seed, ids, m, ns)
    valid = elc_pass(src, tgt, s) if use_elc else np.ones(len(ids), bool)
    P = np.asarray(src, np.float32).astype(np.float64)[s]
    Q = np.asarray(tgt, np.float32).astype(np.float64)[s]
    T, S = svd_fit(P, Q)
    return dict(sample=s, valid=valid, T=T, sv=S)


def well_posed(sv):
    """The fit of a sample is unique and stable when its cross-covariance has rank >= 2 well clear of 0: sigma_2 above 1e-6 of
    sigma_1 (the minimal samples here are 3 or 4 points; a repeated or collinear pair of indices fails this)."""
    return sv[:, 1] > 1e-6 * np.maximum(sv[:, 0], 1e-300)
