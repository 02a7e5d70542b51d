"""Inputs of the tests of PointDSC's tail (lr_pdsc_solve): seeded correspondence sets with features and confidences on which the tail
behaves as if the encoder were trained -- random encoder weights give seeds and neighbourhoods without meaning.  Nothing here is read
from a file; tests/golden/make_golden_pdsc_solve.py runs the reference on exactly these and records what it returns.

  * geometry: pdsc_cases.planted's recipe, with the inlier mask;
  * features: N(0, I_128), plus sqrt(128) u0 (one seeded unit vector) on the inliers: inliers have cosine ~0.5 to each other, ~0 to the rest;
  * confidence: +3 on inliers, -3 on outliers, 10 % of the signs flipped, plus N(0, 1).
"""
import hashlib

import numpy as np

from tests import pdsc_cases

C = 128
SIGMA_D = pdsc_cases.SIGMA_D
PARAMS = dict(num_iterations=10, k=40, refine_iters=20, ratio=0.1, nms_radius=0.6, inlier_threshold=0.6, refine_threshold=1.2, sigma_d=SIGMA_D, sigma=1.0)
# the golden cases: (name, m, inlier ratio, rows duplicated)
# m11: every row an inlier -- one seed over ten neighbours whose matrix is close to rank one, so the reference's power loop leaves early;
# m1000: the inlier of largest confidence is duplicated -- two seeds of equal key, each the other's neighbour at the similarity of itself
GOLDEN = (("m11", 11, 1.0, 0), ("m41", 41, 0.2, 0), ("m42", 42, 0.2, 0), ("m257", 257, 0.2, 0), ("m1000", 1000, 0.2, 1), ("m3000", 3000, 0.2, 0))


def planted(m, seed=0, inlier_ratio=0.2, noise=0.05):
    """pdsc_cases.planted with its inlier mask: (src, tgt, inlier).  The same draws in the same order."""
    rng = np.random.default_rng([seed, m, 1])
    R, t = pdsc_cases._motion(rng)
    src = pdsc_cases._box(rng, m)
    tgt = src @ R.T + t + noise * rng.standard_normal((m, 3))
    out = rng.random(m) >= inlier_ratio
    tgt[out] = pdsc_cases._box(rng, int(out.sum()))
    return src.astype(np.float32), tgt.astype(np.float32), ~out


def trained_like(inlier, seed=0):
    """(feat [m,128], conf [m]) float32 for an inlier mask."""
    m = len(inlier)
    rng = np.random.default_rng([seed, m, 7])
    u0 = rng.standard_normal(C); u0 /= np.linalg.norm(u0)
    feat = rng.standard_normal((m, C)) + np.sqrt(float(C)) * u0 * inlier[:, None]
    sign = np.where(inlier, 1.0, -1.0) * np.where(rng.random(m) < 0.1, -1.0, 1.0)
    conf = 3.0 * sign + rng.standard_normal(m)
    return feat.astype(np.float32), conf.astype(np.float32)


def case(m, seed=0, inlier_ratio=0.2, dup=0):
    """dict(src, tgt, feat, conf, inlier).  dup: the `dup` inliers of largest confidence are copied over the rows behind them (all four
    arrays), so that seeds sit among duplicated rows: equal keys, similarity exactly that of the row to itself."""
    src, tgt, inl = planted(m, seed, inlier_ratio)
    feat, conf = trained_like(inl, seed)
    if dup:
        top = np.argsort(-np.where(inl, conf, -np.inf), kind="stable")[:dup]
        for i in top:
            j = (i + 1) % m
            src[j], tgt[j], feat[j], conf[j], inl[j] = src[i], tgt[i], feat[i], conf[i], inl[i]
    return dict(m=m, src=src, tgt=tgt, feat=feat, conf=conf, inlier=inl)


def golden_case(name):
    for n, m, ratio, dup in GOLDEN:
        if n == name:
            c = case(m, seed=m, inlier_ratio=ratio, dup=dup)
            c["name"] = name
            return c
    raise KeyError(name)


def all_outliers(m, seed=0):
    src, tgt, inl = planted(m, seed, inlier_ratio=0.0)
    feat, conf = trained_like(inl, seed)
    return dict(m=m, src=src, tgt=tgt, feat=feat, conf=conf, inlier=inl)


def checksum(c):
    h = hashlib.sha256()
    for k in ("src", "tgt", "feat", "conf"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()
