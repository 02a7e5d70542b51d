"""Inputs of the tests of the DGR refinement (lr_dgr_refine): seeded planted rigid motions with noise, outliers and clipped weights.
Nothing here is read from a file; tests/golden/make_golden_dgr.py runs the reference's GlobalRegistration on exactly the GOLDEN cases
and records what it returns.
"""
import hashlib

import numpy as np

# what DGR passes for a 0.3 m voxel (deep_global_registration.py:415-421)
PARAMS = dict(quantization_size=0.6, ratio=1e-4, max_iter=1000, max_break=20)
CLIP = 0.05
# the golden cases: (name, seed, m, inlier ratio, noise, angle about z).  `unstable`: the init is the optimum and the s < 1 branches flip, so the
# reference's own float32 and float64 runs disagree on the iteration count -- used only for device-against-restatement equality.
GOLDEN = (("m3000", 0, 3000, 0.4, 0.05, 0.3), ("m500", 1, 500, 0.2, 0.1, 1.0), ("m64", 2, 64, 0.5, 0.02, 0.1), ("m5000", 3, 5000, 0.1, 0.05, 2.0),
          ("m1000", 5, 1000, 0.05, 0.05, 0.5), ("m12000", 6, 12000, 0.3, 0.1, 0.7), ("m7", 7, 7, 0.9, 0.01, 0.2), ("unstable", 4, 2000, 0.9, 0.3, 0.5))
UNSTABLE = ("unstable",)
STABLE = tuple(c[0] for c in GOLDEN if c[0] not in UNSTABLE)


def rot_z(ang):
    return np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])


def planted(seed, m, inlier_ratio, noise, ang, box=40.0, t=(1.0, 2.0, 0.3)):
    """dict(src, tgt [m,3] float32, weights [m] float32, inlier [m] bool, T_gt).  Weights: 0.5 .. 1 on inliers, 0 .. 0.3 on outliers, those
    below CLIP set to 0 (DGR's clipping, deep_global_registration.py:401)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-box, box, (m, 3)).astype(np.float32).astype(np.float64)
    R = rot_z(ang)
    Y = X @ R.T + np.array(t) + noise * rng.standard_normal((m, 3))
    out = rng.random(m) > inlier_ratio
    Y[out] = rng.uniform(-box, box, (int(out.sum()), 3))
    w = np.where(out, rng.random(m) * 0.3, 0.5 + 0.5 * rng.random(m))
    w[w < CLIP] = 0
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(src=X.astype(np.float32), tgt=Y.astype(np.float32), weights=w.astype(np.float32), inlier=~out, T_gt=T)


def golden_case(name):
    for n, *a in GOLDEN:
        if n == name:
            c = planted(*a)
            c["name"] = name
            return c
    raise KeyError(name)


def checksum(c):
    h = hashlib.sha256()
    for k in ("src", "tgt", "weights"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()
