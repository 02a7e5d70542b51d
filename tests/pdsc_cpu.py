"""PointDSC's SC-NonLocal encoder and confidence head restated in numpy -- the yardstick of csrc/lr_pdsc.hip (contract E1-E6:
include/lidarreg.h).

Independent of the device code: the compatibility matrix, the logits and the softmax weights are formed whole, the layers are matrix
products.  dtype float64 is what the GPU is held to (and what tests/test_pdsc_cpu.py holds against the reference's own fp64 run);
dtype float32 measures what fp32 arithmetic alone costs on a case (a tolerance is a multiple of THAT distance, never of the kernel's)."""
import functools

import numpy as np

from lidarregistration_amd import pointdsc

C = 128


def live_rows(src, tgt):
    """E1: a correspondence with a non-finite coordinate is dead."""
    return np.isfinite(src).all(axis=1) & np.isfinite(tgt).all(axis=1)


def column_mean(X, ok):
    """E2: the fp64 column means of X [m,6] over the rows `ok`, in the contract's order: thread t of 1024 adds rows t, t + 1024, ... in
    ascending order (a dead row adds 0), then the halving tree s[t] += s[t + h], h = 512 .. 1; mean = sum / count."""
    m = len(X)
    pad = (m + 1023) // 1024 * 1024
    Z = np.zeros((pad, X.shape[1]), np.float64)
    Z[:m][ok] = np.asarray(X, np.float64)[ok]
    s = np.zeros((1024, X.shape[1]), np.float64)
    for r in range(pad // 1024):
        s = s + Z[r * 1024:(r + 1) * 1024]
    h = 512
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    n = int(ok.sum())
    return s[0] / n if n else np.zeros(X.shape[1])


def corr_pos(src, tgt, ok):
    """E2: [src, tgt] - mean over the live rows, subtracted in fp64 and rounded to fp32 once ([m,6] float32; dead rows 0)."""
    X = np.concatenate([src, tgt], axis=1).astype(np.float64)
    out = np.zeros(X.shape, np.float32)
    out[ok] = (X[ok] - column_mean(X, ok)).astype(np.float32)
    return out


def compat(src, tgt, sigma_d, dtype=np.float64, slab=512):
    """E3: [m,m] max(0, 1 - d^2 / sigma_d^2), d = |s_i - s_j| - |t_i - t_j| on direct differences of the given fp32 coordinates."""
    m = len(src)
    A, B = src.astype(dtype), tgt.astype(dtype)
    out = np.empty((m, m), dtype)
    for i0 in range(0, m, slab):
        da = A[i0:i0 + slab, None, :] - A[None, :, :]
        db = B[i0:i0 + slab, None, :] - B[None, :, :]
        la = np.sqrt((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2])
        lb = np.sqrt((db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1]) + db[..., 2] * db[..., 2])
        d = la - lb
        if dtype == np.float32:
            out[i0:i0 + slab] = np.maximum(np.float32(0), (d * d) * np.float32(-1.0 / (sigma_d * sigma_d)) + np.float32(1))
        else:
            out[i0:i0 + slab] = np.maximum(0.0, 1.0 - d * d / (sigma_d * sigma_d))
    return out


def layer(x, block, relu=False):
    Wt, scale, offset = block
    y = (x @ Wt[:x.shape[1]]) * scale + offset
    return np.maximum(y, 0) if relu else y


def encode(src, tgt, sd, num_layers=12, sigma_d=1.2, dtype=np.float64, m=None):
    """The whole contract on the first m (default: all) correspondences: (features [m,128], confidence [m]) as `dtype`; dead rows get
    feature 0 and confidence -inf.  The live rows are evaluated as a set of their own: a dead row is attended by nobody and enters no
    mean, so it changes nothing for the others."""
    m = len(src) if m is None else int(m)
    src, tgt = np.asarray(src, np.float32)[:m], np.asarray(tgt, np.float32)[:m]
    feat, conf = np.zeros((m, C), dtype), np.full(m, -np.inf, dtype)
    ok = live_rows(src, tgt)
    if not ok.any():
        return feat, conf
    blocks = iter(pointdsc.fold(sd, num_layers, dtype))
    x = layer(corr_pos(src, tgt, ok)[ok].astype(dtype), next(blocks))
    Cm = compat(src[ok], tgt[ok], sigma_d, dtype)
    qscale = dtype(1.0 / np.sqrt(float(C)))
    for _ in range(num_layers):
        h = layer(x, next(blocks), relu=True)
        qkv = layer(h, next(blocks))
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        logits = Cm * ((q @ k.T) * qscale)
        w = np.exp(logits - logits.max(axis=1, keepdims=True))
        w = w / w.sum(axis=1, keepdims=True)
        msg = w @ v
        msg = layer(layer(layer(msg, next(blocks), relu=True), next(blocks), relu=True), next(blocks))
        x = h + msg
    c = layer(layer(layer(x, next(blocks), relu=True), next(blocks), relu=True), next(blocks))
    feat[ok], conf[ok] = x, c[:, 0]
    return feat, conf


@functools.lru_cache(maxsize=None)
def golden_reference(m, num_layers, dtype_name="float64"):
    """encode() of a golden case of tests/pdsc_cases.py, computed once per process and shared (read-only)."""
    from tests import pdsc_cases
    c = pdsc_cases.golden_case(m, num_layers)
    out = encode(c["src"], c["tgt"], c["sd"], num_layers, pdsc_cases.SIGMA_D, np.dtype(dtype_name).type)
    for x in out:
        x.setflags(write=False)
    return out


def bound(dev_feat, dev_conf, ref_feat, ref_conf):
    """The tolerance rule of the device tests: (features, confidence) bounds max(4 x the yardstick deviation, 16 x 2^-23 x max |reference|).
    The factor 4 is the room for another fixed order of summation and the folded BatchNorm, both fp32 roundings of the yardstick's own
    size; the floor covers the cases whose yardstick deviation is a few ulps."""
    fin = np.isfinite(ref_conf)
    return (max(4.0 * dev_feat, 16.0 * 2.0 ** -23 * float(np.abs(ref_feat).max(initial=0.0))),
            max(4.0 * dev_conf, 16.0 * 2.0 ** -23 * float(np.abs(ref_conf[fin]).max(initial=0.0))))
