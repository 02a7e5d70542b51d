"""Contract n1 (F1-F12) of lr_fcgf_extract (include/lidarreg.h) restated in numpy, twice, independent of the library:

  * ``run(..., mode="f64")``: a key lookup and one fp64 matmul per kernel offset -- the conventions (levels, maps, offset order, stage
    order, epilogues), checked in tests/test_fcgf_cpu.py against torch's dense conv3d / conv_transpose3d;
  * ``run(..., mode="chain")``: the exact fp32 arithmetic of F5 / F6 / F8: per output element ONE fmaf chain over ascending offset and,
    inside an offset, ascending input channel.  numpy has no fmaf: ``fmaf32`` emulates it (product in fp64, exact; TwoSum with the addend;
    round-to-odd on the fp64 sum when the error term is non-zero; one cast to fp32) and is checked against libm in the tests.
  * ``mode="f32mm"``: an fp32 matmul per offset, the yardstick d32 of the value check at size (another summation order of the same fp32).

All three take the folded float32 weights (lidarregistration_amd.fcgf.fold): they differ in arithmetic only.
"""
import numpy as np

BIAS = 1 << 20
LIMIT = (1 << 20) - 2


def fmaf32(a, b, c):
    """fmaf(a, b, c) on float32 arrays (broadcast), correctly rounded."""
    a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64); c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)               # TwoSum: p + c = s + e exactly
        inexact = (e != 0) & np.isfinite(s)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)      # round to odd: the double rounding to fp32 is then innocuous
        return s.astype(np.float32)


def pack_keys(c):
    c = np.asarray(c, np.int64) + BIAS
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def status_of(coords):
    """F9: 3 = a cell at or past the range limit (wins), 2 = a duplicate, 0."""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    if (np.abs(c) >= LIMIT).any():
        return 3
    return 2 if len(np.unique(pack_keys(c))) != len(c) else 0


def levels(coords):
    """F1: [level 0 (input order), level 1, 2, 3 (ascending x, y, z)] as int64 [n_l, 3]."""
    out = [np.asarray(coords, np.int64).reshape(-1, 3)]
    for l in range(3):
        t = 2 << l
        out.append(np.unique((out[-1] // t) * t, axis=0))        # floor division; np.unique sorts rows lexicographically
    return out


def kernel_map(out_coords, in_coords, K, step):
    """[(k, out rows, in rows)] for the offsets that have a pair: in = out + o(k) * step, idx(o) x fastest (F2)."""
    h = K // 2
    keys = pack_keys(in_coords)
    order = np.argsort(keys, kind="stable"); sk = keys[order]
    maps = []
    for k in range(K ** 3):
        o = np.array([k % K - h, k // K % K - h, k // (K * K) - h], np.int64)
        c = out_coords + o * step
        ok = ((c + BIAS >= 0) & (c + BIAS < 2 * BIAS)).all(1)
        q = pack_keys(np.where(ok[:, None], c, 0))
        pos = np.minimum(np.searchsorted(sk, q), max(len(sk) - 1, 0))
        hit = ok & (sk[pos] == q) if len(sk) else np.zeros(len(q), bool)
        if hit.any():
            maps.append((k, np.nonzero(hit)[0], order[pos[hit]]))
    return maps


def _conv(x, maps, W, n_out, mode):
    """sum over the maps' offsets of x[in rows] @ W[k] -> [n_out, Cout] in the arithmetic of `mode`."""
    cin, cout = W.shape[1], W.shape[2]
    if mode == "f64":
        acc = np.zeros((n_out, cout), np.float64)
        for k, ro, ri in maps:
            acc[ro] += x[ri].astype(np.float64) @ W[k].astype(np.float64)
        return acc
    acc = np.zeros((n_out, cout), np.float32)
    if mode == "f32mm":
        for k, ro, ri in maps:
            acc[ro] += x[ri] @ W[k]
        return acc
    for k, ro, ri in maps:                           # chain: ascending offset, ascending input channel, one fmaf each
        a = acc[ro]; xi = x[ri]; Wk = W[k]
        for ci in range(cin):
            a = fmaf32(xi[:, ci:ci + 1], Wk[ci:ci + 1, :], a)
        acc[ro] = a
    return acc


def _epilogue(acc, scale, offset, res, relu, mode):
    if mode == "f64":
        y = scale.astype(np.float64) * acc + offset.astype(np.float64)
    else:
        y = fmaf32(scale[None, :], acc, offset[None, :])
    if res is not None:
        y = y + res
    if relu:
        y = np.where(y > 0, y, np.where(np.isnan(y), y, 0)).astype(y.dtype)
    return y


def run(coords, stages, k1=5, feat_in=None, mode="chain", upto=23):
    """The network on distinct in-range cells.  stages: fcgf.fold(sd, k1) (float32).  Returns dict(levels=[4 coordinate sets],
    acts={stage: [n_level, Cout]}, level_of={stage: level}, out=[n,32] the normalised features when upto = 23)."""
    assert status_of(coords) == 0
    dt = np.float64 if mode == "f64" else np.float32
    L = levels(coords)
    n = len(L[0])
    x0 = (np.ones(n, dt) if feat_in is None else np.asarray(feat_in, np.float32).astype(dt))[:, None]
    nb = [kernel_map(L[l], L[l], 3, 1 << l) for l in range(4)]
    dn = [kernel_map(L[l + 1], L[l], 3, 1 << l) for l in range(3)]                 # F3
    up = [kernel_map(L[l], L[l + 1], 3, -(1 << l)) for l in range(3)]              # F4: in = u - o t
    ident = lambda l: [(0, np.arange(len(L[l])), np.arange(len(L[l])))]
    acts, level_of = {}, {}

    class Stop(Exception):
        pass

    def stage(s, x, maps, lvl, res=None, relu=0):
        W, sc, of = stages[s - 1]
        y = _epilogue(_conv(x, maps, W, len(L[lvl]), mode), sc, of, res, relu, mode)
        acts[s], level_of[s] = y, lvl
        if s == upto and s < 23:
            raise Stop
        return y

    def block(s, x, lvl):
        t = stage(s, x, nb[lvl], lvl, None, 1)
        return stage(s + 1, t, nb[lvl], lvl, x, 1)

    out = None
    try:
        x = stage(1, x0, kernel_map(L[0], L[0], k1, 1), 0)
        s1 = block(2, x, 0)
        s2 = block(5, stage(4, s1, dn[0], 1), 1)
        s4 = block(8, stage(7, s2, dn[1], 2), 2)
        s8 = block(11, stage(10, s4, dn[2], 3), 3)
        u = block(14, stage(13, s8, up[2], 2), 2)
        u = block(17, stage(16, np.concatenate([u, s4], 1), up[1], 1), 1)
        u = block(20, stage(19, np.concatenate([u, s2], 1), up[0], 0), 0)
        x = stage(22, np.concatenate([u, s1], 1), ident(0), 0, None, 1)
        f = stage(23, x, ident(0), 0)
        if mode == "f64":
            out = f / (np.sqrt((f * f).sum(1, keepdims=True)) + 1e-8)
        else:
            s = np.zeros((n, 1), np.float32)
            for c in range(32):
                s = fmaf32(f[:, c:c + 1], f[:, c:c + 1], s)
            out = (f / (np.sqrt(s) + np.float32(1e-8))).astype(np.float32)
    except Stop:
        pass
    return dict(levels=L, acts=acts, level_of=level_of, out=out)


# ---- the table hash of csrc/lr_cells.h, for the test that forces one probe chain ---------------------------------------------------
def mix64(k):
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33); k *= np.uint64(0xff51afd7ed558ccd); k ^= k >> np.uint64(33); k *= np.uint64(0xc4ceb9fe1a85ec53)
        return k ^ (k >> np.uint64(33))


def capacity(n):
    c = 1024
    while c < 2 * max(n, 1):
        c <<= 1
    return c


def home_slot(coords, n):
    """The slot a cell's probe sequence starts at in the level-0 table of a cloud of n cells."""
    return (mix64(pack_keys(coords).astype(np.uint64)) & np.uint64(capacity(n) - 1)).astype(np.int64)
