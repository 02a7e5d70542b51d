"""Contract n3 of lr_dgr_inlier (include/lidarreg.h, DESIGN.md §20: F1-F7, F9, F10 of n1 in six dimensions with I1-I5) restated in numpy,
independent of the library, in the three arithmetics of tests/fcgf_cpu.py (whose fmaf32 and _epilogue it shares: they do not know the
dimension):

  * ``run(..., mode="f64")``: a key lookup and one fp64 matmul per offset -- the conventions, checked in tests/test_dgr6_cpu.py against the
    pinned 3-D restatement and against a brute-force dense loop;
  * ``run(..., mode="chain")``: the exact fp32 arithmetic of I3 / F6 / I4.  The chain of an output row is sequential, the rows are
    independent: ``_conv`` walks the rows in lockstep (step j = every row's j-th present neighbour in ascending offset order), so a stage
    costs (most neighbours of one row) x Cin calls of fmaf32 instead of (offsets present anywhere) x Cin; tests/test_dgr6_cpu.py holds it
    to fcgf_cpu._conv's offset-major loop bit for bit;
  * ``mode="f32mm"``: an fp32 matmul per offset, the yardstick d32 of the value check at size.

All take the folded float32 stages (lidarregistration_amd.dgr.inlier_fold, or random ones from ``random_stages``).
"""
import numpy as np

from tests.fcgf_cpu import _epilogue, fmaf32

NK = 729
BIAS = 8
REL_MAX = 1007                 # cell - origin above this on an axis: status 3
WIDTHS = (32, 64, 128, 256, 128, 64, 64, 64)
THIN = (32,) * 8
_POW3 = 3 ** np.arange(6)


def offset_of(k):
    """I1: the offset o in {-1,0,1}^6 of slice k, axis 0 fastest -- the one place the offset order lives in this file."""
    return (int(k) // _POW3) % 3 - 1


def index_of(o):
    return int(((np.asarray(o, np.int64) + 1) * _POW3).sum())


def origin(coords):
    c = np.asarray(coords, np.int64).reshape(-1, 6)
    return (c.min(0) // 8) * 8


def pack_keys(c, org):
    """six 10-bit fields (cell - origin + 8), axis 0 most significant."""
    f = np.asarray(c, np.int64) - org + BIAS
    key = np.zeros(len(f), np.int64)
    for a in range(6):
        key = (key << 10) | f[:, a]
    return key


def status_of(coords):
    """I2: 3 = an axis wider than the extent limit (wins), 2 = a duplicate row, 0."""
    c = np.asarray(coords, np.int64).reshape(-1, 6)
    if len(c) == 0:
        return 0
    if ((c - origin(c)) > REL_MAX).any():
        return 3
    return 2 if len(np.unique(c, axis=0)) != len(c) else 0


def levels(coords):
    """F1 / I2: [level 0 (input order), level 1, 2, 3 (ascending lexicographic, axis 0 most significant)] as int64 [n_l, 6]."""
    out = [np.asarray(coords, np.int64).reshape(-1, 6)]
    for l in range(3):
        t = 2 << l
        out.append(np.unique((out[-1] // t) * t, axis=0))
    return out


OFFSETS = np.stack([offset_of(k) for k in range(NK)])          # [729, 6]


def kernel_map(out_coords, in_coords, step, org):
    """[(k, out rows, in rows)] for the offsets that have a pair, ascending k and out row: in = out + o(k) * step."""
    out_coords = np.asarray(out_coords, np.int64)
    keys = pack_keys(in_coords, org)
    order = np.argsort(keys, kind="stable"); sk = keys[order]
    if len(sk) == 0 or len(out_coords) == 0:
        return []
    ks, ros, ris = [], [], []
    for r0 in range(0, len(out_coords), 1024):
        f = out_coords[r0:r0 + 1024, None, :] + OFFSETS[None] * step - org + BIAS          # [rows, 729, 6] fields
        ok = ((f >= 0) & (f < 1024)).all(2)
        f = np.where(ok[..., None], f, 0)
        q = np.zeros(f.shape[:2], np.int64)
        for a in range(6):
            q = (q << 10) | f[..., a]
        pos = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
        hit = ok & (sk[pos] == q)
        r, k = np.nonzero(hit)
        ks.append(k); ros.append(r + r0); ris.append(order[pos[hit]])
    ks, ros, ris = np.concatenate(ks), np.concatenate(ros), np.concatenate(ris)
    by = np.lexsort((ros, ks))
    ks, ros, ris = ks[by], ros[by], ris[by]
    cut = np.nonzero(np.diff(ks))[0] + 1
    return [(int(k[0]), ro, ri) for k, ro, ri in zip(np.split(ks, cut), np.split(ros, cut), np.split(ris, cut))]


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
    if not maps:
        return acc
    # chain: per output row ascending offset, inside an offset ascending input channel, one fmaf each; the rows in lockstep
    ks = np.concatenate([np.full(len(ro), k, np.int64) for k, ro, _ in maps])
    ros = np.concatenate([ro for _, ro, _ in maps]); ris = np.concatenate([ri for _, _, ri in maps])
    by = np.lexsort((ks, ros))
    ks, ros, ris = ks[by], ros[by], ris[by]
    first = np.concatenate([[0], np.nonzero(np.diff(ros))[0] + 1])
    rank = np.arange(len(ros)) - np.repeat(first, np.diff(np.concatenate([first, [len(ros)]])))
    for j in range(int(rank.max()) + 1):
        sel = rank == j
        rows, kk, xi = ros[sel], ks[sel], x[ris[sel]]
        a = acc[rows]
        for ci in range(cin):
            a = fmaf32(xi[:, ci:ci + 1], W[kk, ci, :], a)
        acc[rows] = a
    return acc


def stage_shapes(widths=WIDTHS):
    """(offsets, Cin, Cout) of the 23 stages (I4)."""
    C1, C2, C3, C4, T4, T3, T2, T1 = widths
    io = [(1, C1), (C1, C1), (C1, C1), (C1, C2), (C2, C2), (C2, C2), (C2, C3), (C3, C3), (C3, C3), (C3, C4), (C4, C4), (C4, C4), (C4, T4), (T4, T4),
          (T4, T4), (T4 + C3, T3), (T3, T3), (T3, T3), (T3 + C2, T2), (T2, T2), (T2, T2), (T2 + C1, T1), (T1, 1)]
    return [(NK if s < 21 else 1, ci, co) for s, (ci, co) in enumerate(io)]


def random_stages(widths=WIDTHS, seed=0, final_bias=None):
    """Folded float32 stages of the given widths: weights scaled so that activations stay of order one through the 23 stages."""
    rng = np.random.default_rng(seed)
    out = []
    for s, (k, cin, cout) in enumerate(stage_shapes(widths)):
        W = rng.standard_normal((k, cin, cout), dtype=np.float32)
        W *= np.float32(1.0 / np.sqrt(cin * min(k, 16)))
        if s < 21:
            sc = rng.uniform(0.5, 1.5, cout).astype(np.float32); of = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
        else:
            sc = np.ones(cout, np.float32); of = np.zeros(cout, np.float32)
        if s == 22:
            of = np.array([rng.uniform(-0.5, 0.5) if final_bias is None else final_bias], np.float32)
        out.append((W, sc, of))
    return out


def widths_of(stages):
    return tuple(int(stages[i][0].shape[-1]) for i in (0, 3, 6, 9, 12, 15, 18, 21))


def run(coords, stages, mode="chain", upto=23):
    """The network on distinct cells inside the extent limit.  Returns dict(levels=[4 coordinate sets], acts={stage: [n_level, Cout]},
    level_of={stage: level}, logit=[n] when upto = 23)."""
    assert status_of(coords) == 0
    dt = np.float64 if mode == "f64" else np.float32
    L = levels(coords)
    org = origin(coords)
    n = len(L[0])
    x0 = np.ones((n, 1), dt)
    acts, level_of = {}, {}
    cache = {}

    def maps(kind, l):
        if (kind, l) not in cache:
            cache[kind, l] = (kernel_map(L[l], L[l], 1 << l, org) if kind == "nb" else
                              kernel_map(L[l + 1], L[l], 1 << l, org) if kind == "dn" else          # F3
                              kernel_map(L[l], L[l + 1], -(1 << l), org))                           # F4: in = u - o t
        return cache[kind, l]

    ident = lambda l: [(0, np.arange(len(L[l])), np.arange(len(L[l])))]

    class Stop(Exception):
        pass

    def stage(s, x, m, lvl, res=None, relu=0):
        W, sc, of = stages[s - 1]
        y = _epilogue(_conv(x, m, W, len(L[lvl]), mode), sc, of, res, relu, mode)      # (scale 1: fmaf(1, acc, bias) is the one add of I4)
        acts[s], level_of[s] = y, lvl
        if s == upto and s < 23:
            raise Stop
        return y

    def block(s, x, lvl):
        t = stage(s, x, maps("nb", lvl), lvl, None, 1)
        return stage(s + 1, t, maps("nb", lvl), lvl, x, 1)

    logit = None
    try:
        x = stage(1, x0, maps("nb", 0), 0)
        s1 = block(2, x, 0)
        s2 = block(5, stage(4, s1, maps("dn", 0), 1), 1)
        s4 = block(8, stage(7, s2, maps("dn", 1), 2), 2)
        s8 = block(11, stage(10, s4, maps("dn", 2), 3), 3)
        u = block(14, stage(13, s8, maps("up", 2), 2), 2)
        u = block(17, stage(16, np.concatenate([u, s4], 1), maps("up", 1), 1), 1)
        u = block(20, stage(19, np.concatenate([u, s2], 1), maps("up", 0), 0), 0)
        x = stage(22, np.concatenate([u, s1], 1), ident(0), 0, None, 1)
        logit = stage(23, x, ident(0), 0)[:, 0]
    except Stop:
        pass
    return dict(levels=L, acts=acts, level_of=level_of, logit=logit)
