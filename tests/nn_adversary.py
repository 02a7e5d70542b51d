"""Adversarial inputs for the f16 filter pass of the NN kernel (csrc/lr_nn16_pass.hip; the error bound it is tested against: csrc/lr_nn16.hip), and an fp64 model of what that pass sees.

The filter pass prunes columns on u' = n1_j - 2 dot16(i, j), a dot product of f16 copies accumulated in fp32, and keeps a column
whenever it could still be within the row's need-th exact distance: the slack that makes this safe is E = 1.05e-3 (n0_i + max_j n1_j)
+ 4e-7.  Random descriptors spend only a small part of it: the rounding errors of competing columns are random and
cancel.  The generators here plant rows where they do not cancel:

* every component sits just above a power of two (the f16 half-ulp is then ~2^-11 relative, the largest it gets);
* the planted neighbour's components, and the query's, sit just below an f16 rounding midpoint: round-to-nearest shrinks |x| of
  both, so dot16 is too small by ~2^-10 dot and the neighbour looks farther away in f16 than it is;
* the decoys sit just above a midpoint (f16 grows them) at a slightly larger exact distance: in f16 they beat the true neighbour,
  which only the margin keeps.

The model is numpy only (no GPU): `filter_model` forms u', E and the thresholds as the kernel does and reports the fraction of the
margin a planted row attains; `exact_d2` is the exact squared distance in integers, the high-precision reference.
"""
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24                # unit roundoff of fp32
CONTRACT_K = 67                 # |d2 of the fp32 fma-chain contract - exact d2| <= 67 u (n0 + n1)  


def _f16_interval(a):
    """|x| (fp32, finite) -> the two adjacent f16 magnitudes lo <= |x| < hi, as fp32."""
    lo = a.astype(np.float16)                                   # RNE; may have rounded up
    lo = np.where(lo.astype(np.float32) > a, np.nextafter(lo, np.float16(0)), lo)
    hi = np.nextafter(lo, np.float16(np.inf))
    lo32 = lo.astype(np.float32)
    hi32 = np.where(np.isinf(hi), np.float32(65536.0), hi.astype(np.float32))
    return lo32, hi32


def steer(v, up, ulps=1):
    """Move every fp32 component of `v` to one side of its f16 rounding midpoint.

    The midpoint is the one between the two f16 magnitudes that enclose |x| (signed zero and f16 subnormals included).  `up=True`
    returns the fp32 value `ulps` fp32 steps above it in magnitude, so that round-to-nearest-even (`(_Float16)x` in nn16_prep_kernel,
    numpy's astype(float16)) grows |x|; `up=False` the value `ulps` steps below it, which rounds towards zero.  Signs are kept; the
    result stays inside the input's f16 interval.  `ulps` may be an array (one count per component)."""
    v = np.asarray(v, np.float32)
    assert np.all(np.isfinite(v)) and np.all(np.abs(v) < 65504.0), "steer: finite values below the f16 maximum"
    a = np.abs(v)
    lo, hi = _f16_interval(a)
    mid = (lo + hi) * np.float32(0.5)                           # exact: lo and hi carry 11 significant bits
    ulps = np.broadcast_to(np.asarray(ulps, np.int64), v.shape)
    assert np.all(ulps >= 1)
    bits = mid.view(np.int32).astype(np.int64)                  # positive fp32: adjacent values are adjacent integers
    r = (bits + np.where(up, ulps, -ulps)).astype(np.int32).view(np.float32)
    return np.copysign(r, v).astype(np.float32)


def rne16(x):
    """Independent round-to-nearest-even to f16 of one fp32 value, in exact rational arithmetic (the check of numpy's rounding)."""
    x = float(np.float32(x))
    if x == 0.0:
        return x
    s, a = (-1.0 if x < 0 else 1.0), Fraction(abs(x))
    e = max(a.numerator.bit_length() - a.denominator.bit_length(), -14)
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    q = Fraction(2) ** (max(e, -14) - 10)                       # f16 quantum of the binade (subnormals: 2^-24)
    n = a / q
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    r = f * q
    if r > 65504:
        return s * float("inf")
    return s * float(r)


# ----------------------------------------------------------------------------- exact reference

def exact_d2_int(F0, F1, pairs):
    """Exact squared distances 2^298 * |F0[i] - F1[j]|^2 as Python integers (every fp32 value is an integer multiple of 2^-149)."""
    F0 = np.asarray(F0, np.float32); F1 = np.asarray(F1, np.float32)
    out = []
    for i, j in pairs:
        acc = 0
        for a, b in zip(F0[i].tolist(), F1[j].tolist()):
            d = int(Fraction(a) * 2 ** 149) - int(Fraction(b) * 2 ** 149)
            acc += d * d
        out.append(acc)
    return out


def exact_d2(F0, F1, pairs):
    """Exact squared distances of (i, j) pairs, correctly rounded to fp64 (the integers of exact_d2_int / 2^298)."""
    return np.array([v / 2 ** 298 for v in exact_d2_int(F0, F1, pairs)], np.float64)


def contract_bound(F0, F1, pairs):
    """The arithmetic contract's bound on |d2_fp32 - d2_exact|: 67 u (n0 + n1)."""
    n0 = _norms64(F0); n1 = _norms64(F1)
    return np.array([CONTRACT_K * U32 * (n0[i] + n1[j]) for i, j in pairs], np.float64)


# ----------------------------------------------------------------------------- fp64 model of the filter pass

def _norms64(F):
    F = np.asarray(F, np.float32).astype(np.float64)
    return np.einsum("ij,ij->i", F, F)


def _h(F):
    return np.asarray(F, np.float32).astype(np.float16).astype(np.float64)


def margin_E(n_row, max_col, n0_only=False):
    """E of a row as the kernel forms it: 1.05e-3 (n_row + max over the column cloud) + 4e-7.  n0_only: the same without the column
    term (what a margin built from the row's own norm would be)."""
    scale = n_row if n0_only else n_row + max_col
    return 1.05e-3 * scale + 4e-7, scale


def filter_model(F0, F1, rows, need=2, cols=None):
    """Forward direction (rows of cloud 0 against all of cloud 1) in fp64 on the f16 copies.

    For each row: u' of every column, U = the need-th smallest u' (the tightest start any sample or tightening round can reach),
    E, the start threshold tau = U + 2E + 6e-6 scale + 2e-6|U| as nn16_passb_kernel forms it, and for the row's planted column
    `cols[r]` (optional) how far above U its u' lies as a fraction of 2E (`frac`), how many columns beat it in f16 (`beaten`),
    whether the start threshold keeps it (`kept`), and the same fraction against a margin built from n0 alone (`frac_n0`) and
    against E without its absolute term 4e-7 (`frac_rel`)."""
    rows = np.asarray(rows)
    H0, H1 = _h(F0)[rows], _h(F1)
    n0 = _norms64(F0)[rows]; n1 = _norms64(F1)
    up = n1[None, :] - 2.0 * (H0 @ H1.T)                        # u' of every (row, column)
    U = np.sort(up, axis=1)[:, need - 1]
    E, scale = margin_E(n0, n1.max())
    En0, _ = margin_E(n0, n1.max(), n0_only=True)
    tau = U + 2.0 * E + 6e-6 * scale + 2e-6 * np.abs(U)
    res = dict(u=up, U=U, E=E, tau=tau, scale=scale)
    if cols is not None:
        cols = np.asarray(cols)
        uj = up[np.arange(len(rows)), cols]
        res.update(u_true=uj, frac=(uj - U) / (2.0 * E), frac_n0=(uj - U) / (2.0 * En0), frac_rel=(uj - U) / (2.0 * (E - 4e-7)),
                   beaten=(up < uj[:, None]).sum(axis=1), kept=uj <= tau)
    return res


def reverse_model(F0, F1, jrows, icols, s_star):
    """Reverse direction as lr_nn16_reverse forms it: the row is cloud-1 point j, the column cloud-0 point i', the threshold comes
    from the exact (contract) distance s* of j's best forward pointer: tau = (d2hi - n_j) + E + 6e-6 scale + 2e-6 d2hi with
    d2hi = s*^2 (1 + 6e-7) and E = 1.05e-3 (n_j + max_i n0_i) + 4e-7.  `frac` = (u' - (d2hi - n_j)) / E: the part of the one-sided
    margin that the column's f16 error uses up (1 = pruned)."""
    jrows = np.asarray(jrows); icols = np.asarray(icols)
    n0 = _norms64(F0); n1 = _norms64(F1)[jrows]
    up = n0[icols] - 2.0 * np.einsum("ij,ij->i", _h(F1)[jrows], _h(F0)[icols])
    s = np.asarray(s_star, np.float32).astype(np.float64)
    d2hi = s * s * (1.0 + 6e-7)
    E, scale = margin_E(n1, n0.max())
    En, _ = margin_E(n1, n0.max(), n0_only=True)
    tau = (d2hi - n1) + E + 6e-6 * scale + 2e-6 * d2hi
    base = d2hi - n1
    return dict(u=up, E=E, tau=tau, frac=(up - base) / E, frac_n0=(up - base) / En, kept=up <= tau)


# ----------------------------------------------------------------------------- generators

@dataclass
class Planted:
    """Clouds with planted rows.  Forward: `rows` (cloud 0) have the planted neighbour `true` (cloud 1) and `decoys[r]` (cloud-1
    columns that beat it in f16).  Reverse: cloud-1 points `jrow` whose best forward pointer is `istar`, and cloud-0 points `iprime`
    exactly closer to them that point elsewhere (at `j1`)."""
    F0: np.ndarray
    F1: np.ndarray
    need: int
    form: str
    rows: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    true: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    decoys: list = field(default_factory=list)
    jrow: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    istar: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    iprime: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    j1: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


def _layout(dim, rng, target=1.0):
    """Binade exponents of a template row: components 2^e or 2^(e+1) so that the squared norm is about `target`."""
    a = 2.0 ** np.floor(np.log2(np.sqrt(target / dim)))
    n_hi = int(np.clip(round((target / a ** 2 - dim) / 3.0), 0, dim))
    mag = np.full(dim, a)
    mag[rng.permutation(dim)[:n_hi]] *= 2.0
    return mag


def _template(mag, rng, lo_step=16, hi_step=24):
    """A signed template just above powers of two: component k at mag_k (1 + s 2^-10), s in [lo_step, hi_step)."""
    sgn = rng.choice([-1.0, 1.0], size=mag.shape)
    return sgn, mag * (1.0 + rng.integers(lo_step, hi_step, size=mag.shape) * 2.0 ** -10)


def _at(sgn, m, up, rng, deep=1):
    """Signed, steered fp32 row from magnitudes m: up / down, a random 1..deep fp32 steps from the midpoint."""
    return steer((sgn * m).astype(np.float32), up, rng.integers(1, deep + 1, size=m.shape))


def _cloud(n, dim, rng, norm2):
    """Random directions with squared norms `norm2` (a scalar or an (n,) array)."""
    X = rng.standard_normal((n, dim))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return (X * np.sqrt(np.asarray(norm2, np.float64)).reshape(-1, 1)).astype(np.float32)


def _ballast(row, target):
    """Set the last component so that the squared norm is `target` (keeps the column norms of the sign form within 1e-4)."""
    row = row.astype(np.float64)
    rest = float(np.dot(row[:-1], row[:-1]))
    assert rest < target, (rest, target)
    out = row.copy()
    out[-1] = np.copysign(np.sqrt(target - rest), row[-1] if row[-1] != 0 else 1.0)
    return out.astype(np.float32)


def forward(n0=6000, n1=6000, dim=32, n_rows=48, need=2, n_decoys=3, form="plain", seed=0, query_scale=1.0, lift=0, subnormal=False,
            spread_decoys=False):
    """Plant `n_rows` query rows in a random cloud pair.

    Row r: query q (cloud 0) and its planted neighbour t (cloud 1), both just below an f16 midpoint in every component, t a few
    fp32 steps from q; `n_decoys` columns just above a midpoint, each moved 4..6 f16 steps per component towards zero from q (sign
    form: half of them outwards), an exact d2 gap far above the contract's rounding.  form "sign": every column norm within 1e-4 (a ballast last component); "plain": the
    random columns' norms spread over [0.7, 1] (a wider spread loosens the sampled start thresholds until the candidate store
    overflows).  query_scale < 1 shrinks the planted query and its columns; lift = p > 0 makes the planted columns 2^p times the
    query (the same mantissas, so they round the same way; the decoys one f16 step farther out in a quarter of the components):
    with n0 << n1_j the column terms of E carry the bound.  subnormal: planted components of 1..3 f16 subnormal quanta (~1e-7), the
    f16 products of the matrix cores at the bottom of their range.  (The cloud stays ordinary: in a cloud this small everywhere
    E's absolute term 4e-7 admits every column, the candidate store overflows and the exact scan decides every row -- by design,
    and a test of nothing.)
    spread_decoys: decoys over all column tiles (else scattered at random, which is the same for a handful)."""
    rng = np.random.default_rng(seed)
    assert form in ("sign", "plain")
    target = 1.0
    if form == "sign":
        F0 = _cloud(n0, dim, rng, target)
        F1 = _cloud(n1, dim, rng, target)
    else:
        F0 = _cloud(n0, dim, rng, rng.uniform(0.7, 1.0, n0))
        F1 = _cloud(n1, dim, rng, rng.uniform(0.7, 1.0, n1))
    cols_per_row = 1 + n_decoys
    assert n_rows * cols_per_row <= n1 and n_rows <= n0
    rows = np.sort(rng.choice(n0, n_rows, replace=False))
    free = rng.permutation(n1)
    if spread_decoys:
        # column k * band + r for member k of row r: every row's decoys are spread evenly over the whole column range
        band = n1 // cols_per_row
        assert n_rows <= band
        free = (np.arange(cols_per_row)[None, :] * band + rng.permutation(band)[:n_rows, None]).reshape(-1)
    true, decoys = np.empty(n_rows, np.int64), []
    for r, i in enumerate(rows):
        cj = free[r * cols_per_row:(r + 1) * cols_per_row]
        if subnormal:
            # 1..3 subnormal quanta (2^-24 ~ 6e-8); query just below the midpoint, the neighbour within two fp32 steps of it, the
            # decoys just above it, ~1e-9 per component farther away: an exact gap far above the contract's rounding at these norms
            # (~1e-18), far below the f16 error of u' (~1e-13), and both far below E's absolute term
            sgn = rng.choice([-1.0, 1.0], size=dim)
            base = 2.0 ** -24 * rng.integers(1, 4, size=dim)
            deep = rng.integers(2 ** 16, 2 ** 17, size=dim)
            q = steer((sgn * base).astype(np.float32), False, deep)
            t = steer((sgn * base).astype(np.float32), False, deep + rng.integers(0, 2, size=dim))
            decs = [steer((sgn * base).astype(np.float32), True, rng.integers(2 ** 17, 2 ** 18, size=dim)) for _ in range(n_decoys)]
        else:
            if form == "sign":                                  # the last component is the ballast
                mag = np.append(_layout(dim - 1, rng, 0.95 * target * query_scale), 0.0)
            else:
                mag = _layout(dim, rng, target * query_scale)
            sgn, base = _template(mag, rng, 7, 11)
            q = _at(sgn, base, False, rng)
            t = _at(sgn, base, False, rng, deep=64)
            decs = []
            if lift:
                L = 2.0 ** lift
                t = (q * np.float32(L)).astype(np.float32)
                for _ in range(n_decoys):
                    step = np.zeros(dim); step[rng.permutation(dim)[:max(1, dim // 4)]] = 1.0
                    decs.append(_at(sgn, L * (base + mag * 2.0 ** -10 * step), True, rng))
            for _ in range(0 if lift else n_decoys):
                step = mag * 2.0 ** -10 * rng.integers(4, 7, size=dim)
                if form == "sign":
                    # half of the squared-norm change inwards, half outwards: the ballast, and so the decoy's extra distance, stays small
                    order, acc, way = np.argsort(-base * step), 0.0, np.zeros(dim)
                    for k in order:
                        way[k] = -1.0 if acc >= 0 else 1.0
                        acc += way[k] * base[k] * step[k]
                    step = step * way
                else:
                    step = -step        # (towards the power of two: a decoy's relative f16 error is a little larger than the query's)
                decs.append(_at(sgn, base + step, True, rng))
            if form == "sign":
                q, t = _ballast(q, target), _ballast(t, target)
                decs = [_ballast(d, target) for d in decs]
        F0[i] = q
        F1[cj[0]] = t
        for k, d in enumerate(decs):
            F1[cj[1 + k]] = d
        true[r] = cj[0]
        decoys.append(np.asarray(cj[1:], np.int64))
    return Planted(F0=F0, F1=F1, need=need, form=form, rows=rows, true=true, decoys=decoys)


def reverse(n0=6000, n1=6000, dim=32, n_groups=48, form="plain", seed=0):
    """Plant `n_groups` groups for the reverse (mutual) pass.

    j (cloud 1) and i' (cloud 0) both sit just below an f16 midpoint in every component (dot16 too small by ~2^-10 dot: i' looks
    farther from j in f16 than it is); i' lies 4..6 f16 steps per component from j, i* (cloud 0) on the opposite side at a
    slightly larger exact distance, so j is i*'s nearest point and i*'s pair (i*, j) sets the reverse threshold of row j; j1
    (cloud 1) is closer to i' than j, so i' points at j1 and has j as its SECOND neighbour -- the s2 ordering of the reverse pass
    admits it, and only the reverse margin E keeps it: the mutual list then drops i*."""
    rng = np.random.default_rng(seed)
    target = 1.0
    if form == "sign":
        F0 = _cloud(n0, dim, rng, target); F1 = _cloud(n1, dim, rng, target)
    else:
        F0 = _cloud(n0, dim, rng, rng.uniform(0.7, 1.0, n0)); F1 = _cloud(n1, dim, rng, rng.uniform(0.7, 1.0, n1))
    assert 2 * n_groups <= min(n0, n1)
    c0 = rng.permutation(n0)[:2 * n_groups].reshape(n_groups, 2)
    c1 = rng.permutation(n1)[:2 * n_groups].reshape(n_groups, 2)
    for g in range(n_groups):
        mag = np.append(_layout(dim - 1, rng, 0.95 * target), 0.0) if form == "sign" else _layout(dim, rng, target)
        sgn, base = _template(mag, rng, 7, 10) if form == "sign" else _template(mag, rng, 1, 4)
        step = mag * 2.0 ** -10
        off = rng.integers(4, 7, size=dim).astype(np.float64)  # plain: outwards, i' stays close to the power of two as well
        if form == "sign":
            # half of the squared-norm change inwards, half outwards: the ballasts of i', i*, j1 and j stay close
            acc = 0.0
            for k in np.argsort(-base * off):
                w = -1.0 if acc >= 0 else 1.0
                acc += w * base[k] * off[k]
                off[k] *= w
        j = _at(sgn, base, False, rng)
        ip = _at(sgn, base + off * step, False, rng)
        # i*: the mirror image of i' about j, one more f16 step per component (exactly farther, by far more than the contract's rounding)
        ist = _at(sgn, base - (off + np.sign(off)) * step, True, rng)
        # j1: between i' and j, closer to i'
        j1 = _at(sgn, base + np.round(off * 0.7) * step, True, rng)
        if form == "sign":
            j, ip, ist, j1 = (_ballast(v, target) for v in (j, ip, ist, j1))
        F1[c1[g, 0]] = j; F1[c1[g, 1]] = j1
        F0[c0[g, 0]] = ip; F0[c0[g, 1]] = ist
    return Planted(F0=F0, F1=F1, need=2, form=form, jrow=c1[:, 0].astype(np.int64), j1=c1[:, 1].astype(np.int64),
                   iprime=c0[:, 0].astype(np.int64), istar=c0[:, 1].astype(np.int64))


def norm_spread(F):
    """(max - min) / max of the squared row norms: the filter pass takes the sign form of its test when this is <= 1e-4."""
    n = _norms64(F)
    return float((n.max() - n.min()) / n.max())


def forward_fractions(p):
    """Attained fractions of the forward margin 2E (and of a margin built from n0 alone) for the planted rows of `p`."""
    return filter_model(p.F0, p.F1, p.rows, p.need, p.true)


def reverse_fractions(p, s_star):
    """Attained fractions of the reverse margin E for the planted groups of `p`; s_star[g] = contract distance of (istar, jrow)."""
    return reverse_model(p.F0, p.F1, p.jrow, p.iprime, s_star)


# ----------------------------------------------------------------------------- the cases both test files run

CASES = {
    # name: (generator, keyword arguments)
    "top2_plain": (forward, dict(seed=11)),
    "top1_plain": (forward, dict(need=1, n_decoys=2, seed=12)),
    "top2_sign": (forward, dict(form="sign", seed=13)),
    "tighten": (forward, dict(n0=4000, n1=8000, n_rows=40, n_decoys=70, spread_decoys=True, seed=14)),
    "small_query": (forward, dict(query_scale=2.0 ** -6, lift=1, seed=15)),
    # (few: columns at the origin are candidates of every row whose neighbours are far, and too many overflow the store)
    "subnormal": (forward, dict(subnormal=True, n_rows=2, n_decoys=2, seed=16)),
    "dim8": (forward, dict(dim=8, seed=17)),
    "dim31": (forward, dict(dim=31, seed=18)),
    "reverse_plain": (reverse, dict(seed=19)),
    "reverse_sign": (reverse, dict(form="sign", seed=20)),
}

_MADE = {}


def make(name):
    """The planted clouds of case `name` (built once per process)."""
    if name not in _MADE:
        gen, kw = CASES[name]
        _MADE[name] = gen(**kw)
    return _MADE[name]
