"""The adversarial NN inputs (tests/nn_adversary.py) do what they claim, without a GPU: in an fp64 model of the f16 filter pass the
planted neighbour is beaten by its decoys and only the margin keeps it, the margin is used up to the measured fractions below, the
oracle's answer is the planted one, and the oracle's distances agree with the exact ones within the arithmetic contract."""
import numpy as np
import pytest

from tests import nn_adversary as A

FORWARD = [k for k, (g, _) in A.CASES.items() if g is A.forward]
REVERSE = [k for k, (g, _) in A.CASES.items() if g is A.reverse]

# Floors of the attained fraction of the margin, measured on these seeds: forward u'(true) - U over 2E, reverse
# u'(i') - (d2hi - n_j) over E.  The forward pass can reach about half of 2E: the shared query rounds one way, so only the
# neighbour's side of the error adds up (plain 0.453-0.455); the sign form loses a little to its ballast component (0.434-0.448).
# The reverse pass is one-sided and reaches 0.918-0.919 (sign form: 0.872-0.901).
FLOOR = {"top2_plain": 0.45, "top1_plain": 0.45, "tighten": 0.45, "dim8": 0.45, "dim31": 0.45, "top2_sign": 0.42,
         "reverse_plain": 0.90, "reverse_sign": 0.85}


def _contract_ok(F0, F1, pairs, s):
    """|s^2 - d2_exact| within 67 u (n0 + n1) (+ the rounding of the square root and of s^2)."""
    d2 = A.exact_d2(F0, F1, pairs)
    s64 = np.asarray(s, np.float32).astype(np.float64)
    tol = A.contract_bound(F0, F1, pairs) + 2.0 ** -21 * s64 * s64 + 1e-30
    return np.abs(s64 * s64 - d2) <= tol, np.abs(s64 * s64 - d2) / A.contract_bound(F0, F1, pairs)


@pytest.mark.parametrize("name", FORWARD)
def test_forward_plant_is_pruned_without_the_margin_and_kept_with_it(name, oracle):
    p = A.make(name)
    m = A.forward_fractions(p)
    # in f16, at least `need` decoys beat the true neighbour: a start threshold without the 2E margin would prune it ...
    assert np.all(m["beaten"] >= p.need), m["beaten"]
    assert np.all(m["u_true"] > m["U"])
    # ... and with it, it stays
    assert np.all(m["kept"])
    print(f"\n{name}: forward fraction of 2E {m['frac'].min():.3f}-{m['frac'].max():.3f}, of a 2E built from n0 alone "
          f"{m['frac_n0'].min():.3f}-{m['frac_n0'].max():.3f}, without the absolute term {m['frac_rel'].min():.3g}-{m['frac_rel'].max():.3g}, "
          f"column norm spread {A.norm_spread(p.F1):.2e}")
    if name in FLOOR:
        assert m["frac"].min() >= FLOOR[name], m["frac"].min()
    if name == "small_query":
        # n0 << n1 of the planted columns: a margin built from the query's norm alone would be crossed
        assert m["frac_n0"].min() >= 1.1, m["frac_n0"].min()
    if name == "subnormal":
        # deep f16 subnormals (the planted rows' squared norms ~1e-13): the f16 error of u' is tiny against E, but it still puts
        # every decoy ahead of the neighbour (above); the matrix cores must keep subnormal products
        assert A._norms64(p.F0[p.rows]).max() < 1e-12 and np.all(np.abs(p.F0[p.rows]) < 2.0 ** -14)
    if p.form == "sign":
        assert A.norm_spread(p.F1) <= 1e-4
    else:
        assert A.norm_spread(p.F1) > 1e-2
    # the oracle (the contract) names the planted neighbour; the exact order agrees, and so does the contract's distance
    o1, o2, s1, s2 = oracle.nn_top2(p.F0, p.F1)
    assert np.array_equal(o1[p.rows], p.true)
    for r, i in enumerate(p.rows):
        ex = A.exact_d2_int(p.F0, p.F1, [(i, p.true[r])] + [(i, j) for j in p.decoys[r]])
        assert ex[0] < min(ex[1:]), (name, r)
        if p.need == 2:
            assert o2[i] in p.decoys[r]
    ok, rel = _contract_ok(p.F0, p.F1, list(zip(p.rows, p.true)), s1[p.rows])
    assert ok.all(), rel.max()
    sec = [(i, o2[i]) for i in p.rows]
    ok2, rel2 = _contract_ok(p.F0, p.F1, sec, s2[p.rows])
    assert ok2.all(), rel2.max()
    print(f"{name}: oracle |d2 - exact| up to {max(rel.max(), rel2.max()):.3f} of the contract's 67u(n0+n1)")


@pytest.mark.parametrize("name", REVERSE)
def test_reverse_plant_uses_up_the_reverse_margin(name, oracle):
    p = A.make(name)
    o1, o2, s1, s2 = oracle.nn_top2(p.F0, p.F1)
    # i* points at j, i' points at j1 and has j as its second neighbour; i' is exactly closer to j than i* is
    assert np.array_equal(o1[p.istar], p.jrow) and np.array_equal(o1[p.iprime], p.j1) and np.array_equal(o2[p.iprime], p.jrow)
    for g in range(len(p.jrow)):
        a, b = A.exact_d2_int(p.F0, p.F1, [(p.iprime[g], p.jrow[g]), (p.istar[g], p.jrow[g])])
        assert a < b, g
    m = A.reverse_fractions(p, s1[p.istar])
    print(f"\n{name}: reverse fraction of E {m['frac'].min():.3f}-{m['frac'].max():.3f}, of an E built from n_j alone "
          f"{m['frac_n0'].min():.3f}-{m['frac_n0'].max():.3f}, row norm spread {A.norm_spread(p.F0):.2e}")
    assert np.all(m["kept"]) and m["frac"].max() < 1.0
    assert m["frac"].min() >= FLOOR[name], m["frac"].min()
    assert m["frac_n0"].min() >= 1.1
    if p.form == "sign":
        assert A.norm_spread(p.F0) <= 1e-4 and A.norm_spread(p.F1) <= 1e-4
    # the mutual filter of the contract drops i* (j's reverse neighbour is i')
    mut = oracle.nn_to_mutual(p.F0, p.F1, np.arange(len(p.F0)), o1, o2)
    assert not np.isin(p.istar, mut[0]).any()
    ok, rel = _contract_ok(p.F0, p.F1, list(zip(p.istar, p.jrow)) + list(zip(p.iprime, p.jrow)),
                           np.concatenate([s1[p.istar], s2[p.iprime]]))
    assert ok.all(), rel.max()


def _binade_samples(rng):
    xs = [0.0, -0.0]
    for e in range(-26, 16):                     # below the smallest f16 subnormal .. the top binade
        m = rng.random(24)
        xs += list((1.0 + m) * 2.0 ** e)
        xs += [2.0 ** e, 2.0 ** e * (1 + 2.0 ** -11), 2.0 ** e * (2 - 2.0 ** -12)]
    xs = np.array(xs, np.float32)
    xs = xs[np.abs(xs) < 65504.0]
    sg = np.where(rng.random(xs.shape) < 0.5, -1.0, 1.0).astype(np.float32)
    return np.concatenate([xs, sg * xs, -xs]).astype(np.float32)


@pytest.mark.parametrize("up", [False, True])
def test_steer_rounds_as_numpy_and_the_device_conversion_do(up):
    """steer() puts a value one fp32 step from its f16 midpoint; numpy's float16 conversion (round to nearest even, like the
    device's (_Float16) conversion) then rounds it the requested way, and an independent exact RNE agrees with numpy on the
    steered values, their neighbours across the midpoint, and the midpoints themselves (ties to even), on every binade, signed
    zero and the f16 subnormals included."""
    rng = np.random.default_rng(5)
    x = _binade_samples(rng)
    r = A.steer(x, up)
    a = np.abs(x).astype(np.float64)
    h = np.abs(r.astype(np.float16).astype(np.float64))
    lo, hi = A._f16_interval(np.abs(x))
    assert np.all(lo <= a) and np.all(a < hi)
    assert np.array_equal(h, (hi if up else lo).astype(np.float64))
    assert np.array_equal(np.signbit(r), np.signbit(x))                     # signed zero keeps its sign
    # one fp32 step back is the midpoint itself: r is adjacent to it
    back = np.nextafter(np.abs(r), np.float32(0) if up else np.float32(np.inf))
    mid = (lo.astype(np.float64) + hi) / 2
    tie = back.astype(np.float64) == mid
    assert np.all(tie)
    # inside the input's f16 interval
    assert np.all(np.abs(r) > lo) and np.all(np.abs(r) < hi)
    # numpy's conversion against an exact round-to-nearest-even
    for v in np.concatenate([r, back, -back]):
        want = A.rne16(v)
        got = float(np.float32(v).astype(np.float16))
        assert got == want and np.signbit(got) == np.signbit(want), (v, got, want)
    # a multi-step steer stays on its side
    r5 = A.steer(x, up, 5)
    assert np.array_equal(np.abs(r5.astype(np.float16).astype(np.float64)), h)
    # ties at the midpoint go to the even neighbour (numpy and the exact reference)
    ev = np.where((lo.astype(np.float16).view(np.uint16) & 1) == 0, lo, hi).astype(np.float64)
    assert np.array_equal(np.abs(mid.astype(np.float32).astype(np.float16).astype(np.float64)), ev)


def test_exact_d2_is_exact():
    """exact_d2 against Fraction arithmetic on fp32 values that cancel catastrophically and span the exponent range."""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    F0 = (rng.standard_normal((6, 32)) * 2.0 ** rng.integers(-30, 10, (6, 32))).astype(np.float32)
    F1 = F0.copy()
    F1[:, ::3] = np.nextafter(F1[:, ::3], np.float32(np.inf))
    F1[5] = np.float32(1e-40)                                               # fp32 subnormals
    pairs = [(i, j) for i in range(6) for j in range(6)]
    ints = A.exact_d2_int(F0, F1, pairs)
    for (i, j), v in zip(pairs, ints):
        ref = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(F0[i], F1[j]))
        assert Fraction(v, 2 ** 298) == ref
