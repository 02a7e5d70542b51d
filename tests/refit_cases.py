"""Seeded cases for the stage after RANSAC (tests/refit_cpu.py restates it): sizes at the thread, block and staging edges of
refit_moments_kernel (256 threads x 4 pairs = 1 024 pairs per block, partials summed 64 blocks = 65 536 pairs at a time), inlier
patterns aimed at the slots of that layout, listed pairs with a live count, weights, rows without a partner, and pairs exactly on the
threshold.  Each case carries the condition that makes the reference decisive; tests/test_refit_cpu.py checks it.

Generic pairs keep a margin.  A pair is built as q = T p + e with |e| drawn from [0, 0.58] m (inlier) or [0.62, 3] m (outlier), so
|T p - q|^2 lies outside (0.336, 0.384) around thr2 = 0.36 up to the float32 rounding of q (< 1e-4 m^2 at these coordinates).  What the
comparison needs is far less: the kernel's fp64 d2 differs from the exact one by at most refit_cpu.d2_bound(d2, M, 2^-53, 7), and with
the coordinates used here -- clouds within 20 m of rigid_hp.LIDAR_OFFSET, translations below 50 m, so M < 600 m -- that is
1.01 (2 sqrt(3) 0.6 * 7 * 2^-53 * 600 + ...) < 1.0e-12 m^2 at the threshold.  MARGIN = 1e-9 m^2 is that bound with a factor 1 000 to
spare; every generic pair's exact d2 is at least MARGIN away from thr2 (pairs that are not are redrawn).

Boundary pairs are exact: coordinates and the shift of T are dyadic with few bits and the rotation is the identity, so every fp64
operation of the kernel's expression -- and every float32 operation of lr_score_d2 -- is exact, and d2 == thr2 is decided by the
comparison alone.
"""
import functools

import numpy as np

from tests import refit_cpu as rc
from tests import rigid_hp as hp

THR2 = 0.36                      # (2 * 0.3)^2 (FR.py:105)
MARGIN = 1e-9
BLOCK, WAVE, THREADS = 1024, 64, 256
SMALL = (1, 2, 3, 4, 255, 256, 257, 1023, 1024, 1025, 2049)
LARGE = (65536, 65537, 66561)
MASK_SIZES = (1, 63, 64, 65, 255, 256, 257, 65537)


# ------------------------------------------------------------------------------------------------------------ inlier patterns
def pattern(name, n):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "last_block":                  # only the last, partial block
        return i >= (n - 1) // BLOCK * BLOCK
    if name == "lane0":                       # only lane 0 of each wave
        return i % WAVE == 0
    if name == "u3":                          # only the fourth pair of each thread
        return (i % BLOCK) // THREADS == 3
    if name == "two":
        return (i == 0) | (i == n - 1)
    if name == "three":
        return (i == 0) | (i == n // 2) | (i == n - 1)
    if name == "block64":                     # only the first block of the second staging chunk
        return (i >= 64 * BLOCK) & (i < 65 * BLOCK)
    raise KeyError(name)


def _model(rng):
    T = np.eye(4)
    T[:3, :3] = hp.random_rot(rng)
    T[:3, 3] = rng.uniform(-30, 30, 3)
    return T


def _pairs(rng, n, inl, T, offset=hp.LIDAR_OFFSET, r_in=0.58):
    """P [n,3] float32 and Q [n,3] float32 with q = T p + e, |e| by the pattern (inliers up to r_in); every pair at least MARGIN from
    THR2 (exactly)."""
    P = (rng.uniform(-20, 20, (n, 3)) + offset).astype(np.float32)
    Q = np.zeros((n, 3), np.float32)
    todo = np.arange(n)
    while todo.size:
        k = todo.size
        d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = np.where(inl[todo], rng.uniform(0.0, r_in, k), rng.uniform(0.62, 3.0, k))
        Q[todo] = (P[todo].astype(np.float64) @ T[:3, :3].T + T[:3, 3] + d * r[:, None]).astype(np.float32)
        got, gap, _ = rc.exact_d2(P[todo], Q[todo], T, THR2)
        todo = todo[(np.abs(gap) < MARGIN) | (got != inl[todo])]
    return P, Q


def _scatter(rng, Q, n1=None):
    """xyz1 holding Q's rows in a random order (and n1 - n rows that no pair names), idx1 with xyz1[idx1[i]] = Q[i]."""
    n = Q.shape[0]
    n1 = n if n1 is None else n1
    idx1 = rng.permutation(n1)[:n].astype(np.int32)
    xyz1 = (rng.uniform(-20, 20, (n1, 3)) + hp.LIDAR_OFFSET).astype(np.float32)
    xyz1[idx1] = Q
    return xyz1, idx1


def _case(name, kind, **kw):
    c = dict(name=name, kind=kind, thr2=THR2, idx0=None, m=None, F0=None, F1=None, exact=False)
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------------------ plain refit
def plain_specs():
    specs = []
    for n in SMALL:
        if n <= 4:
            pats = ["all", "none"] + (["two"] if n >= 2 else []) + (["three"] if n >= 3 else [])
        elif n <= 257:
            pats = ["all", "lane0"]
        else:
            pats = ["all", "none", "last_block", "lane0", "u3", "two", "three"]
        specs += [(n, p) for p in pats]
    specs += [(65536, "lane0"), (65537, "all"), (66561, "block64")]
    return specs


@functools.lru_cache(maxsize=None)
def plain_case(n, pat):
    rng = np.random.default_rng([11, n, sum(map(ord, pat))])
    T = _model(rng)
    inl = pattern(pat, n)
    P, Q = _pairs(rng, n, inl, T)
    xyz1, idx1 = _scatter(rng, Q)
    return _case(f"plain n={n} {pat}", "plain", xyz0=P, xyz1=xyz1, idx1=idx1, T=T, planted=inl)


# ------------------------------------------------------------------------------------------------------------ listed pairs (refit = 2)
LISTED = [("perm", 2049, 0), ("perm", 2049, 1), ("perm", 2049, 3), ("perm", 2049, 1024), ("perm", 2049, 1025), ("perm", 2049, 2049),
          ("repeats", 2049, 1025), ("repeats", 2049, 2049), ("perm", 66561, 65537)]


@functools.lru_cache(maxsize=None)
def listed_case(how, L, m):
    """Lists of allocated length L of which m rows are live.  Rows at and beyond m name inlier pairs, in range: a kernel that reads
    them counts more pairs and fits another transform, and faults nowhere.  Among the live rows every third is an outlier."""
    rng = np.random.default_rng([12, L, m, len(how)])
    T = _model(rng)
    n0 = L
    idx0 = (rng.permutation(n0) if how == "perm" else rng.integers(0, n0 // 4, L)).astype(np.int32)
    live_in = np.arange(L) % 3 != 2
    live_in[max(m - 1, 0)] = True                                     # the last live row counts: a count one short shows
    want = np.where(np.arange(L) < m, live_in, True)                  # per list row
    # a point may be listed more than once: its status is that of its first row, so later rows of a repeated point follow it
    first = np.full(n0, -1, np.int64)
    for c in range(L - 1, -1, -1):
        first[idx0[c]] = c
    inl_pt = np.zeros(n0, bool)
    inl_pt[first >= 0] = want[first[first >= 0]]
    P, Q = _pairs(rng, n0, inl_pt, T)
    xyz1, nn = _scatter(rng, Q)
    idx1 = nn[idx0]                                                   # the partner of point idx0[c]
    return _case(f"listed {how} L={L} m={m}", "listed", xyz0=P, xyz1=xyz1, idx1=idx1, idx0=idx0, m=m, T=T, planted=inl_pt[idx0])


# ------------------------------------------------------------------------------------------------------------ weights (refit = 3)
WEIGHTED = [("identical", 32), ("identical", 5), ("dominant", 32), ("dominant", 5), ("below_one", 32), ("below_one", 5), ("ordinary", 32),
            ("ordinary", 5), ("two", 32), ("one", 5)]


@functools.lru_cache(maxsize=None)
def weighted_case(how, dim, r_in=0.58):
    """257 pairs, descriptors of `dim` columns (r_in: how far an inlier lies from T p at most -- 0.05 where a RANSAC run has to find T
    again from the pairs and keep them in):
      identical   F1[idx1[i]] = F0[i]: distance 0, every weight is the clamp's 1e12
      dominant    one inlier at feature distance 2^-20 among distances of about 1: its weight is 10^6 times the others'
      below_one   distances of several thousand: 170 inliers whose weights sum to less than 1
      ordinary    distances of about 1
      two / one   two inliers / one: the unweighted gate (fewer than 3) does not apply under weights"""
    n = 257
    rng = np.random.default_rng([13, dim, sum(map(ord, how))])
    T = _model(rng)
    inl = np.arange(n) % 3 != 2
    if how == "two":
        inl = pattern("two", n)
    if how == "one":
        inl = np.arange(n) == 100
    P, Q = _pairs(rng, n, inl, T, r_in=r_in)
    xyz1, idx1 = _scatter(rng, Q)
    scale = 4096.0 if how == "below_one" else 1.0
    F0 = (rng.normal(size=(n, dim)) * scale).astype(np.float32)
    F1 = np.zeros((n, dim), np.float32)
    F1[idx1] = F0 if how == "identical" else (F0 + rng.normal(size=(n, dim)) * scale * 0.3).astype(np.float32)
    if how == "dominant":
        F0[0] = np.round(F0[0] * 16) / 16
        F1[idx1[0]] = F0[0]; F1[idx1[0], 0] += np.float32(2.0 ** -20)
    return _case(f"weighted {how} dim={dim}", "weighted", xyz0=P, xyz1=xyz1, idx1=idx1, T=T, F0=F0, F1=F1, planted=inl)


# ------------------------------------------------------------------------------------------------------------ rows without a partner
@functools.lru_cache(maxsize=None)
def skip_case(n=1025):
    """idx1[i] = -1 on every fifth row and on the last: those rows are skipped, whatever their point is."""
    c = dict(plain_case(n, "all"))
    idx1 = c["idx1"].copy()
    idx1[::5] = -1; idx1[-1] = -1
    c.update(name=f"skip n={n}", kind="skip", idx1=idx1, planted=idx1 >= 0)
    return c


# ------------------------------------------------------------------------------------------------------------ exact boundary
NEXT64 = float(np.nextafter(0.375, np.inf))
NEXT32 = float(np.nextafter(np.float32(0.375), np.float32(np.inf)))
# residuals T p - q: A on the threshold 0.375 = 0.5^2 + 0.25^2 + 0.25^2, B just inside, C just outside, then five plain inliers
_RES = np.array([[0.5, 0.25, 0.25], [0.5, 0.25, 0.25 - 2.0 ** -11], [0.5, 0.25, 0.25 + 2.0 ** -11],
                 [0.125, 0.0, 0.0], [0.0, 0.125, 0.0], [0.0, 0.0, -0.125], [0.25, -0.125, 0.0], [-0.125, 0.0, 0.25]])
BOUNDARY = {"at": (0.375, [False, True, False]), "next64": (NEXT64, [True, True, False]), "next32": (NEXT32, [True, True, False])}


@functools.lru_cache(maxsize=None)
def boundary_case(which):
    """thr2 = 0.375: pair A (d2 == thr2) is out; thr2 = the next fp64 (for the mask: the next float32) above: A is in."""
    thr2, abc = BOUNDARY[which]
    T = np.eye(4); T[:3, 3] = [0.5, -0.25, 2.0]
    base = np.array([80.0, -61.0, 2.5])
    steps = np.array([[0, 0, 0], [1, 2, 0], [-3, 1, 1], [2, -2, 0.5], [0.5, 4, -1], [-1.5, -0.5, 2], [4, 0.25, 0.75], [-2, 3, -0.25]])
    P = (base + steps).astype(np.float32)
    Q = (P.astype(np.float64) + T[:3, 3] - _RES).astype(np.float32)
    planted = np.array(abc + [True] * 5)
    return _case(f"boundary {which}", "boundary", xyz0=P, xyz1=Q, idx1=np.arange(8, dtype=np.int32), T=T, thr2=thr2, planted=planted,
                 exact=True)


# ------------------------------------------------------------------------------------------------------------ mask
@functools.lru_cache(maxsize=None)
def mask_case(m):
    """m pairs src[c] <-> tgt[c], two in three inliers, every one far outside the float32 rounding of lr_score_d2 (refit_cpu.mask's
    bound: about 4e-4 m^2 at these coordinates; the pairs stay 0.02 m^2 away)."""
    rng = np.random.default_rng([14, m])
    T = _model(rng)
    inl = np.arange(m) % 3 != 1
    P, Q = _pairs(rng, m, inl, T)
    return dict(name=f"mask m={m}", src=P, tgt=Q, T=T, thr2=THR2, planted=inl)


# ------------------------------------------------------------------------------------------------------------ the comparison
def oracle_refit(orc, c, thr2=None, rows=None, use_idx0=True, m_shift=0):
    """The oracle on a case, the way oracle.register_pair drives it (refit = 2: the listed pairs gathered, then the identity list).
    The keyword arguments plant mistakes (test_planted_mistakes_are_noticed): another threshold, only the first `rows` rows, the point
    list ignored, the live count shifted."""
    thr2 = c["thr2"] if thr2 is None else thr2
    if c["idx0"] is not None:
        m = int(np.clip(c["m"] + m_shift, 0, len(c["idx0"])))
        m = m if rows is None else min(m, rows)
        i0 = c["idx0"][:m] if use_idx0 else np.arange(m)
        return orc.refit(c["xyz0"][i0], c["xyz1"][c["idx1"][:m]], np.arange(m), c["T"], thr2=thr2)
    n = len(c["idx1"]) if rows is None else rows
    F = {} if c["F0"] is None else dict(feats0=c["F0"][:n], feats1=c["F1"])
    return orc.refit(c["xyz0"][:n], c["xyz1"], c["idx1"][:n], c["T"], thr2=thr2, **F)


def problems(T, n, ref, c):
    """What is wrong with (T, n) as an answer to case c: a list of strings, empty when nothing is."""
    out = []
    if n != ref["n_refit"]:
        out.append(f"{c['name']}: {n} inliers, restatement {ref['n_refit']}")
    if ref["ref"] is None:
        if not np.array_equal(T, c["T"]):
            out.append(f"{c['name']}: T must stay T_in")
    else:
        try:
            hp.check(T, ref["ref"], raw=True, where=c["name"])
        except AssertionError as e:
            out.append(str(e))
    return out


# ------------------------------------------------------------------------------------------------------------ references, computed once
def all_refit_cases():
    cases = [plain_case(n, p) for n, p in plain_specs()]
    cases += [listed_case(*s) for s in LISTED]
    cases += [weighted_case(*s) for s in WEIGHTED]
    cases += [skip_case(), boundary_case("at"), boundary_case("next64")]
    return cases


_REF = {}


def reference(case, **kw):
    """refit_cpu.refit of the case, computed once per process and shared (read-only) by every test that needs it."""
    key = (case["name"], tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = rc.refit(case["xyz0"], case["xyz1"], case["idx1"], case["T"], case["thr2"], idx0=case["idx0"], m=case["m"],
                             F0=case["F0"], F1=case["F1"], **kw)
    return _REF[key]


def pad32(F):
    return np.ascontiguousarray(np.pad(np.asarray(F, np.float32), ((0, 0), (0, 32 - F.shape[1]))))
