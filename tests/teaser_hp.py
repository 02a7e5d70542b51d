"""Generators and high-precision references for the TEASER back end (csrc/lr_teaser.hip), stage by stage.

Everything here runs on the CPU.  The contract is DESIGN.md §10 / include/lidarreg.h as restated in tests/teaser_cpu.py; this module
adds what that restatement cannot say about itself:
  1. graph     band_pairs(): correspondences whose fp64 consistency value sits within a few float32 roundings of the threshold, a
               float32 model of the device's two-level test (edge32_model, written from DESIGN §10), and a 40-digit evaluation;
  2. clique    generators that aim at one exit of the reduction each (tc.reduction_model labels them) and clustered instances that
               leave thousands of vertices to the exact search; omega_check() proves a returned clique maximum without the device;
  3. rotation  gnc_ref(): the contract's GNC-TLS loop in numpy longdouble (64-bit mantissa; mpmath is too slow for K = 4 100 times
               tens of iterations) with every 3x3 SVD and the final fit in mpmath, and the margin of every decision it takes;
  4. voting    vote_exact(): x = b - R a, the 2n endpoint costs and their order in exact integer arithmetic (stronger than 40
               digits: no rounding at all), with the error bounds of the device's one-pass cost and of its mean.
eps = 2^-52 throughout.
"""
from fractions import Fraction

import networkx as nx
import numpy as np
from mpmath import mp

from tests import rigid_hp as rh
from tests import teaser_cpu as tc

EPS = 2.0 ** -52
DPS = 40
BAND = 1e-6                # coefficient of the device's guard band: band = BAND (da + db) + BAND thr  
MARGIN = 1e-9              # relative margin below which a decision of the reference is "in the flip band"

SCALES = [(1.0, 0.0), (30.0, 0.0), (300.0, 0.0), (3000.0, 0.0), (30.0, 1000.0)]          # (half extent, cloud offset) in metres
THRESHOLDS = [(0.05, 1.0), (0.05, 0.5), (0.3, 1.0), (0.3, 0.5), (1.0, 1.0), (1.0, 0.5)]  # (noise_bound, cbar2)


def thr_of(noise_bound, cbar2):
    """The fp64 threshold the library forms: 2 beta sqrt(cbar2)."""
    return 2.0 * noise_bound * np.sqrt(cbar2)


# ------------------------------------------------------------------------------------------------------------------ 1. graph
def _len64(p, q):
    d = np.asarray(p, np.float32).astype(np.float64) - np.asarray(q, np.float32).astype(np.float64)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def d64(ai, aj, bi, bj):
    """The contract's value | |a_i - a_j| - |b_i - b_j| | in fp64 on the promoted inputs, operation order of tc.graph."""
    return np.abs(_len64(ai, aj) - _len64(bi, bj))


def edge32_model(ai, aj, bi, bj, thr, band_scale=1.0):
    """float32 model of the device's first-level test as DESIGN §10 states it: distances and their difference in float32 (one
    rounding per operation, (dx dx + dy dy) + dz dz, correctly rounded sqrt), thr32 = (float)thr, band = 1e-6 (da + db) + 1e-6 thr32.
    Returns diff32, thr32, band, plain (the decision of fp32 alone: diff32 <= thr32), inband (the pair goes to the fp64 re-test) and
    final (the two-level decision with the band scaled by band_scale; 0 = no band)."""
    f = np.float32
    ai, aj, bi, bj = (np.asarray(v, f) for v in (ai, aj, bi, bj))
    da_, db_ = ai - aj, bi - bj
    da = np.sqrt((da_[..., 0] * da_[..., 0] + da_[..., 1] * da_[..., 1]) + da_[..., 2] * da_[..., 2])
    db = np.sqrt((db_[..., 0] * db_[..., 0] + db_[..., 1] * db_[..., 1]) + db_[..., 2] * db_[..., 2])
    thr32 = f(thr)
    diff = np.abs(da - db)
    band = (f(BAND) * (da + db) + f(BAND) * thr32) * f(band_scale)
    yes, no = diff <= thr32 - band, diff > thr32 + band
    exact = d64(ai, aj, bi, bj) <= thr
    return dict(diff32=diff, thr32=thr32, band=band, da=da, db=db, plain=diff <= thr32, inband=~yes & ~no,
                final=np.where(yes, True, np.where(no, False, exact)))


_WALK = np.array([(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)], np.float32)


def band_pairs(scale, thr, n, seed, offset=0.0, rounds=6):
    """n correspondences pairs (a_i, a_j, b_i, b_j), float32 [n,3] each, whose fp64 value d lies as close to thr as float32
    coordinates allow, on either side.  a_i, a_j, b_i are uniform in offset +- scale; b_j starts on a random ray from b_i at length
    |a_i - a_j| +- thr and then walks over neighbouring float32 values (+-2 ulp per coordinate, `rounds` times), keeping the
    candidate with the smallest |d - thr|.  Candidates closer to thr than 64 eps (da + db) are not taken: there the fp64 evaluation's
    own rounding decides, which says nothing about a float32 band."""
    rng = np.random.default_rng(seed)
    f = np.float32
    ai = (rng.uniform(-scale, scale, (n, 3)) + offset).astype(f)
    aj = (rng.uniform(-scale, scale, (n, 3)) + offset).astype(f)
    bi = (rng.uniform(-scale, scale, (n, 3)) + offset).astype(f)
    da = _len64(ai, aj)
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    sign[da - thr < 0.1 * da + 1e-3] = 1.0
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    bj = (bi.astype(np.float64) + (da + sign * thr)[:, None] * u).astype(f)
    for _ in range(rounds):
        cand = bj[:, None, :] + _WALK[None, :, :] * np.spacing(np.abs(bj))[:, None, :]            # float32 neighbours
        db = _len64(bi[:, None, :], cand)
        score = np.abs(np.abs(da[:, None] - db) - thr)
        score[score <= 64 * EPS * (da[:, None] + db)] = np.inf
        bj = cand[np.arange(n), np.argmin(score, axis=1)]
    return ai, aj, bi, bj


def d_mp(ai, aj, bi, bj):
    """The same value at DPS digits: list of mpf, one per pair (the float32 inputs are exact)."""
    out = []
    with mp.workdps(DPS):
        for k in range(len(ai)):
            la = mp.sqrt(mp.fsum((mp.mpf(float(ai[k, c])) - mp.mpf(float(aj[k, c]))) ** 2 for c in range(3)))
            lb = mp.sqrt(mp.fsum((mp.mpf(float(bi[k, c])) - mp.mpf(float(bj[k, c]))) ** 2 for c in range(3)))
            out.append(abs(la - lb))
    return out


def mp_edges(ai, aj, bi, bj, thr):
    """(edge per pair at DPS digits, keep mask): pairs the 40-digit value puts within 2 fp64 ulps of thr are dropped (keep False)."""
    d = d_mp(ai, aj, bi, bj)
    with mp.workdps(DPS):
        t = mp.mpf(float(thr))
        edge = np.array([v <= t for v in d])
        keep = np.array([abs(v - t) > 2 * float(np.spacing(thr)) for v in d])
    return edge, keep


def filler(m, scale, seed, offset=0.0, special=True):
    """m ordinary correspondences at the given scale (b = a + noise of 0.3 m), the first rows replaced by the non-finite and
    coincident cases of the contract when special: NaN, +Inf, -Inf in a or b (no edge), and two coincident points."""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(-scale, scale, (m, 3)) + offset).astype(np.float32)
    b = (a + rng.normal(0, 0.3, (m, 3))).astype(np.float32)
    if special and m >= 8:
        a[0, 1] = np.nan
        b[1, 2] = np.nan
        a[2, 0] = np.inf
        b[3, 0] = -np.inf
        a[4], b[4] = (np.inf, -np.inf, np.nan), (np.nan, np.nan, np.nan)
        a[6], b[6] = a[5], b[5]                                           # coincident in both clouds
        a[7] = a[5]                                                       # coincident in a only
    return a, b


def pack(pairs, fill, lead=0):
    """One M-point problem: `lead` filler rows, then pair k as vertices (lead + 2k, lead + 2k + 1), then the rest of the filler.
    Returns (a, b, index of the first pair vertex)."""
    ai, aj, bi, bj = pairs
    n = len(ai)
    pa = np.empty((2 * n, 3), np.float32)
    pb = np.empty((2 * n, 3), np.float32)
    pa[0::2], pa[1::2], pb[0::2], pb[1::2] = ai, aj, bi, bj
    fa, fb = fill
    return np.concatenate([fa[:lead], pa, fa[lead:]]), np.concatenate([fb[:lead], pb, fb[lead:]]), lead


def band_problem(scale, offset, noise_bound, cbar2, n, seed, m_fill, lead):
    """The packed problem of one (scale, threshold) cell of the sweep: (a, b, pairs, lead)."""
    thr = thr_of(noise_bound, cbar2)
    pairs = band_pairs(scale, thr, n, seed, offset)
    a, b, lead = pack(pairs, filler(m_fill, scale, seed + 1, offset), lead)
    return a, b, pairs, lead


# ------------------------------------------------------------------------------------------------------------------ 2. clique
def is_clique(A, c):
    c = np.asarray(c, np.int64)
    return bool(np.all(A[np.ix_(c, c)] | np.eye(len(c), dtype=bool)))


def omega_check(A, c, planted=0, nx_vertices=400):
    """Proof that the ascending clique c is maximum in the graph A, independent of the device: it is a clique of size K >= planted,
    and no clique of K + 1 vertices exists -- each of its vertices would have degree >= K, so it would lie in the K-core, and the
    maximum clique of that core (networkx, exact) is smaller than K + 1.  A core of more than nx_vertices vertices is beyond what
    networkx finishes in a minute; there clique_exceeds() (a CPU branch and bound, checked against networkx in the CPU tests) gives
    the same proof.  Returns the size of that core."""
    c = np.asarray(c, np.int64)
    K = len(c)
    assert np.all(np.diff(c) > 0), "clique not strictly ascending"
    assert is_clique(A, c), "not a clique under tc.graph"
    assert K >= planted, (K, planted)
    core = _k_core_mask(A, K)
    n = int(core.sum())
    idx = np.nonzero(core)[0]
    if n > nx_vertices:
        assert not clique_exceeds(A[np.ix_(idx, idx)], K), f"a clique of more than {K} vertices exists"
    elif n:
        w = len(nx.max_weight_clique(tc.to_nx(A[np.ix_(idx, idx)]), None)[0])
        assert w <= K, f"a clique of {w} > {K} vertices exists"
    return n


def clique_exceeds(A, K):
    """True iff the boolean adjacency A holds a clique of more than K vertices.  A plain branch and bound of its own (Tomita's
    greedy-colouring bound, vertices by descending degree, bitsets as Python integers): for graphs too large for networkx."""
    n = A.shape[0]
    order = np.argsort(-A.sum(1), kind="stable")
    B = A[np.ix_(order, order)]
    adj = [int.from_bytes(np.packbits(B[i], bitorder="little").tobytes(), "little") for i in range(n)]

    def colour(P):
        out, k = [], 0
        while P:
            k += 1
            Q = P
            while Q:
                v = (Q & -Q).bit_length() - 1
                Q &= ~adj[v] & ~(1 << v)
                P &= ~(1 << v)
                out.append((v, k))
        return out

    def expand(P, size):
        for v, k in reversed(colour(P)):
            if size + k <= K:
                return False
            if size + 1 > K:
                return True
            Pn = P & adj[v]
            if Pn and expand(Pn, size + 1):
                return True
            P &= ~(1 << v)
        return False

    return expand((1 << n) - 1, 0)


def _k_core_mask(A, k):
    """Vertices of the k-core of the boolean adjacency A (iterated removal of degree < k), numpy."""
    alive = np.ones(A.shape[0], bool)
    deg = A.sum(1).astype(np.int64)
    while True:
        drop = alive & (deg < k)
        if not drop.any():
            return alive
        alive &= ~drop
        deg -= A[:, drop].sum(1)


def random_planted(seed, m, noise=0.35, outlier_scale=3.0):
    """Planted set whose noise exceeds beta: the planted points are not a clique themselves, the search has work to do."""
    rng = np.random.default_rng(seed)
    n_in = int(rng.integers(5, max(6, m // 3)))
    return tc.planted(m, n_in, seed, noise=noise, outlier_scale=outlier_scale)[:2]


def clusters(sizes, n_out, seed, extent=30.0, noise=0.05):
    """J disjoint rigid clusters (cluster j: sizes[j] points spread over the whole extent, its own random motion, per-axis noise
    +-noise so that it is an exact clique for beta >= sqrt(3) noise) plus n_out uniformly random outliers, shuffled.
    Returns (a, b, labels) with label -1 for outliers; omega >= max(sizes) by construction."""
    rng = np.random.default_rng(seed)
    A, B, lab = [], [], []
    for j, s in enumerate(sizes):
        R = rh.random_rot(rng)
        t = rng.uniform(-5, 5, 3)
        p = rng.uniform(-extent, extent, (s, 3))
        A.append(p)
        B.append(p @ R.T + t + rng.uniform(-noise, noise, (s, 3)))
        lab += [j] * s
    A.append(rng.uniform(-extent, extent, (n_out, 3)))
    B.append(rng.uniform(-extent, extent, (n_out, 3)))
    lab += [-1] * n_out
    a, b, lab = np.concatenate(A), np.concatenate(B), np.array(lab)
    perm = rng.permutation(len(a))
    return a[perm].astype(np.float32), b[perm].astype(np.float32), lab[perm]


def two_motions(n1, n2, n_out, seed, angle=0.02, extent=20.0, noise=0.02):
    """Two motions that differ by a rotation of `angle` rad about the z axis through the origin: a point at distance rho from the
    axis moves by rho * angle between them, so points with rho * angle well under beta are consistent with both sets.  Near-maximum
    cliques that share vertices.  Returns (a, b)."""
    rng = np.random.default_rng(seed)
    R1 = rh.random_rot(rng)
    R2 = R1 @ rh.rot(np.array([0.0, 0.0, 1.0]), angle)
    t = rng.uniform(-5, 5, 3)
    p1 = rng.uniform(-extent, extent, (n1, 3))
    p2 = rng.uniform(-extent, extent, (n2, 3))
    po = rng.uniform(-extent, extent, (n_out, 3))
    a = np.concatenate([p1, p2, po])
    b = np.concatenate([p1 @ R1.T + t + rng.uniform(-noise, noise, (n1, 3)), p2 @ R2.T + t + rng.uniform(-noise, noise, (n2, 3)),
                        rng.uniform(-extent, extent, (n_out, 3))])
    perm = rng.permutation(len(a))
    return a[perm].astype(np.float32), b[perm].astype(np.float32)


EXIT_CASES = [  # (seed, m, noise, outlier_scale) -> (exit, search improves on LB?)
    ((2, 98, 0.35, 3.0), "empty_incumbent", None),
    ((5, 209, 0.35, 3.0), "search", False),
    ((9, 157, 0.35, 3.0), "search", False),
    ((3, 135, 0.35, 3.0), "search", True),
    ((1, 61, 0.35, 3.0), "search", True),
]


# ------------------------------------------------------------------------------------------------------------------ 3. rotation
def slab(n_in, n_out, seed, beta=0.3, bad=0.0, extent=50.0, offset=0.0, lift=1.1, noise=0.01):
    """Planted set for the rotation and voting stages.  The inliers lie in a slab (normal = the cloud's z axis, half thickness
    0.25 m, half extent `extent`), move rigidly and get per-axis noise +-noise.  A share `bad` of them is lifted along the moved
    normal by +-lift * beta (random sign): lengths change only in second order, so the lifted points stay in the clique, but a chain
    TIM between a point lifted up and one lifted down is 2 lift beta > 2 beta off -- a rotation outlier inside the clique.  With
    bad = 1 about half of the TIMs are outliers and the ballot compaction writes a strict subset in every chunk.
    Returns (a, b, T_gt, inlier mask)."""
    rng = np.random.default_rng(seed)
    m = n_in + n_out
    p = np.column_stack([rng.uniform(-extent, extent, n_in), rng.uniform(-extent, extent, n_in), rng.uniform(-0.25, 0.25, n_in)])
    R = rh.random_rot(rng)
    t = rng.uniform(-5, 5, 3)
    lifted = rng.random(n_in) < bad
    sgn = np.where(rng.random(n_in) < 0.5, 1.0, -1.0) * lifted
    e = rng.uniform(-noise, noise, (n_in, 3))
    e[:, 2] += sgn * lift * beta
    off = np.full(3, float(offset))
    tw = t + off - R @ off                                              # the same motion in world-frame coordinates
    a = np.concatenate([p + off, rng.uniform(-extent, extent, (n_out, 3)) + off])
    b = np.concatenate([(p + off + e) @ R.T + tw, rng.uniform(-extent, extent, (n_out, 3)) + off])
    perm = rng.permutation(m)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, tw
    mask = (np.arange(m) < n_in)[perm]
    return a[perm].astype(np.float32), b[perm].astype(np.float32), T, mask


MIRROR_H = 338.0 / 1024.0          # the lift of mirror_loop: 1.1 beta for beta = 0.3, a multiple of 2^-10


def mirror_loop(n, seed):
    """n (a multiple of 4) correspondences whose voting on the z axis has two mathematically equal minima, for beta = 0.3 and
    cbar2 = 1.44.  The a-points form a closed planar polygon (z = 0, every coordinate a multiple of 2^-10), b = a + t + (0, 0, +-h) with
    the signs + + - - ... and h = MIRROR_H: the two groups are 2h = 2.2 beta apart, too far for one voting window, close enough for
    every chain TIM to be a rotation inlier (TIM bound 2.4 beta).  The TIMs that cross from + to - are a permutation of those that
    cross back, so sum w delta A = 0 whatever weight GNC gives the crossing TIMs and R = I is the optimum of every fit; x = b - R a
    is then t +- h up to the rounding of R.  Returns (a, b, T_gt)."""
    assert n % 4 == 0
    rng = np.random.default_rng(seed)
    q = 2.0 ** -10
    m = n // 4
    v = np.round(rng.uniform(-4, 4, (m, 2)) / q) * q                  # + to - crossings; the - to + crossings are v rolled by one
    u = np.round(rng.uniform(-4, 4, (2 * m, 2)) / q) * q              # TIMs inside a group
    u[-1] -= u.sum(0) + 2 * v.sum(0)                                  # close the polygon
    steps = np.empty((n, 2))
    steps[0::4], steps[1::4], steps[2::4], steps[3::4] = u[0::2], v, u[1::2], np.roll(v, 1, 0)
    p = np.zeros((n, 3))
    p[1:, :2] = np.cumsum(steps[:-1], 0)
    sgn = np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0)
    t = np.array([3.0, -2.0, 1.0])
    b = p + t
    b[:, 2] += sgn * MIRROR_H
    T = np.eye(4)
    T[:3, 3] = t
    a32, b32 = p.astype(np.float32), b.astype(np.float32)
    assert np.array_equal(a32, p) and np.array_equal(b32, b)          # exactly representable
    return a32, b32, T


ROT_ROWS = {  # name -> (K list, generator kw, solver kw)
    "default": ([3, 4, 63, 64, 65, 255, 256, 257, 511, 1023, 1025, 4100], dict(noise=0.15), dict()),
    "lifted": ([64, 65, 257, 511, 1025, 4100], dict(bad=1.0), dict()),
    "offset": ([65, 257, 1025], dict(bad=1.0, offset=1000.0), dict()),
    "cap1": ([65, 257, 1025], dict(bad=1.0), dict(max_iterations=1)),
    "cap3": ([65, 257, 1025], dict(bad=1.0), dict(max_iterations=3)),
    "factor1.1": ([65, 257], dict(bad=1.0), dict(gnc_factor=1.1)),
    "factor2": ([65, 257, 1025], dict(bad=1.0), dict(gnc_factor=2.0)),
    "cost1e-6": ([65, 257, 1025], dict(bad=1.0), dict(cost_threshold=1e-6)),
    "beta0.05": ([65, 257, 1025], dict(bad=1.0, beta=0.05, noise=0.002), dict(noise_bound=0.05)),
    "beta1_cbar0.5": ([65, 257, 1025], dict(bad=1.0, beta=0.7, noise=0.02), dict(noise_bound=1.0, cbar2=0.5)),
    "no_start": ([65, 257], dict(noise=0.001), dict()),
}


def rot_case(row, K):
    _, gkw, skw = ROT_ROWS[row]
    a, b, T, mask = slab(K, K + 6, 7000 + K, **gkw)
    return a, b, T, mask, skw


ROT_CASES = [(row, K) for row in ROT_ROWS for K in ROT_ROWS[row][0]]


def _svd_rot_mp(H):
    """R = V diag(1,1,det(V U^T)) U^T of the 3x3 H (numpy longdouble or float64) at DPS digits; returns (R longdouble, R mp)."""
    with mp.workdps(DPS):
        Hm = mp.matrix([[mp.mpf(float(np.float64(H[i, j]))) + mp.mpf(float(H[i, j] - np.longdouble(np.float64(H[i, j])))) for j in range(3)]
                        for i in range(3)])
        U, S, Vt = mp.svd_r(Hm)
        V = Vt.T
        d = 1 if rh._det3(V * U.T) >= 0 else -1
        R = V * mp.diag([1, 1, d]) * U.T
        Rl = np.array([[np.longdouble(float(R[i, j])) + np.longdouble(float(R[i, j] - mp.mpf(float(R[i, j])))) for j in range(3)]
                       for i in range(3)], np.longdouble)
        return Rl, R


def gnc_ref(a, b, clique, noise_bound=0.3, cbar2=1.0, gnc_factor=1.4, max_iterations=10000, cost_threshold=1e-16, **_):
    """The contract's GNC-TLS loop (tc.rotation, include/lidarreg.h) with K-sized arrays in numpy longdouble and every 3x3 SVD in
    mpmath.  Returns a dict:
      R (fp64), Rmp, w (final weights), inliers (w >= 0.5), iters, fit (rigid_hp.fit of the weights the returned R was fitted to:
      kappa_raw and the 40-digit optimum), and the margins of the decisions that fix the outcome:
        m_weight  min |w - 0.5| / 0.5 over the final weights,
        m_start   | 2 max r / nb2 - 1 | (the sign of mu decides whether GNC starts),
        m_stop    min over the stopping tests of | |cost - prev| - cost_threshold | / (cost_threshold + 64 K eps cost): 64 K eps cost
                  bounds what the fp64 sums of K terms can move the cost by, so below 1 the device may stop an iteration apart
                  (a test between two fits of the same 0/1 weights is exempt: both sides are the same bits).
      A threshold crossing inside the loop (r against th1 or th2) needs no margin: the weight is continuous there (0 at th1, 1 at
      th2), a flip moves it by rounding only."""
    L = np.longdouble
    a, b = np.asarray(a, np.float32).astype(L), np.asarray(b, np.float32).astype(L)
    c = np.asarray(clique)
    K = len(c)
    A, B = a[np.roll(c, -1)] - a[c], b[np.roll(c, -1)] - b[c]
    nb2 = L((2.0 * noise_bound) * (2.0 * noise_bound) * cbar2)
    w = np.ones(K, L)
    w_fit = w_prev = w.copy()
    R, _ = _svd_rot_mp((A * w[:, None]).T @ B)
    res = lambda R: np.sum((B - A @ R.T) ** 2, 1)
    r = res(R)
    x = 2 * r.max() / nb2 - 1
    out = dict(m_start=float(abs(x)), m_stop=np.inf, iters=0)
    mu = 1 / x if x != 0 else L(np.inf)
    if mu > 0:
        prev = L(0)
        for it in range(1, max_iterations + 1):
            r = res(R)
            th1, th2 = (mu + 1) / mu * nb2, mu / (mu + 1) * nb2
            cost = np.sum(w * r)
            with np.errstate(divide="ignore", invalid="ignore"):
                mid = np.sqrt(nb2 * mu * (mu + 1) / np.where(r > 0, r, 1)) - mu
            w = np.where(r >= th1, L(0), np.where(r <= th2, L(1), mid))
            mu = mu * L(gnc_factor)
            out["iters"] = it
            d = abs(cost - prev)
            # the same binary weights twice: the same H, R, residuals and cost to the last bit on any machine, the difference is 0
            settled = it > 1 and np.array_equal(w_fit, w_prev) and np.all((w_fit == 0) | (w_fit == 1))
            if not settled:
                out["m_stop"] = min(out["m_stop"], float(abs(d - cost_threshold) / (cost_threshold + 64 * K * EPS * cost)))
            if d < cost_threshold:
                break
            prev = cost
            w_prev = w_fit
            w_fit = w.copy()
            R, _ = _svd_rot_mp((A * w[:, None]).T @ B)
    inl = (w >= 0.5) if mu > 0 else np.ones(K, bool)
    fit = rh.fit(A.astype(np.float64), B.astype(np.float64), w_fit.astype(np.float64), centred=False)
    out.update(R=fit["R"], Rmp=fit["Rmp"], w=w.astype(np.float64), inliers=inl, n_rot=int(inl.sum()), fit=fit, started=bool(mu > 0),
               m_weight=float(np.min(np.abs(w - 0.5)) / 0.5) if mu > 0 else np.inf, K=K)
    return out


def gnc_in_band(ref, max_iterations):
    """True when a decision of the reference run is closer than MARGIN to flipping (a stop test that the iteration cap overrides
    does not count)."""
    stop = ref["m_stop"] < 1.0 + MARGIN and ref["iters"] < max_iterations
    return bool(ref["m_weight"] < MARGIN or ref["m_start"] < MARGIN or stop)


# ------------------------------------------------------------------------------------------------------------------ 4. voting
_SX = 1400                 # common binary scale: every fp64 R entry (down to 2^-1074) times a float32 (down to 2^-149) is an integer


def _int(v, s):
    fr = Fraction(float(v)) * (1 << s)
    assert fr.denominator == 1
    return fr.numerator


def x_exact(a, b, R, pts):
    """x = b - R a of the points `pts` as exact integers scaled by 2^_SX: [n][3] Python ints.  R: the device's fp64 rotation."""
    Ri = [[_int(R[i, j], _SX - 200) for j in range(3)] for i in range(3)]
    out = []
    for p in pts:
        ai = [_int(a[p, j], 200) for j in range(3)]
        out.append([_int(b[p, i], _SX) - sum(Ri[i][j] * ai[j] for j in range(3)) for i in range(3)])
    return out


def vote_exact(X, beta):
    """Adaptive voting on one axis in exact arithmetic.  X: n integers (x scaled by 2^_SX).  Endpoints ordered by (value, entry before
    exit, index); after each one the cost sum_in (x - mean)^2 + beta |out| of the consensus set, two-pass in exact rationals.
    Returns a list over the endpoints in key order of dicts(key=(value int, type, index), cnt, cost (float, correctly rounded),
    cost_q (Fraction), mean_q (Fraction, in metres), pos); entries with an empty set are left out."""
    n = len(X)
    B = _int(beta, _SX)
    Q = 1 << _SX
    ends = sorted([(X[i] - B, 0, i) for i in range(n)] + [(X[i] + B, 1, i) for i in range(n)])
    cnt = s1 = s2 = 0
    out = []
    for pos, (v, t, i) in enumerate(ends):
        if t == 0:
            cnt += 1; s1 += X[i]; s2 += X[i] * X[i]
        else:
            cnt -= 1; s1 -= X[i]; s2 -= X[i] * X[i]
        if cnt == 0:
            continue
        cost_q = Fraction(s2 * cnt - s1 * s1, cnt * Q * Q) + Fraction(B * (n - cnt), Q)
        out.append(dict(key=(v, t, i), cnt=cnt, cost=float(cost_q), cost_q=cost_q, mean_q=Fraction(s1, cnt * Q), pos=pos))
    return out


def x_error(a, b, pts):
    """Bound on the device's rounding in x = b - ((R0 ax + R1 ay) + R2 az): three products, two sums and one difference, each within
    eps/2 relative, |R_ij| <= 1: 4 eps (|b| + |ax| + |ay| + |az|) (first order, with room)."""
    a, b = np.asarray(a, np.float64)[pts], np.asarray(b, np.float64)[pts]
    return 4 * EPS * float((np.abs(b).max(1) + np.abs(a).sum(1)).max())


def cost_error(cnt, beta, ex):
    """Bound on the device's one-pass cost s2 - s1^2 / cnt with d = x - v, |d| <= 2 beta: each of the cnt-term sums is within
    cnt eps of its absolute sum (s2 <= 4 beta^2 cnt, s1^2 / cnt <= 4 beta^2 cnt), the square, quotient and difference add 4 eps, and an
    error ex in every x moves the cost by at most 2 sum |d| ex <= 4 beta cnt ex."""
    return 8 * beta * beta * cnt * (cnt + 4) * EPS + 4 * beta * cnt * ex


def mean_error(cnt, xmax, ex):
    """Bound on the device's translation estimate given its own R: the mean of cnt doubles in [-xmax, xmax], summed in any order
    (worst case (cnt - 1) eps sum |x| / cnt <= cnt eps xmax), plus the error ex of the x themselves and the final division."""
    return cnt * EPS * xmax + ex + EPS * xmax
