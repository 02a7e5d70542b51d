"""Inputs of the bit-for-bit tests of PointDSC's tail (tests/test_pdsc_solve_exact_cpu.py, tests/test_gpu_pdsc_solve_exact.py).  Builders
only, nothing is read from a file; each asserts the conditions its case rests on and returns what it measured next to the inputs.

  * lattice(): features on a lattice -- S4's similarities and S5's dot products are exact in fp32 in ANY summation order, so the reference
    of S4 is a matmul plus S4's stable order at any m, and ties are everywhere: across the k'-th place, across key chunks;
  * crafted_s2(): S2's decision boundaries at rows on both sides of the 256-row tile edges of ps_nms_kernel / ps_rank_kernel;
  * zero_feature_seed(): a live row with an all-zero feature and the largest confidence;
  * zero_matrix(), subnormal_weights(), refine_rounds(): S5 - S9 where the planted cases do not reach.
"""
import functools

import numpy as np

from tests import pdsc_solve_cases as cases
from tests import pdsc_solve_cpu as cpu

C = 128
P = cases.PARAMS
GRID = 64          # every lattice similarity is a multiple of 1 / GRID


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- lattice features --------------------------------------------------------------------------------------------------------------------
def lattice_features(inlier, seed=0):
    """float32 [m,128]: every row has 4, 16 or 64 non-zero entries of +-1 at seeded positions (norms 2, 4, 8: S3 gives +-1/2, +-1/4, +-1/8
    exactly), set in pairs of adjacent channels (2, 8 or 32 of the 64 pairs, one sign per pair: with single channels the top eight of
    8 192 rows tie across the eighth place on 86 % of the seeds only); inliers take 85 % of their signs from one seeded pattern, so that
    they are nearer to each other than to the rest; about 10 % of the rows carry a copy of another row's feature."""
    m = len(inlier)
    rng = np.random.default_rng([seed, m, 11])
    nnz = rng.choice(np.array([4, 16, 64]), m)
    rank = np.argsort(np.argsort(rng.random((m, C // 2)), axis=1), axis=1)
    sign = rng.choice(np.array([-1.0, 1.0]), (m, C // 2))
    common = rng.choice(np.array([-1.0, 1.0]), C // 2)
    sign = np.where(inlier[:, None] & (rng.random((m, C // 2)) < 0.85), common[None, :], sign)
    feat = np.repeat(np.where(rank < (nnz // 2)[:, None], sign, 0.0), 2, axis=1).astype(np.float32)
    assert np.isin(np.count_nonzero(feat, axis=1), [4, 16, 64]).all()
    dst = rng.choice(m, m // 10, replace=False)
    orig = np.setdiff1d(np.arange(m), dst)
    feat[dst] = feat[rng.choice(orig, len(dst))]
    return feat


def lattice_conditions(c, **params):
    """Asserts what a lattice case rests on; returns the measurements."""
    p = dict(P, **params)
    src, tgt, feat, conf = c["src"], c["tgt"], c["feat"], c["conf"]
    m = len(conf)
    live = cpu.live_rows(src, tgt, feat, conf)
    fn = cpu.normalize32(feat, live)
    nz = fn[fn != 0]
    assert np.isin(np.abs(nz), [0.5, 0.25, 0.125]).all()
    seeds = cpu.pick_seeds(src, conf, live, p["nms_radius"], p["ratio"])
    ns, kp = len(seeds), min(p["k"], int(live.sum()) - 1)
    assert kp < int(live.sum()) - 1
    pl = cpu.plan(ns, m)
    chunk = np.arange(m) // pl["per"]
    tie_kth, pairs, crossing = 0, 0, 0
    for lo in range(0, ns, 512):
        sd = seeds[lo:lo + 512]
        s32 = fn[sd] @ fn.T
        s = cpu.sims_exact(fn, sd).astype(np.float64)
        assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s), "a float32 matmul is not exact on these features"
        assert np.array_equal(np.rint(s * GRID), s * GRID)
        s[:, ~live] = -np.inf
        s[np.arange(len(sd)), sd] = -np.inf
        two = -np.partition(-s, (kp - 1, kp), axis=1)[:, kp - 1:kp + 1]
        tied = two[:, 0] == two[:, 1]
        tie_kth += int(tied.sum())
        group = (s == two[:, :1]) & tied[:, None]                          # the rows at the k'-th value, where it is tied across the k'-th place
        lo_c = np.where(group, chunk[None, :], m).min(1)
        hi_c = np.where(group, chunk[None, :], -1).max(1)
        crossing += int((tied & (hi_c > lo_c)).sum())
        nbr = cpu.knn_contract(s32, live, sd, p["k"], grid=GRID)
        v = np.take_along_axis(s, nbr, 1)
        assert (v[:, :-1] >= v[:, 1:]).all() and (v[:, -1] == two[:, 0]).all()
        pairs += int((v[:, :-1] == v[:, 1:]).sum())
    got = dict(n_seeds=ns, kp=kp, plan=pl, tie_kth=tie_kth / ns, tied_pairs=pairs / ns, crossing=crossing)
    assert got["tie_kth"] >= 0.9, got
    assert pl["chunks"] == 1 or crossing >= 1, got
    return got


@functools.lru_cache(maxsize=None)
def lattice(m, seed=0, ratio=None, k=None):
    """A planted case (geometry and confidence of pdsc_solve_cases) over lattice features, its conditions asserted under the parameters
    the tests run it with."""
    src, tgt, inl = cases.planted(m, seed)
    _, conf = cases.trained_like(inl, seed)
    c = dict(m=m, src=src, tgt=tgt, feat=lattice_features(inl, seed), conf=conf, inlier=inl)
    c["params"] = {k_: v for k_, v in (("ratio", ratio), ("k", k)) if v is not None}
    c["measured"] = lattice_conditions(c, **c["params"])
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def zero_feature_seed(m=700):
    """The lattice case with one live row of all-zero features and the largest confidence: the first seed, every similarity 0 (S3 divides
    by max(0, 1e-12)), its neighbours the first k' live rows other than itself by index."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in lattice(m).items()}
    z = 300
    c["feat"][z] = 0
    c["conf"][z] = c["conf"].max() + np.float32(1)
    live = cpu.live_rows(c["src"], c["tgt"], c["feat"], c["conf"])
    seeds = cpu.pick_seeds(c["src"], c["conf"], live, P["nms_radius"], P["ratio"])
    fn = cpu.normalize32(c["feat"], live)
    assert live[z] and seeds[0] == z and not fn[z].any()
    nbr = cpu.knn_contract(cpu.sims_exact(fn, seeds[:1]), live, seeds[:1], P["k"], grid=GRID)
    assert nbr[0].tolist() == list(range(P["k"])) and z > P["k"]
    c["measured"] = lattice_conditions(c)
    c["zero_row"] = z
    return _frozen(c)


# ---- S2's decision boundaries across tile edges ---------------------------------------------------------------------------------------------
CRAFTED_M = 701
CRAFTED_PARAMS = dict(ratio=1.0, k=8)          # every live row is a seed: the whole of S2's order is an output


@functools.lru_cache(maxsize=None)
def crafted_s2():
    """case(701) with crafted rows outside the box (|y| >= 100; the planted rows have |y| <= 40), each group on both sides of an edge of
    the 256-row tiles (256, 512):
      rows 255 / 256: fp32 distance exactly (float)nms_radius, neither suppresses the other;
      rows 511 / 700: one ulp closer, the lower confidence is suppressed;
      rows 254 / 513: equal confidences inside the radius, both stay -- and are equal keys across tiles;
      rows 253 > 258 > 600: a chain inside the radius, 600 is suppressed by the suppressed 258, not by 253 (0.8 away);
      row 512: a local maximum of negative confidence, which sorts behind every zero key.
    With ratio = 1 every live row is a seed, so the suppressed rows (key 0) appear in ascending index across the tiles."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cases.case(CRAFTED_M).items()}
    src, conf = c["src"], c["conf"]
    R = np.float32(P["nms_radius"])
    inside = np.nextafter(R, np.float32(0))
    top = np.float32(np.ceil(conf.max()))
    rows = {255: ((0, 100, 0), top + 1), 256: ((R, 100, 0), top + 2),
            511: ((0, 110, 0), top + 3), 700: ((inside, 110, 0), top + 4),
            254: ((0, 120, 0), top + 5), 513: ((0.25, 120, 0), top + 5),
            253: ((0, 130, 0), top + 8), 258: ((0.4, 130, 0), top + 7), 600: ((0.8, 130, 0), top + 6),
            512: ((0, 140, 0), -1.0)}
    for i, (xyz, cf) in rows.items():
        src[i] = np.array(xyz, np.float32)
        conf[i] = np.float32(cf)
    assert (np.abs(np.delete(src, list(rows), 0)[:, 1]) <= 40).all() and CRAFTED_M % 256
    assert cpu.dist32(src[[255]], src[[256]])[0] == R and cpu.dist32(src[[511]], src[[700]])[0] == inside < R
    assert cpu.dist32(src[[253]], src[[600]])[0] >= R > max(cpu.dist32(src[[253]], src[[258]])[0], cpu.dist32(src[[258]], src[[600]])[0])
    live = cpu.live_rows(src, c["tgt"], c["feat"], conf)
    key = cpu.seed_keys(conf, cpu.local_max(src, conf, live, P["nms_radius"]))
    assert [float(key[i]) for i in (255, 256, 511, 700, 254, 513, 253, 258, 600, 512)] == \
        [top + 1, top + 2, 0.0, top + 4, top + 5, top + 5, top + 8, 0.0, 0.0, -1.0]
    order = cpu.seed_order(key, live, CRAFTED_M).tolist()
    assert order[:6] == [253, 254, 513, 700, 256, 255]
    zeros = [i for i in order if key[i] == 0]
    assert zeros == sorted(zeros) and {258, 511, 600} <= set(zeros) and len({i // 256 for i in zeros}) == 3
    assert order.index(512) > order.index(zeros[-1])
    c["crafted"] = sorted(rows)
    return _frozen(c)


# ---- S5 - S9 ----------------------------------------------------------------------------------------------------------------------------------
ZERO_SIGMA_D = 1e-3


@functools.lru_cache(maxsize=None)
def zero_matrix(m=257, seed=0):
    """All outliers under sigma_d = 1e-3: every length difference inside a neighbour list is at least 1e-3 (asserted), so every M is 0,
    every weight is 0, H = 0 and every seed transform is the identity."""
    c = cases.all_outliers(m, seed)
    r = cpu.solve_contract(c["src"], c["tgt"], c["feat"], c["conf"], **dict(P, sigma_d=ZERO_SIGMA_D))
    M = cpu.matrix_chain(r["fn"], c["src"], c["tgt"], r["knn"], P["sigma"], ZERO_SIGMA_D)
    assert not M.any() and not r["weights"].any() and r["n_seeds"] > 0
    assert all(np.array_equal(T, np.eye(4)) for T in r["seed_T"])
    c["contract"] = r
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def subnormal_weights():
    """case(257) at num_iterations = 20: the power iteration drives the weights of the outliers in a list through the fp32 subnormals to
    zero.  Asserted on the chain restatement: at least one subnormal weight, and at least one weight that is zero now and was not at
    num_iterations = 10."""
    c = cases.case(257)
    r10 = cpu.solve_contract(c["src"], c["tgt"], c["feat"], c["conf"], **P)
    r20 = cpu.solve_contract(c["src"], c["tgt"], c["feat"], c["conf"], **dict(P, num_iterations=20))
    tiny = np.float32(np.finfo(np.float32).tiny)
    w10, w20 = r10["weights"], r20["weights"]
    assert np.array_equal(r10["knn"], r20["knn"])
    got = dict(subnormal=int(((w20 != 0) & (np.abs(w20) < tiny)).sum()), zeros=int((w20 == 0).sum()), new_zeros=int(((w20 == 0) & (w10 != 0)).sum()), of=w20.size)
    assert got["subnormal"] >= 1 and got["new_zeros"] >= 1, got
    c["measured"], c["contract"] = got, r20
    return _frozen(c)


REFINE_THRESHOLD = 0.25


@functools.lru_cache(maxsize=None)
def refine_rounds():
    """planted(1290, seed 3, 30 % inliers, 15 cm noise) under refine_threshold = 0.25: the inlier count keeps changing, S9 runs at least
    four fits before two counts are equal (asserted on the fp64 restatement), and stops at the cap with refine_iters = 2."""
    src, tgt, inl = cases.planted(1290, seed=3, inlier_ratio=0.3, noise=0.15)
    feat, conf = cases.trained_like(inl, 3)
    c = dict(m=1290, src=src, tgt=tgt, feat=feat, conf=conf, inlier=inl)
    r = cpu.solve(src, tgt, feat, conf, **dict(P, refine_threshold=REFINE_THRESHOLD))
    capped = cpu.solve(src, tgt, feat, conf, **dict(P, refine_threshold=REFINE_THRESHOLD, refine_iters=2))
    assert 4 <= r["refine_rounds"] < P["refine_iters"] and capped["refine_rounds"] == 2 and not np.array_equal(capped["T"], r["T"])
    c["measured"] = dict(rounds=r["refine_rounds"])
    return _frozen(c)


EMPTY = dict(m=0, src=np.zeros((0, 3), np.float32), tgt=np.zeros((0, 3), np.float32), feat=np.zeros((0, 128), np.float32), conf=np.zeros(0, np.float32))
