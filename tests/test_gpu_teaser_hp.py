"""lr_teaser / lr_teaser_batch on the MI355X at the sizes its kernels tile and at its decision boundaries, against the
high-precision references of tests/teaser_hp.py.  Every case asserts the path it was built for."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import rigid_hp as rh
from tests import teaser_cpu as tc
from tests import teaser_hp as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    from lidarregistration_amd import _ext, teaser
    _ext.build()
    assert torch.cuda.is_available()
    return teaser


def _adjacency(sets, k, **kw):
    """lr_teaser_batch over `sets`, then pair k's graph read back from byte 256 of its arena (include/lidarreg.h)."""
    import torch
    from lidarregistration_amd import _ext
    n = len(sets)
    A = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a, _ in sets]
    B = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for _, b in sets]
    ms = [len(a) for a, _ in sets]
    per = _ext.lib().lr_teaser_scratch_bytes(max(ms))
    scratch = torch.full((per * n,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.zeros(176 * n, dtype=torch.uint8, device="cuda")
    p = _ext.TeaserParams(node_budget=1, **kw)                    # the graph is what is read: the later stages are cut short
    V = ctypes.c_void_p * n
    _ext.check(_ext.lib().lr_teaser_batch(n, V(*[t.data_ptr() for t in A]), V(*[t.data_ptr() for t in B]), (ctypes.c_int32 * n)(*ms), None,
                                           ctypes.byref(p), res.data_ptr(), None, scratch.data_ptr(), scratch.numel(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    m, W = ms[k], (max(ms) + 63) // 64
    words = scratch[k * per + 256:k * per + 256 + m * W * 8].cpu().numpy().view(np.uint64).reshape(m, W)
    bits = np.unpackbits(words.view(np.uint8).reshape(m, W, 8)[:, :, ::-1], axis=2, bitorder="big")
    bits = bits.reshape(m, W, 64)[:, :, ::-1].reshape(m, W * 64)
    return bits[:, :m].astype(bool)


# ------------------------------------------------------------------------------------------------------------------ 1. graph
@pytest.mark.parametrize("scale,offset", hp.SCALES)
@pytest.mark.parametrize("nb,cb", hp.THRESHOLDS)
def test_band_adjacency_bit_identical(T, scale, offset, nb, cb):
    k = hp.THRESHOLDS.index((nb, cb))
    big = (nb, cb) == (0.3, 1.0)                                  # one cell per scale at 4 097 + pairs: rows past 64 x 64, chunks past 4
    a, b, P, lead = hp.band_problem(scale, offset, nb, cb, 256, 1000 + k, 4097 if big else 333, 1)
    ref = tc.graph(a, b, nb, cb)
    e = hp.d64(*P) <= hp.thr_of(nb, cb)
    i = lead + 2 * np.arange(256)
    assert np.array_equal(ref[i, i + 1], e)
    G = _adjacency([(a, b)], 0, noise_bound=nb, cbar2=cb)
    wrong = np.argwhere(G != ref)
    assert len(wrong) == 0, f"{len(wrong)} adjacency bits differ from fp64, first {wrong[:4].tolist()}"
    if not big:
        # the same pair as pair 2 of a ragged batch whose widest pair sets the row stride
        rng = np.random.default_rng(k)
        other = [(rng.uniform(-5, 5, (m, 3)).astype(np.float32), rng.uniform(-5, 5, (m, 3)).astype(np.float32)) for m in (1500, 70)]
        G2 = _adjacency([other[0], other[1], (a, b)], 2, noise_bound=nb, cbar2=cb)
        assert np.array_equal(G2, ref)


# ------------------------------------------------------------------------------------------------------------------ 2. clique
def _same_everywhere(T, a, b, first, **kw):
    """Determinism: the same call again, and as pair 0 and pair 5 of a batch, returns the identical result."""
    again = T.teaser_dev(a, b, **kw)
    assert np.array_equal(again[0], first[0]) and again[1] == first[1] and np.array_equal(again[2], first[2])
    small = [hp.random_planted(40 + s, 50)[:2] for s in range(4)]
    out, _ = T.teaser_batch_dev([a] + [s[0] for s in small] + [a], [b] + [s[1] for s in small] + [b], **kw)
    for k in (0, 5):
        assert np.array_equal(out[k][0], first[0]) and out[k][1] == first[1] and np.array_equal(out[k][2], first[2]), k


@pytest.mark.parametrize("case,label,improves", hp.EXIT_CASES)
def test_peel_exits(T, case, label, improves):
    a, b = hp.random_planted(*case)
    A = tc.graph(a, b)
    mc, lb, nu, nr, ex = tc.reduction_model(A, 1.0)
    assert ex == label
    first = T.teaser_dev(a, b, kcore_threshold=1.0)
    _, info, c = first
    assert info["max_core"] == mc and info["lb"] == lb and info["exact"] == 1 and info["K"] == len(c)
    hp.omega_check(A, c)
    if label == "empty_incumbent":
        assert info["nodes"] == 0 and info["K"] == lb
    else:
        assert (info["K"] > lb) == improves
        assert info["nodes"] > 0                            # the search branched: on these seeds the root bound does not close it
    _same_everywhere(T, a, b, first, kcore_threshold=1.0)


def test_shortcut_boundary(T):
    a, b, _, _ = tc.planted(128, 70, 3, noise=0.02)
    A = tc.graph(a, b)
    mc = tc.reduction_model(A, 1.0)[0]
    import networkx as nx
    core = nx.core_number(tc.to_nx(A))
    top = sorted(v for v, k in core.items() if k == mc)
    _, hit, c = T.teaser_dev(a, b, kcore_threshold=(mc - 1) / 128.0)          # just hit
    assert hit["lb"] == 0 and hit["max_core"] == mc and hit["nodes"] == 0 and list(c) == top
    _, miss, c2 = T.teaser_dev(a, b, kcore_threshold=mc / 128.0)              # max_core == kcore_threshold * M: strict >, missed
    m2 = tc.reduction_model(A, mc / 128.0)
    assert m2[4] != "shortcut" and miss["lb"] == m2[1] > 0 and miss["max_core"] == mc
    hp.omega_check(A, c2, planted=70)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_overlapping_motions(T, seed):
    a, b = hp.two_motions(60, 57, 180, seed)
    A = tc.graph(a, b)
    first = T.teaser_dev(a, b, kcore_threshold=1.0)
    _, info, c = first
    m = tc.reduction_model(A, 1.0)
    assert info["max_core"] == m[0] and info["lb"] == m[1] and info["exact"] == 1
    hp.omega_check(A, c, planted=60)
    _same_everywhere(T, a, b, first, kcore_threshold=1.0)


WIDE = dict(sizes=list(range(100, 140)), n_out=600, seed=5, noise=0.3)      # per-axis noise at beta: the clusters are no exact cliques


@pytest.fixture(scope="module")
def wide():
    a, b, lab = hp.clusters(**WIDE)
    A = tc.graph(a, b)
    return a, b, A, tc.reduction_model(A, 0.5)


def test_search_wide_bitsets_exact(T, wide):
    """More than 4 096 vertices reach the search, which branches and improves on the greedy bound: words 2..8 of a lane's bitsets
    hold live candidates while it runs.  The maximum is proved on the CPU (the K-core is almost the whole graph: clique_exceeds)."""
    a, b, A, (mc, lb, nu, nr, ex) = wide
    assert ex == "search" and nr > 4096 and lb - nu > 0
    first = T.teaser_dev(a, b)
    _, info, c = first
    print(f"M {len(a)} max_core {mc} LB {lb} nU {nu} nR {nr}: K {info['K']} nodes {info['nodes']} exact {info['exact']}")
    assert info["max_core"] == mc and info["lb"] == lb
    assert info["exact"] == 1 and info["nodes"] > 0 and info["K"] == len(c) > lb
    assert hp.omega_check(A, c) > 4096
    _same_everywhere(T, a, b, first)


def test_search_wide_bitsets_budget_cut(T, wide):
    """The WEAKER, budget-cut form of the same instance: stopped after 50 branch nodes, the result is a valid clique no smaller than
    the greedy bound, reported as inexact."""
    a, b, A, (mc, lb, nu, nr, ex) = wide
    _, info, c = T.teaser_dev(a, b, node_budget=50)
    assert info["max_core"] == mc and info["lb"] == lb
    assert info["exact"] == 0 and info["nodes"] == 50
    assert hp.is_clique(A, c) and np.all(np.diff(c) > 0) and info["K"] == len(c) >= lb


def test_index_arithmetic_above_16384(T):
    a, b, lab = hp.clusters([9000], 8000, 9, extent=100.0)          # 17 000 correspondences: the k-core shortcut fires
    _, info, c = T.teaser_dev(a, b)
    assert info["lb"] == 0 and info["exact"] == 1 and info["max_core"] >= 8999 and info["K"] == len(c) >= 9000
    assert np.all(np.diff(c) > 0) and set(np.nonzero(lab == 0)[0]) <= set(c.tolist())
    sub = c[:: max(1, len(c) // 1500)]                                   # a sample of the members is mutually consistent
    assert hp.is_clique(tc.graph(a[sub], b[sub]), np.arange(len(sub)))


# ------------------------------------------------------------------------------------------------------------------ 3. + 4.
def _check_rot_vote(T, a, b, K_planted, skw, row):
    """One case against both references.  Returns (T, info, clique, facts) with facts = dict(angle = angle / (32 eps kappa),
    t = worst |t - mean| / bound over the axes, accepted = per axis the endpoints within the cost error of the minimum)."""
    Tg, info, c = T.teaser_dev(a, b, **skw)
    K = info["K"]
    assert K_planted - max(2, K_planted // 50) <= K <= K_planted + 6, (K, K_planted)     # the size this case was built to tile
    ref = hp.gnc_ref(a, b, c, **skw)
    cap = skw.get("max_iterations", 10000)
    assert not hp.gnc_in_band(ref, cap), f"{row} K {K}: reference decision in the flip band, pick another seed"
    assert info["gnc_iters"] == ref["iters"] and info["n_rot_inliers"] == ref["n_rot"] and info["status"] == 0, (info, ref["iters"], ref["n_rot"])
    if row == "no_start":
        assert info["gnc_iters"] == 0 and info["n_rot_inliers"] == K
    if row in ("cap1", "cap3"):
        assert info["gnc_iters"] == cap
    if row not in ("default", "no_start", "mirror") and K >= 64:
        assert info["n_rot_inliers"] < 0.85 * K                       # the compaction writes a strict subset
    # R: the bound of rigid_hp (raw moments)
    R = Tg[:3, :3]
    kap = ref["fit"]["kappa_raw"]
    assert kap * hp.EPS < 1e-3
    ang = rh.angle(R, ref["fit"])
    assert ang <= 32 * hp.EPS * kap, f"{row} K {K}: angle {ang:.3e} > 32 eps kappa {32 * hp.EPS * kap:.3e}"
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12
    facts = dict(angle=ang / (32 * hp.EPS * kap), t=0.0, accepted=[])
    # voting in exact arithmetic on the device's own R
    beta = skw.get("noise_bound", 0.3)
    pts = c[ref["inliers"]]
    X = hp.x_exact(a, b, R, pts)
    ex = hp.x_error(a, b, pts)
    n_trans = np.ones(len(pts), bool)
    for axis in range(3):
        xs = [v[axis] for v in X]
        ends = hp.vote_exact(xs, beta)
        cmin = min(e["cost_q"] for e in ends)
        ok = [e for e in ends if float(e["cost_q"] - cmin) <= 2 * hp.cost_error(e["cnt"], beta, ex)]
        facts["accepted"].append(ok)
        xmax = max(abs(float(Fraction(v, 1 << hp._SX))) for v in xs)
        dev_t = Tg[axis, 3]
        ratios = [abs(float(Fraction(dev_t) - e["mean_q"])) / hp.mean_error(e["cnt"], xmax, ex) for e in ok]
        assert min(ratios) <= 1.0, f"{row} K {K} axis {axis}: t {dev_t!r} is the mean of no endpoint within the cost error of the minimum ({len(ok)} accepted, best ratio {min(ratios):.2f})"
        facts["t"] = max(facts["t"], min(ratios))
        xf = np.array([float(Fraction(v, 1 << hp._SX)) for v in xs])
        margin = np.abs(np.abs(xf - dev_t) - beta)
        assert margin.min() > hp.MARGIN * beta, f"{row} K {K}: translation-inlier decision in the flip band, pick another seed"
        n_trans &= np.abs(xf - dev_t) <= beta
    assert info["n_trans_inliers"] == int(n_trans.sum())
    print(f"{row} K {K}: gnc {info['gnc_iters']} n_rot {info['n_rot_inliers']} angle / (32 eps kappa) {facts['angle']:.3f}, |t - mean| / bound {facts['t']:.3f}")
    return Tg, info, c, facts


@pytest.mark.parametrize("row,K", hp.ROT_CASES)
def test_rotation_translation_tiles(T, row, K):
    a, b, Tgt, mask, skw = hp.rot_case(row, K)
    Tg, info, c, _ = _check_rot_vote(T, a, b, K, skw, row)
    if K >= 63 and row not in ("cap1", "cap3"):
        from lidarregistration_amd import metrics
        assert metrics.rotation_error_deg(Tg, Tgt) < 1.0


def test_vote_mirror_tie(T):
    """Two mathematically equal minima on the z axis (hp.mirror_loop): the rounding of R breaks the tie, the device may take either
    group's mean and nothing else.  Asserted to have been reached: both minima are within the cost error of each other."""
    a, b, Tgt = hp.mirror_loop(512, 11)
    Tg, info, c, facts = _check_rot_vote(T, a, b, 512, dict(noise_bound=0.3, cbar2=1.44), "mirror")
    assert info["K"] == 512 and info["n_rot_inliers"] == 512 and info["gnc_iters"] > 0
    ok = facts["accepted"][2]
    means = sorted(float(e["mean_q"]) for e in ok)
    assert len(ok) >= 2 and means[-1] - means[0] > 2 * hp.MIRROR_H - 1e-9, "the tie was not reached"
    assert abs(abs(Tg[2, 3] - Tgt[2, 3]) - hp.MIRROR_H) < 1e-9              # one of the two groups, not their middle


def test_batch_equals_single_mixed_K(T):
    cases = [hp.rot_case("lifted", 4100), hp.rot_case("default", 3), hp.rot_case("lifted", 257), hp.rot_case("default", 1023),
             hp.rot_case("lifted", 64), hp.rot_case("default", 256)]
    out, _ = T.teaser_batch_dev([c[0] for c in cases], [c[1] for c in cases])
    for k, cs in enumerate(cases):
        Ts, info, c = T.teaser_dev(cs[0], cs[1])
        assert np.array_equal(out[k][0], Ts) and out[k][1] == info and np.array_equal(out[k][2], c), k
