"""CPU tests of tests/teaser_hp.py: the adversarial generators reach what they aim at, and the references agree with each other,
before any GPU is involved."""
from fractions import Fraction

import numpy as np
import pytest

from tests import teaser_cpu as tc
from tests import teaser_hp as hp

N_PAIRS = 256              # per (scale, threshold) cell
# per scale: pairs (of 6 x 256) where the float32 decision alone differs from fp64, as measured at the committed seeds
MIN_DISAGREE = {(1.0, 0.0): 700, (30.0, 0.0): 750, (300.0, 0.0): 700, (3000.0, 0.0): 700, (30.0, 1000.0): 500}


def _cells(scale, offset):
    for k, (nb, cb) in enumerate(hp.THRESHOLDS):
        thr = hp.thr_of(nb, cb)
        yield thr, hp.band_pairs(scale, thr, N_PAIRS, 1000 + k, offset)


@pytest.mark.parametrize("scale,offset", hp.SCALES)
def test_band_pairs_have_teeth(scale, offset):
    disagree, worst, total, dropped = 0, 0.0, 0, 0
    caught = {s: 0 for s in (0.0, 1 / 32, 1 / 16, 1 / 8, 1 / 4, 1 / 2)}
    for thr, P in _cells(scale, offset):
        mdl = hp.edge32_model(*P, thr)
        d = hp.d64(*P)
        e64 = d <= thr
        # (c) every pair takes the fp64 re-test on the device
        assert mdl["inband"].all()
        assert np.array_equal(mdl["final"], e64)
        # within a few float32 roundings of the distances from thr, on both sides
        assert np.all(np.abs(d - thr) <= 4 * np.spacing(np.float32(1.0)) * (mdl["da"] + mdl["db"]))
        assert 0.2 < e64.mean() < 0.8
        # fp64 (the contract) against 40 digits
        em, keep = hp.mp_edges(*P, thr)
        dropped += int((~keep).sum())
        assert np.array_equal(em[keep], e64[keep])
        disagree += int((mdl["plain"] != e64).sum())
        total += len(d)
        worst = max(worst, float(np.max(np.abs(mdl["diff32"].astype(np.float64) - d) / (mdl["da"].astype(np.float64) + mdl["db"]))))
        for s in caught:
            caught[s] += int((hp.edge32_model(*P, thr, band_scale=s)["final"] != e64).sum())
    print(f"scale {scale} offset {offset}: fp32 != fp64 on {disagree}/{total}, |diff32 - diff64| / (da + db) <= {worst:.3e} "
          f"= {worst / hp.BAND:.3f} of the band coefficient, wrong edges by band multiple {caught}")
    assert dropped <= 0.01 * total                                           # (cap) otherwise the generator is wrong
    assert disagree >= MIN_DISAGREE[(scale, offset)] >= 50                   # (a) the pairs a zero band gets wrong
    assert worst < hp.BAND                                                   # (b) the band covers what float32 really does here
    assert caught[0.0] == disagree and caught[1 / 16] >= 1                   # the model says: a band cut to 1/16 is caught


def test_packed_problem_matches_pairs():
    a, b, P, lead = hp.band_problem(30.0, 0.0, 0.3, 0.5, 64, 5, 333, 1)
    assert a.shape == (333 + 128, 3) and lead == 1
    G = tc.graph(a, b, 0.3, 0.5)
    e = hp.d64(*P) <= hp.thr_of(0.3, 0.5)
    assert np.array_equal(G[lead + 2 * np.arange(64), lead + 2 * np.arange(64) + 1], e)
    f = lambda r: r if r < lead else r + 128                                 # filler row r in the packed problem
    nonfinite = [f(r) for r in range(5)]
    assert not G[nonfinite].any() and not G[:, nonfinite].any()              # NaN / Inf rows: no edge
    assert G[f(5), f(6)] and not G[f(5), f(7)]                               # coincident in both clouds / in one only


@pytest.mark.parametrize("case,label,improves", hp.EXIT_CASES)
def test_reduction_model_exits_as_labelled(case, label, improves):
    import networkx as nx
    a, b = hp.random_planted(*case)
    A = tc.graph(a, b)
    mc, lb, nu, nr, ex = tc.reduction_model(A, 1.0)
    assert ex == label
    if improves is not None:
        om = len(nx.max_weight_clique(tc.to_nx(A), None)[0])
        assert (om > lb) == improves and nr > 0 and lb - nu > 0


def test_reduction_model_shortcut_boundary():
    a, b, _, _ = tc.planted(128, 70, 3, noise=0.02)
    A = tc.graph(a, b)
    mc = tc.reduction_model(A, 1.0)[0]
    assert mc >= 69
    assert tc.reduction_model(A, mc / 128.0)[4] != "shortcut"               # max_core == kcore_threshold * M: strict >
    assert tc.reduction_model(A, (mc - 1) / 128.0)[4] == "shortcut"


def test_unreachable_exits_never_labelled():
    """'empty_universal' and 'search_target_nonpositive' cannot be reached (reduction_model's docstring): a scan agrees."""
    seen = set()
    for seed in range(60):
        a, b = hp.random_planted(seed, 24 + (seed * 37) % 120, 0.35 + 0.05 * (seed % 3), 3.0 - 0.5 * (seed % 3))
        seen.add(tc.reduction_model(tc.graph(a, b), 1.0)[4])
    assert seen <= {"empty_incumbent", "search"} and len(seen) == 2


def test_clique_exceeds_matches_networkx():
    import networkx as nx
    for case, _, _ in hp.EXIT_CASES:
        A = tc.graph(*hp.random_planted(*case))
        om = len(nx.max_weight_clique(tc.to_nx(A), None)[0])
        assert hp.clique_exceeds(A, om - 1) and not hp.clique_exceeds(A, om)
    a, b = hp.two_motions(60, 57, 180, 0)
    A = tc.graph(a, b)
    om = len(nx.max_weight_clique(tc.to_nx(A), None)[0])
    assert om >= 60 and hp.clique_exceeds(A, om - 1) and not hp.clique_exceeds(A, om)


def test_greedy_matches_definition():
    a, b = hp.random_planted(3, 135)
    A = tc.graph(a, b)
    c = tc.greedy_clique(A, 0, np.zeros(135, bool))
    assert hp.is_clique(A, c) and 0 in c
    assert not np.any(A[:, c].all(1))                                        # maximal


@pytest.mark.parametrize("row,K", hp.ROT_CASES)
def test_reference_flip_band(row, K):
    """The committed seeds keep the reference alone out of the flip band (the cap is 10 % of a row; kept here: no case at all), with
    the planted set standing in for the device's clique (the device test checks again with the clique it gets)."""
    a, b, T, mask, skw = hp.rot_case(row, K)
    c = np.nonzero(mask)[0]
    ref = hp.gnc_ref(a, b, c, **skw)
    assert not hp.gnc_in_band(ref, skw.get("max_iterations", 10000))
    if row == "no_start":
        assert not ref["started"] and ref["iters"] == 0
    elif row in ("cap1", "cap3"):
        assert ref["iters"] == skw["max_iterations"]
    elif row != "default":                                  # default: per-axis noise 0.15 sits on both sides of the start test
        assert ref["started"] and ref["iters"] >= 2
    if row not in ("default", "no_start") and K >= 64:
        assert 0.2 * K < ref["n_rot"] < 0.8 * K
    out = tc.solve_from_clique(a, b, c, **skw)
    assert out["iters"] == ref["iters"] and out["n_rot"] == ref["n_rot"]       # fp64 numpy and longdouble agree on the decisions


def test_vote_exact_matches_sweep():
    rng = np.random.default_rng(4)
    x = rng.normal(0, 0.4, 90)
    X = [hp._int(v, hp._SX) for v in x]
    ends = hp.vote_exact(X, 0.3)
    best = min(ends, key=lambda e: (e["cost_q"], e["key"]))
    est, cost, pos = tc.vote(x, 0.3)
    assert best["pos"] == pos and abs(float(best["mean_q"]) - est) < 1e-14 and abs(best["cost"] - cost) < 1e-12


def test_mirror_loop_ties():
    a, b, T = hp.mirror_loop(512, 11)
    kw = dict(noise_bound=0.3, cbar2=1.44)
    c = np.arange(512)
    assert hp.is_clique(tc.graph(a, b, **kw), c)
    ref = hp.gnc_ref(a, b, c, **kw)
    assert ref["started"] and ref["n_rot"] == 512 and not hp.gnc_in_band(ref, 10000)
    assert np.abs(ref["R"] - np.eye(3)).max() < 1e-15                        # R = I is the optimum of every fit
    X = hp.x_exact(a, b, np.eye(3), list(c))
    ends = hp.vote_exact([v[2] for v in X], 0.3)
    cmin = min(e["cost_q"] for e in ends)
    means = {e["mean_q"] for e in ends if e["cost_q"] == cmin}
    assert means == {1 + Fraction(hp.MIRROR_H), 1 - Fraction(hp.MIRROR_H)}   # two mathematically equal minima
