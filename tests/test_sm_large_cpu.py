"""The yardsticks of tests/test_gpu_sm_large.py, without a GPU: the closed form for planted line sets (sm_cpu.planted_v) against the numpy
restatement, the integer conditions that make the planted sets exact in fp32, and the conditions on the three golden-backed inputs
(tests/golden/g23_sm_large.npz, read -- never recomputed here: tests/golden/make_golden_sm_large.py)."""
import os

import numpy as np
import pytest

from tests import sm_cases, sm_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g23_sm_large.npz"))
LARGE = sm_cases.large_cases()
PLANTED = [c["name"] for c in LARGE if c["kind"] == "planted"]
RECORDED = [c["name"] for c in LARGE if c.get("large")]


def test_large_case_list():
    assert PLANTED == ["planted_ties_3100_k310", "planted_ties_3100_k465", "planted_zeros_2500", "planted_limit_32767"]
    assert [(n, len(sm_cases.by_name(n)["a"]), sm_cases.by_name(n)["ratio"]) for n in RECORDED] == [
        ("gap_8193_409", 8193, 0.05), ("full_20001", 20001, 0.05), ("full_32768", 32768, 0.05)]
    assert not {c["name"] for c in LARGE} & {c["name"] for c in sm_cases.cases()}
    c = sm_cases.by_name("planted_ties_3100_k310")
    assert c["K"] == 310 and len(c["pairs"]) == 310 and c["expect_sel"] == tuple(i for p in range(0, 1550, 10) for i in (p, p + 1))
    assert max(c["expect_sel"]) > 1024                                      # the cut lies in the second selection pass
    c = sm_cases.by_name("planted_ties_3100_k465")
    assert c["K"] == 465 and c["expect_sel"][-1] == 2320 and 2321 not in c["expect_sel"] and c["expect_sel"][-1] > 2048      # odd: a pair is separated, third pass
    c = sm_cases.by_name("planted_zeros_2500")
    assert c["K"] == 1500 and c["expect_sel"] == tuple(range(1500)) and not c["pairs"]
    c = sm_cases.by_name("planted_limit_32767")
    assert len(c["a"]) == 32767 and len(c["a"]) % 4 == 3 and c["b"][32766, 0] == 327660.0
    assert c["pairs"][:2] == ((0, 32766), (1, 32765)) and c["K"] == len(c["pairs"]) == 34 == sm_cpu.top_k(32767, c["ratio"])
    assert c["expect_sel"] == (0, 1) + tuple(i for p in range(1000, 17000, 1000) for i in (p, p + 1))


def test_planted_v_equals_the_restatement():
    """The closed form against sm_cpu.sm in fp64, to 1e-14: on planted_equal_at_cut and on a 257-row set, at several iteration counts."""
    c = sm_cases.by_name("planted_equal_at_cut")
    pairs = [(p, p + 1) for p in range(0, 100, 10)]
    for it in (1, 2, 10, 37):
        assert np.abs(sm_cpu.planted_v(100, pairs, it) - sm_cpu.sm(c["a"], c["b"], c["thr"], c["ratio"], it)["v"]).max() <= 1e-14
    a, b = sm_cases.line(257)
    pairs = [(0, 256), (1, 200), (64, 65), (130, 131)]
    for p, q in pairs:
        sm_cases.plant_pair(b, p, q)
    r = sm_cpu.sm(a, b, 0.6, 0.02)
    assert np.abs(sm_cpu.planted_v(257, pairs) - r["v"]).max() <= 1e-14 and np.count_nonzero(r["v"]) == 8
    assert not sm_cpu.planted_v(50, []).any()


@pytest.mark.parametrize("name", PLANTED)
def test_planted_sets_are_exact_in_fp32(name):
    """For each planted row q, in exact integer arithmetic: d(q, partner) = 0 and |d(q, j)| >= 2 for every other j (two rows that are
    both unplanted keep line()'s d = 2 |i - j|); every coordinate is an integer below 2^24, so the device's fp32 chain is exact --
    sqrtf(fl(x^2)) = |x| in binary floating point.  O(M x planted): M x M is not formed."""
    c = sm_cases.by_name(name)
    a, b, M = c["a"], c["b"], len(c["a"])
    assert np.abs(a).max() < 2 ** 24 and np.abs(b).max() < 2 ** 24
    partner = {}
    for p, q in c["pairs"]:
        partner[p], partner[q] = q, p
    a0, b0 = sm_cases.line(M)
    assert np.array_equal(a, a0) and set(np.flatnonzero(b[:, 0] != b0[:, 0])) <= set(partner)      # only planted rows were moved
    for q, mate in partner.items():
        d = sm_cpu.planted_distances(a, b, q)
        assert d[mate] == 0
        d[[q, mate]] = 99
        assert np.abs(d).min() >= 2, (name, q, int(np.abs(d).argmin()))
    # what the closed form then says of the case: the number of equal non-zero values, and the selection under the tie rule
    v = sm_cpu.planted_v(M, c["pairs"])
    assert np.count_nonzero(v) == 2 * len(c["pairs"]) and len(set(v[v > 0])) <= 1
    assert tuple(sm_cpu.select(v, c["K"])) == c["expect_sel"]


@pytest.mark.parametrize("name", RECORDED)
def test_golden_belongs_to_these_inputs(name):
    c = sm_cases.by_name(name)
    assert str(GOLD[name + "/sha256"]) == sm_cases.checksum(c), "tests/sm_cases.py changed: regenerate with tests/golden/make_golden_sm_large.py"
    assert int(GOLD[name + "/seed"]) == sm_cases.LARGE_SEEDS[name]
    v = GOLD[name + "/v"]
    assert int(GOLD[name + "/K"]) == sm_cpu.top_k(len(c["a"]), c["ratio"]) and v.dtype == np.float64 and v.shape == (len(c["a"]),)
    assert np.isfinite(v).all() and (v >= 0).all() and abs(np.sqrt((v * v).sum()) - 1) < 1e-5


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_cases_meet_their_conditions(name):
    """Conditions on the inputs, from the recorded fp64 vector alone: a relative gap >= 1e-3 at the cut of the gap case, at most 5 % of
    K entries within 1e-5 max v of the cut on the other two.  The recorded scalars are those of the recorded vector."""
    c, v, K = sm_cases.by_name(name), GOLD[name + "/v"], int(GOLD[name + "/K"])
    s = np.sort(v)[::-1]
    gap = (s[K - 1] - s[K]) / s[0]
    near = int((np.abs(v - s[K - 1]) <= 1e-5 * s[0]).sum())
    d32, dseq = float(GOLD[name + "/d32"]), float(GOLD[name + "/d32_seq256"])
    print(f"{name}: K {K}, gap {gap:.3e}, near {near}; fp32 restatements vs fp64: blocked {d32 / s[0]:.2e}, in the contract's order (256 CUs) {dseq / s[0]:.2e} of max v")
    assert gap == float(GOLD[name + "/gap"]) and near == int(GOLD[name + "/near"])
    if c["kind"] == "gap":
        assert gap >= 1e-3
        labels = np.unpackbits(GOLD[name + "/labels"])[:len(v)]
        assert labels.sum() == K and np.array_equal(np.flatnonzero(labels), sm_cpu.select(v, K))       # the reference's own SM()
        assert GOLD[name + "/T"].shape == (4, 4)
    else:
        assert near <= 0.05 * K
    # fp32 costs something and not much: the yardstick of the eigenvector test is neither 0 nor loose
    assert 0 < d32 < 1e-5 * s[0] and 0 < dseq < 1e-4 * s[0]


def test_plan_restatement():
    """sm_cpu.plan against the figures of DESIGN §11.2 at 256 compute units."""
    assert sm_cpu.plan(4096) == (64, 32, 128) and sm_cpu.plan(2048) == (32, 32, 64)
    assert sm_cpu.plan(32768) == (512, 4, 8192) and sm_cpu.plan(20001) == (313, 6, 3336) and sm_cpu.plan(8193)[:2] == (129, 15)
    assert sm_cpu.plan(3) == (1, 1, 4) and sm_cpu.plan(0) == (1, 1, 4)


def test_power_chunked32_is_the_power_iteration():
    """One chunk per row and a handful of columns: the sequential fp32 sum is numpy's, so the two fp32 restatements agree to rounding; on
    a planted set (integers) they agree with the closed form."""
    c = sm_cases.by_name("cluster_1000_300")
    C = sm_cpu.compat(c["a"], c["b"], c["thr"], np.float32)
    v64 = sm_cpu.reference("cluster_1000_300")["v"]
    for per in (1000, 64):
        assert np.abs(sm_cpu.power_chunked32(C, per) - v64).max() <= 4 * np.abs(sm_cpu.reference("cluster_1000_300", "float32")["v"] - v64).max()
    c = sm_cases.by_name("planted_equal_at_cut")
    C = sm_cpu.compat(c["a"], c["b"], c["thr"], np.float32)
    assert np.abs(sm_cpu.power_chunked32(C, 28) - sm_cpu.planted_v(100, [(p, p + 1) for p in range(0, 100, 10)])).max() <= 1e-7


def test_thresholds_change_the_eigenvector():
    """A condition on cluster_1000_300: the fp64 vectors at inlier_threshold 0.1 / 0.3 / 2.0 differ from the one at 0.6 by far more than
    the eigenvector tolerance (100 x here), so a call that ignores the parameter fails the GPU test."""
    c = sm_cases.by_name("cluster_1000_300")
    v06 = sm_cpu.reference("cluster_1000_300")["v"]
    tol = max(16 * np.abs(sm_cpu.reference("cluster_1000_300", "float32")["v"] - v06).max(), 1e-6 * v06.max())
    for thr in (0.1, 0.3, 2.0):
        d = np.abs(sm_cpu.sm(c["a"], c["b"], thr, c["ratio"])["v"] - v06).max()
        print(f"inlier_threshold {thr}: |v - v(0.6)|_inf = {d:.2e}, tolerance {tol:.2e}")
        assert d > 100 * tol


def test_iterations_change_the_eigenvector():
    """The same for iterations 1 / 2 against 10 on cluster_1000_300; 37 has converged to within the tolerance of 10 or not -- it is
    compared with its own reference either way."""
    c = sm_cases.by_name("cluster_1000_300")
    v10 = sm_cpu.reference("cluster_1000_300")["v"]
    tol = max(16 * np.abs(sm_cpu.reference("cluster_1000_300", "float32")["v"] - v10).max(), 1e-6 * v10.max())
    for it in (1, 2):
        assert np.abs(sm_cpu.sm(c["a"], c["b"], c["thr"], c["ratio"], it)["v"] - v10).max() > 100 * tol


def test_device_side_k_rule():
    """K of the kcut ratios on the live counts the GPU test passes as m_dev (rows padded to 200)."""
    assert [sm_cpu.top_k(m, q) for m, q in ((100, 0.29), (60, 0.05), (59, 0.05), (30, 0.1), (20, 0.1))] == [28, 3, 2, 3, 2]
