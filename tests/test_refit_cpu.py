"""The stage after RANSAC on the CPU: the cases of tests/refit_cases.py meet the conditions that make the restatement
(tests/refit_cpu.py) decisive, the oracle's refit -- its own copy of the arithmetic, not part of lr_contract.h -- and its mask agree
with the restatement on all of them, and the comparison notices each of five planted mistakes."""
import os
import subprocess

import numpy as np
import pytest

from tests import refit_cases as cases
from tests import refit_cpu as rc
from tests import rigid_hp as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = cases.all_refit_cases()
IDS = [c["name"] for c in ALL]


oracle_refit, problems = cases.oracle_refit, cases.problems


# ------------------------------------------------------------------------------------------------------------ the cases' conditions
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_conditions(c):
    ref = cases.reference(c)
    live = c["planted"][ref["rows"]]
    assert np.array_equal(ref["inlier"], live), "the pairs are not what the case planted"
    if c["exact"]:
        # every fp64 operation of the kernel's expression is exact: the fp64 evaluation in its order, the integers and mpmath agree
        P = c["xyz0"][ref["i0"]].astype(np.float64); Q = c["xyz1"][ref["i1"]].astype(np.float64); T = c["T"]
        r = [(((T[a, 0] * P[:, 0] + T[a, 1] * P[:, 1]) + T[a, 2] * P[:, 2]) + T[a, 3]) - Q[:, a] for a in range(3)]
        d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        inl_mp, gap_mp = rc.exact_d2_mp(P, Q, T, c["thr2"])
        assert np.array_equal(d2, ref["d2"]) and np.array_equal(d2 - c["thr2"], ref["gap"])
        assert np.array_equal(inl_mp, ref["inlier"]) and np.array_equal(gap_mp, ref["gap"])
        assert d2[0] == 0.375 and ref["gap"][0] == 0.375 - c["thr2"] and d2[1] < 0.375 < d2[2]
        return
    assert ref["M"] < 600.0                                   # what refit_cases.MARGIN was derived for
    assert 1000.0 * rc.d2_bound(cases.THR2, 600.0, rc.U64, 7) <= cases.MARGIN
    assert np.all(np.abs(ref["gap"]) >= cases.MARGIN)
    assert np.all(np.abs(ref["gap"]) >= 1000.0 * rc.d2_bound(ref["d2"], ref["M"], rc.U64, 7))


@pytest.mark.parametrize("m", cases.MASK_SIZES)
def test_mask_case_conditions(m):
    c = cases.mask_case(m)
    ref = rc.mask(c["src"], c["tgt"], c["T"], c["thr2"])
    assert np.array_equal(ref["inlier"], c["planted"])
    assert np.all(np.abs(ref["gap"]) > rc.SAFETY * ref["bound"])


def test_patterns_hit_the_slots_they_name():
    n = 66561
    assert cases.pattern("last_block", 1025).sum() == 1 and cases.pattern("last_block", 65537).nonzero()[0].tolist() == [65536]
    assert cases.pattern("last_block", 1024).sum() == 1024 and cases.pattern("last_block", 2049).sum() == 1
    i = cases.pattern("lane0", n).nonzero()[0]
    assert np.all(i % 64 == 0) and i.size == (n + 63) // 64
    i = cases.pattern("u3", 2049).nonzero()[0]
    assert np.all((i % 1024) // 256 == 3) and i.size == 512
    i = cases.pattern("block64", n).nonzero()[0]
    assert i[0] == 65536 and i[-1] == 66559 and i.size == 1024
    assert cases.pattern("two", 1025).sum() == 2 and cases.pattern("three", 1025).sum() == 3
    sizes = {n for n, _ in cases.plain_specs()}
    assert sizes == {1, 2, 3, 4, 255, 256, 257, 1023, 1024, 1025, 2049, 65536, 65537, 66561}


# ------------------------------------------------------------------------------------------------------------ the restatement itself
def test_integer_decision_equals_mpmath():
    for c in (cases.plain_case(257, "lane0"), cases.plain_case(1025, "three"), cases.weighted_case("ordinary", 5)):
        ref = cases.reference(c)
        inl, gap = rc.exact_d2_mp(c["xyz0"][ref["i0"]], c["xyz1"][ref["i1"]], c["T"], c["thr2"])
        assert np.array_equal(inl, ref["inlier"]) and np.array_equal(gap, ref["gap"])
    c = cases.plain_case(66561, "block64")
    ref = cases.reference(c)
    s = np.r_[0:40, 65530:65560, 66550:66561]
    inl, gap = rc.exact_d2_mp(c["xyz0"][s], c["xyz1"][c["idx1"][s]], c["T"], c["thr2"])
    assert np.array_equal(inl, ref["inlier"][s]) and np.array_equal(gap, ref["gap"][s])


def test_both_fit_routes_agree():
    """1 025 inliers down the mpmath route and down the exact-moment route: the same rotation and translation to 1e-25."""
    c = cases.plain_case(1025, "all")
    a = cases.reference(c)["ref"]
    b = cases.reference(c, route="moments")["ref"]
    T = np.eye(4); T[:3, :3] = b["R"]
    assert hp.angle(T, a) <= 1e-15 and np.abs(a["R"] - b["R"]).max() == 0.0 and np.abs(a["t"] - b["t"]).max() == 0.0
    assert abs(float(a["fstar"] - b["fstar"])) <= 1e-25 * float(a["fstar"])
    assert max(abs(float(a["Hmp"][i, j] - b["Hmp"][i, j])) for i in range(3) for j in range(3)) <= 1e-25 * a["scale"]
    assert abs(a["kappa_raw"] - b["kappa_raw"]) <= 1e-9 * a["kappa_raw"]


def test_gates_of_the_restatement():
    c = cases.plain_case(1025, "all")
    r = rc.refit(c["xyz0"], c["xyz1"], c["idx1"], c["T"], c["thr2"], have_model=False)
    assert np.array_equal(r["T"], c["T"]) and r["n_refit"] == 0 and r["status"] == 1 and r["ref"] is None
    for n, pat, want in ((1025, "two", 2), (1025, "none", 0), (2, "all", 2), (1, "all", 1), (3, "all", 3)):
        c = cases.plain_case(n, pat)
        r = cases.reference(c)
        assert r["n_refit"] == want and r["status"] == 0
        assert (r["ref"] is None and np.array_equal(r["T"], c["T"])) == (want < 3)
    # under weights fewer than 3 pairs are fitted all the same, and n_refit is their number, not their weight sum
    for how, dim, want in (("two", 32, 2), ("one", 5, 1)):
        r = cases.reference(cases.weighted_case(how, dim))
        assert r["n_refit"] == want and r["ref"] is not None


def test_weights_of_the_cases():
    for dim in (32, 5):
        r = cases.reference(cases.weighted_case("identical", dim))
        assert np.all(r["w"] == 1.0 / float(np.float32(1e-12))) and r["n_refit"] == len(r["w"]) > 100
        r = cases.reference(cases.weighted_case("dominant", dim))
        assert r["w"][0] == 2.0 ** 20 and np.all(r["w"][1:] < 8.0)
        r = cases.reference(cases.weighted_case("below_one", dim))
        assert 0.0 < r["w"].sum() < 1.0 and r["n_refit"] > 100          # (int) of the weight sum would say 0
    # a narrow descriptor is a 32-wide one with zero columns
    c = cases.weighted_case("ordinary", 5)
    r = cases.reference(c)
    w32 = rc.weights(cases.pad32(c["F0"]), cases.pad32(c["F1"]), r["i0"][r["inlier"]], r["i1"][r["inlier"]])
    assert np.array_equal(w32, r["w"])


# ------------------------------------------------------------------------------------------------------------ the oracle against it
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_oracle_refit_equals_restatement(oracle, c):
    T, n = oracle_refit(oracle, c)
    bad = problems(T, n, cases.reference(c), c)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("refit", [1, 2, 3])
@pytest.mark.parametrize("mode", ["MNN", "no_filter"])
def test_oracle_register_pair_equals_restatement(oracle, refit, mode):
    """oracle.register_pair's refit_on_orig 1 / 2 / 3 against the restatement fed the same lists and the same RANSAC model."""
    from lidarregistration_amd import synth
    p = synth.make_pair(N=700, N1=650, rho=0.5, s=0.9, seed=77)
    kw = dict(mode=mode, iters=400, sample_size=3, seed=51)
    e0 = oracle.register_pair(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], refit_on_orig=0, **kw)
    e = oracle.register_pair(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], refit_on_orig=refit, **kw)
    assert e0["ransac"]["best_h"] >= 0 and e0["ransac"] == e["ransac"]
    lists = dict(idx0=e["idx0"], m=len(e["idx0"])) if refit == 2 else {}
    F = dict(F0=p["feats0"], F1=p["feats1"]) if refit == 3 else {}
    ref = rc.refit(p["xyz0"], p["xyz1"], e["idx1"] if refit == 2 else e["idx1_orig"], e0["T"], cases.THR2, **lists, **F)
    assert np.all(np.abs(ref["gap"]) > 1000.0 * rc.d2_bound(ref["d2"], ref["M"], rc.U64, 7))
    assert ref["n_refit"] >= 30 and (refit != 2 or mode != "MNN" or len(e["idx0"]) < 700)
    bad = problems(e["T"], e["n_refit"], ref, dict(name=f"register_pair refit={refit} {mode}", T=e0["T"]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("m", cases.MASK_SIZES)
def test_oracle_mask_equals_exact_decision(oracle, m):
    c = cases.mask_case(m)
    ref = rc.mask(c["src"], c["tgt"], c["T"], c["thr2"])
    got, n = oracle.inlier_mask(c["src"], c["tgt"], c["T"], c["thr2"])
    sure = np.abs(ref["gap"]) > rc.SAFETY * ref["bound"]
    assert sure.all() and np.array_equal(got, ref["inlier"]) and n == int(ref["inlier"].sum())


@pytest.mark.parametrize("which", ["at", "next32"])
def test_oracle_mask_on_the_exact_boundary(oracle, which):
    c = cases.boundary_case(which)
    ref = rc.mask(c["xyz0"], c["xyz1"], c["T"], c["thr2"])
    got, n = oracle.inlier_mask(c["xyz0"], c["xyz1"], c["T"], c["thr2"])
    assert np.array_equal(ref["inlier"], c["planted"]) and np.array_equal(got, c["planted"]) and n == int(c["planted"].sum())
    assert (ref["gap"][0] == 0.0) == (which == "at")


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _noticed(orc, **kw):
    """The cases on which the comparison of test_oracle_refit_equals_restatement fails when the oracle is driven with **kw."""
    hit = []
    for c in ALL:
        if c["kind"] == "listed" or not ({"use_idx0", "m_shift"} & set(kw)):
            T, n = oracle_refit(orc, c, **{k: (v(c) if callable(v) else v) for k, v in kw.items()})
            if problems(T, n, cases.reference(c), c):
                hit.append(c["name"])
    return hit


def test_planted_mistakes_are_noticed(oracle, tmp_path):
    """Each mistake is planted on the oracle's side of the comparison -- by how it is driven or, for the clamp, in a scratch build of
    oracle.c -- and the comparison with the restatement must fail on the case that was built for it (and only where it should)."""
    clean = _noticed(oracle)
    assert clean == []
    # `<` replaced by `<=`: d2 <= thr2 is d2 < nextafter(thr2)
    hit = _noticed(oracle, thr2=lambda c: float(np.nextafter(c["thr2"], np.inf)))
    assert hit == ["boundary at"], hit
    # the last partial block dropped
    hit = _noticed(oracle, rows=lambda c: (len(c["idx1"]) if c["idx0"] is None else c["m"]) // 1024 * 1024)
    assert "plain n=1025 last_block" in hit and "plain n=65537 all" in hit and "plain n=1023 all" in hit and "listed perm L=2049 m=1025" in hit
    assert not [h for h in hit if " n=1024 " in h or " n=65536 " in h]
    # idx0 ignored
    hit = _noticed(oracle, use_idx0=False)
    assert {"listed perm L=2049 m=1025", "listed repeats L=2049 m=2049", "listed perm L=66561 m=65537", "listed perm L=2049 m=1"} <= set(hit)
    # the live count off by one, either way
    for shift in (1, -1):
        hit = _noticed(oracle, m_shift=shift)
        assert {"listed perm L=2049 m=1024", "listed perm L=2049 m=1025", "listed perm L=66561 m=65537", "listed perm L=2049 m=3"} <= set(hit), (shift, hit)
    # the weight clamp removed: a scratch build of the oracle
    src = open(os.path.join(ROOT, "oracle", "oracle.c")).read()
    clamp = "fmaxf(sqrtf(acc), 1e-12f)"
    assert src.count(clamp) == 1
    src = src.replace('#include "../lidarregistration_amd/csrc/lr_contract.h"',
                      f'#include "{os.path.join(ROOT, "lidarregistration_amd", "csrc", "lr_contract.h")}"').replace(clamp, "sqrtf(acc)")
    (tmp_path / "oracle.c").write_text(src)
    so = str(tmp_path / "liboracle_noclamp.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-mfma", "-mavx2", "-o", so, str(tmp_path / "oracle.c"), "-lm"])
    import ctypes
    mut = ctypes.CDLL(so)

    class Mutant:
        @staticmethod
        def refit(xyz0, xyz1, idx1, T, thr2=None, feats0=None, feats1=None):
            real = oracle.lib
            oracle.lib = lambda: mut
            try:
                return oracle.refit(xyz0, xyz1, idx1, T, thr2=thr2, feats0=feats0, feats1=feats1)
            finally:
                oracle.lib = real

    hit = _noticed(Mutant)
    assert hit == ["weighted identical dim=32", "weighted identical dim=5"], hit
