"""The builders of tests/filter_edges.py really hit their boundaries, and the plain restatement as well as the oracle reproduce what
the reference itself returned on them (tests/golden/g15_filter_edges.npz).  No GPU."""
import numpy as np
import pytest

from tests import filter_edges as fe
from tests.conftest import Args, golden

F32 = np.float32
NAMES = list(fe.all_clouds())


@pytest.fixture(scope="module")
def g15():
    return golden("g15_filter_edges.npz")


def _cloud(name):
    return fe.all_clouds()[name]()


# ----------------------------------------------------------------------------- the builders hit what they aim at
@pytest.mark.parametrize("name,G", [("b3", 3), ("b10", 10), ("b23", 23), ("b10d5", 10)])
def test_boundary_clouds_sit_on_every_interior_edge(name, G):
    c = _cloud(name)
    ax = c["axes"]
    assert c["F0"].shape[1] == (5 if name.endswith("d5") else 32)
    # the extrema are where the builder put them, so the arithmetic of the Axis objects is the cloud's
    for a in (0, 1):
        assert c["xyz0"][:, a].min() == ax[a].m and c["xyz0"][:, a].max() == ax[a].M
    qi, qj = fe.cells_ref(c["xyz0"][:, 0], c["xyz0"][:, 1], G)
    assert qi.max() == G - 1 and qj.max() == G - 1 and qi.min() == 0 and qj.min() == 0
    exact = below = 0
    seen = set()
    for pos, a, k, side, _ in c["planted"]:
        x = c["xyz0"][pos, a]
        q = (qi, qj)[a][pos]
        # side 0: the LAST float32 of quadrant k - 1; side 1: the FIRST of quadrant k
        assert q == (k - 1 if side == 0 else k)
        assert ax[a].quad(np.nextafter(x, F32(np.inf if side == 0 else -np.inf))) == (k if side == 0 else k - 1)
        p = ax[a].prod(x)
        exact += int(side == 1 and p == F32(k)); below += int(side == 0 and p == np.nextafter(F32(k), F32(0)))
        seen.add((a, k, side))
    assert seen == {(a, k, s) for a in (0, 1) for k in range(1, G) for s in (0, 1)}
    print(f"{name}: {len(c['planted'])} planted pairs, G * X_ an exact integer for {exact}, the last float below one for {below}")
    assert exact >= G - 1 and below >= 1
    # crowded cells far above their quota, sparse cells with room for one more: the planted pairs decide
    r = fe.gpf_ref(c, G, factor=c["factor"])
    odd = np.add.outer(np.arange(G), np.arange(G)) % 2 == 1
    hr = r["quota"].max()
    assert (r["counts"][~odd] >= hr + 2).all() and (r["counts"][odd] + 1 <= hr).all()
    assert fe.planted_pairs_matter(c) == 0
    # no two scores of a cell tie (the reference's argsort is not stable)
    key = np.stack([r["qi"] * G + r["qj"], r["nfd"].astype(np.float64)], 1)
    assert len(np.unique(key, axis=0)) == len(key)


@pytest.mark.parametrize("which", ["x", "y", "xy"])
def test_wide_clouds_have_a_pair_in_a_cell_that_does_not_exist(which):
    c = fe.wide_cloud(which)
    G = 10
    for a, name in enumerate("xy"):
        X = c["xyz0"][:, a]
        rng = F32(X.max() - X.min())
        den = F32(rng + F32(1e-3))
        assert (den == rng) == (name in which)                       # float32 absorbed the EPS
    qi, qj = fe.cells_ref(c["xyz0"][:, 0], c["xyz0"][:, 1], G)
    assert (qi.max() == G) == ("x" in which) and (qj.max() == G) == ("y" in which)
    r = fe.gpf_ref(c, G, factor=c["factor"])
    top_y = c["anchors"][3]
    if "y" in which:
        # the largest y: quadrant G in a column < G - 1, best score of the cloud -- kept wherever it is counted, so a wrapped flat index shows
        assert qj[top_y] == G and qi[top_y] == 2 and r["nfd"][top_y] == r["nfd"].min() and top_y not in r["idx0"]
        alt = fe.gpf_ref(c, G, factor=c["factor"])
        keep, _, _ = fe.select_ref(np.where(np.arange(len(qi)) == top_y, 3, qi), np.where(np.arange(len(qi)) == top_y, 0, qj), r["nfd"], G, r["TOTAL"])
        wrapped = np.flatnonzero(keep)
        assert top_y in wrapped and not np.array_equal(wrapped, alt["idx0"])
    if "x" in which:
        assert qi[c["anchors"][1]] == G and c["anchors"][1] not in r["idx0"]
    assert fe.planted_pairs_matter(c) == 0                           # (the edge k = G between the last cell and no cell included)
    assert {k for _, _, k, _, _ in c["planted"]} >= {G}


def _instrumented(counts, TOTAL, sum_fn=fe.sum_numpy):
    """A copy of the bisection (matching.py:160-179) that records the way it went."""
    apply_height = lambda h: (counts < h) * counts + (~(counts < h)) * h
    max_h, min_h, steps, log = TOTAL, 0, 0, []
    cur = (max_h + min_h) / 2
    while np.abs(max_h - min_h) > 2:
        t = sum_fn(apply_height(cur))
        if t == TOTAL:
            log.append("=="); break
        elif t < TOTAL:
            log.append("<"); min_h = cur
        elif t > TOTAL:
            log.append(">"); max_h = cur
        cur = (max_h + min_h) / 2
        steps += 1
    return dict(log=log, final=cur, hr=np.round(cur), quota=apply_height(np.round(cur)))


def test_waterfill_cases_take_the_branches_they_are_named_for():
    cases = {c["name"]: c for c in fe.waterfill_cases()}
    run = lambda n, s=fe.sum_numpy: _instrumented(cases[n]["counts"].astype(np.float64), cases[n]["factor"] * cases[n]["num_bb"], s)
    for name, total, hr in (("total0", 0.0, 0), ("total1", 1.0, 0), ("total2", 2.0, 1), ("total1.5", 1.5, 1)):
        r = run(name)
        assert cases[name]["factor"] * 64 == total and r["log"] == [] and r["hr"] == hr          # the loop is never entered
    r = run("total3")
    assert len(r["log"]) >= 1
    r = run("eq_break")
    assert r["log"][-1] == "==" and len(r["log"]) >= 3
    r = run("half_even")
    assert r["final"] % 1 == 0.5 and int(r["final"]) % 2 == 0 and r["hr"] == int(r["final"])           # k + 0.5 -> k
    r = run("half_odd")
    assert r["final"] % 1 == 0.5 and int(r["final"]) % 2 == 1 and r["hr"] == int(r["final"]) + 1       # k + 0.5 -> k + 1
    r = run("quota_eq_count")
    cf, qf = cases["quota_eq_count"]["counts"].ravel(), r["quota"].ravel()
    assert any(qf[k] == cf[k] >= 2 and qf[k + 1] == cf[k + 1] - 1 for k in range(len(cf) - 1))
    r = run("total_above_sum")
    assert set(r["log"]) == {"<"} and (r["quota"] == cases["total_above_sum"]["counts"]).all()
    # the summation order decides: numpy's pairwise order and a left-to-right sum end at different rounded heights
    per_width = {}
    for name in cases:
        if name.startswith("order_g"):
            G = cases[name]["counts"].shape[0]
            assert run(name)["hr"] != run(name, fe.sum_left_to_right)["hr"], name
            per_width[G] = per_width.get(G, 0) + 1
    print("order-sensitive water-filling cases per width:", per_width)
    assert per_width.get(8, 0) >= 3 and per_width.get(16, 0) >= 3 and per_width.get(64, 0) >= 3
    # (20 000 seeded trials each find none at 2 and 11 and one at 12: DESIGN.md 3.2)
    assert set(per_width) <= {8, 12, 16, 64}


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("wf_")])
def test_waterfill_clouds_have_the_planned_counts(name):
    c = _cloud(name)
    case = next(k for k in fe.waterfill_cases() if "wf_" + k["name"] == name)
    qi, qj = fe.cells_ref(c["xyz0"][:, 0], c["xyz0"][:, 1], c["G"])
    got = np.bincount((qi * c["G"] + qj).astype(np.int64), minlength=c["G"] ** 2).reshape(c["G"], c["G"])
    assert np.array_equal(got, case["counts"]) and int(c["is_bb"].sum()) == case["num_bb"]


def test_prosac_lists_cover_the_lengths_and_values():
    L = fe.prosac_lists()
    assert {len(v) for v in L.values()} >= {1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 9217}
    assert len(np.unique(L["all_equal"])) == 1 and len(np.unique(L["two_values"])) == 2
    q = L["inf_nan"]
    assert np.isposinf(q).sum() == 1 and np.isneginf(q).sum() == 1 and np.isnan(q).sum() == 1
    assert np.isnan(L["many_nan"]).sum() > 2000
    g = L["gpf_shape"]
    assert ((g > 0.9999) & (g < 1)).sum() > 400 and (g < 0).sum() > 2000
    for name, q in L.items():
        o = fe.prosac_expected(q)
        k = np.where(np.isnan(q), np.inf, q)[o]
        assert (k[1:] >= k[:-1]).all() and sorted(o.tolist()) == list(range(len(q)))
        tie = k[1:] == k[:-1]
        assert (np.diff(o)[tie] > 0).all()                           # ties by index


# ----------------------------------------------------------------------------- the lists are the true neighbours
@pytest.mark.parametrize("name", ["b10", "b10d5", "wide_y", "wf_quota_eq_count", "wf_order_g8_0"])
def test_clouds_carry_their_true_neighbour_lists(oracle, name):
    c = _cloud(name)
    i0, i1, i2, _ = oracle.find_2nn(c["F0"], c["F1"])
    assert np.array_equal(i1, c["i1"]) and np.array_equal(i2, c["i2"])
    is_bb, num = oracle.mark_best_buddies(c["F0"], c["F1"], c["i0"], c["i1"])
    assert np.array_equal(is_bb, c["is_bb"])


# ----------------------------------------------------------------------------- the fixture
def _same(g15, name, tag, i0, i1, i2, score):
    assert np.array_equal(np.asarray(i0), g15[f"{name}_{tag}_idx0"]), (name, tag)
    assert np.array_equal(np.asarray(i1), g15[f"{name}_{tag}_idx1"]) and np.array_equal(np.asarray(i2), g15[f"{name}_{tag}_idx2"])
    assert np.array_equal(np.asarray(score, F32).view(np.uint32), g15[f"{name}_{tag}_score"]), (name, tag)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(g15, name):
    c = _cloud(name)
    assert np.array_equal(np.frombuffer(bytes.fromhex(fe.checksum(c)), np.uint8), g15[f"{name}_sha"]), "the builder drifted from the fixture"
    assert tuple(g15[f"{name}_cfg"]) == (c["G"], c["factor"], c["cap"])
    r = fe.gpf_ref(c, c["G"], factor=c["factor"])
    _same(g15, name, "gpf", r["idx0"], r["idx1"], r["idx2"], r["score"])
    r = fe.gpf_ref(c, c["G"], cap=c["cap"])
    _same(g15, name, "bbf", r["idx0"], r["idx1"], r["idx2"], r["score"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference(oracle, g15, name):
    c = _cloud(name)
    a = Args(GPF_grid_wid=c["G"], GPF_factor=c["factor"], GPF_max_matches=c["cap"])
    e = oracle.Grid_Prioritized_Filter(c["F0"], c["F1"], c["i0"], c["i1"], c["i2"], c["xyz0"], a)
    _same(g15, name, "gpf", e[0], e[1], e[2], e[6])
    e = oracle.Grid_Prioritized_Filter(c["F0"], c["F1"], c["i0"], c["i1"], c["i2"], c["xyz0"], a, BB_first=True)
    _same(g15, name, "bbf", e[0], e[1], e[2], e[6])
