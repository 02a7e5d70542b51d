"""The numpy restatement of lr_pdsc_solve's contract (tests/pdsc_solve_cpu.py) against the recording of the reference's own tail
(tests/golden/g26_pdsc_solve.npz), and the contract's deviations from the reference.  No GPU.

Bounds, fixed before the figures were read:
  * indices and counts: equal -- seeds up to the order inside a group of equal keys (the reference's argsort leaves it open; S2 fixes it),
    neighbour lists on the seeds without a duplicated row;
  * weights: 1e-5 max|w| + 1e-7 -- the allclose tolerance the reference's loop leaves early under (rtol 1e-5), and E3's fp32 rounding of
    -1/sigma_d^2 (2^-24 relative on the matrix, which ten iterations do not amplify beyond 1e-7);
  * seed transforms and the unrefined best: a quarter of the reference's own fp32-vs-fp64 deviation (the yardstick of the device tests: the
    restatement has to be clearly nearer to fp64 than fp32 is), floor 1e-9;
  * the refined transform: 1e-8 (the refinement depends on the seed's transform only through its inlier set).
"""
import numpy as np
import pytest

from tests import pdsc_solve_cases as cases
from tests import pdsc_solve_cpu as cpu
from tests.conftest import golden

NAMES = [c[0] for c in cases.GOLDEN]


@pytest.fixture(scope="module")
def g26():
    return golden("g26_pdsc_solve.npz")


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name in NAMES:
        c = cases.golden_case(name)
        out[name] = (c, cpu.solve(c["src"], c["tgt"], c["feat"], c["conf"], **cases.PARAMS))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_recording(g26, solved, name):
    c, r = solved[name]
    m = c["m"]
    assert str(g26[name + "/sha256"]) == cases.checksum(c), "the fixture was recorded from other inputs"
    rec_seeds = g26[name + "/seeds"].astype(np.int64)
    key = cpu.seed_keys(c["conf"], cpu.local_max(c["src"], c["conf"], r["live"], cases.PARAMS["nms_radius"]))
    assert set(rec_seeds) == set(r["seeds"]) and np.array_equal(key[rec_seeds], key[r["seeds"]])
    if len(set(key[r["seeds"]])) == len(r["seeds"]):
        assert np.array_equal(rec_seeds, r["seeds"])
    row = {int(s): i for i, s in enumerate(r["seeds"])}
    at = np.array([row[int(s)] for s in rec_seeds])         # our row of the recording's seed
    assert np.array_equal(g26[name + "/counts"], r["counts"][at])
    assert r["seeds"][r["best_rank"]] == rec_seeds[int(g26[name + "/best"])] or r["counts"][at][int(g26[name + "/best"])] == r["best_count"]
    assert r["best_count"] == g26[name + "/counts"].max() and np.array_equal(np.unpackbits(g26[name + "/labels"])[:m], r["labels"])
    same = np.array([set(a) == set(b) for a, b in zip(g26[name + "/knn"], r["knn"][at])])
    assert same.mean() >= 0.95
    if c["inlier"].size and name != "m1000":
        assert same.all() and np.array_equal(g26[name + "/knn"], r["knn"][at])
    w_rec, w = g26[name + "/weights"][same], r["weights"][at][same]
    order = lambda w_, k_: np.stack([a[np.argsort(b)] for a, b in zip(w_, k_)])
    dw = np.abs(order(w_rec, g26[name + "/knn"][same]) - order(w, r["knn"][at][same])).max()
    dT = np.abs(g26[name + "/seed_T"][same] - r["seed_T"][at][same]).max()
    dB, dR = np.abs(g26[name + "/T_best"] - r["T_best"]).max(), np.abs(g26[name + "/T"] - r["T"]).max()
    print(f"{name}: weights {dw:.2e} seed T {dT:.2e} (yardstick {g26[name + '/dev_seed_T']:.2e}) T_best {dB:.2e} T {dR:.2e}")
    assert dw <= 1e-5 * np.abs(w_rec).max() + 1e-7
    assert dT <= max(float(g26[name + "/dev_seed_T"]) / 4, 1e-9)
    assert dB <= max(float(g26[name + "/dev_seed_T"]) / 4, 1e-9)
    assert dR <= 1e-8


def test_the_recording_covers_what_it_should(g26):
    assert bool(g26["m11/early"]) and not bool(g26["m3000/early"])
    for name in NAMES:
        c = g26[name + "/counts"]
        assert g26[name + "/same_set"] >= 0.95
        assert int(g26[name + "/best"]) == int(np.argmax(c))          # the first of the largest, also in the reference
    assert (g26["m3000/counts"] == g26["m3000/counts"].max()).sum() > 1          # the first-maximum rule is exercised
    c = cases.golden_case("m1000")
    s = g26["m1000/seeds"]
    assert len(np.unique(c["conf"][s])) < len(s)        # two seeds of equal key


def test_fp32_restatement_is_a_yardstick(g26, solved):
    """S3-S6 in numpy's fp32 deviate from fp64 as the reference's own fp32 run does (0.5 .. 2 x on the seed transforms where no loop left early)."""
    for name in ("m257", "m1000", "m3000"):
        c, r = solved[name]
        r32 = cpu.solve(c["src"], c["tgt"], c["feat"], c["conf"], dtype=np.float32, **cases.PARAMS)
        assert np.array_equal(r32["seeds"], r["seeds"]) and np.array_equal(r32["counts"], r["counts"])
        same = np.array([set(a) == set(b) for a, b in zip(r32["knn"], r["knn"])])
        ratio = np.abs(r32["seed_T"] - r["seed_T"])[same].max() / float(g26[name + "/dev_seed_T"])
        print(name, "fp32 restatement / reference's deviation", ratio)
        assert same.mean() >= 0.95 and 0.5 <= ratio <= 2.0


def test_normalize32_is_the_stated_order():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((64, 128)).astype(np.float32)
    f[3] = 0; f[4] *= np.float32(1e-30); f[5] *= np.float32(1e20)
    live = np.ones(64, bool); live[7] = False
    fn = cpu.normalize32(f, live)
    assert fn.dtype == np.float32 and not fn[3].any() and not fn[7].any() and np.isfinite(fn).all()
    assert not fn[5].any()                              # the sum of squares overflows: the row is 0, as F.normalize's
    ok = np.r_[0:3, 6, 8:64]
    assert np.abs(np.linalg.norm(fn[ok].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.abs(fn[ok] - cpu.normalize(f, live)[ok]).max() < 2e-7


# ---- the deviations ---------------------------------------------------------------------------------------------------------------------
def test_equal_keys_sort_by_ascending_index_and_negative_maxima_behind_the_zeros():
    src = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [20.1, 0, 0], [30, 0, 0], [40, 0, 0]], np.float32)
    conf = np.array([2.0, -1.0, 1.0, 3.0, 2.0, 3.0], np.float32)
    live = np.ones(6, bool)
    lm = cpu.local_max(src, conf, live, 0.6)
    assert lm.tolist() == [True, True, False, True, True, True]
    key = cpu.seed_keys(conf, lm)
    assert key.tolist() == [2.0, -1.0, 0.0, 3.0, 2.0, 3.0]
    # 3 and 5 tie at 3, 0 and 4 at 2; row 2 (suppressed, key 0) sorts before row 1 (a maximum of negative score)
    assert cpu.seed_order(key, live, 6).tolist() == [3, 5, 0, 4, 2, 1]


def test_nms_distance_is_the_fp32_expression_at_the_radius():
    R = np.float32(0.6)
    src = np.array([[0, 0, 0], [float(R), 0, 0], [np.nextafter(R, np.float32(0)), 5, 0], [0, 5, 0]], np.float32)
    conf = np.array([1.0, 2.0, 1.0, 2.0], np.float32)
    lm = cpu.local_max(src, conf, np.ones(4, bool), 0.6)
    assert lm.tolist() == [True, True, False, True]     # at exactly (float)R the neighbour does not suppress; one ulp inside it does


def test_self_is_dropped_by_index_not_by_position():
    c = cases.case(64, seed=3, dup=1)
    live = np.ones(64, bool)
    fn = cpu.normalize(c["feat"], live)
    i = int(np.argmax(np.where(c["inlier"], c["conf"], -np.inf)))
    j = (i + 1) % 64
    assert np.array_equal(c["feat"][i], c["feat"][j])
    nbr, val = cpu.knn(fn, live, np.array([i, j]), 40)
    assert nbr[0, 0] == j and nbr[1, 0] == i and i not in nbr[0] and j not in nbr[1] and abs(val[0, 0] - 1) < 1e-12


def test_k_is_capped_by_the_live_rows():
    c = cases.case(12, seed=1, inlier_ratio=1.0)
    r = cpu.solve(c["src"], c["tgt"], c["feat"], c["conf"], **cases.PARAMS)
    assert r["status"] == 0 and r["knn"].shape == (1, 11) and sorted(r["knn"][0].tolist() + [int(r["seeds"][0])]) == list(range(12))


@pytest.mark.parametrize("m", [0, 1, 5, 9])
def test_no_seed_is_status_2_and_the_identity(m):
    c = cases.case(m, seed=2) if m else dict(src=np.zeros((0, 3), np.float32), tgt=np.zeros((0, 3), np.float32), feat=np.zeros((0, 128), np.float32), conf=np.zeros(0, np.float32))
    r = cpu.solve(c["src"], c["tgt"], c["feat"], c["conf"], **cases.PARAMS)
    assert r["status"] == (2 if m else 1) and np.array_equal(r["T"], np.eye(4)) and not r["labels"].any() and r["n_seeds"] == 0


def test_dead_rows_are_never_seeds_neighbours_or_counted():
    c = cases.case(300, seed=4)
    best = int(np.argmax(c["conf"]))
    src, tgt, feat, conf = c["src"].copy(), c["tgt"].copy(), c["feat"].copy(), c["conf"].copy()
    dead = np.array([best, 7, 100, 299])
    src[best, 1] = np.nan; tgt[7, 0] = np.inf; conf[100] = -np.inf; feat[299, 127] = np.nan
    r = cpu.solve(src, tgt, feat, conf, **cases.PARAMS)
    assert r["dead"] == 4 and r["n_seeds"] == 29 and r["status"] == 0
    assert not np.isin(dead, r["seeds"]).any() and not np.isin(dead, r["knn"]).any() and not r["labels"][dead].any()
    keep = np.setdiff1d(np.arange(300), dead)
    q = cpu.solve(src[keep], tgt[keep], feat[keep], conf[keep], **cases.PARAMS)
    assert np.array_equal(keep[q["seeds"]], r["seeds"]) and np.array_equal(q["counts"], r["counts"]) and np.abs(q["T"] - r["T"]).max() < 1e-12


def test_plan_thresholds():
    """What tests/test_gpu_pdsc_solve.py states from the kernel's plan: the smallest m of two key chunks and of two seed blocks (ratio 0.1)."""
    ns = lambda m: cpu.n_seeds(m, 0.1)
    assert cpu.plan(ns(32), 32)["chunks"] == 1 and cpu.plan(ns(33), 33)["chunks"] == 2
    assert cpu.plan(ns(1289), 1289)["nsb"] == 1 and cpu.plan(ns(1290), 1290)["nsb"] == 2
    assert cpu.plan(3276, 32768) == dict(nsb=26, chunks=8, per=4096)
    for m in (0, 1, 33, 257, 1290, 12000, 32768):
        for s in (0, 1, ns(m), m):
            p = cpu.plan(s, m)
            assert p["chunks"] >= 1 and p["per"] % 32 == 0 and p["per"] * p["chunks"] >= m and p["per"] * (p["chunks"] - 1) < max(m, 1)
            assert p["nsb"] * p["chunks"] <= cpu.max_blocks(max(s, 1))
