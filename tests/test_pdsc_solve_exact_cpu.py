"""The yardstick of tests/test_gpu_pdsc_solve_exact.py proved before the device is held to it: the contract's own arithmetic of
tests/pdsc_solve_cpu.py (solve_contract and its stages) and the builders of tests/pdsc_solve_exact_cases.py.  No GPU.

  * fmaf32 against libm's fmaf where the result is a subnormal float32, half-ulp ties of the subnormal grid included;
  * solve_contract against the recording of the reference's tail within the bounds tests/test_pdsc_solve_cpu.py uses for the fp32
    yardstick (0.5 .. 2 x the reference's own fp32-vs-fp64 deviation), and with the fp64 restatement's seeds, counts and best seed;
  * the lattice premise: the chain and the matmul give the same similarities, and the whole tail the same bits;
  * every builder's conditions at every size the GPU file uses, and the kNN plans of those sizes.
"""
import ctypes
import ctypes.util

import numpy as np
import pytest

from tests import pdsc_solve_cases as cases
from tests import pdsc_solve_cpu as cpu
from tests import pdsc_solve_exact_cases as ex
from tests.conftest import golden
from tests.fcgf_cpu import fmaf32

NAMES = [c[0] for c in cases.GOLDEN]
P = cases.PARAMS


@pytest.fixture(scope="module")
def g26():
    return golden("g26_pdsc_solve.npz")


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name in NAMES:
        c = cases.golden_case(name)
        a = (c["src"], c["tgt"], c["feat"], c["conf"])
        out[name] = (c, cpu.solve(*a, **P), cpu.solve_contract(*a, **P))
    return out


# ---- fmaf32 ---------------------------------------------------------------------------------------------------------------------------------
def test_fmaf32_is_libm_fmaf_on_subnormal_results():
    """Round to odd in fp64, then one narrowing: correctly rounded on the subnormals' grid of 2^-149 too, ties to even."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    u = 2.0 ** -149
    tiny = float(np.finfo(np.float32).tiny)
    abc = []
    # a b = (1/4, 1/2, 3/4) ulp of the subnormal grid, on an even and an odd multiple c of it, both signs: the half-ulp ties go to even
    for a, b in ((2.0 ** -75, 2.0 ** -76), (2.0 ** -75, 2.0 ** -75), (3 * 2.0 ** -76, 2.0 ** -75), (5 * 2.0 ** -77, 2.0 ** -75)):
        for n in (0, 1, 2, 3, 1000, 1001, 2 ** 22, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1):
            for sa in (1.0, -1.0):
                for sc in (1.0, -1.0):
                    abc.append((sa * a, b, sc * n * u))
    # a tie whose exact sum needs more than 53 bits: c normal, a b = half an ulp of the SUBNORMAL result after cancellation
    abc += [(1.0 + 2.0 ** -23, tiny, -tiny), (1.0 - 2.0 ** -24, tiny, -tiny), (1.5, 3 * u, -4 * u), (0.5, 3 * u, 0.0), (0.5, u, 0.0), (0.5, -u, 0.0)]
    rng = np.random.default_rng(17)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-80, -60, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-80, -60, n)).astype(np.float32)
    c = (rng.integers(-2 ** 12, 2 ** 12, n) * u).astype(np.float32)
    abc += list(zip(a.tolist(), b.tolist(), c.tolist()))
    a, b, c = (np.array(x, np.float32) for x in zip(*abc))
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    got = fmaf32(a, b, c)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    sub = (want != 0) & (np.abs(want) < np.float32(tiny))
    exact = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)          # (exact here: the three lie within 53 bits of each other)
    ties = np.abs(np.abs(exact / u) % 1.0 - 0.5) == 0
    assert sub.sum() > 3000 and ties.sum() >= 40
    assert (np.abs(got[ties].astype(np.float64) / u) % 2 == 0).all()                       # to even


# ---- the chain restatement against the recording and the fp64 restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_contract_decides_as_the_fp64_restatement(solved, name):
    """The same seeds, counts and best seed on the golden cases; the same neighbour sets on >= 95 % of the seeds."""
    c, r64, r = solved[name]
    assert r["status"] == r64["status"] == 0 and np.array_equal(r["seeds"], r64["seeds"])
    assert np.array_equal(r["counts"], r64["counts"]) and r["best_rank"] == r64["best_rank"] and r["best_index"] == r64["best_index"]
    assert np.array_equal(r["labels"], r64["labels"]) and r["n_labels"] == r["best_count"] == r64["best_count"] and r["refine_rounds"] == r64["refine_rounds"]
    same = np.array([set(a) == set(b) for a, b in zip(r["knn"], r64["knn"])])
    assert same.mean() >= 0.95
    assert r["weights"].dtype == np.float32 and r["knn"].dtype == np.int64 and r["seed_T"].dtype == np.float64


@pytest.mark.parametrize("name", ("m257", "m1000", "m3000"))
def test_contract_is_a_yardstick_against_the_recording(g26, solved, name):
    """The chain restatement deviates from fp64 as the reference's own fp32 run does: 0.5 .. 2 x on the seed transforms (the bound of
    test_pdsc_solve_cpu.test_fp32_restatement_is_a_yardstick), and stays within the recording's bounds of tests/test_gpu_pdsc_solve.py."""
    c, r64, r = solved[name]
    assert str(g26[name + "/sha256"]) == cases.checksum(c)
    same = np.array([set(a) == set(b) for a, b in zip(r["knn"], r64["knn"])])
    ratio = np.abs(r["seed_T"] - r64["seed_T"])[same].max() / float(g26[name + "/dev_seed_T"])
    print(name, "chain restatement / reference's deviation", ratio)
    assert 0.5 <= ratio <= 2.0
    rec_seeds = g26[name + "/seeds"].astype(np.int64)
    row = {int(s): i for i, s in enumerate(r["seeds"])}
    at = np.array([row[int(s)] for s in rec_seeds])
    rule = lambda yard, ref: max(4 * yard, 16 * 2.0 ** -23 * float(np.abs(ref).max(initial=0.0)))
    kp = g26[name + "/knn"].shape[1]
    eq = np.array([set(a) == set(b) for a, b in zip(g26[name + "/knn"], r["knn"][at][:, :kp])])
    order = lambda w_, k_: np.stack([a[np.argsort(b)] for a, b in zip(w_, k_)])
    dw = np.abs(order(g26[name + "/weights"][eq], g26[name + "/knn"][eq]) - order(r["weights"][at][eq], r["knn"][at][eq])).max()
    dT = np.abs(g26[name + "/seed_T"][eq] - r["seed_T"][at][eq]).max()
    assert eq.mean() >= 0.95 and dw <= rule(float(g26[name + "/dev_weights"]), g26[name + "/weights"]) and dT <= rule(float(g26[name + "/dev_seed_T"]), g26[name + "/seed_T"])
    assert np.abs(g26[name + "/T"] - r["T"]).max() <= rule(float(g26[name + "/dev_T"]), g26[name + "/T"])


def test_stages_in_the_contracts_association_are_the_fp64_stages(solved):
    """S7 - S9 as the kernels associate them against the numpy forms (SVD Kabsch, einsum residuals) on the same inputs."""
    c, r64, r = solved["m257"]
    src, tgt, live = c["src"], c["tgt"], r["live"]
    Ts = cpu.seed_transforms(src, tgt, r["knn"], r["weights"])
    assert np.abs(Ts - r["seed_T"]).max() < 1e-9
    assert np.abs(cpu.resid_contract(r["seed_T"], src, tgt) - cpu.residuals(r["seed_T"], src, tgt)).max() < 1e-12
    assert cpu.resid_contract(r["T"], src, tgt).shape == (257,)
    T, rounds = cpu.refine(r["T_best"], src, tgt, live, P["refine_threshold"], P["refine_iters"])
    assert rounds == r["refine_rounds"] and np.abs(T - r["T"]).max() < 1e-12


def test_butterfly_is_normalize32s():
    rng = np.random.default_rng(3)
    f = rng.standard_normal((16, 128)).astype(np.float32)
    p = f[:, 0::2] * f[:, 0::2] + f[:, 1::2] * f[:, 1::2]
    den = np.maximum(np.sqrt(cpu.butterfly64(p)), np.float32(1e-12))
    assert np.array_equal(cpu.normalize32(f, np.ones(16, bool)), f / den[:, None])


# ---- the lattice premise -----------------------------------------------------------------------------------------------------------------------
def test_lattice_chain_is_the_matmul():
    c = ex.lattice(257)
    a = (c["src"], c["tgt"], c["feat"], c["conf"])
    live = np.ones(257, bool)
    fn = cpu.normalize32(c["feat"], live)
    seeds = cpu.pick_seeds(c["src"], c["conf"], live, P["nms_radius"], P["ratio"])
    assert np.array_equal(cpu.sims_chain(fn, seeds), cpu.sims_exact(fn, seeds))
    assert np.array_equal(cpu.sims_chain(fn[:, ::-1].copy(), seeds), cpu.sims_exact(fn, seeds))         # another order of the channels
    chain, exact = cpu.solve_contract(*a, **P), cpu.solve_contract(*a, lattice=True, **P)
    for k in ("seeds", "knn", "weights", "seed_T", "counts", "T_best", "T", "labels"):
        assert chain[k].tobytes() == exact[k].tobytes(), k
    # the partition on the integer key is the stable order
    s = cpu.sims_exact(fn, seeds)
    assert np.array_equal(cpu.knn_contract(s, live, seeds, 40, grid=ex.GRID), cpu.knn_contract(s, live, seeds, 40))


# ---- the builders' conditions at every size the GPU file uses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(257,), (1290,), (4127,), (8192, 0, 1.0, 8), (8200, 0, 1.0, 8), (32768,)], ids=lambda a: f"m{a[0]}")
def test_lattice_conditions(args):
    """lattice() asserts them; what it measured is printed (DESIGN.md §17.3 records it)."""
    c = ex.lattice(*args)
    g = c["measured"]
    print(args, g)
    assert g["tie_kth"] >= 0.9 and (g["plan"]["chunks"] == 1 or g["crossing"] >= 1) and g["tied_pairs"] >= 4
    assert np.isin(np.count_nonzero(c["feat"], axis=1), [4, 16, 64]).all()
    dup = len(c["feat"]) - len(np.unique(c["feat"], axis=0))
    assert dup >= 0.05 * c["m"]          # about 10 % of the rows are given another row's feature (rows of four entries also coincide by chance)


def test_other_builders_conditions():
    z = ex.zero_feature_seed()
    assert z["measured"]["tie_kth"] >= 0.9 and not z["feat"][z["zero_row"]].any()
    c = ex.crafted_s2()
    assert c["m"] == ex.CRAFTED_M and c["crafted"] == [253, 254, 255, 256, 258, 511, 512, 513, 600, 700]
    assert {i // 256 for i in c["crafted"]} == {0, 1, 2}
    s = ex.subnormal_weights()
    print("subnormal weights", s["measured"])
    assert s["measured"]["subnormal"] >= 1 and s["measured"]["new_zeros"] >= 1
    r = ex.refine_rounds()
    print("refine rounds", r["measured"])
    full = cpu.solve_contract(r["src"], r["tgt"], r["feat"], r["conf"], **dict(P, refine_threshold=ex.REFINE_THRESHOLD))
    cap = cpu.solve_contract(r["src"], r["tgt"], r["feat"], r["conf"], **dict(P, refine_threshold=ex.REFINE_THRESHOLD, refine_iters=2))
    assert full["refine_rounds"] == r["measured"]["rounds"] >= 4 and cap["refine_rounds"] == 2 and cap["T"].tobytes() != full["T"].tobytes()
    zm = ex.zero_matrix()
    assert not zm["contract"]["weights"].any() and np.array_equal(zm["contract"]["T_best"], np.eye(4))


@pytest.mark.parametrize("m, ratio, nsb, chunks, per", [(224, 0.1, 1, 7, 32), (225, 0.1, 1, 8, 32), (1290, 0.1, 2, 7, 192), (4127, 0.1, 4, 8, 544),
                                                        (8192, 1.0, 64, 8, 1024), (8200, 1.0, 65, 7, 1184), (32768, 0.1, 26, 8, 4096)])
def test_plans_of_the_sizes(m, ratio, nsb, chunks, per):
    assert cpu.plan(cpu.n_seeds(m, ratio), m) == dict(nsb=nsb, chunks=chunks, per=per)
