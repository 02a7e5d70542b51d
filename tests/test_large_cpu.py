"""The yardsticks of the tests past 65 536 points per cloud (tests/test_gpu_large.py) without a GPU: the k-d-tree search nn_tree against
the brute-force nn on every nearest-neighbour case the suite has, the threshold every case of tests/large_cases.py is named for, what
each case claims about itself, and the restatement against the reference's recorded run at full size
(tests/golden/g20_refine_z_large.npz)."""
import os

import numpy as np
import pytest

from tests import bbrf_cases, bbrf_cpu, large_cases, overlap_cpu, refine_z_cases, refine_z_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g20_refine_z_large.npz"))
NN = refine_z_cases.nn_cases()
LARGE_NN = large_cases.nn_cases()
TH = large_cases.THRESHOLDS
G = large_cases.GOLDEN_NAME


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def tree_equals_brute(A, B):
    """nn_tree == nn in idx, the bits of dist and of the second distance, and info.  Returns the number of queries nn_tree handed to nn."""
    st = {}
    want, got = refine_z_cpu.nn(A, B, second=True), refine_z_cpu.nn_tree(A, B, second=True, stats=st)
    plain = refine_z_cpu.nn_tree(A, B)
    assert got[2] == want[2] == plain[2]
    assert np.array_equal(got[1], want[1]) and np.array_equal(plain[1], want[1]) and got[1].dtype == want[1].dtype
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(plain[0]), bits(want[0]))
    assert np.array_equal(bits(got[3]), bits(want[3]))
    return st["fallback"]


@pytest.mark.parametrize("group", ["sizes", "ties", "edges", "other"])
def test_nn_tree_equals_brute_force_on_the_existing_cases(group):
    pick = dict(sizes=lambda n: n.startswith("size_"), ties=lambda n: n.startswith(("ties", "dup", "same")),
                edges=lambda n: n.startswith(("far", "outside", "one_cell", "single", "line", "plane", "faces", "offset")))
    names = [n for n in sorted(NN) if (pick[group](n) if group in pick else not any(f(n) for f in pick.values()))]
    assert names
    fell = {n: tree_equals_brute(NN[n]["A"], NN[n]["B"]) for n in names}
    if group == "ties":                                  # where the lowest index decides, the decision is the brute-force search's own
        lattice = [n for n in names if n.startswith("ties_lattice")]
        assert len(lattice) == 4 and all(fell[n] >= 125 + 3 * 180 for n in lattice) and fell["duplicates"] == 65
        assert fell["same_point_twice"] == 65            # fewer than TREE_K live targets: every query
    if group == "other":
        assert fell["scan_3000"] == 0                    # and on a scan the tree serves every query
        assert "nonfinite" in names and "all_targets_nonfinite" in names and fell["all_targets_nonfinite"] == 0


@pytest.mark.parametrize("name", sorted(LARGE_NN))
def test_nn_tree_equals_brute_force_on_the_large_cases(name):
    """The full-size scan pair is 5.6e9 distances for the brute-force search, too many for a test: there every 16th query (and the last
    64) is compared, against the whole target; every other case in full."""
    p = LARGE_NN[name]
    A = p["A"]
    if p.get("tree"):
        A = np.concatenate([A[::16], A[-64:]])
    tree_equals_brute(A, p["B"])
    if p.get("tree"):
        d, ind, _ = refine_z_cpu.nn_tree(p["A"], p["B"])
        part = refine_z_cpu.nn_tree(A, p["B"])
        assert np.array_equal(np.concatenate([ind[::16], ind[-64:]]), part[1]) and np.array_equal(bits(np.concatenate([d[::16], d[-64:]])), bits(part[0]))


def test_search_argument_changes_nothing():
    """refine_z and bbrf over nn_tree return what they return over nn."""
    p = refine_z_cases.refine_cases()["scan_3000_reps10"]
    assert refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], search=refine_z_cpu.nn_tree) == refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"])
    for name in ("ties_lattice", "nonfinite", "run_2049_gap"):
        p = bbrf_cases.loop_cases()[name]
        a, alog = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], **p["params"])
        b, blog = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], search=refine_z_cpu.nn_tree, **p["params"])
        assert np.array_equal(bits(alog), bits(blog)) and all(np.array_equal(a[k], b[k]) for k in a)


# ---- every case crosses the threshold it is named for (computed from the sizes, not read from the library) --------------------------------
def test_cloud_cases_cross_their_thresholds():
    C = large_cases.cloud_cases()
    rows = {}
    for name, (X, voxel, T) in C.items():
        r = overlap_cpu.voxel_mean(X, voxel, T)
        rows[name] = r["rows"]
        if large_cases.expect_rows(name) is not None:
            assert r["rows"] == large_cases.expect_rows(name), name
        assert r["status"] == 0 and r["dropped"] == (2 if "nan" in name else 0)
    for kind in ("own_cell", "own_cell_nan", "one_cell"):
        assert [TH["three_passes"](len(C[f"{kind}_{n}"][0])) for n in large_cases.EDGE] == [False, True, True]
    assert [TH["third_digit"](rows[f"own_cell_{n}"]) for n in large_cases.EDGE] == [False, False, True]          # row 65 536 exists at 65 537 only
    assert TH["three_passes"](70001) and TH["blocks_before"](70001) and not TH["third_digit"](rows["few_cells_70001"])
    assert not TH["blocks_before"](65537) and TH["blocks_before"](65793)                                          # (block 257 begins at point 65 792)
    assert (rows["scan_a_v0.3"], rows["scan_b_v0.3"]) == (75199, 74958)
    assert all(TH["third_digit"](rows[f"scan_{c}_v0.3"]) and TH["blocks_before"](len(C[f"scan_{c}_v0.3"][0])) for c in "ab")
    assert all(TH["three_passes"](len(C[f"scan_{c}_v1.0"][0])) and not TH["third_digit"](rows[f"scan_{c}_v1.0"]) for c in "ab")
    # the dropped points sit in the middle and at the end, and every row lies in front of them in the sort
    for n in large_cases.EDGE:
        X = C[f"own_cell_nan_{n}"][0]
        assert np.flatnonzero(~np.isfinite(X).all(axis=1)).tolist() == [n // 2, n - 1]
    # few_cells: shuffled -- the points of a cell are not consecutive
    r = overlap_cpu.voxel_mean(*C["few_cells_70001"])
    assert r["counts"].min() >= 100 and (np.diff(r["row_of"]) != 0).mean() > 0.99


@pytest.mark.parametrize("n", large_cases.EDGE)
def test_one_cell_sum_depends_on_the_order(n):
    """One n-point segment: its left-to-right sum differs from the right-to-left one, and the restatement's centroid is the former."""
    X, voxel, T = large_cases.cloud_cases()[f"one_cell_{n}"]
    r = overlap_cpu.voxel_mean(X, voxel, T)
    fwd, rev = np.zeros(3), np.zeros(3)
    for p in X:
        fwd += p
    for p in X[::-1]:
        rev += p
    assert (bits(fwd) != bits(rev)).any() and np.array_equal(bits(fwd / float(n)), bits(r["cent"][0])) and r["counts"].tolist() == [n]


def test_pair_cases_cross_their_thresholds():
    for name, p in large_cases.pair_cases().items():
        r = overlap_cpu.overlap(p["A"], p["B"], p["T"], p["voxel"], p["radius"])
        assert r["status"] == 0 and 0.5 < r["frac_sym"] <= r["frac"] < 1.0
        assert TH["three_passes"](len(p["A"])) and TH["blocks_before"](len(p["A"]))
        assert TH["third_digit"](min(r["n0_ds"], r["n1_ds"])) == (p["voxel"] == 0.3)
    batch = large_cases.batch_pairs()
    assert tuple((len(p["A"]), len(p["B"])) for p in batch) == large_cases.BATCH_SIZES == ((70001, 257), (257, 70001), (0, 65536), (257, 257))
    assert TH["three_passes"](max(max(len(p["A"]), len(p["B"])) for p in batch)) and not TH["three_passes"](257) and 257 >= 256     # 257 alone: two passes
    assert any(p["T"] is not None for p in batch) and any(p["T"] is None for p in batch)
    want = [overlap_cpu.overlap(p["A"], p["B"], p["T"], p["voxel"], p["radius"]) for p in batch]
    assert [w["status"] for w in want] == [0, 0, 1, 0] and all(0 < w["n_overlap"] for w in want if w["status"] == 0)


def test_nn_cases_cross_their_thresholds():
    c = LARGE_NN
    for n1 in (65537, 70001):
        p = c[f"grid_257_{n1}"]
        assert (len(p["A"]), len(p["B"])) == (257, n1) and TH["init_rounds"](n1)
    assert not TH["init_rounds"](65536) and not TH["blocks_before"](65537) and TH["blocks_before"](70001)
    for n0 in (65537, 70001):
        p = c[f"blocks_{n0}_1025"]
        assert (len(p["A"]), len(p["B"])) == (n0, 1025) and large_cases.cdiv(n0, 256) > 256
        mid = p["middle"]
        assert mid.min() < 256 and mid.max() == n0 - 1 and (mid >= 65536).any() and len(set(mid.tolist())) == len(mid)
        open_at = stays_open(p["A"], p["B"], mid)
        assert open_at == [True, True, False], n0
    mid = c["blocks_70001_1025"]["middle"]
    assert set(range(257, large_cases.cdiv(70001, 256))) <= set((mid // 256).tolist())       # an open query in every block that needs the second round
    p = c["scan"]
    assert (len(p["A"]), len(p["B"])) == (75199, 74958) and TH["init_rounds"](74958) and TH["blocks_before"](75199) and TH["blocks_before"](74958)


def stays_open(A, B, mid):
    """By the code a query stays open when the shells 0 .. 3 around its cell hold no target point and do not cover the grid.  For the
    automatic cell, a quarter of it and four times it: True when no target point lies within 3.5 cells (Chebyshev) of any query of rows
    `mid` and none in a cell less than 4 cell indices away (every such query stays open); False when the shells around every one of
    them cover the grid (none stays open); anything else fails."""
    assert np.array_equal(B.min(axis=0), np.zeros(3)) and np.array_equal(B.max(axis=0), np.full(3, 100.0))       # the box begins at the origin
    auto = refine_z_cases.auto_cell(B)
    cheb = np.abs(A[mid][:, None, :] - B[None, :, :]).max(axis=2).min(axis=1)       # Chebyshev distance to the nearest target point
    out = []
    for cell in (0.0, 0.25 * auto, 4.0 * auto):
        e, dim = large_cases.grid_of(B, cell)
        ca, cb = np.floor(A[mid] / e).astype(int), np.floor(B / e).astype(int)
        covered = bool((ca.max(axis=0) - large_cases.SHELL_CAP <= 0).all() and (ca.min(axis=0) + large_cases.SHELL_CAP >= dim - 1).all())
        if cheb.min() > 3.5 * e:
            gap = np.abs(ca[:, None, :] - cb[None, :, :]).max(axis=2).min(axis=1)
            assert gap.min() > large_cases.SHELL_CAP and not covered
            out.append(True)
        else:
            assert covered and dim.max() <= 3
            out.append(False)
    return out


def test_far_rounds_geometry():
    """At the automatic cell and at a quarter of it (which the rule doubles back to the automatic one: 46^3 cells exceed the table) every
    middle query stays open.  At four times the automatic cell the grid has 3 cells per axis and shell 1 around the centre covers it
    -- a 100 m box leaves no room for 3.5 such cells --: no query is open there, the case then only pins the result."""
    p = LARGE_NN["far_rounds"]
    A, B, mid = p["A"], p["B"], p["middle"]
    assert len(B) == 1025 and len(mid) == 8193 + 257 and len(A) == len(mid) + 257 and TH["far_rounds"](len(mid))
    assert stays_open(A, B, mid) == [True, True, False]
    assert (np.abs(A[mid] - 50.0) <= 1.0).all()
    assert (np.abs(np.delete(A, mid, axis=0)[:, None, :] - B[None, :, :]).max(axis=2).min(axis=1) < 0.5).all()    # the others sit inside the clusters


def test_refine_cases_cross_their_thresholds():
    c = large_cases.refine_cases()
    assert [large_cases.cdiv(len(c[f"lifted_{n}"]["A"]), 1024) for n in (65537, 66561)] == [65, 66]
    for name, p in c.items():
        assert TH["runs"](len(p["A"])), name
        r, trace = large_cases.refine_trace(name)
        for k, v in p.get("expect", {}).items():
            assert r[k] == v, (name, k, r)
    assert not TH["runs"](65536)
    # two_pairs: in every repeat the valid pairs are source 0 (run 0) and source 65 536 (run 64), nothing else
    r, trace = large_cases.refine_trace("two_pairs")
    p = c["two_pairs"]
    assert (len(p["A"]), len(p["B"])) == (65537, 1025) and r["repeats"] == 10 and r["n_valid"] == 2 and r["status"] == 0
    assert all(np.flatnonzero(t["valid"]).tolist() == [0, 65536] for t in trace) and 65536 // 1024 == 64
    assert all((t["xy"][1:-1] > 0.35).all() for t in trace)
    one = refine_z_cpu.refine_z(p["A"][:-1], p["B"], search=refine_z_cpu.nn_tree)                   # without the pair of run 64: another dz
    assert one["n_valid"] == 1 and one["dz"] != r["dz"]
    r, trace = large_cases.refine_trace("scan")
    assert r["repeats"] == 10 and abs(r["dz"] + refine_z_cases.Z_OFF) < 1e-3 and min(int(t["valid"].sum()) for t in trace) > 40000
    assert np.flatnonzero(trace[0]["valid"]).max() >= 65536


def test_bbrf_and_normals_cases_cross_their_thresholds():
    c = large_cases.bbrf_cases_large()
    assert [(len(p["A"]), len(p["B"])) for p in c.values()] == [(65537, 1025), (1025, 65537), (75199, 74958), (75199, 74958)]
    assert all(p["params"] == dict(n_iter=3) for p in c.values())
    for name in ("bb_65537_1025", "scan_z", "scan_generic"):
        assert TH["runs"](len(c[name]["A"]))
    assert TH["init_rounds"](65537) and not TH["runs"](1025)
    for name, p in c.items():
        trace = []
        r, log = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], trace=trace, search=refine_z_cpu.nn_tree, **p["params"])
        assert r["status"] == 0 and r["iters_run"] == 3 and (log[:, 7] > 1000).all(), name
        pairs = np.flatnonzero(trace[0]["keep"])
        if TH["runs"](len(p["A"])):                                                                 # pairs in run 0 and in run 64
            assert (pairs < 1024).any() and (pairs >= 65536).any(), name
    assert np.array_equal(c["scan_z"]["nA"], bbrf_cases.z_normals(75199)) and not np.array_equal(c["scan_generic"]["nA"], c["scan_z"]["nA"])
    n = large_cases.normals_case()
    assert len(n["X"]) == 74958 and TH["blocks_before"](74958) and (n["radius"], n["max_nn"]) == (0.6, 13)


def test_ball_neighbours_are_the_contracts():
    """The neighbour lists handed to the normals' restatement at full size equal bbrf_cpu.neighbours where that one is affordable, ties
    at the cut and non-finite points included."""
    cases = bbrf_cases.normals_cases()
    for name in ("size_1025", "ties_at_cut", "many_candidates", "nonfinite", "exactly_3", "all_default", "all_nonfinite"):
        p = cases[name]
        got, want = large_cases.ball_neighbours(p["X"], p["radius"], p["max_nn"]), bbrf_cpu.neighbours(p["X"], p["radius"], p["max_nn"])
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), name
    p = large_cases.normals_case()
    nb = large_cases.ball_neighbours(p["X"], p["radius"], p["max_nn"])
    sizes = np.bincount([len(x) for x in nb], minlength=14)
    assert sizes[0] == 0 and sizes[1:3].sum() > 1000 and sizes[13] > 1000 and sizes[3:13].min() > 1000      # defaults, full lists and every length between


# ---- the golden pair at full size -----------------------------------------------------------------------------------------------------
def test_restatement_against_the_reference_at_full_size():
    """The bound of tests/test_refine_z_cpu.py, 40 n 2^-53 Zmax on dz (repeat r of the means: r tenths of it); equal valid counts; the
    first repeat's indices equal by their hash."""
    p = large_cases.golden_case()
    assert str(GOLD[G + "/sha256"]) == refine_z_cases.checksum(p["A"], p["B"], p["T"]), "regenerate with tests/golden/make_golden_refine_z.py large"
    r, trace = large_cases.golden_trace()
    means, nvalid = GOLD[G + "/means"], GOLD[G + "/nvalid"]
    assert r["status"] == 0 and r["repeats"] == len(means) == len(trace) == 10
    assert large_cases.index_hash(trace[0]["ind"]) == str(GOLD[G + "/ind0_sha256"])
    assert [int(t["valid"].sum()) for t in trace] == nvalid.tolist() and r["n_valid"] == nvalid[-1]
    zmax = float(np.abs(trace[0]["z"][trace[0]["valid"]]).max())
    assert abs(zmax - float(GOLD[G + "/zmax"])) <= 1e-12 * zmax
    bound = 40.0 * len(p["A"]) * 2.0 ** -53 * float(GOLD[G + "/zmax"])
    print(f"{G}: |dz - dz_ref| = {abs(r['dz'] - float(GOLD[G + '/dz'])):.3e}, bound {bound:.3e}")
    for k, t in enumerate(trace):
        assert abs(t["mean"] - means[k]) <= bound * (k + 1) / 10.0, (k, t["mean"], means[k])
    assert abs(r["dz"] - float(GOLD[G + "/dz"])) <= bound
    assert sorted(GOLD.files) == sorted(G + "/" + k for k in ("dz", "means", "nvalid", "zmax", "sha256", "ind0_sha256"))


def test_golden_inputs_keep_their_distance_from_every_threshold_at_full_size():
    margins = refine_z_cases.check_conditions(large_cases.golden_case(), G, trace=large_cases.golden_trace()[1])
    print(G, "margins: nn %.2e gate %.2e stop %.2e" % margins)
    assert min(margins) >= refine_z_cases.MIN_GAP
