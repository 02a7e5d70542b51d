"""The yardsticks of lr_nn3 / lr_refine_z without a GPU: the numpy restatement (tests/refine_z_cpu.py) against what the reference's own
refine_motion_Z_only returned (tests/golden/g18_refine_z.npz) and against scipy's k-d tree, the order of the two-level sum, the median,
the conditions on the golden inputs, the refusals that need no device, and the ABI mirrors."""
import ctypes
import os
import re

import numpy as np
import pytest

from lidarregistration_amd import _ext
from tests import refine_z_cases, refine_z_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g18_refine_z.npz"))
GOLDEN = refine_z_cases.golden_cases()
NN = refine_z_cases.nn_cases()
U = 2.0 ** -53


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def golden_bound(name):
    """40 n 2^-53 Zmax on dz: ten repeats x numerator and denominator x a margin of 2 (the reference sums pairwise, the contract in its
    fixed tree); repeat r (1-based) of the means gets r tenths of it."""
    return 40.0 * len(GOLDEN[name]["A"]) * U * float(GOLD[name + "/zmax"])


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_restatement_against_the_reference(name):
    p = GOLDEN[name]
    assert str(GOLD[name + "/sha256"]) == refine_z_cases.checksum(p["A"], p["B"], p["T"]), "tests/refine_z_cases.py changed: regenerate with tests/golden/make_golden_refine_z.py"
    r, trace = refine_z_cases.golden_trace(name)
    means, nvalid = GOLD[name + "/means"], GOLD[name + "/nvalid"]
    assert r["status"] == 0 and r["repeats"] == len(means) == len(trace)
    assert np.array_equal(trace[0]["ind"], GOLD[name + "/ind0"])
    assert [int(t["valid"].sum()) for t in trace] == nvalid.tolist() and r["n_valid"] == nvalid[-1]
    zmax = float(np.abs(trace[0]["z"][trace[0]["valid"]]).max())
    assert abs(zmax - float(GOLD[name + "/zmax"])) <= 1e-12 * zmax
    bound = golden_bound(name)
    print(f"{name}: |dz - dz_ref| = {abs(r['dz'] - float(GOLD[name + '/dz'])):.3e}, bound {bound:.3e}")
    for k, t in enumerate(trace):
        assert abs(t["mean"] - means[k]) <= bound * (k + 1) / 10.0, (k, t["mean"], means[k])
    assert abs(r["dz"] - float(GOLD[name + "/dz"])) <= bound
    assert r["last_step"] == trace[-1]["mean"]


def test_golden_covers_the_stop_and_the_full_loop():
    reps = {n: len(GOLD[n + "/means"]) for n in GOLDEN}
    assert reps["g_scan_3000"] == reps["g_scan_20000"] == 10 and reps["g_small_converges"] < 10
    assert abs(GOLD["g_small_converges/means"][-1]) < 1e-6 <= np.abs(GOLD["g_small_converges/means"][:-1]).min()
    assert (len(GOLDEN["g_scan_3000"]["A"]), len(GOLDEN["g_scan_3000"]["B"])) == (2783, 2819)
    assert abs(float(GOLD["g_scan_3000/dz"]) + 0.38) < 1e-3 and abs(float(GOLD["g_scan_20000/dz"]) + 0.371) < 1e-3


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_inputs_keep_their_distance_from_every_threshold(name):
    margins = refine_z_cases.check_conditions(GOLDEN[name], name)
    print(name, "margins: nn %.2e gate %.2e stop %.2e" % margins)
    assert min(margins) >= refine_z_cases.MIN_GAP


def _check_against_scipy(A, B):
    from scipy.spatial import cKDTree
    d, ind, info, d2nd = refine_z_cpu.nn(A, B, second=True)
    okA, okB = np.isfinite(A).all(axis=1), np.isfinite(B).all(axis=1)
    assert (info["n0_dropped"], info["n1_dropped"], info["status"]) == (int((~okA).sum()), int((~okB).sum()), int(not okB.any()))
    assert (ind[~okA] == -1).all() and np.isinf(d[~okA]).all()
    if not okB.any() or not okA.any():
        assert (ind == -1).all()
        return 0
    live = np.flatnonzero(okB)
    ds, js = cKDTree(B[live]).query(A[okA], k=1)
    clear = d2nd[okA] - d[okA] > 0
    assert np.array_equal(ind[okA][clear], live[js][clear])
    assert (np.abs(ds - d[okA]) <= np.spacing(d[okA])).all()                     # 1 ulp
    assert (d[okA] == np.sqrt(refine_z_cpu.d2_matrix(A[okA], B[ind[okA]]).diagonal())).all() if okA.sum() <= 2048 else True
    return int(clear.sum())


@pytest.mark.parametrize("group", ["sizes", "ties", "edges", "other"])
def test_brute_force_equals_scipy(group):
    """Equal ind wherever the nearest is strictly nearer than the second, equal d to 1 ulp, on every case."""
    pick = dict(sizes=lambda n: n.startswith("size_"), ties=lambda n: n.startswith(("ties", "dup", "same")),
                edges=lambda n: n.startswith(("far", "outside", "one_cell", "single", "line", "plane", "faces", "offset")))
    names = [n for n in sorted(NN) if (pick[group](n) if group in pick else not any(f(n) for f in pick.values()))]
    assert names
    clear = sum(_check_against_scipy(NN[n]["A"], NN[n]["B"]) for n in names)
    assert clear > 0 or group == "ties"
    if group == "other":
        for name in sorted(GOLDEN):
            p = GOLDEN[name]
            _check_against_scipy(refine_z_cpu.transform(p["A"], p["T"]), p["B"])


def test_nn_cases_are_what_they_claim():
    for name, p in NN.items():
        if "expect" in p:
            assert refine_z_cpu.nn(p["A"], p["B"])[1].tolist() == p["expect"], name
    # the lattice: 8 and 2 equally near targets, and the restatement picks the lowest index among them
    p = NN["ties_lattice_cell1.0"]
    M = refine_z_cpu.d2_matrix(p["A"], p["B"])
    ties = (M == M.min(axis=1, keepdims=True)).sum(axis=1)
    assert sorted(set(ties.tolist())) == [1, 2, 8] and (ties == 8).sum() == 125 and (ties == 2).sum() == 3 * 180
    _, ind, _ = refine_z_cpu.nn(p["A"], p["B"])
    assert all(ind[i] == np.flatnonzero(M[i] == M[i].min())[0] for i in range(len(ind)))
    # in cell-1 terms the winner lies in another cell than the query's for many of them
    own = (np.floor(p["B"][ind]) == np.floor(p["A"])).all(axis=1)
    assert 100 < (~own).sum() and own.sum() > 100
    far = NN["far_queries"]
    d, _, _ = refine_z_cpu.nn(far["A"], far["B"])
    assert (d[:140] > 900).all() and (d[140:] < 0.1).all()
    out = NN["outside_the_grid"]
    lo, hi = out["B"].min(axis=0), out["B"].max(axis=0)
    sides = {(a, s) for q in out["A"] for a in range(3) for s, beyond in ((-1, q[a] < lo[a]), (1, q[a] > hi[a])) if beyond}
    assert len(sides) == 6 and any(((q < lo) | (q > hi)).all() for q in out["A"])
    f = NN["faces_cell0.5"]
    q = f["A"] / 0.5
    assert sum(q[2 * k, k // 11] == np.floor(q[2 * k, k // 11]) and np.floor(q[2 * k + 1, k // 11]) == q[2 * k, k // 11] - 1 for k in range(33)) == 33
    nf = refine_z_cpu.nn(NN["nonfinite"]["A"], NN["nonfinite"]["B"])
    assert (nf[2]["n0_dropped"], nf[2]["n1_dropped"]) == (3, 4) and (nf[1] == -1).sum() == 3
    assert refine_z_cpu.nn(NN["all_targets_nonfinite"]["A"], NN["all_targets_nonfinite"]["B"])[2]["status"] == 1
    assert refine_z_cpu.nn(NN["nonfinite_nearest"]["A"], NN["nonfinite_nearest"]["B"])[1].min() >= 1


def test_refine_cases_are_what_they_claim():
    cases = refine_z_cases.refine_cases()
    seen = set()
    for name, p in cases.items():
        if "expect" not in p:
            continue
        r = refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], p["max_repeats"], p["min_change"])
        for k, v in p["expect"].items():
            assert r[k] == v, (name, k, r)
        seen.add(r["status"])
    assert seen == {0, 1, 2}
    trace = []
    p = cases["coincide_few"]
    r = refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], trace=trace)
    assert 50 < (trace[0]["z"][trace[0]["valid"]] == 0).sum() < 200 and np.isfinite(r["dz"]) and r["repeats"] > 1
    trace = []
    p = cases["on_the_gate"]
    refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], trace=trace)
    assert (trace[0]["xy"][1::2] == p["gate"]).all() and trace[0]["valid"][1::2].all() and not trace[0]["valid"][::2].any()
    assert [refine_z_cpu.refine_z(cases[f"scan_3000_reps{k}"]["A"], cases[f"scan_3000_reps{k}"]["B"], cases[f"scan_3000_reps{k}"]["T"],
                                  max_repeats=k)["repeats"] for k in (1, 2)] == [1, 2]


def test_two_level_sum_is_not_numpys_sum():
    """3000 terms of mixed magnitude: the fixed tree, numpy's pairwise sum and the plain left-to-right sum give three different doubles;
    the tree is the run sums (1024, 1024, 952 terms) summed in order."""
    rng = np.random.default_rng(3)
    t = rng.normal(size=3000) * 10.0 ** rng.uniform(-6, 6, size=3000)
    s = refine_z_cpu.two_level_sum(t)
    plain = 0.0
    for v in t:
        plain += v
    assert s != np.sum(t) and s != plain
    runs = []
    for k in range(0, 3000, 1024):
        a = 0.0
        for v in t[k:k + 1024]:
            a += v
        runs.append(a)
    assert s == (runs[0] + runs[1]) + runs[2]
    assert refine_z_cpu.two_level_sum(np.zeros(0)) == 0.0 and refine_z_cpu.two_level_sum(t[:5]) == (((t[0] + t[1]) + t[2]) + t[3]) + t[4]


def test_median():
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 4, 255, 256, 1001, 4096):
        w = 1.0 / np.abs(rng.normal(size=n))
        assert refine_z_cpu.median(w) == np.median(w)
    odd = np.array([3.0, 1.0, 2.0]); even = np.array([4.0, 1.0, 3.0, 2.0])
    assert refine_z_cpu.median(odd) == 2.0 and refine_z_cpu.median(even) == 2.5
    tied = np.array([1.0, 5.0, 5.0, 9.0]); tied_odd = np.array([5.0, 5.0, 5.0, 1.0, 9.0])
    assert refine_z_cpu.median(tied) == 5.0 and refine_z_cpu.median(tied_odd) == 5.0
    some_inf = np.array([1.0, np.inf, 2.0, np.inf, 3.0]); half_inf = np.array([1.0, np.inf, np.inf, 2.0])
    assert refine_z_cpu.median(some_inf) == 3.0 and refine_z_cpu.median(half_inf) == np.inf == np.median(half_inf)
    assert refine_z_cpu.median(np.array([0.0, 1e-310, 2e-310])) == 1e-310                  # subnormals order as integers too


def test_struct_mirrors_match_the_header():
    N, P, R = _ext.Nn3Params, _ext.RefineZParams, _ext.RefineZResult
    assert ctypes.sizeof(N) == 16 and N.struct_size.offset == 0 and N.cell.offset == 8
    assert ctypes.sizeof(P) == 32 and (P.max_repeats.offset, P.xy_gate.offset, P.min_change.offset, P.cell.offset) == (4, 8, 16, 24)
    assert ctypes.sizeof(R) == 40 and (R.status.offset, R.n_valid.offset, R.n1_dropped.offset, R.dz.offset, R.last_step.offset) == (0, 8, 16, 24, 32)
    n, p = N(), P()
    assert (n.struct_size, n.reserved, n.cell) == (16, 0, 0.0)
    assert (p.struct_size, p.max_repeats, p.xy_gate, p.min_change, p.cell) == (32, 10, 0.3, 1e-6, 0.0)
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    for struct, mirror in (("lr_nn3_params", N), ("lr_refine_z_params", P), ("lr_refine_z_result", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f[0] for f in mirror._fields_]
    exported = set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", hdr))
    assert exported == set(_ext.SYMBOLS) and len(_ext.SYMBOLS) == len(set(_ext.SYMBOLS))
    L = _ext.lib()
    assert all(hasattr(L, s) for s in _ext.SYMBOLS) and L.lr_version() == 103


def test_scratch_sizes():
    L = _ext.lib()
    ns = (0, 1, 255, 256, 257, 4097, 1 << 22)
    for fn in (L.lr_nn3_scratch_bytes, L.lr_refine_z_scratch_bytes):
        for sizes in ([fn(n, n) for n in ns], [fn(n, 7) for n in ns], [fn(7, n) for n in ns]):
            assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
        for a, b in ((-1, 5), (5, -1), ((1 << 22) + 1, 5), (5, (1 << 22) + 1)):
            assert fn(a, b) == 0
    assert all(L.lr_refine_z_scratch_bytes(n, n) > L.lr_nn3_scratch_bytes(n, n) for n in ns)


def test_refusals_come_before_any_device_call():
    """struct_size, the parameter ranges, the sizes, null pointers, short and misaligned scratch -- all before the first HIP call: safe
    without a device.  Every message names the argument."""
    L = _ext.lib()
    one, big = ctypes.c_void_p(256), 1 << 40
    err = lambda: L.lr_last_error().decode()

    def nn3(p, n0=10, n1=10, xyz0=one, xyz1=one, idx=one, dist=one, info=one, scratch=one, nbytes=big):
        return L.lr_nn3(xyz0, n0, xyz1, n1, ctypes.byref(p) if p is not None else None, idx, dist, info, scratch, nbytes, None)

    def rz(p, n0=10, n1=10, xyz0=one, xyz1=one, res=one, scratch=one, nbytes=big):
        return L.lr_refine_z(xyz0, n0, xyz1, n1, None, ctypes.byref(p) if p is not None else None, res, scratch, nbytes, None)
    p = _ext.Nn3Params(); p.struct_size = 8
    assert nn3(p) == -1 and "lr_nn3_params.struct_size is 8" in err()
    p = _ext.RefineZParams(); p.struct_size = 24
    assert rz(p) == -1 and "lr_refine_z_params.struct_size is 24" in err()
    assert nn3(None) == -1 and "params" in err() and rz(None) == -1 and "params" in err()
    for cell in (-1.0, float("inf"), float("nan")):
        assert nn3(_ext.Nn3Params(cell=cell)) == -1 and "cell" in err()
        assert rz(_ext.RefineZParams(cell=cell)) == -1 and "cell" in err()
    for kw, word in ((dict(xy_gate=0.0), "xy_gate"), (dict(xy_gate=-0.3), "xy_gate"), (dict(xy_gate=float("inf")), "xy_gate"), (dict(xy_gate=float("nan")), "xy_gate"),
                     (dict(min_change=-1e-9), "min_change"), (dict(min_change=float("inf")), "min_change"), (dict(min_change=float("nan")), "min_change"),
                     (dict(max_repeats=0), "max_repeats"), (dict(max_repeats=65), "max_repeats"), (dict(max_repeats=-1), "max_repeats")):
        assert rz(_ext.RefineZParams(**kw)) == -1 and word in err(), kw
    for call, p, out in ((nn3, _ext.Nn3Params(), "info"), (rz, _ext.RefineZParams(), "res")):
        for kw, word in ((dict(n0=-1), "n0"), (dict(n1=-1), "n1"), (dict(n0=(1 << 22) + 1), "n0"), (dict(n1=(1 << 22) + 1), "n1"), (dict(xyz0=None), "xyz0"),
                         (dict(xyz1=None), "xyz1"), ({out: None}, "null"), (dict(scratch=None), "scratch"), (dict(nbytes=1024), "scratch too small"),
                         (dict(scratch=ctypes.c_void_p(264)), "aligned")):
            assert call(p, **kw) == -1 and word in err(), (call.__name__, kw)
    assert nn3(_ext.Nn3Params(), idx=None) == -1 and "idx" in err() and nn3(_ext.Nn3Params(), dist=None) == -1 and "dist" in err()
    # (n == 0 needs no point array: it gets as far as the device check, which a machine without a GPU answers with an error of its own)


def test_refine_motion_still_refuses_the_flag():
    from lidarregistration_amd import overlap
    with pytest.raises(NotImplementedError, match="refine_GT"):
        overlap.refine_motion(np.eye(4), np.zeros((3, 3)), np.zeros((3, 3)), refine_GT_Z_only=True)
    for name in ("nearest_neighbour", "nearest_neighbour_dev", "refine_motion_Z_only", "refine_GT", "refine_session", "refine_z_dev"):
        assert callable(getattr(overlap, name))
