"""The numpy restatement of contract Y (tests/symicp_cpu.py) against independent arithmetic, its statuses and its accuracy on the scan
pair, and what lr_symicp / lr_normals2 refuse without a device."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

from lidarregistration_amd import _ext, synth
from tests import bbrf_cases, bbrf_cpu, large_cases, overlap_cpu, refine_z_cpu, symicp_cases, symicp_cpu
from tests.conftest import rot_diff_rad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LOOP = symicp_cases.loop_cases()
BOUNDARY = symicp_cases.boundary_cases()


def run(p, **kw):
    return symicp_cpu.symicp(p["A"], p["nA"], p["B"], p["nB"], T_init=p.get("T_init"), **p["params"], **kw)


@pytest.mark.parametrize("seed", range(6))
def test_solve_against_numpy(seed):
    """Bound: Cholesky's backward error is |dH| <= g(3n+1) |L||L^T| (Higham, Accuracy and Stability, thm 10.4), so its relative forward
    error is at most n (3n + 1) u cond2(H) = 114 u cond; LAPACK's LU with partial pivoting adds at most 3 n^3 u cond = 648 u cond at a
    growth factor of 1 (thm 9.5).  Together 762 u cond2(H), taken as 768."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(40, 6)) * 10.0 ** rng.uniform(-2, 2, size=6)
    H, g = C.T @ C, C.T @ rng.normal(size=40)
    st, x, piv = symicp_cpu.cholesky_solve(H.tolist(), g.tolist(), 1e-12)
    want = np.linalg.solve(H, g)
    assert st == 0 and len(piv) == 6 and all(d > 0 for d in piv)
    bound = 768.0 * U * np.linalg.cond(H)
    assert np.linalg.norm(np.array(x, float) - want) <= bound * np.linalg.norm(want), (np.linalg.norm(np.array(x, float) - want) / np.linalg.norm(want), bound)
    # only the upper triangle is read
    Hu = np.triu(H) + np.tril(np.full((6, 6), np.nan), -1)
    assert [float(v) for v in symicp_cpu.cholesky_solve(Hu.tolist(), g.tolist(), 1e-12)[1]] == [float(v) for v in x]


def test_pivot_rule():
    H = np.diag([4.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    assert symicp_cpu.cholesky_solve(H.tolist(), [8.0, 1, 1, 1, 1, 1], 1e-9)[1][0] == 2.0
    H[2, 2] = 0.0
    st, x, piv = symicp_cpu.cholesky_solve(H.tolist(), [1.0] * 6, 1e-9)
    assert (st, x, piv) == (2, None, [4.0, 1.0, 0.0])                                         # 0 > eps 0 fails: detected, not solved
    H[2, 2] = math.nan
    assert symicp_cpu.cholesky_solve(H.tolist(), [1.0] * 6, 1e-9)[0] == 2
    H[2, 2] = 1.0; H[0, 1] = H[1, 0] = 2.0                                                     # d_1 = 1 - 1 = 0
    assert symicp_cpu.cholesky_solve(H.tolist(), [1.0] * 6, 1e-9)[::2] == (2, [4.0, 0.0])
    H[1, 1] = 1.0 + 1e-8                                                                        # d_1 = 1e-8 > 1e-9 H_11
    assert symicp_cpu.cholesky_solve(H.tolist(), [1.0] * 6, 1e-9)[0] == 0
    assert symicp_cpu.cholesky_solve(H.tolist(), [1.0] * 6, 1e-7)[0] == 2


def test_split_rotation_against_rodrigues():
    """R is the rotation about a by atan |a|: against cos, sin of the library's atan to a few ulp; R R^T - I; dW = R R by twice the angle."""
    rng = np.random.default_rng(3)
    for mag in (0.0, 1e-9, 1e-4, 0.01, 0.3, 1.0, 7.0):
        a = rng.normal(size=3); a *= mag / np.linalg.norm(a)
        c, R, aa = symicp_cpu.half_rotation(a)
        R = np.array(R, float)
        th = math.atan(np.linalg.norm(a))
        u = a / np.linalg.norm(a) if mag else np.zeros(3)
        K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
        want = math.cos(th) * np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * np.outer(u, u)
        assert np.abs(R - want).max() <= 8 * U, (mag, np.abs(R - want).max())
        assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * U
        assert abs(float(c) - math.cos(th)) <= 2 * U and float(aa) == float((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        W2 = math.cos(2 * th) * np.eye(3) + math.sin(2 * th) * K + (1.0 - math.cos(2 * th)) * np.outer(u, u)
        assert np.abs(np.array(bbrf_cpu.mat3(R.tolist(), R.tolist())) - W2).max() <= 16 * U


def slow_tree(t):
    """Y4 spelt out with Python floats, independent of numpy's reshapes."""
    total = 0.0
    for s in range(0, len(t), 1024):
        v = []
        for lane in range(64):
            acc = 0.0
            for x in t[s + 16 * lane:s + 16 * lane + 16]:
                acc = acc + float(x)
            v.append(acc)
        h = 32
        while h >= 1:
            for lane in range(h):
                v[lane] = v[lane] + v[lane + h]
            h //= 2
        total = total + v[0]
    return total


@pytest.mark.parametrize("n", (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049, 3000))
def test_sum_tree(n):
    rng = np.random.default_rng(n)
    t = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)
    got = float(symicp_cpu.tree_sum(t))
    assert got == slow_tree(t)
    assert abs(got - math.fsum(t)) <= n * U * math.fsum(np.abs(t))
    two = symicp_cpu.tree_sum(np.stack([t, -t], axis=1))
    assert two[0] == got and two[1] == -got
    if n == 3000:          # the order is the tree's own: neither the running sum nor Z6's two-level sum
        assert len({got, float(np.cumsum(t)[-1]), float(refine_z_cpu.two_level_sum(t))}) == 3


def test_cross_product_and_rows():
    rng = np.random.default_rng(5)
    Uv, V = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    assert np.abs(symicp_cpu.cross3(Uv, V) - np.cross(Uv, V)).max() <= 4 * U * 10
    p = BOUNDARY["dot_signs"]
    i = np.arange(len(p["A"]))
    rows, ok = symicp_cpu.rows(p["A"], p["nA"], p["B"], p["nB"], i, i, 0.6, 0.0)
    assert ok.all()
    n = p["nA"][-3:] + np.array([1.0, -1.0, 1.0])[:, None] * p["nB"][-3:]                       # s = +1, -1 and +1 at a zero product
    assert np.array_equal(rows[-3:, 15], n[:, 0] * n[:, 0])                                     # c_3 c_3 = n_x n_x
    assert np.array_equal(rows[-3:, 20], n[:, 2] * n[:, 2])                                     # c_5 c_5 = n_z n_z
    d = p["B"][-3:] - p["A"][-3:]
    assert np.array_equal(rows[-3:, 27], bbrf_cpu.dot3(d, n) ** 2)


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_acceptance_boundaries(name):
    p = BOUNDARY[name]
    trace = []
    r, log = run(p, trace=trace)
    assert log[0, 0] == p["expect"]["pairs0"] == r["n_pairs"] and r["status"] == 0
    if name == "backward_only":
        f, rr = trace[0]["f"], trace[0]["r"]
        assert rr[12] == 0 and f[0] == 0 and np.array_equal(f, np.arange(12)) and np.array_equal(rr[:12], np.arange(12))


def test_statuses_and_stops():
    for name in ("five_pairs", "plane_z_normals", "step_overflows", "same"):
        p = LOOP[name]
        trace = []
        r, log = run(p, trace=trace)
        for k, v in p["expect"].items():
            assert (log[0, 0] if k == "pairs0" else r[k]) == v, (name, k)
        assert not log[r["iters_run"]:].any() and np.isfinite(r["B_to_A"]).all()
        if r["status"]:
            assert np.array_equal(r["B_to_A"], np.eye(4)) and r["converged"] == 0 and not log[0, 2:].any()      # the pose stays
        if name == "plane_z_normals":
            assert trace[0]["piv"][2] == 0.0 and len(trace[0]["piv"]) == 3                      # exactly singular: detected, not solved
        if name == "step_overflows":
            assert trace[0]["x"] is not None and not np.isfinite(trace[0]["x"]).all() and log[0, 1] == np.inf
        if name == "same":
            assert np.array_equal(r["T"], np.eye(4)) and log[0, 2] == 0.0 and log[0, 3] == 0.0 and log[0, 1] == 0.0
    r, log = run(LOOP["iters_50"])
    assert r["iters_run"] == 50 and r["converged"] == 0 and r["status"] == 0 and log[:, 0].all()
    r, _ = run(LOOP["nonfinite"])
    assert r["status"] == 0 and np.isfinite(r["T"]).all() and r["n_pairs"] > 100


def test_planted_motion_is_recovered():
    p = LOOP["planted"]
    r, log = run(p)
    assert r["status"] == 0 and r["converged"] == 1 and 1 < r["iters_run"] < p["params"]["n_iter"]
    M = p["truth"]
    assert np.abs(r["B_to_A"] - M).max() <= 1e-9 and np.abs(r["T"] @ M - np.eye(4)).max() <= 1e-9
    assert r["mean_sq"] <= 1e-18


def test_t_init_equals_a_moved_cloud_at_iteration_0():
    p = LOOP["t_init"]
    M = p["T_init"]
    r, log = run(p)
    Bm, nBm = symicp_cpu.move(p["B"], p["nB"], M[:3, :3].tolist(), M[:3, 3].tolist())
    r2, log2 = symicp_cpu.symicp(p["A"], p["nA"], Bm, nBm, **p["params"])
    assert np.array_equal(log[0, :2], log2[0, :2]) and log[0, 0] > 200                           # the same B', pairs and residual
    assert np.abs(r["B_to_A"] - r2["B_to_A"] @ M).max() <= 1e-12


def test_struct_mirrors_match_the_header():
    P, R = _ext.SymicpParams, _ext.SymicpResult
    assert ctypes.sizeof(P) == 64 and (P.struct_size.offset, P.n_iter.offset, P.max_dist.offset, P.min_cos.offset, P.eps_rot.offset, P.eps_trans.offset,
                                       P.piv_eps.offset, P.cell.offset, P.T_init.offset) == (0, 4, 8, 16, 24, 32, 40, 48, 56)
    assert ctypes.sizeof(R) == 280 and (R.T.offset, R.B_to_A.offset, R.status.offset, R.iters_run.offset, R.converged.offset, R.n_pairs.offset,
                                        R.mean_sq.offset) == (0, 128, 256, 260, 264, 268, 272)
    p = P()
    d = symicp_cpu.DEFAULTS
    assert (p.struct_size, p.n_iter, p.max_dist, p.min_cos, p.eps_rot, p.eps_trans, p.piv_eps, p.cell, p.T_init) == \
        (64, d["n_iter"], d["max_dist"], d["min_cos"], d["eps_rot"], d["eps_trans"], d["piv_eps"], 0.0, None)
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    for struct, mirror in (("lr_symicp_params", P), ("lr_symicp_result", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f[0] for f in mirror._fields_]
    L = _ext.lib()
    assert all(hasattr(L, s) for s in ("lr_symicp_scratch_bytes", "lr_symicp", "lr_normals2")) and L.lr_version() == 103
    from lidarregistration_amd import bbrf, symicp
    for name in ("normals_counted", "symicp_dev", "symmetric_icp"):
        assert callable(getattr(symicp, name))
    nd = symicp_cpu.NORMAL_DEFAULTS
    assert (symicp.NORMAL_RADIUS, symicp.NORMAL_MAX_NN, symicp.MIN_NB) == (nd["normal_radius"], nd["max_nn"], nd["min_nb"])
    import inspect
    assert inspect.signature(bbrf.refinement_sample).parameters["symmetric"].default is False


# the constants tests/test_bbrf_cpu.py pins (read there from a build of the commit before lr_nn3.h was shared), and lr_bbrf's / lr_normals'
# own sizes as the parent of this file's commit returned them
NS = (0, 1, 257, 4097, 30000, 4194304)
PARENT_SIZES = {"lr_nn3_scratch_bytes": (17920, 17920, 26112, 198400, 1441280, 201392896),
                "lr_refine_z_scratch_bytes": (27392, 27392, 46848, 388096, 2770432, 386016256)}


def test_scratch_sizes():
    from tests import test_bbrf_cpu
    assert PARENT_SIZES == test_bbrf_cpu.PARENT_SIZES and NS == test_bbrf_cpu.NS
    L = _ext.lib()
    for fn, want in PARENT_SIZES.items():
        assert tuple(getattr(L, fn)(n, n) for n in NS) == want
    for n in NS:
        assert L.lr_normals_scratch_bytes(n) == L.lr_nn3_scratch_bytes(n, n)                    # lr_normals2 takes lr_normals' scratch
        m = max(n, 1)
        own = 1024 + 2 * _al(m * 24) + 2 * _al(m * 4) + _al((2 * (m // 1024) + 2) * 256)
        assert L.lr_symicp_scratch_bytes(n, n) == own + 2 * L.lr_nn3_scratch_bytes(n, n)
        assert L.lr_bbrf_scratch_bytes(n, n, 100) == 1024 + 2 * _al(m * 24) + 2 * _al(m * 4) + _al((m // 1024 + 1) * 64) + 2 * L.lr_nn3_scratch_bytes(n, n)
    sizes = [L.lr_symicp_scratch_bytes(n, 7) for n in NS]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    for a in ((-1, 5), (5, -1), ((1 << 22) + 1, 5), (5, (1 << 22) + 1)):
        assert L.lr_symicp_scratch_bytes(*a) == 0


def _al(x):
    return (x + 255) & ~255


def test_refusals_come_before_any_device_call():
    """struct_size, the parameter ranges, the sizes, null pointers, short and misaligned scratch -- all before the first HIP call: safe
    without a device.  Every message names the argument."""
    L = _ext.lib()
    one, big = ctypes.c_void_p(256), 1 << 40
    err = lambda: L.lr_last_error().decode()
    nan, inf = float("nan"), float("inf")

    def sy(p, n0=10, n1=10, xyzA=one, nrmA=one, xyzB=one, nrmB=one, res=one, log=one, scratch=one, nbytes=big):
        return L.lr_symicp(xyzA, nrmA, n0, xyzB, nrmB, n1, ctypes.byref(p) if p is not None else None, res, log, scratch, nbytes, None)

    def nm(n=10, xyz=one, radius=0.01, max_nn=13, out=one, cnt=one, info=one, scratch=one, nbytes=big):
        return L.lr_normals2(xyz, n, radius, max_nn, out, cnt, info, scratch, nbytes, None)
    p = _ext.SymicpParams(); p.struct_size = 56
    assert sy(p) == -1 and "lr_symicp_params.struct_size is 56" in err()
    assert sy(None) == -1 and "params" in err()
    for kw, word in ((dict(n_iter=0), "n_iter"), (dict(n_iter=1001), "n_iter"), (dict(n_iter=-1), "n_iter"),
                     (dict(max_dist=0.0), "max_dist"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=inf), "max_dist"), (dict(max_dist=nan), "max_dist"),
                     (dict(min_cos=-0.1), "min_cos"), (dict(min_cos=1.0001), "min_cos"), (dict(min_cos=nan), "min_cos"),
                     (dict(eps_rot=0.0), "eps_rot"), (dict(eps_rot=-1.0), "eps_rot"), (dict(eps_rot=inf), "eps_rot"), (dict(eps_rot=nan), "eps_rot"),
                     (dict(eps_trans=0.0), "eps_trans"), (dict(eps_trans=inf), "eps_trans"), (dict(eps_trans=nan), "eps_trans"),
                     (dict(piv_eps=0.0), "piv_eps"), (dict(piv_eps=-1e-9), "piv_eps"), (dict(piv_eps=inf), "piv_eps"), (dict(piv_eps=nan), "piv_eps"),
                     (dict(cell=-1.0), "cell"), (dict(cell=inf), "cell"), (dict(cell=nan), "cell")):
        assert sy(_ext.SymicpParams(**kw)) == -1 and word in err() and err().startswith("lr_symicp:"), kw
    for kw, word in ((dict(n0=-1), "n0"), (dict(n1=-1), "n1"), (dict(n0=(1 << 22) + 1), "n0"), (dict(n1=(1 << 22) + 1), "n1"), (dict(xyzA=None), "xyzA"),
                     (dict(nrmA=None), "nrmA"), (dict(xyzB=None), "xyzB"), (dict(nrmB=None), "nrmB"), (dict(res=None), "result"),
                     (dict(scratch=None), "scratch"), (dict(nbytes=1024), "scratch too small"), (dict(scratch=ctypes.c_void_p(264)), "aligned")):
        assert sy(_ext.SymicpParams(), **kw) == -1 and word in err(), kw
    assert sy(_ext.SymicpParams(min_cos=0.0), nbytes=1024) == -1 and "scratch too small" in err()       # 0 and 1 are legal
    assert sy(_ext.SymicpParams(min_cos=1.0), nbytes=1024) == -1 and "scratch too small" in err()
    for kw, word in ((dict(radius=0.0), "radius"), (dict(radius=nan), "radius"), (dict(max_nn=0), "max_nn"), (dict(max_nn=33), "max_nn"),
                     (dict(n=-1), "n must"), (dict(n=(1 << 22) + 1), "n must"), (dict(xyz=None), "xyz"), (dict(out=None), "normals_out"),
                     (dict(info=None), "info"), (dict(scratch=None), "scratch"), (dict(nbytes=1024), "scratch too small"),
                     (dict(scratch=ctypes.c_void_p(264)), "aligned")):
        assert nm(**kw) == -1 and word in err() and err().startswith("lr_normals2:"), kw
    assert nm(cnt=None, nbytes=1024) == -1 and "scratch too small" in err()                       # a null count is legal


def test_neighbour_counts_of_the_restatement():
    for name, p in symicp_cases.normals_cases().items():
        nrm, cnt = symicp_cpu.normals_counted(p["X"], p["radius"], p["max_nn"])
        want, info = bbrf_cpu.normals(p["X"], p["radius"], p["max_nn"])
        ok = np.isfinite(p["X"]).all(axis=1) if len(p["X"]) else np.zeros(0, bool)
        assert np.array_equal(nrm, want) and cnt.dtype == np.int32 and (cnt[~ok] == 0).all() and (cnt[ok] >= 1).all() and (cnt <= p["max_nn"]).all()
        assert int(((cnt < 3) & ok).sum()) == info["n_default"]
    p = symicp_cases.normals_cases()["scan_counts"]
    cnt = symicp_cpu.normals_counted(p["X"], p["radius"], p["max_nn"])[1]
    assert cnt.max() == p["max_nn"] and cnt.min() < 3 and len(set(cnt.tolist())) >= 6
    # a horizontal patch yields exactly (0, 0, 1), as the default does: only the count tells them apart
    flat = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [50.0, 0.0, 0.0]])
    nrm, cnt = symicp_cpu.normals_counted(flat, 2.0, 13)
    assert np.array_equal(nrm, bbrf_cases.z_normals(5)) and cnt.tolist() == [4, 4, 4, 4, 1]


# ---- accuracy at the chosen defaults ------------------------------------------------------------------------------------------------------
STARTS = {"0.8deg_5cm": (0.8, 0.05), "3deg_0.5m": (3.0, 0.5)}


@functools.lru_cache(maxsize=None)
def accuracy_pair():
    """synth.make_scan_pair(30000, 30000) down-sampled at 0.3, normals and counts at the defaults (neighbour lists from a k-d tree plus the
    contract's (d2, index) sort, as tests/large_cases.py), points below min_nb dropped: (a, na, b, nb, T)."""
    A0, B0, T = synth.make_scan_pair(30000, 30000)
    nd = symicp_cpu.NORMAL_DEFAULTS
    out = []
    for X in (A0, B0):
        x = overlap_cpu.voxel_mean(X, 0.3)["cent"]
        nrm, cnt = symicp_cpu.normals_counted(x, nd["normal_radius"], nd["max_nn"], nbrs=large_cases.ball_neighbours(x, nd["normal_radius"], nd["max_nn"]))
        out += [x[cnt >= nd["min_nb"]], nrm[cnt >= nd["min_nb"]]]
    return (*out, T)


def pose_errors(M, truth):
    return float(np.linalg.norm(M[:3, 3] - truth[:3, 3])), math.degrees(rot_diff_rad(M, truth))


@pytest.mark.parametrize("start", sorted(STARTS))
def test_accuracy_against_point_to_point_icp(start):
    """From both starts the restatement at the defaults is no worse, in translation and in rotation, than a point-to-point ICP from the
    same start on the same clouds at the same distance.  Measured (te m / re deg), symmetric against point-to-point:
    0.8 deg / 5 cm: 0.0060 / 0.0120 against 0.0546 / 0.0287; 3 deg / 0.5 m: 0.0499 / 0.0186 against 0.3528 / 0.0845."""
    a, na, b, nb, T = accuracy_pair()
    off = bbrf_cases.small_motion(71, *STARTS[start])
    M = off @ T                                                     # cloud 0 under the true motion, off by `off`: the truth B -> A is `off`
    A = overlap_cpu.transform(a, M)
    nA = bbrf_cpu.rot3(M[:3, :3].tolist(), na)
    d = symicp_cpu.DEFAULTS
    r, log = symicp_cpu.symicp(A, nA, b, nb, search=refine_z_cpu.nn_tree, **d)
    te, re = pose_errors(r["B_to_A"], off)
    P = symicp_cpu.icp_p2p(A, b, n_iter=d["n_iter"], max_dist=d["max_dist"], eps_rot=d["eps_rot"], eps_trans=d["eps_trans"], search=refine_z_cpu.nn_tree)
    pte, pre = pose_errors(P, off)
    print(f"{start}: symmetric te {te:.4f} re {re:.4f} iters {r['iters_run']} converged {r['converged']} pairs {r['n_pairs']}; point-to-point te {pte:.4f} re {pre:.4f}")
    assert r["status"] == 0 and te <= pte and re <= pre
