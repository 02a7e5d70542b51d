"""lr_sm / lr_sm_batch (csrc/lr_sm.hip) on the GPU where tests/test_gpu_sm.py stops: above one 1 024-entry selection pass and up to the
accepted maximum of 32 768 correspondences, with iterations / inlier_threshold / top_ratio varied, null outputs, batches of 64, one large
pair beside small ones, live counts in a batch and a guard band behind the scratch.  Cases: sm_cases.large_cases().  References: the
closed form for planted line sets (sm_cpu.planted_v), the recorded fp64 eigenvectors of tests/golden/g23_sm_large.npz (and, on
gap_8193_409, what the reference's own SM() returned), the numpy restatement computed on the fly for the small cases."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import sm_cases, sm_cpu
from tests.test_gpu_sm import _bytes, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = sm_cases.large_cases()
PLANTED = [c["name"] for c in LARGE if c["kind"] == "planted"]
RECORDED = [c["name"] for c in LARGE if c.get("large")]


@pytest.fixture(scope="module")
def S():
    import torch
    from lidarregistration_amd import _ext, sm
    _ext.build()
    assert torch.cuda.is_available()
    return sm


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "g23_sm_large.npz"))


def check_transform(c, out, unique_fit=None):
    """test_gpu_sm.test_transform's checks of one call: weight_sum, a proper rotation, and the fp64 weighted Kabsch over the call's OWN
    labels and eig (<= 1e-9 / 1e-8 m) -- or, on a collinear selection, its weighted residual."""
    T, info, labels, eig = out
    w = eig.astype(np.float64) * labels
    assert info["status"] == 0 and abs(info["weight_sum"] - w.sum()) <= 1e-12 * max(1.0, w.sum())
    R = T[:3, :3]
    assert np.isfinite(T).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    Tk = sm_cpu.kabsch_weighted(c["a"], c["b"], w)
    if c["unique_fit"] if unique_fit is None else unique_fit:
        dr, dt = sm_cpu.rot_dist(T, Tk), sm_cpu.trans_dist(T, Tk)
        print(f"{c['name']}: vs fp64 weighted Kabsch over the call's own labels and eig: |dR|_F {dr:.2e}, |dt| {dt:.2e} m")
        assert dr <= 1e-9 and dt <= 1e-8
    else:
        use = w > 0
        A, B = c["a"][use].astype(np.float64), c["b"][use].astype(np.float64)
        res = np.sqrt((w[use] * (((A @ R.T + T[:3, 3]) - B) ** 2).sum(1)).sum())
        ref = np.sqrt((w[use] * (((A @ Tk[:3, :3].T + Tk[:3, 3]) - B) ** 2).sum(1)).sum())
        assert res <= ref + 1e-6


def check_scratch_independence(S, c, first, **kw):
    for poison in (0x00, 0xFF):
        assert _bytes(S.sm_dev(c["a"], c["b"], top_ratio=c["ratio"], poison=poison, **kw)) == _bytes(first), (c["name"], poison)


# ---- planted sets above one selection pass: closed-form reference -------------------------------------------------------------------
@pytest.mark.parametrize("name", PLANTED)
def test_planted(S, name):
    c = sm_cases.by_name(name)
    out = T, info, labels, eig = run(S, name)
    v = sm_cpu.planted_v(len(c["a"]), c["pairs"])
    err = float(np.abs(eig.astype(np.float64) - v).max())
    print(f"{name}: |v_gpu - v_closed-form|_inf = {err:.3e} ({err / max(v.max(), 1e-300):.2e} of max v)")
    assert err <= 1e-6 * v.max()
    assert not eig[v == 0].any() and (eig[v > 0] > 0).all() and len(set(eig[v > 0])) <= 1          # exact zeros elsewhere; the ties are ties
    assert tuple(np.flatnonzero(labels)) == c["expect_sel"] and set(np.unique(labels)) <= {0, 1}
    assert info["K"] == c["K"] == int(labels.sum()) and info["m"] == len(c["a"])
    if c["pairs"]:
        check_transform(c, out)
    else:
        assert info["status"] == 1 and info["weight_sum"] == 0.0 and np.array_equal(T, np.eye(4))
    check_scratch_independence(S, c, out)


# ---- full-size random cases: recorded fp64 eigenvector -----------------------------------------------------------------------------
def recorded_tol(name):
    """max(16 x the recorded |v_fp32-restatement - v_fp64|_inf, 1e-6 max v), the rule of test_gpu_sm.eig_tol: (tol, d32, max v)."""
    g = gold()
    d32, vmax = float(g[name + "/d32"]), float(g[name + "/v"].max())
    return max(16.0 * d32, 1e-6 * vmax), d32, vmax


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_eigenvector(S, name):
    """Measured on the MI355X (256 CUs), |eig - v_fp64|_inf of max v and the share of the factor 16 used: 4.27e-7 (0.96) at 8 193,
    7.64e-7 (1.71) at 20 001, 1.48e-6 (3.04) at 32 768, where a lane's fp32 sum runs over 8 192 terms in sequence."""
    c = sm_cases.by_name(name)
    assert str(gold()[name + "/sha256"]) == sm_cases.checksum(c)
    _, info, _, eig = run(S, name)
    v = gold()[name + "/v"]
    tol, d32, vmax = recorded_tol(name)
    err = float(np.abs(eig.astype(np.float64) - v).max())
    print(f"{name}: |v_gpu - v_fp64|_inf = {err:.3e} ({err / vmax:.2e} of max v), fp32 restatement {d32 / vmax:.2e}: {err / d32:.2f} of the factor 16 used; "
          f"plan at 256 CUs {sm_cpu.plan(len(v))}, restatement in that order {float(gold()[name + '/d32_seq256']) / vmax:.2e}")
    assert np.isfinite(eig).all() and (eig >= 0).all() and info["m"] == len(v)
    assert err <= tol


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_labels(S, name):
    c, g = sm_cases.by_name(name), gold()
    _, info, labels, eig = run(S, name)
    v, K = g[name + "/v"], int(g[name + "/K"])
    assert set(np.unique(labels)) <= {0, 1} and int(labels.sum()) == info["K"] == K == sm_cpu.top_k(len(c["a"]), c["ratio"]) and info["status"] == 0
    assert np.array_equal(np.flatnonzero(labels), sm_cpu.select(eig, K))      # the K largest of the call's OWN eig under the tie rule
    want = np.zeros(len(v), np.uint8); want[sm_cpu.select(v, K)] = 1
    diff = np.flatnonzero(labels != want)
    print(f"{name}: {len(diff)} labels differ from the fp64 restatement's")
    if len(diff):
        tol = recorded_tol(name)[0]
        cut = np.sort(v)[::-1][K - 1]
        assert (np.abs(v[diff] - cut) <= tol).all(), (name, diff, v[diff] - cut, tol)
    if c["kind"] == "gap":
        assert np.array_equal(labels, np.unpackbits(g[name + "/labels"])[:len(labels)])       # the reference's own SM()


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_transform(S, name):
    c = sm_cases.by_name(name)
    out = run(S, name)
    check_transform(c, out)
    if c["kind"] == "gap":
        Tg = gold()[name + "/T"].astype(np.float64)
        da, dt = sm_cpu.rot_angle(out[0], Tg), sm_cpu.trans_dist(out[0], Tg)
        print(f"{name}: vs the reference's SM(): {da:.2e} rad, {dt:.2e} m")
        assert da <= 1e-4 and dt <= 1e-3


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_scratch_independence(S, name):
    check_scratch_independence(S, sm_cases.by_name(name), run(S, name))


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compat_of(name, thr, dtype_name):
    c = sm_cases.by_name(name)
    C = sm_cpu.compat(c["a"], c["b"], thr, np.dtype(dtype_name).type)
    C.setflags(write=False)
    return C


def check_eig(name, eig, thr, iterations):
    """The rule of test_gpu_sm.eig_tol against the restatement at these parameters, fp64 and fp32."""
    v64 = sm_cpu.power(compat_of(name, thr, "float64"), iterations)
    v32 = sm_cpu.power(compat_of(name, thr, "float32"), iterations)
    tol = max(16.0 * float(np.abs(v32.astype(np.float64) - v64).max()), 1e-6 * float(v64.max()))
    err = float(np.abs(eig.astype(np.float64) - v64).max())
    print(f"{name} thr {thr} iterations {iterations}: |v_gpu - v_fp64|_inf = {err:.3e}, tol {tol:.3e}")
    assert np.isfinite(eig).all() and (eig >= 0).all() and err <= tol
    return v64


@pytest.mark.parametrize("name,iterations", [("cluster_1000_300", 1), ("cluster_1000_300", 2), ("cluster_1000_300", 37), ("ragged_65", 1000)])
def test_iterations(S, name, iterations):
    c = sm_cases.by_name(name)
    T, info, labels, eig = out = S.sm_dev(c["a"], c["b"], top_ratio=c["ratio"], inlier_threshold=c["thr"], iterations=iterations)
    assert (eig != -1.0).all()                           # eig_out is written after the LAST iteration, also when it is the first
    check_eig(name, eig, c["thr"], iterations)
    assert np.array_equal(np.flatnonzero(labels), sm_cpu.select(eig, info["K"])) and info["K"] == sm_cpu.top_k(len(c["a"]), c["ratio"])
    check_transform(c, out)


@pytest.mark.parametrize("thr", [0.1, 0.3, 2.0])
def test_inlier_threshold(S, thr):
    c = sm_cases.by_name("cluster_1000_300")
    T, info, labels, eig = out = S.sm_dev(c["a"], c["b"], top_ratio=c["ratio"], inlier_threshold=thr)
    check_eig(c["name"], eig, thr, 10)
    assert np.array_equal(np.flatnonzero(labels), sm_cpu.select(eig, info["K"]))
    check_transform(c, out)


def test_top_ratio_one(S):
    """K = M: everything is selected, so the fit meets every entry of weight 0 -- on planted_nonfinite three with non-finite coordinates,
    which are not read."""
    c = sm_cases.by_name("cluster_1000_300")
    T, info, labels, eig = out = S.sm_dev(c["a"], c["b"], top_ratio=1.0)
    assert info["K"] == 1000 and labels.all() and np.array_equal(eig, run(S, c["name"])[3])
    check_transform(c, out)
    c = sm_cases.by_name("planted_nonfinite")
    T, info, labels, eig = out = S.sm_dev(c["a"], c["b"], top_ratio=1.0)
    bad = list(c["bad"])
    assert info["K"] == 200 and labels.all() and not eig[bad].any() and np.count_nonzero(eig) > 100
    check_transform(c, out)                               # (kabsch_weighted reads the entries of positive weight only)
    rest = np.ones(200, bool); rest[bad] = False
    Tr = sm_cpu.kabsch_weighted(c["a"][rest], c["b"][rest], eig[rest].astype(np.float64))
    assert sm_cpu.rot_dist(T, Tr) <= 1e-9 and sm_cpu.trans_dist(T, Tr) <= 1e-8


@pytest.mark.parametrize("name,K", [("kcut_100_0.29", 28), ("kcut_60_0.05", 3), ("kcut_59_0.05", 2), ("kcut_30_0.1", 3), ("kcut_20_0.1", 2)])
def test_device_side_k(S, name, K):
    """Rows padded to 200, the live count on the device: K = (int)((double)m * top_ratio) is formed there, and everything is what the
    call on the live rows alone returns (every order of summation follows the live count)."""
    import torch
    c = sm_cases.by_name(name)
    m = len(c["a"])
    fill = sm_cases.synth(200 - m, 50, 77)
    a, b = np.concatenate([c["a"], fill[0]]), np.concatenate([c["b"], fill[1]])
    md = torch.tensor([m], dtype=torch.int32, device="cuda")
    T, info, labels, eig = S.sm_dev(a, b, m_dev=md, top_ratio=c["ratio"])
    T0, info0, labels0, eig0 = run(S, name)
    assert info["K"] == K == c["K"] and info["m"] == m and info["status"] == sm_cpu.reference(name)["status"] == (1 if K < 3 else 0)
    assert info == info0 and np.array_equal(T, T0) and len(eig) == 200
    assert np.array_equal(labels[:m], labels0) and np.array_equal(eig[:m], eig0) and not labels[m:].any() and not eig[m:].any()


def raw_single(c, eig=True, labels=True, guard=0, fill=0xC3):
    """lr_sm through ctypes with nullable outputs and `guard` bytes behind the scratch whose exact size is passed: (result struct bytes,
    eig, labels, the guard bytes after the call)."""
    import torch
    from lidarregistration_amd import _ext
    L = _ext.lib()
    a, b = torch.from_numpy(c["a"]).cuda(), torch.from_numpy(c["b"]).cuda()
    m = len(c["a"])
    need = L.lr_sm_scratch_bytes(m)
    scratch = torch.full((need + guard,), fill, dtype=torch.uint8, device="cuda")
    res = torch.zeros(ctypes.sizeof(_ext.SmResult), dtype=torch.uint8, device="cuda")
    e = torch.full((m,), -1.0, dtype=torch.float32, device="cuda") if eig else None
    lab = torch.full((m,), 255, dtype=torch.uint8, device="cuda") if labels else None
    p = _ext.SmParams(top_ratio=c["ratio"], inlier_threshold=c["thr"])
    rc = L.lr_sm(a.data_ptr(), b.data_ptr(), m, None, ctypes.byref(p), res.data_ptr(), e.data_ptr() if eig else None, lab.data_ptr() if labels else None,
                 scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.lr_last_error()
    torch.cuda.synchronize()
    return res.cpu().numpy().tobytes(), None if e is None else e.cpu().numpy(), None if lab is None else lab.cpu().numpy(), scratch[need:].cpu().numpy()


def test_null_outputs(S):
    """eig_out null, labels_out null, both null: the result struct is byte for byte the full call's, and the output that is asked for too."""
    import torch
    from lidarregistration_amd import corrset
    c = sm_cases.by_name("ragged_257")
    full, e0, l0, _ = raw_single(c)
    T0, info0, labels0, eig0 = run(S, "ragged_257")
    assert np.array_equal(e0, eig0) and np.array_equal(l0, labels0) and info0["status"] == 0
    r, e, lab, _ = raw_single(c, eig=False)
    assert r == full and e is None and np.array_equal(lab, l0)
    r, e, lab, _ = raw_single(c, labels=False)
    assert r == full and lab is None and np.array_equal(e, e0)
    assert raw_single(c, eig=False, labels=False)[0] == full
    call = corrset.BatchCall(S.SOLVER, [c["a"]], [c["b"]], outputs=False, top_ratio=c["ratio"])      # ... and through the batched entry point
    call.launch(torch.cuda.current_stream().cuda_stream)
    assert call.res.cpu().numpy().tobytes() == full and call.outs == [None, None]
    (T, info), = call.results()
    assert np.array_equal(T, T0) and info == info0


# ---- batches: byte for byte the single calls ----------------------------------------------------------------------------------------
def test_batch_of_64(S):
    """LR_MAX_BATCH pairs: what sm_setup_kernel's 64 threads and the by-value descriptor table are sized for."""
    sizes = (3, 60, 63, 64, 65, 257, 999, 2049)
    names = [f"ragged_{sizes[k % 8]}" for k in range(62)]
    names.insert(17, None)                               # an M = 0 pair
    names.insert(40, "planted_equal_at_cut")
    assert len(names) == 64
    cs = [None if n is None else sm_cases.by_name(n) for n in names]
    assert {c["ratio"] for c in cs if c} == {0.1}
    empty = np.zeros((0, 3), np.float32)
    out, _ = S.sm_batch_dev([empty if c is None else c["a"] for c in cs], [empty if c is None else c["b"] for c in cs], top_ratio=0.1, poison=0xFF)
    assert len(out) == 64
    for k, (n, o) in enumerate(zip(names, out)):
        if n is None:
            assert np.array_equal(o[0], np.eye(4)) and o[1] == dict(status=1, K=0, m=0, weight_sum=0.0) and len(o[2]) == 0
        else:
            assert _bytes(o) == _bytes(run(S, n)), (k, n)


def test_one_large_pair_beside_small_ones(S):
    """One pair of 20 001 sets mx, the arena stride and the launch grid; the small pairs beside it run under them and still return what
    their own single calls do.  Once per ratio of the picked cases (a call has one top_ratio), every pair in both batches."""
    pick = ["full_20001", "ragged_65", "planted_ties_3100_k310", "ragged_3"]
    cs = [sm_cases.by_name(n) for n in pick]
    empty = np.zeros((0, 3), np.float32)
    ratios = sorted({c["ratio"] for c in cs})
    assert ratios == [0.05, 0.1]
    for ratio in ratios:
        out, _ = S.sm_batch_dev([c["a"] for c in cs] + [empty], [c["b"] for c in cs] + [empty], top_ratio=ratio, poison=0xFF)
        for c, o in zip(cs, out):
            single = run(S, c["name"]) if c["ratio"] == ratio else S.sm_dev(c["a"], c["b"], top_ratio=ratio)
            assert _bytes(o) == _bytes(single), (c["name"], ratio)
            assert o[1]["K"] == sm_cpu.top_k(len(c["a"]), ratio)
        T, info, labels, eig = out[-1]
        assert np.array_equal(T, np.eye(4)) and info == dict(status=1, K=0, m=0, weight_sum=0.0) and len(labels) == 0
    assert tuple(np.flatnonzero(out[2][2])) == cs[2]["expect_sel"]          # (the last batch ran at 0.1, the tie set's own ratio)


def test_m_dev_in_a_batch(S):
    """Live counts on the device for some pairs of a batch and none for others: 150, 0, 500 (clamped to the 200 rows) and null."""
    import torch
    c = sm_cases.by_name("planted_duplicate")
    lives = (150, 0, 500, None)
    mds = [None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda") for v in lives]
    out, _ = S.sm_batch_dev([c["a"]] * 4, [c["b"]] * 4, m_devs=mds, top_ratio=c["ratio"], poison=0xFF)
    for live, md, o in zip(lives, mds, out):
        single = run(S, c["name"]) if md is None else S.sm_dev(c["a"], c["b"], m_dev=md, top_ratio=c["ratio"])
        assert _bytes(o) == _bytes(single), live
        m = 200 if live is None else min(live, 200)
        assert o[1]["m"] == m and o[1]["K"] == sm_cpu.top_k(m, c["ratio"]) and not o[2][m:].any() and not o[3][m:].any()
    assert _bytes(out[2]) == _bytes(out[3])              # clamped to all rows = no live count


def test_guard_band_behind_the_scratch(S):
    """The scratch is 4 096 bytes longer than the size that is passed (npairs * lr_sm_scratch_bytes(mx)), the tail holds 0xC3: it still
    does after a call at the accepted maximum and after a 3-pair batch at M = 2 049."""
    import torch
    from lidarregistration_amd import corrset
    c = sm_cases.by_name("full_32768")
    _, e, lab, tail = raw_single(c, guard=4096, fill=0xC3)
    assert len(tail) == 4096 and (tail == 0xC3).all()
    assert np.array_equal(e, run(S, c["name"])[3]) and np.array_equal(lab, run(S, c["name"])[2])
    c = sm_cases.by_name("ragged_2049")
    call = corrset.BatchCall(S.SOLVER, [c["a"]] * 3, [c["b"]] * 3, top_ratio=c["ratio"])
    from lidarregistration_amd import _ext
    need = 3 * _ext.lib().lr_sm_scratch_bytes(2049)
    assert call.scratch.numel() == need
    big = torch.full((need + 4096,), 0xC3, dtype=torch.uint8, device="cuda")
    call._args = (*call._args[:-2], big.data_ptr(), need)
    call.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (big[need:].cpu().numpy() == 0xC3).all()
    for o in S._decode(call):
        assert _bytes(o) == _bytes(run(S, c["name"]))
