"""lr_bbrf / lr_normals and their Python mirror (lidarregistration_amd/bbrf.py) against the numpy restatement of the contract
(tests/bbrf_cpu.py): every field of the result block, every log row and every normal bit for bit, under poisoned scratch and at three
cells.  Needs an MI355X."""
import ctypes
import os

import numpy as np
import pytest

from tests import bbrf_cases, bbrf_cpu, refine_z_cases, refine_z_cpu
from tests.conftest import rot_diff_rad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g19_bbrf.npz"))
GOLDEN = bbrf_cases.golden_cases()
SIZE = bbrf_cases.size_cases()
LOOP = bbrf_cases.loop_cases()
NORMALS = bbrf_cases.normals_cases()
KEYS = ("T", "B_to_A", "status", "best_iter", "best_loss", "n_pairs_best", "iters_run")


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, bbrf, overlap
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.bb = bbrf; ns.ov = overlap
    return ns


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def exact(r):
    """The result block with its doubles as bit patterns."""
    return {k: (bits(r[k]).tolist() if isinstance(r[k], np.ndarray) else float(r[k]).hex() if isinstance(r[k], float) else r[k]) for k in KEYS}


def cells(p):
    B = np.asarray(p["B"]).reshape(-1, 3)
    auto = refine_z_cases.auto_cell(B) if len(B) else 1.0
    return ((0.0, None), (0.25 * auto, 0x00), (4.0 * auto, 0xFF))


def check(lr, p, ref=None, cell_set=None):
    want, wlog = ref if ref is not None else bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], **p["params"])
    for cell, poison in (cell_set or cells(p)):
        r, log = lr.bb.bbr_f_dev(p["A"], p["B"], p["nA"], p["nB"], poison=poison, cell=cell, **p["params"])
        assert exact(r) == exact(want), (cell, r, want)
        assert np.array_equal(bits(log.cpu().numpy()), bits(wlog)), (cell, log.cpu().numpy(), wlog)
    for k, v in p.get("expect", {}).items():
        assert r[k] == v
    return r, log.cpu().numpy()


def log_pairs(lr, p):
    """The device's pair count of iteration 0."""
    return int(lr.bb.bbr_f_dev(p["A"], p["B"], p["nA"], p["nB"], **p["params"])[1][0, 7])


@pytest.mark.parametrize("n0", bbrf_cases.SIZES)
def test_sizes_equal_the_restatement(lr, n0):
    for n1 in bbrf_cases.SIZES:
        r, _ = check(lr, SIZE[f"size_{n0}_{n1}"])
        assert r["status"] == (1 if n0 == 0 or n1 == 0 else 0)


@pytest.mark.parametrize("name", sorted(LOOP))
def test_loop_cases_equal_the_restatement(lr, name):
    check(lr, LOOP[name])


def test_loop_behaviour(lr):
    r, log = check(lr, LOOP["same"], cell_set=((0.0, None),))
    assert r["n_pairs_best"] == 300 and not log[:, :6].any() and r["best_iter"] == 0           # clamped terms, no gradient: nothing moves
    assert np.array_equal(r["T"], np.eye(4))
    r, log = check(lr, LOOP["quarter"], cell_set=((0.0, None),))
    assert r["best_loss"] == 0.5 and log[0, 7] == 300
    r, log = check(lr, LOOP["run_2049_gap"], cell_set=((0.0, None),))
    assert log[0, 7] == 1025                                                                    # the middle run holds no pair
    r, log = check(lr, LOOP["no_pair_at_2"], cell_set=((0.0, None),))
    assert log[2, 7] == 0 and log[2, 6] == np.inf and not log[3:].any()
    p = LOOP["ties_lattice"]
    trace = []
    bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], trace=trace, **p["params"])
    M = refine_z_cpu.d2_matrix(p["A"], p["B"])
    f, keep = trace[0]["f"], trace[0]["keep"]
    assert keep.sum() == log_pairs(lr, p) and keep.any()
    for i in np.flatnonzero(keep):                                                              # the corners of a cell tie: the lowest index is the buddy
        tied = np.flatnonzero(M[:, f[i]] == M[:, f[i]].min())
        assert len(tied) >= 4 and tied[0] == i and np.flatnonzero(M[i] == M[i].min())[0] == f[i]


def test_null_log_and_mirror_defaults(lr):
    p = LOOP["iters_2"]
    want, _ = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], **p["params"])
    r, log = lr.bb.bbr_f_dev(p["A"], p["B"], p["nA"], p["nB"], want_log=False, **p["params"])
    assert log is None and exact(r) == exact(want)
    q = lr.ext.BbrfParams()
    assert (q.n_iter, q.angles_lr, q.trans_lr, q.beta1, q.beta2, q.eps, q.cell) == (100, 2e-4, 2e-4, 0.9, 0.999, 1e-8, 0.0)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases_through_the_device(lr, name):
    """100 iterations: the device equals the restatement bit for bit and follows the reference's recorded trajectory within the bounds
    of tests/test_bbrf_cpu.py."""
    p = GOLDEN[name]
    if name == "g_scan_generic":                   # (the 3 000-point restatement takes seconds: it is run on one of the two large cases)
        r, log = lr.bb.bbr_f_dev(p["A"], p["B"], p["nA"], p["nB"], poison=0xFF)
        log = log.cpu().numpy()
    else:
        want, wlog, _ = bbrf_cases.golden_run(name)
        r, log = check(lr, p, ref=(want, wlog), cell_set=((0.0, 0xFF),))
    g = lambda k: GOLD[f"{name}/{k}"]
    assert str(g("sha256")) == bbrf_cases.checksum(p["A"], p["nA"], p["B"], p["nB"])
    assert np.abs(log[:, :6] - g("params")).max() <= 1e-6
    assert (np.abs(log[:, 6] - g("loss")) <= 1e-6 * (1.0 + g("loss"))).all() and r["best_iter"] == int(g("argmin"))
    assert log[0, 7] == g("npairs")[0]
    off = np.abs(log[:, 7] - g("npairs"))
    assert off.max() <= 2 and (off > 0).sum() <= 5
    assert rot_diff_rad(r["T"], g("T")) <= 1e-6 and np.abs(r["T"][:3, 3] - g("T")[:3, 3]).max() <= 1e-6


def test_refusals_on_the_device(lr):
    """Short, misaligned and foreign scratch, a stream of another device; nothing is launched, a good call still works afterwards."""
    torch, L = lr.torch, lr.ext.lib()
    p = SIZE["size_257_257"]
    t = lambda X: torch.from_numpy(np.ascontiguousarray(X)).cuda()
    a, na, b, nb = t(p["A"]), t(p["nA"]), t(p["B"]), t(p["nB"])
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()
    res = torch.zeros(ctypes.sizeof(lr.ext.BbrfResult), dtype=torch.uint8, device="cuda")
    log = torch.zeros((3, 8), dtype=torch.float64, device="cuda")
    nrm = torch.zeros((257, 3), dtype=torch.float64, device="cuda"); info = torch.zeros(4, dtype=torch.int32, device="cuda")
    need = max(L.lr_bbrf_scratch_bytes(257, 257, 3), L.lr_normals_scratch_bytes(257))
    scratch = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    pb = lr.ext.BbrfParams(n_iter=3)

    def bb(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_bbrf(a.data_ptr(), na.data_ptr(), 257, b.data_ptr(), nb.data_ptr(), 257, ctypes.byref(pb), res.data_ptr(), log.data_ptr(), ptr, nbytes, st)

    def nm(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_normals(a.data_ptr(), 257, 1.5, 13, nrm.data_ptr(), info.data_ptr(), ptr, nbytes, st)
    host = np.zeros(need + 256, np.uint8)
    hp = (host.ctypes.data + 255) & ~255
    for call, size in ((bb, L.lr_bbrf_scratch_bytes(257, 257, 3)), (nm, L.lr_normals_scratch_bytes(257))):
        assert call() == 0
        assert call(nbytes=size - 1) == -1 and "scratch too small" in err()
        assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
        assert call(ptr=hp) == -1 and "not device memory" in err()
        L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)
        try:
            assert call() == -1 and "device" in err()
        finally:
            L.lr_debug_fake_current_device(-1)
        assert call() == 0
    torch.cuda.synchronize()
    want, wlog = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], n_iter=3)
    r = lr.ext.BbrfResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert (r.status, r.best_iter, r.best_loss, r.iters_run) == (want["status"], want["best_iter"], want["best_loss"], want["iters_run"])
    assert np.array_equal(bits(log.cpu().numpy()), bits(wlog))
    assert np.array_equal(bits(nrm.cpu().numpy()), bits(bbrf_cpu.normals(p["A"], 1.5, 13)[0]))


def test_call_can_be_captured_into_a_graph(lr):
    """No host synchronisation, no allocation, the loop never driven from the host: lr_bbrf recorded once on a side stream and replayed on
    other contents of the same buffers gives what the eager calls give, bit for bit."""
    torch, L = lr.torch, lr.ext.lib()
    p = LOOP["z_normals"]
    n0, n1 = len(p["A"]), len(p["B"])
    inputs = [p["A"], p["A"] + np.array([0.0, 0.05, 0.125]), p["B"][:n0] + np.array([0.0, 0.0, 0.25])]
    t = lambda X: torch.from_numpy(np.ascontiguousarray(X)).cuda()
    A = torch.empty((n0, 3), dtype=torch.float64, device="cuda"); na, b, nb = t(p["nA"]), t(p["B"]), t(p["nB"])
    res = torch.zeros(ctypes.sizeof(lr.ext.BbrfResult), dtype=torch.uint8, device="cuda")
    log = torch.zeros((3, 8), dtype=torch.float64, device="cuda")
    sc = torch.empty(L.lr_bbrf_scratch_bytes(n0, n1, 3), dtype=torch.uint8, device="cuda")
    pb = lr.ext.BbrfParams(n_iter=3)
    s = torch.cuda.Stream()

    def call():
        lr.ext.check(L.lr_bbrf(A.data_ptr(), na.data_ptr(), n0, b.data_ptr(), nb.data_ptr(), n1, ctypes.byref(pb), res.data_ptr(), log.data_ptr(),
                               sc.data_ptr(), sc.numel(), s.cuda_stream))

    def outputs():
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (res, log)]

    def load(x):
        A.copy_(torch.from_numpy(np.ascontiguousarray(x))); torch.cuda.synchronize()
    eager = []
    for x in inputs:
        load(x); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k, (x, want) in list(enumerate(zip(inputs, eager)))[::-1]:
        load(x); sc.fill_(0xFF if k & 1 else 0x00); log.fill_(7.0); g.replay()
        assert outputs() == want
    assert len(set(e[0] for e in eager)) == 3
    want, wlog = bbrf_cpu.bbrf(inputs[1], p["nA"], p["B"], p["nB"], n_iter=3)
    assert np.array_equal(bits(np.frombuffer(eager[1][1], np.float64).reshape(3, 8)), bits(wlog))


@pytest.mark.parametrize("name", sorted(NORMALS))
def test_normals_equal_the_restatement(lr, name):
    p = NORMALS[name]
    want, winfo = bbrf_cpu.normals(p["X"], p["radius"], p["max_nn"])
    for poison in (None, 0x00, 0xFF):
        got, info = lr.bb.normals_dev(p["X"], p["radius"], p["max_nn"], poison=poison)
        assert info == winfo
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    if "plane" in p:
        assert (np.abs(np.abs(want @ p["plane"]) - 1.0) < 1e-9).all()
    if name in ("all_default", "exactly_2"):
        assert winfo["n_default"] == len(p["X"])


def test_python_mirror_end_to_end(lr):
    """calc_normals' default, BBR_F with the global generator's subsets, refinement_sample's columns."""
    from lidarregistration_amd import synth
    a, b, raw = refine_z_cases.scan_pair(3000)
    assert np.array_equal(lr.bb.calc_normals(a), bbrf_cases.z_normals(len(a)))                # radius 0.01 at voxel 0.3: all (0, 0, 1)
    p = GOLDEN["g_small"]
    np.random.seed(5)
    M, elapsed, info, log = lr.bb.BBR_F(p["A"], p["B"], return_info=True)
    np.random.seed(5)
    ia = np.random.permutation(len(p["A"]))[:30000]; ib = np.random.permutation(len(p["B"]))[:30000]
    want, wlog = bbrf_cpu.bbrf(p["A"][ia], bbrf_cases.z_normals(len(ia)), p["B"][ib], bbrf_cases.z_normals(len(ib)))
    assert np.array_equal(bits(M), bits(want["T"])) and np.array_equal(bits(log), bits(wlog)) and elapsed > 0.0
    np.random.seed(5)
    M2, _ = lr.bb.BBR_F(p["A"], p["B"])
    assert np.array_equal(bits(M2), bits(M))
    # refinement_sample on a small pair: the ICP columns are those of overlap.refine_motion's ICP
    A, B, T = synth.make_scan_pair(3000, 3000)
    init = bbrf_cases.small_motion(81, 0.5, 0.05) @ T
    row = lr.bb.refinement_sample(T, init, A, B, rot_thresh=5.0, trans_thresh=2.0)
    assert row.shape == (12,) and np.isnan(row[8:]).all() and np.isfinite(row[:8]).all()
    icp_full = lr.ov.refine_motion(init, A, B, True, 0.3)                                       # icp_mot @ init
    gt = T @ np.linalg.inv(init)
    from lidarregistration_amd.ransac import icp_dev
    a32, b32 = lr.ov.refine_inputs(init, A, B, True, 0.3)
    icp_mot, _ = icp_dev(a32, b32, np.eye(4), max_dist=0.6)
    assert np.array_equal(bits(icp_mot @ init), bits(icp_full))
    assert np.array_equal(row[:3], lr.bb.calc_errors(icp_mot, gt, 5.0, 2.0))
    assert row[4] in (0.0, 1.0) and row[5] < 0.2 and row[6] < 2.0
