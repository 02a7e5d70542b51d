"""The DGR refinement on the GPU (csrc/lr_dgr.hip), all through the C ABI (lidarregistration_amd.dgr's ctypes calls): the device against
the numpy restatement of the contract (tests/dgr_cpu.py) BIT FOR BIT -- result block, log, T -- with the scratch pre-filled with 0xFF; the
Python layers against the recording of the reference (tests/golden/g27_dgr.npz) and the ground truth.

The contract is fp64 with + - * / sqrt only, in a fixed association and a fixed summation tree, so equality is the rule and
no tolerance appears below except where a Python layer is held to the reference or to the ground truth:
  * dgr.GlobalRegistration on the stable golden cases: iterations and break_count of the reference's float64 run; R, t, loss within the
    a13 tolerance of DESIGN.md §0 (2e-5: the init is the contract's fp64 fit, the reference's is its float32 one; measured 1e-5 at most);
  * DGRTail.register: the recall thresholds of the harness (5 degrees, 2 m) against the planted motion.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, corrset, dgr
from tests import dgr_cases as cases
from tests import dgr_cpu as cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g27_dgr.npz"))
P = cases.PARAMS


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    """the restatement's G3 is the oracle library's lr_rt_from_moments"""
    return oracle


def bits(v):
    """The doubles' bit patterns (+0.0 and -0.0 differ); every NaN counts as the same one: no contract fixes a payload."""
    v = np.asarray(v, np.float64)
    return np.ascontiguousarray(np.where(np.isnan(v), np.nan, v)).view(np.uint64)


def same(dev, ref, tag=""):
    """(T, info) of the device == the restatement's dict, bit for bit; the log too where both have one."""
    T, info = dev
    got = tuple(info[k] for k in ("status", "L", "iterations", "break_count"))
    want = tuple(ref[k] for k in ("status", "L", "iterations", "break_count"))
    assert got == want, (tag, got, want)
    for k in ("w1", "loss"):
        assert bits(info[k]) == bits(ref[k]), (tag, k, info[k], ref[k])
    assert np.array_equal(bits(T), bits(ref["T"])), (tag, np.abs(T - ref["T"]).max())
    if "log" in info and "log" in ref:
        bad = np.nonzero((bits(info["log"]) != bits(ref["log"])).any(1))[0]
        assert bad.size == 0, (tag, "first differing log row", int(bad[0]))


def both(c, tag="", **kw):
    """The device (scratch 0xFF, with log) and the restatement on one case: asserts equality, returns the restatement."""
    kw = dict(P, **kw)
    w, T0, md = c.get("weights"), c.get("T_init"), c.get("m_dev")
    m_dev = None if md is None else torch.tensor([md], dtype=torch.int32, device="cuda")
    d = dgr.refine(c["src"], c["tgt"], w, T0, m_dev, log=True, poison=0xFF, **kw)
    r = cpu.refine(c["src"], c["tgt"], w, T0, md, **kw)
    same(d, r, tag)
    return r


@functools.lru_cache(maxsize=None)
def dense(m, seed=0, inlier_ratio=0.5):
    """A planted case in which every row is live (weights 0.05 .. 1)."""
    c = cases.planted(seed, m, inlier_ratio, 0.05, 0.4)
    c["weights"] = np.maximum(c["weights"], np.float32(0.05))
    return c


# ---- sizes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 2, 3, 1023, 1024, 1025, 2049, 32768])
def test_sizes(L):
    r = both(dense(L, seed=L), max_iter=25 if L > 3000 else 40)
    assert r["L"] == L and r["status"] == (0 if L else 1)
    if L > 3:
        assert r["iterations"] >= 20                 # (at least twenty steps were compared row by row)


def test_m_dev_below_m():
    c = dict(dense(2049, seed=5), m_dev=1500)
    r = both(c, max_iter=30)
    assert r["L"] == 1500
    same(dgr.refine(c["src"][:1500], c["tgt"][:1500], c["weights"][:1500], max_iter=30, **{k: v for k, v in P.items() if k != "max_iter"}), r)
    assert both(dict(c, m_dev=-3))["status"] == 1 and both(dict(c, m_dev=10 ** 6), max_iter=5)["L"] == 2049


# ---- dead rows ----------------------------------------------------------------------------------------------------------------------------
def test_dead_rows_interleaved():
    """Dead rows of every kind, placed so that the compaction crosses lane, wave and 1024-row boundaries."""
    c = {k: np.array(v) for k, v in dense(3500, seed=11).items()}
    i = np.arange(3500)
    w, src, tgt = c["weights"], c["src"], c["tgt"]
    w[i % 3 == 1] = 0.0
    w[60:70] = -1.0
    w[1000:1100] = 0.01                              # clipped
    w[2047:2050] = np.nan
    w[130] = np.inf
    src[63, 1] = np.inf; tgt[64, 2] = np.nan; src[1024, 0] = -np.inf
    r = both(c, clip=0.05, max_iter=40)
    live = cpu.live_rows(src, tgt, w, 0.05)
    assert r["L"] == live.sum() and 0 < r["L"] < 2400
    # the same live rows handed over without the dead ones: the same bits
    same(dgr.refine(src[live], tgt[live], w[live], clip=0.05, max_iter=40, **{k: v for k, v in P.items() if k != "max_iter"}), r)


def test_every_weight_clipped():
    c = dict(dense(700, seed=3))
    c["weights"] = np.full(700, 0.01, np.float32)
    r = both(c, clip=0.05)
    assert (r["status"], r["L"], r["w1"]) == (1, 0, 0.0) and np.array_equal(r["T"], np.eye(4))


# ---- boundaries ---------------------------------------------------------------------------------------------------------------------------
def test_wsum_threshold_at_and_below_w1():
    c = dense(1025, seed=7)
    w1 = float(cpu.tree_sum(c["weights"].astype(np.float64))[0])
    at = both(c, wsum_threshold=w1, max_iter=3)
    assert at["status"] == 0 and at["w1"] == w1
    above = both(c, wsum_threshold=float(np.nextafter(w1, np.inf)), max_iter=3)
    assert above["status"] == 2 and above["w1"] == w1 and above["L"] == 1025 and np.array_equal(above["T"], np.eye(4))


def test_max_iter_1():
    r = both(dense(500, seed=9), max_iter=1)
    assert r["iterations"] == 0 and r["break_count"] == 1          # iteration 0 always counts


def test_stop_at_iteration_0_on_exact_correspondences():
    rng = np.random.default_rng(0)
    src = rng.integers(-40, 40, (300, 3)).astype(np.float32)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    tgt = src @ R.T + np.array([3, -2, 1], np.float32)
    for T0 in (None, np.block([[R.astype(np.float64), np.array([[3.0], [-2.0], [1.0]])], [np.zeros((1, 3)), np.ones((1, 1))]])):
        r = both(dict(src=src, tgt=tgt, weights=np.ones(300, np.float32), T_init=T0))
        assert r["status"] == 0 and r["iterations"] == 0 and r["break_count"] == 0 and r["loss"] < 1e-7
        assert not r["log"][1:].any()


def test_stop_by_break_count():
    c = cases.golden_case("m64")
    r = both(c, clip=cases.CLIP)
    assert r["break_count"] == 20 and 20 < r["iterations"] < 999 and min(r["margins"]) > 1e-3


def test_ratio_0_runs_all_1000_iterations():
    r = both(dense(1024, seed=13), ratio=0.0)
    assert r["iterations"] == 999 and r["break_count"] == 0 and r["log"][999, 9] > 1e-7


# ---- crafted inputs -------------------------------------------------------------------------------------------------------------------------
def test_branch_boundary_s_equals_1():
    """Under the identity and q = 0.5 a residual of exactly (0.5, 0, 0) has s == 1 exactly: the outer branch."""
    c = dense(200, seed=17)
    src, tgt = np.array(c["src"]), np.array(c["tgt"])
    src[5] = (0, 0, 0); tgt[5] = (0.5, 0, 0)
    src[6] = (1, 2, 3); tgt[6] = (1, 2, 2.5)
    r = both(dict(src=src, tgt=tgt, weights=c["weights"], T_init=np.eye(4)), quantization_size=0.5, max_iter=6)
    assert r["s_gap"] == 0.0


@pytest.mark.parametrize("kind", ["zero_first_column", "parallel_columns", "nan"])
def test_T_init_at_the_clamps(kind):
    c = dict(dense(300, seed=19))
    T0 = np.eye(4)
    if kind == "zero_first_column":
        T0[:3, 0] = 0.0
    elif kind == "parallel_columns":
        T0[:3, 1] = 2.0 * T0[:3, 0]
    else:
        T0[1, 3] = np.nan
    c["T_init"] = T0
    r = both(c, max_iter=30)
    if kind == "nan":
        assert r["status"] == 3 and r["iterations"] == 0 and np.isnan(r["loss"])
    else:
        assert r["status"] == 0 and np.isfinite(r["T"]).all()
        o = cpu.rotation(r["p0"])
        assert (o["na"] < cpu.CLAMP) if kind == "zero_first_column" else (o["nu"] < cpu.CLAMP)


def test_nan_weight_and_inf_coordinate_are_dead():
    c = {k: np.array(v) for k, v in dense(100, seed=23).items()}
    c["weights"][7] = np.nan
    c["src"][40, 2] = np.inf
    r = both(c, max_iter=20)
    assert r["L"] == 98 and r["status"] == 0 and np.isfinite(r["T"]).all()


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64])
def test_batch_equals_one_by_one(n):
    ms = [(37 * k * k + 5) % 1500 for k in range(n)]
    ms[0] = 1300
    if n == 64:
        ms[3], ms[10] = 0, 2049
    cs = [dense(m, seed=100 + k) for k, m in enumerate(ms)]
    kw = dict(P, max_iter=30, clip=0.1)
    call = corrset.BatchCall(dgr.SOLVER, [c["src"] for c in cs], [c["tgt"] for c in cs], weights=[c["weights"] for c in cs], poison=0xFF, **kw)
    call.launch(torch.cuda.current_stream().cuda_stream)
    raw, out = call.raw(), call.results()
    for k, c in enumerate(cs):
        one = corrset.BatchCall(dgr.SOLVER, [c["src"]], [c["tgt"]], weights=[c["weights"]], single=True, poison=0x00, **kw)
        one.launch(torch.cuda.current_stream().cuda_stream)
        assert one.raw()[0] == raw[k], k
    for k in (0, n - 1):
        same(out[k], cpu.refine(cs[k]["src"], cs[k]["tgt"], cs[k]["weights"], **kw), k)


def test_batch_with_T_init_m_dev_and_null_entries():
    cs = [dense(m, seed=200 + m) for m in (900, 1100, 400)]
    T0 = cases.planted(0, 1, 1.0, 0.0, 0.35)["T_gt"]
    m_devs = [None, torch.tensor([777], dtype=torch.int32, device="cuda"), None]
    kw = dict(P, max_iter=20)
    call = corrset.BatchCall(dgr.SOLVER, [c["src"] for c in cs], [c["tgt"] for c in cs], None, m_devs, weights=[cs[0]["weights"], cs[1]["weights"], None],
                             T_inits=[None, T0, T0], poison=0xFF, **kw)
    call.launch(torch.cuda.current_stream().cuda_stream)
    out = call.results()
    same(out[0], cpu.refine(cs[0]["src"], cs[0]["tgt"], cs[0]["weights"], **kw), 0)
    same(out[1], cpu.refine(cs[1]["src"], cs[1]["tgt"], cs[1]["weights"], T0, 777, **kw), 1)
    same(out[2], cpu.refine(cs[2]["src"], cs[2]["tgt"], None, T0, **kw), 2)


def test_null_weights_and_null_log():
    c = dense(1500, seed=29)
    r = both(dict(src=c["src"], tgt=c["tgt"]), max_iter=30)
    assert r["w1"] == 1500.0
    same(dgr.refine(c["src"], c["tgt"], None, log=False, poison=0xFF, **dict(P, max_iter=30)), r)


def test_unstable_case():
    """The case on which the reference's own precisions part (the init is the optimum, the s < 1 branches flip): device == restatement."""
    c = cases.golden_case("unstable")
    r = both(c, clip=cases.CLIP)
    assert r["status"] == 0 and r["iterations"] > 100 and r["s_gap"] < 1e-4


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    L = _ext.lib()
    c = dense(64, seed=31)
    t = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("src", "tgt", "weights")}
    res = torch.zeros(ctypes.sizeof(_ext.DgrResult) * 2, dtype=torch.uint8, device="cuda")
    sc = torch.empty(L.lr_dgr_scratch_bytes(64) * 2 + 256, dtype=torch.uint8, device="cuda")
    before = res.clone()

    def single(p, m=64, src=t["src"], scratch=None, nbytes=None, result=res):
        scratch = sc.data_ptr() if scratch is None else scratch
        return L.lr_dgr_refine(src.data_ptr() if src is not None else None, t["tgt"].data_ptr(), m, None, t["weights"].data_ptr(), None,
                               ctypes.byref(p) if p is not None else None, result.data_ptr() if result is not None else None, None, scratch,
                               sc.numel() if nbytes is None else nbytes, None)

    def refused(rc, word):
        msg = L.lr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)       # LR_EINVAL

    p = dgr.params()
    p.struct_size = 56
    refused(single(p), "struct_size")
    refused(single(None), "null params")
    bad = dict(max_iter=(0, 1001, -1), max_break=(0, -5), quantization_size=(0.0, -1.0, np.nan, np.inf), lr=(0.0, -0.1, np.nan, np.inf),
               gamma=(0.0, -0.5, 1.5, np.nan), ratio=(-1e-9, np.nan, np.inf), clip=(-0.1, np.nan, np.inf), wsum_threshold=(-1.0, np.nan, np.inf))
    for name, values in bad.items():
        for v in values:
            refused(single(dgr.params(**{name: v})), name)
    ok = dgr.params()
    refused(single(ok, m=32769), "more than 32768")
    refused(single(ok, m=-1), "negative")
    refused(single(ok, src=None), "null")
    refused(single(ok, result=None), "null")
    refused(single(ok, nbytes=L.lr_dgr_scratch_bytes(64) - 1), "scratch too small")
    refused(single(ok, scratch=sc.data_ptr() + 8), "256-byte aligned")
    two = (ctypes.c_void_p * 2)(t["src"].data_ptr(), t["src"].data_ptr())
    tg = (ctypes.c_void_p * 2)(t["tgt"].data_ptr(), t["tgt"].data_ptr())
    mm = (ctypes.c_int32 * 2)(64, 64)
    for n in (0, 65):
        refused(L.lr_dgr_refine_batch(n, two, tg, mm, None, None, None, ctypes.byref(ok), res.data_ptr(), sc.data_ptr(), sc.numel(), None), "npairs")
    odd = (ctypes.c_void_p * 2)(None, t["src"].data_ptr() + 4)
    refused(L.lr_dgr_refine_batch(2, two, tg, mm, None, None, odd, ctypes.byref(ok), res.data_ptr(), sc.data_ptr(), sc.numel(), None), "T_init")
    refused(L.lr_dgr_refine_batch(2, two, tg, mm, None, None, None, ctypes.byref(ok), res.data_ptr(), sc.data_ptr(), L.lr_dgr_scratch_bytes(64), None), "scratch too small")
    torch.cuda.synchronize()
    assert torch.equal(res, before), "a refused call launched something"
    assert L.lr_dgr_scratch_bytes(-1) == 0 and L.lr_dgr_scratch_bytes(32769) == 0 and L.lr_dgr_scratch_bytes(32768) >= 32768 * 32
    assert L.lr_version() == 103


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------
def test_call_can_be_captured_into_a_graph():
    """One lr_dgr_refine (m = 1200, an m_dev buffer, a log) recorded on a side stream and replayed on other inputs and live counts gives the
    bytes of the eager calls, whatever the scratch held."""
    L = _ext.lib()
    m = 1200
    configs = [(dense(m, seed=41), 1200), (dense(m, seed=42), 1025), (dense(m, seed=43), 0)]
    dev = dict(src=torch.empty((m, 3), dtype=torch.float32, device="cuda"), tgt=torch.empty((m, 3), dtype=torch.float32, device="cuda"),
               weights=torch.empty(m, dtype=torch.float32, device="cuda"))
    m_dev = torch.empty(1, dtype=torch.int32, device="cuda")
    p = dgr.params(**dict(P, max_iter=30))
    log = torch.empty((30, 10), dtype=torch.float64, device="cuda")
    res = torch.zeros(ctypes.sizeof(_ext.DgrResult), dtype=torch.uint8, device="cuda")
    sc = torch.empty(L.lr_dgr_scratch_bytes(m), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def call():
        _ext.check(L.lr_dgr_refine(dev["src"].data_ptr(), dev["tgt"].data_ptr(), m, m_dev.data_ptr(), dev["weights"].data_ptr(), None, ctypes.byref(p),
                                   res.data_ptr(), log.data_ptr(), sc.data_ptr(), sc.numel(), s.cuda_stream))

    def load(cfg, poison):
        c, live = cfg
        for k, t in dev.items():
            t.copy_(torch.from_numpy(np.array(c[k])))
        m_dev.fill_(live); res.fill_(0x55); log.fill_(7.0); sc.fill_(poison)
        torch.cuda.synchronize()

    def outputs():
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (res, log)]
    eager = []
    for cfg in configs:
        load(cfg, 0x00); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k, (cfg, want) in list(enumerate(zip(configs, eager)))[::-1] + [(0, (configs[0], eager[0]))]:
        load(cfg, 0xFF if k & 1 else 0x00); g.replay()
        assert outputs() == want, k
    assert len(set(e[0] for e in eager)) == 3
    for (c, live), e in zip(configs, eager):
        r = _ext.DgrResult.from_buffer_copy(e[0])
        ref = cpu.refine(c["src"], c["tgt"], c["weights"], None, live, **dict(P, max_iter=30))
        same((np.array(r.T).reshape(4, 4), dict(dgr._info(r), log=np.frombuffer(e[1], np.float64).reshape(30, 10))), ref, live)


# ---- the Python layers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.STABLE)
def test_GlobalRegistration_on_the_golden_cases(name):
    """The reference's call shape on its own recorded cases.  The weights' zeros are DGR's clipped rows; they are dead here (w <= 0)."""
    c = cases.golden_case(name)
    assert str(GOLD[name + "/sha256"]) == cases.checksum(c)
    R, t, info = dgr.GlobalRegistration(c["src"], c["tgt"], torch.from_numpy(c["weights"]).reshape(-1, 1), break_threshold_ratio=P["ratio"],
                                        quantization_size=P["quantization_size"])
    assert sorted(info) == ["break_count", "iterations", "loss"] and R.shape == (3, 3) and t.shape == (1, 3)
    ref = cpu.refine(c["src"], c["tgt"], c["weights"], **P)
    assert np.array_equal(R.numpy(), ref["T"][:3, :3]) and np.array_equal(t.numpy().ravel(), ref["T"][:3, 3])
    if name != "m7":      # (m7's float32 and float64 runs already part on the iteration count: its count hangs on the init's last bits)
        assert (info["iterations"], info["break_count"]) == (int(GOLD[name + "/f64/iterations"]), int(GOLD[name + "/f64/break_count"]))
    dR, dt = np.abs(R.numpy() - GOLD[name + "/f64/R"]).max(), np.abs(t.numpy().ravel() - GOLD[name + "/f64/t"]).max()
    print(f"{name}: |dR| {dR:.2e} |dt| {dt:.2e} |dloss| {abs(info['loss'] - float(GOLD[name + '/f64/loss'])):.2e}")
    assert dR <= 2e-5 and dt <= 2e-5


def _scan_pair(seed, m=6000, inlier_ratio=0.3):
    c = cases.planted(seed, m, inlier_ratio, 0.05, 0.3)
    rng = np.random.default_rng(seed + 1)
    perm = rng.permutation(m)
    xyz1 = c["tgt"][perm]                            # the target cloud in another order: idx1 undoes it
    idx1 = np.argsort(perm)
    return c, c["src"], xyz1, np.arange(m), idx1


def _recall(T, T_gt):
    cos = (np.trace(T[:3, :3].T @ T_gt[:3, :3]) - 1) / 2
    return np.degrees(np.arccos(np.clip(cos, -1, 1))), np.linalg.norm(T[:3, 3] - T_gt[:3, 3])


def test_DGRTail_takes_the_refinement_path():
    c, xyz0, xyz1, idx0, idx1 = _scan_pair(61)
    tail = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=0.05, use_icp=True)
    out = tail.register(xyz0, xyz1, idx0, idx1, c["weights"])
    assert tail.last["path"] == "refinement" and tail.last["status"] == 0 and tail.last["w1"] >= 6000 * 0.05
    ref = cpu.refine(c["src"], c["tgt"], c["weights"], ratio=1e-4, quantization_size=0.6, clip=0.05, wsum_threshold=6000 * 0.05)
    assert np.array_equal(out["base"], ref["T"])
    for k in ("base", "w_icp"):
        re, te = _recall(out[k], c["T_gt"])
        assert re < 5.0 and te < 2.0, (k, re, te)
    # the hook: no weights given, the same result
    hooked = dgr.DGRTail(weights_fn=lambda a, b, i, j: c["weights"], use_icp=False).register(xyz0, xyz1, idx0, idx1)
    assert np.array_equal(hooked["base"], out["base"]) and hooked["w_icp"] is hooked["base"]


def test_DGRTail_takes_the_safeguard_path():
    c, xyz0, xyz1, idx0, idx1 = _scan_pair(67)
    tail = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=0.05, use_icp=True)
    # 1800 weights of 0.06 and 4200 clipped ones: 108 < max(4000, 6000) * 0.05
    out = tail.register(xyz0, xyz1, idx0, idx1, np.where(c["inlier"], np.float32(0.06), np.float32(0.01)))
    assert tail.last["path"] == "safeguard" and tail.last["status"] == 2 and tail.last["ransac"]["best_count"] > 1000
    for k in ("base", "w_icp"):
        re, te = _recall(out[k], c["T_gt"])
        assert re < 5.0 and te < 2.0, (k, re, te)
