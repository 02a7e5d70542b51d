"""lr_fcgf_extract on the GPU (csrc/lr_fcgf.hip through lidarregistration_amd.fcgf) against the numpy restatements of tests/fcgf_cpu.py.

Contract n1 is bit-exact (F5): the small cases are compared bit pattern by bit pattern with the fmaf-chain restatement, for the whole
network and stage by stage through `tap`.  At size the device is held to the fp64 restatement within 4 x d32, d32 being what ANOTHER
fp32 summation order (one matmul per offset) costs on the same input, measured here on the CPU; nothing is derived from what the kernel
returns.  Cases: tests/fcgf_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, fcgf, synth
from tests import fcgf_cases, fcgf_cpu

pytestmark = pytest.mark.gpu
CASES = fcgf_cases.small_cases()
SEED = 0


@functools.lru_cache(maxsize=None)
def stages(k1):
    return fcgf.fold(fcgf_cases.make_state_dict(SEED, k1), k1)


@functools.lru_cache(maxsize=None)
def model(k1=5):
    return fcgf.FCGF.from_state_dict(fcgf_cases.make_state_dict(SEED, k1), k1)


@functools.lru_cache(maxsize=None)
def chain(name, k1=5):
    """The fmaf-chain restatement of a small case, computed once and shared (read-only)."""
    r = fcgf_cpu.run(CASES[name], stages(k1), k1, mode="chain")
    for a in list(r["acts"].values()) + [r["out"]]:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def scan_cells(n0, seed=3):
    """The distinct 0.3 m cells of a synth.make_scan_pair frame of n0 returns (4 400 -> about 4 000 cells, 40 000 -> about 30 000)."""
    xyz = synth.make_scan_pair(n0=n0, seed=seed)[0]
    c = np.unique(np.floor(xyz / 0.3).astype(np.int32), axis=0)
    c = c[np.random.default_rng(seed).permutation(len(c))]
    c.setflags(write=False)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(t):
    return t.cpu().numpy()


# ---- 4. bit-equality with the chain restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k1", [(n, 5) for n in CASES] + [(n, 3) for n in fcgf_cases.K3_CASES], ids=lambda v: str(v))
def test_network_is_bit_equal_to_the_fmaf_chain(name, k1):
    m = model(k1)
    got = host(m.features(CASES[name]))
    assert m.last_info == dict(status=0, n=len(CASES[name]), n_tap=len(CASES[name]))
    want = chain(name, k1)["out"]
    assert got.shape == want.shape and np.isfinite(got).all()
    bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
    assert bad.size == 0, (name, k1, bad[:8], np.abs(got - want).max())


@pytest.mark.parametrize("s", range(1, 24))
def test_every_tap_is_bit_equal_and_carries_its_level(s):
    name = fcgf_cases.ALL_TAPS_CASE
    r = chain(name)
    act, tc = model().tap(CASES[name], s)
    lvl = r["level_of"][s]
    assert np.array_equal(host(tc), r["levels"][lvl]) and model().last_info["n_tap"] == len(r["levels"][lvl])
    assert act.shape == r["acts"][s].shape and np.array_equal(bits(host(act)), bits(r["acts"][s])), (s, np.abs(host(act) - r["acts"][s]).max())


# ---- 5. coordinate sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "block3_origin", "two_clusters", "random129", "one_chain", "scan4000"])
def test_coarse_coordinate_sets_in_contract_order(name):
    cells = fcgf_cases.one_chain_cells(256) if name == "one_chain" else np.array(scan_cells(4400)) if name == "scan4000" else CASES[name]
    if name == "one_chain":
        assert len(np.unique(fcgf_cpu.home_slot(cells, len(cells)))) == 1          # 256 cells on one probe chain of the level-0 table
    L = fcgf_cpu.levels(cells)
    for s, lvl in ((4, 1), (7, 2), (10, 3)):
        act, tc = model().tap(cells, s)
        assert np.array_equal(host(tc), L[lvl]), (name, s)
        assert act.shape == (len(L[lvl]), 32 << lvl)


def test_cells_at_the_ends_of_the_21_bit_fields_decode_and_lose_their_outside_neighbours():
    """The tap's cells are decoded from the levels' keys.  Four cells at +-(2^20 - 3), the last cells inside the range limit: the level-3
    parent of -(2^20 - 3) is -2^20, biased field 0, and its -8 neighbour (like the -4 one of stage 10's table) leaves the field: absent."""
    M = (1 << 20) - 3
    cells = np.array([[M, 0, 0], [-M, 0, 0], [0, -M, M], [-M, -M, -M]], np.int32)
    assert fcgf_cpu.status_of(cells) == 0
    r = fcgf_cpu.run(cells, stages(5), 5, mode="chain")
    assert r["levels"][3].min() == -(1 << 20) and (r["levels"][3] + fcgf_cpu.BIAS).min() == 0
    for s, lvl in ((1, 0), (4, 1), (7, 2), (10, 3)):
        act, tc = model().tap(cells, s)
        assert model().last_info == dict(status=0, n=4, n_tap=len(r["levels"][lvl]))
        assert np.array_equal(host(tc), r["levels"][lvl]), (s, host(tc))
        assert act.shape == r["acts"][s].shape and np.array_equal(bits(host(act)), bits(r["acts"][s])), s
    assert np.array_equal(bits(host(model().features(cells))), bits(r["out"])) and model().last_info["status"] == 0      # stages 11, 12: the -8 neighbour


# ---- 6. F10 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [4400, 40000], ids=["n4000", "n30000"])
def test_same_bits_whatever_the_scratch_the_row_order_or_a_shift_by_eight(n0):
    cells = np.array(scan_cells(n0))
    n = len(cells)
    assert abs(n - (4000 if n0 == 4400 else 30000)) < 0.2 * n
    m = model()
    a = host(m.features(cells, poison=0xFF))
    assert m.last_info["status"] == 0 and np.isfinite(a).all() and np.allclose(np.linalg.norm(a, axis=1), 1.0, atol=1e-5)
    assert np.array_equal(bits(a), bits(host(m.features(cells, poison=0x00))))
    L = fcgf_cpu.levels(cells)                          # (the coarse sets at this size too: the sort's global steps, cheap on the CPU)
    for s, lvl in ((4, 1), (10, 3)):
        assert np.array_equal(host(m.tap(cells, s)[1]), L[lvl]), (s, lvl)
    perm =np.random.default_rng(1).permutation(n)
    assert np.array_equal(bits(a[perm]), bits(host(m.features(cells[perm]))))
    lim = fcgf_cpu.LIMIT - 10
    hi = (lim - cells.max(0)) // 8 * 8                  # the largest cell of each axis lands within 8 of +(2^20 - 12) ...
    lo = -((cells.min(0) + lim) // 8 * 8)               # ... and the smallest within 8 of -(2^20 - 12)
    for shift in ([8, -16, 24], [hi[0], lo[1], 0], [lo[0], 0, hi[2]]):
        moved = (cells + np.asarray(shift, np.int64)).astype(np.int32)
        assert np.abs(moved).max() < fcgf_cpu.LIMIT
        assert np.array_equal(bits(a), bits(host(m.features(moved)))), shift
    assert np.abs(cells + np.array([hi[0], lo[1], 0])).max() >= lim - 8


# ---- 7. value check at size -------------------------------------------------------------------------------------------------------------
def test_values_at_4000_cells_within_four_times_the_fp32_yardstick():
    """d32 = max |fp32 matmul-per-offset restatement - fp64 restatement| on this input; the device must lie within 4 x d32 of fp64: the two
    fp32 evaluations differ in summation order only, while a wrong map entry shows at order 1.
    Measured: n = 4 069, d32 = 2.17e-07, the device 3.17e-07 from fp64, bound 8.69e-07."""
    cells = np.array(scan_cells(4400))
    r64 =fcgf_cpu.run(cells, stages(5), 5, mode="f64")
    assert np.linalg.norm(r64["acts"][23], axis=1).min() > 1e-3            # precondition: F8 divides by nothing small
    d32 = float(np.abs(fcgf_cpu.run(cells, stages(5), 5, mode="f32mm")["out"] - r64["out"]).max())
    got = host(model().features(cells))
    dev = float(np.abs(got - r64["out"]).max())
    print(f"n = {len(cells)}: d32 = {d32:.3e}, device vs fp64 = {dev:.3e}, bound 4 x d32 = {4 * d32:.3e}")
    assert d32 > 0 and dev <= 4 * d32


# ---- 8. statuses and refusals -----------------------------------------------------------------------------------------------------------
def test_statuses_duplicate_range_limit_empty_and_null_feat_in():
    m = model()
    cells = np.array(CASES["random65"])
    dup = cells.copy(); dup[-1] = dup[7]                                     # a duplicate in the last row
    out = m.features(dup)
    assert m.last_info == dict(status=2, n=65, n_tap=0) and not host(out).any() and out.shape == (65, 32)
    for v in (fcgf_cpu.LIMIT, -fcgf_cpu.LIMIT):
        far = cells.copy(); far[3, 1] = v
        assert fcgf_cpu.status_of(far) == 3
        out = m.features(far)
        assert m.last_info["status"] == 3 and not host(out).any()
    far = dup.copy(); far[0, 2] = fcgf_cpu.LIMIT                              # both: the range limit wins
    m.features(far); assert m.last_info["status"] == 3
    m.tap(dup, 5); assert m.last_info == dict(status=2, n=65, n_tap=0)
    edge = cells.copy(); edge[3] = [fcgf_cpu.LIMIT - 1, -(fcgf_cpu.LIMIT - 1), fcgf_cpu.LIMIT - 1]      # the last admitted cell
    out = host(m.features(edge)); assert m.last_info["status"] == 0 and np.isfinite(out).all()
    out = m.features(np.zeros((0, 3), np.int32))
    assert m.last_info == dict(status=0, n=0, n_tap=0) and out.shape == (0, 32)
    ones = host(m.features(cells, feat_in=np.ones(65, np.float32)))
    assert np.array_equal(bits(ones), bits(chain("random65")["out"]))        # NULL feat_in = explicit ones
    f = np.random.default_rng(2).uniform(0.5, 2.0, 65).astype(np.float32)
    want = fcgf_cpu.run(cells, stages(5), 5, feat_in=f, mode="chain")["out"]
    assert np.array_equal(bits(host(m.features(cells, feat_in=f))), bits(want))
    f[5] = np.nan                                                             # carried, not screened
    assert np.isnan(host(m.features(cells, feat_in=f))).any()


def test_refusals_that_need_a_device():
    L = _ext.lib()
    m = model()
    n = 65
    cells = torch.from_numpy(np.array(CASES["random65"])).cuda()
    need = L.lr_fcgf_scratch_bytes(n)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 32), dtype=torch.float32, device="cuda")
    p = _ext.FcgfParams()
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()

    def call(ptr=None, nbytes=need, w=m.weights.data_ptr(), wb=m.weights.numel() * 4):
        return L.lr_fcgf_extract(cells.data_ptr(), None, n, w, wb, ctypes.byref(p), res.data_ptr(), out.data_ptr(), None,
                                 scratch.data_ptr() if ptr is None else ptr, nbytes, st)
    assert call() == 0
    assert call(nbytes=need - 1) == -1 and "scratch too small" in err()
    assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
    assert call(w=m.weights.data_ptr() + 4) == -1 and "16-byte" in err()
    assert call(wb=m.weights.numel() * 4 - 4) == -1 and "weights_bytes" in err()
    hostbuf = np.zeros(need + 256, np.uint8)
    assert call(ptr=(hostbuf.ctypes.data + 255) & ~255) == -1 and "not device memory" in err()
    L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)          # (the hook only: no memory or stream of another device)
    try:
        assert call() == -1 and "device" in err()
    finally:
        L.lr_debug_fake_current_device(-1)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(out)), bits(chain("random65")["out"]))
    assert L.lr_version() == 103


# ---- 9. the Python layer ----------------------------------------------------------------------------------------------------------------
def test_extract_is_dedup_floor_ones_and_extract_pair_feeds_FR():
    from lidarregistration_amd import FR
    m = model()
    raw0, raw1, T = synth.make_scan_pair(n0=6000, seed=5)
    xyz, feats, sel = m.extract(raw0, 0.3)
    cells = np.floor(raw0[host(sel)] / 0.3).astype(np.int32)
    assert len(np.unique(cells, axis=0)) == len(cells) == xyz.shape[0] and feats.shape == (len(cells), 32)
    assert np.array_equal(host(xyz), raw0[host(sel)].astype(np.float32))
    assert np.array_equal(bits(host(feats)), bits(host(m.features(cells))))
    x0, x1, f0, f1 = m.extract_pair(raw0, raw1)
    assert f0.shape == (x0.shape[0], 32) and f1.shape == (x1.shape[0], 32) and np.array_equal(bits(host(f0)), bits(host(feats)))

    class A:
        mode = "MNN"; codebase = "GC"; iters = 2000; fast_rejection = "ELC"
    Tr, elapsed, *_ = FR.FR(x0, x1, f0, f1, A, T)
    assert np.asarray(Tr).shape == (4, 4) and np.isfinite(np.asarray(Tr)).all()      # random weights: the motion itself means nothing
