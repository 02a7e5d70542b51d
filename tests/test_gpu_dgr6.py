"""lr_dgr_inlier on the GPU (csrc/lr_dgr6.hip through lidarregistration_amd.dgr) against the numpy restatements of tests/dgr6_cpu.py.

Contract n3 is bit-exact (I3): the small cases are compared bit pattern by bit pattern with the fmaf-chain restatement, the whole network
and stage by stage through `tap`, on ResUNetBN2C's widths; every one of the 729 offsets of every map kind on a thin network (32 channels
everywhere).  At size the device is held to the fp64 restatement within 4 x d32, d32 being what ANOTHER fp32 summation order (one matmul
per offset) costs on the same input, measured here on the CPU; nothing is derived from what the kernel returns.  Cases: tests/dgr6_cases.py.
The chain references are computed once per module and shared, read-only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, dgr, fcgf, synth
from tests import dgr6_cases, dgr6_cpu, fcgf_cases

pytestmark = pytest.mark.gpu
CASES = dgr6_cases.small_cases()
WIDTHS, THIN = dgr6_cpu.WIDTHS, dgr6_cpu.THIN


@functools.lru_cache(maxsize=None)
def stages(widths):
    st = dgr6_cpu.random_stages(widths, seed=0)
    for W, s, o in st:
        W.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def model(widths):
    return dgr.InlierNet.from_stages(stages(widths))


@functools.lru_cache(maxsize=None)
def chain(name, widths=WIDTHS, upto=23):
    """The fmaf-chain restatement of a case, computed once and shared (read-only)."""
    cells = CASES[name] if name in CASES else {"block3": dgr6_cases.block3, "motifs": dgr6_cases.motifs}[name]()
    r = dgr6_cpu.run(cells, stages(widths), mode="chain", upto=upto)
    for a in list(r["acts"].values()) + ([r["logit"]] if r["logit"] is not None else []):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def corr_rows():
    rows = dgr6_cases.correspondences()
    rows.setflags(write=False)
    return rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(t):
    return t.cpu().numpy()


# ---- 1. bit-equality with the chain restatement, ResUNetBN2C's widths ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_logits_are_bit_equal_to_the_fmaf_chain(name):
    m = model(WIDTHS)
    got = host(m.logits(CASES[name]))
    assert m.last_info == dict(status=0, n=len(CASES[name]), n_tap=len(CASES[name]))
    want = chain(name)["logit"]
    assert got.shape == want.shape and np.isfinite(got).all()
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, (name, bad[:8], np.abs(got - want).max())


@pytest.mark.parametrize("s", range(1, 24))
def test_every_tap_is_bit_equal_and_carries_its_level(s):
    name = dgr6_cases.ALL_TAPS_CASE
    r = chain(name)
    m = model(WIDTHS)
    act, tc = m.tap(CASES[name], s)
    lvl = r["level_of"][s]
    assert np.array_equal(host(tc), r["levels"][lvl]) and m.last_info["n_tap"] == len(r["levels"][lvl])
    assert act.shape == r["acts"][s].shape and np.array_equal(bits(host(act)), bits(r["acts"][s])), (s, np.abs(host(act) - r["acts"][s]).max())


@pytest.mark.parametrize("name", ["one", "block2_far", "single_coarse3", "two_far_clusters", "clusters65"])
def test_coarse_levels_in_contract_order(name):
    L = dgr6_cpu.levels(CASES[name])
    m = model(WIDTHS)
    for s, lvl in ((4, 1), (7, 2), (10, 3)):
        act, tc = m.tap(CASES[name], s)
        assert np.array_equal(host(tc), L[lvl]), (name, s)
        assert act.shape == (len(L[lvl]), WIDTHS[lvl])
    if name == "block2_far":
        assert len(L[1]) == 2 and len(L[0]) == 65
    if name == "single_coarse3":
        assert len(L[3]) == 1


# ---- 2. every offset of every map kind, thin widths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_3x6_block_meets_all_729_offsets_in_one_tile(s):
    cells = dgr6_cases.block3()
    r = chain("block3", THIN, 3)
    org = dgr6_cpu.origin(cells)
    assert len(cells) == 729 and len(dgr6_cpu.kernel_map(cells[364:365].astype(np.int64), cells, 1, org)) == 729       # the centre row
    act, tc = model(THIN).tap(cells, s)
    assert np.array_equal(host(tc), cells) and np.array_equal(bits(host(act)), bits(r["acts"][s])), (s, np.abs(host(act) - r["acts"][s]).max())


@pytest.mark.parametrize("s", [4, 19, 23])
def test_the_729_motifs_meet_every_entry_of_the_strided_and_transposed_maps(s):
    """Coarse cell v_o receives offset o (F3, tap 4), fine cell v_o + o receives offset o from coarse v_o (F4, tap 19); 23 = the logits.
    The reference is the chain restatement of the 1 458-row cloud itself -- with the lockstep chain it costs about a second, so it needs
    no assembly from the motifs; tests/test_dgr6_cpu.py checks that assembly on 8 motifs, and the last lines here hold 8 motifs computed
    alone against the device's rows of the whole cloud."""
    cells = dgr6_cases.motifs()
    r = chain("motifs", THIN)
    m = model(THIN)
    if s == 23:
        got = host(m.logits(cells))
        assert m.last_info["status"] == 0 and np.array_equal(bits(got), bits(r["logit"])), np.abs(got - r["logit"]).max()
        for k in (0, 1, 121, 364, 365, 500, 607, 728):
            alone = dgr6_cpu.run(dgr6_cases.motifs([k]), stages(THIN), mode="chain")["logit"]
            assert np.array_equal(bits(got[2 * k:2 * k + 2]), bits(alone)), k
        return
    act, tc = m.tap(cells, s)
    lvl = r["level_of"][s]
    assert np.array_equal(host(tc), r["levels"][lvl]) and np.array_equal(bits(host(act)), bits(r["acts"][s])), (s, np.abs(host(act) - r["acts"][s]).max())


# ---- 3. F9 / I2: statuses ---------------------------------------------------------------------------------------------------------------
def test_statuses_duplicate_extent_limit_and_empty():
    m = model(THIN)
    cells = np.array(CASES["clusters65"])
    dup = cells.copy(); dup[-1] = dup[7]                                     # a duplicate in the last row
    out = m.logits(dup)
    assert dgr6_cpu.status_of(dup) == 2 and m.last_info == dict(status=2, n=65, n_tap=0) and not host(out).any() and out.shape == (65,)
    m.tap(dup, 5); assert m.last_info == dict(status=2, n=65, n_tap=0)
    org = dgr6_cpu.origin(cells)
    for a in (0, 3, 5):
        far = cells.copy(); far[3, a] = org[a] + dgr6_cpu.REL_MAX + 1        # one past the limit
        assert dgr6_cpu.status_of(far) == 3
        out = m.logits(far)
        assert m.last_info == dict(status=3, n=65, n_tap=0) and not host(out).any()
        both = far.copy(); both[-1] = both[7]                                # with a duplicate: the limit wins
        m.logits(both); assert m.last_info["status"] == 3
        edge = cells.copy(); edge[3, a] = org[a] + dgr6_cpu.REL_MAX          # the last admitted extent
        assert dgr6_cpu.status_of(edge) == 0
        got = host(m.logits(edge))
        assert m.last_info["status"] == 0
        assert np.array_equal(bits(got), bits(dgr6_cpu.run(edge, stages(THIN), mode="chain")["logit"])), a
    out = m.logits(np.zeros((0, 6), np.int32))
    assert m.last_info == dict(status=0, n=0, n_tap=0) and out.shape == (0,)


# ---- 4. F10 -----------------------------------------------------------------------------------------------------------------------------
def test_same_bits_whatever_the_scratch_the_row_order_or_a_shift_by_eight():
    rows = np.array(corr_rows())
    n = len(rows)
    assert 3000 < n < 5000 and dgr6_cpu.status_of(rows) == 0
    m = model(WIDTHS)
    a = host(m.logits(rows, poison=0xFF))
    assert m.last_info["status"] == 0 and np.isfinite(a).all() and a.std() > 0
    assert np.array_equal(bits(a), bits(host(m.logits(rows, poison=0x00))))
    perm = np.random.default_rng(1).permutation(n)
    assert np.array_equal(bits(a[perm]), bits(host(m.logits(rows[perm]))))
    for ax in range(6):
        shift = np.zeros(6, np.int64); shift[ax] = 8 * (ax + 1) * (-1) ** ax * 1000
        assert np.array_equal(bits(a), bits(host(m.logits((rows + shift).astype(np.int32))))), ax
    assert np.array_equal(bits(a), bits(host(m.logits((rows + np.array([8, -16, 24, -8, 800, -8000])).astype(np.int32)))))
    L = dgr6_cpu.levels(rows)                           # the coarse sets at this size too (the sort, four rounds above one chunk)
    for s, lvl in ((4, 1), (10, 3)):
        assert np.array_equal(host(m.tap(rows, s)[1]), L[lvl]), (s, lvl)


# ---- 5. value check at size -------------------------------------------------------------------------------------------------------------
def test_values_at_4000_rows_within_four_times_the_fp32_yardstick():
    """d32 = max |fp32 matmul-per-offset restatement - fp64 restatement| of the logits on this input; the device must lie within 4 x d32 of
    fp64: the two fp32 evaluations differ in summation order only, while a wrong map entry shows at order 1.
    Measured: n = 4 069, logits up to 0.68, d32 = 1.11e-07, the device 1.42e-07 from fp64, bound 4.45e-07."""
    rows = np.array(corr_rows())
    r64 = dgr6_cpu.run(rows, stages(WIDTHS), mode="f64")["logit"]
    d32 = float(np.abs(dgr6_cpu.run(rows, stages(WIDTHS), mode="f32mm")["logit"] - r64).max())
    got = host(model(WIDTHS).logits(rows))
    dev = float(np.abs(got - r64).max())
    print(f"n = {len(rows)}: |logit| up to {np.abs(r64).max():.3e}, d32 = {d32:.3e}, device vs fp64 = {dev:.3e}, bound 4 x d32 = {4 * d32:.3e}")
    assert d32 > 0 and dev <= 4 * d32


# ---- 6. the Python layer ----------------------------------------------------------------------------------------------------------------
def test_weights_are_the_sigmoid_of_the_restatements_logits():
    rng = np.random.default_rng(4)
    xyz0 = rng.uniform(-3, 3, (300, 3)); xyz1 = rng.uniform(-3, 3, (280, 3))
    c0, k0 = np.unique(np.floor(xyz0 / 0.3).astype(np.int64), axis=0, return_index=True)
    xyz0 = xyz0[np.sort(k0)]
    idx0 = np.arange(len(xyz0)); idx1 = rng.integers(0, len(xyz1), len(xyz0))
    rows = np.concatenate([np.floor(xyz0 / 0.3), np.floor(xyz1 / 0.3)[idx1]], 1).astype(np.int32)
    m = model(THIN)
    assert np.array_equal(host(m.coords6(xyz0, xyz1, idx0, idx1, 0.3)), rows)
    want = dgr6_cpu.run(rows, stages(THIN), mode="chain")["logit"]
    assert np.array_equal(bits(host(m.logits(rows))), bits(want))
    w = m.weights(xyz0, xyz1, idx0, idx1, voxel_size=0.3)
    assert w.dtype == torch.float32 and w.shape == (len(rows),)
    assert np.array_equal(bits(host(w)), bits(host(torch.sigmoid(torch.from_numpy(want).cuda()))))
    assert np.allclose(host(w), 1.0 / (1.0 + np.exp(-want.astype(np.float64))), rtol=1e-6, atol=0)
    fn = functools.partial(m.weights, voxel_size=0.3)                       # the weights_fn of DGRTail
    tail = dgr.DGRTail(voxel_size=0.3, weights_fn=fn, use_icp=False)
    a = tail.register(xyz0, xyz1, idx0, idx1)
    b = dgr.DGRTail(voxel_size=0.3, use_icp=False).register(xyz0, xyz1, idx0, idx1, weights=w)
    assert np.array_equal(a["base"], b["base"])
    state = dgr6_cases.make_state_dict(THIN, seed=3)
    net = dgr.InlierNet.from_state_dict(state)
    assert np.array_equal(bits(host(net.logits(rows))), bits(dgr6_cpu.run(rows, dgr.inlier_fold(state), mode="chain")["logit"]))
    with pytest.raises(ValueError, match="at most 131072"):
        m.logits(np.zeros((131073, 6), np.int32))


@functools.lru_cache(maxsize=None)
def fcgf_model():
    return fcgf.FCGF.from_state_dict(fcgf_cases.make_state_dict(0, 5), 5)


def test_register_is_the_tail_on_the_networks_own_weights():
    raw0, raw1, T = synth.make_scan_pair(n0=6000, seed=5)
    reg = dgr.DGR(fcgf_model(), model(THIN), voxel_size=0.3)
    res = reg.register(raw0, raw1)
    L = reg.last
    m = L["m"]
    assert 3000 < m <= dgr.MAX_TAIL and L["m_tail"] == m
    # the stages, each against its own entry: voxel de-duplication, FCGF, the feature nearest neighbour, the 6-D cells
    x0, f0, sel0 = fcgf_model().extract(raw0, 0.3)
    x1, f1, sel1 = fcgf_model().extract(raw1, 0.3)
    assert m == x0.shape[0] and np.array_equal(host(L["xyz0"]), host(x0)) and np.array_equal(host(L["xyz1"]), host(x1))
    from lidarregistration_amd.matching import find_nn
    i0, i1, _ = find_nn(f0, f1)
    assert np.array_equal(host(L["idx0"]), i0.numpy()) and np.array_equal(host(L["idx1"]), i1.numpy())
    rows = np.concatenate([np.floor(raw0[host(sel0)] / 0.3), np.floor(raw1[host(sel1)] / 0.3)[i1.numpy()]], 1).astype(np.int32)
    w = torch.sigmoid(model(THIN).logits(rows))
    assert np.array_equal(bits(host(L["weights"])), bits(host(w)))
    want = dgr.DGRTail(voxel_size=0.3).register(x0, x1, i0, i1, weights=w)
    assert np.array_equal(res["base"], want["base"]) and np.array_equal(res["w_icp"], want["w_icp"])
    assert np.isfinite(res["base"]).all() and L["tail"]["path"] in ("refinement", "safeguard")
    only = reg.register(raw0, raw1, only_calc_weights=True)
    assert torch.is_tensor(only) and np.array_equal(bits(host(only)), bits(host(w)))


def test_register_drops_the_clipped_rows_of_a_set_above_the_tails_limit():
    """More than 32 768 correspondences: the rows below the clip never reach the tail, the weight-sum threshold keeps the original count.
    The final bias is set from the logits' own quantile so that a few thousand rows survive the clip."""
    raw0, raw1, T = synth.make_scan_pair(n0=60000, seed=7)
    base = dgr.DGR(fcgf_model(), model(THIN), voxel_size=0.3, clip_weight_thresh=0.05)
    w0 = host(base.register(raw0, raw1, only_calc_weights=True)).astype(np.float64)
    m = len(w0)
    assert dgr.MAX_TAIL < m <= dgr.MAX_N
    w0 = np.clip(w0, 1e-7, 1 - 1e-7)
    logit0 = np.log(w0 / (1 - w0))
    st = [tuple(s) for s in stages(THIN)]
    shift = np.log(0.05 / 0.95) - np.quantile(logit0, 1 - 3000.0 / m)
    st[22] = (st[22][0], st[22][1], (st[22][2] + np.float32(shift)).astype(np.float32))
    net = dgr.InlierNet.from_stages(st)
    reg = dgr.DGR(fcgf_model(), net, voxel_size=0.3, clip_weight_thresh=0.05)
    res = reg.register(raw0, raw1)
    L = reg.last
    w = host(L["weights"])
    keep = (w > 0) & (w >= np.float32(0.05))
    assert L["m"] == m and 1000 < keep.sum() < 10000 and L["m_tail"] == int(keep.sum())
    assert np.array_equal(host(L["idx0_tail"]), np.nonzero(keep)[0]) and np.array_equal(host(L["idx1_tail"]), host(L["idx1"])[keep])
    assert np.array_equal(bits(host(L["weights_tail"])), bits(w[keep]))
    w1 = float(w[keep].astype(np.float64).sum())
    info = L["tail"]
    expect = "refinement" if w1 >= max(4000, m) * 0.05 * (1 + 1e-9) else "safeguard" if w1 <= max(4000, m) * 0.05 * (1 - 1e-9) else info["path"]
    assert info["path"] == expect and info["L"] == int(keep.sum())
    want = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=0.05).register(L["xyz0"], L["xyz1"], np.nonzero(keep)[0], host(L["idx1"])[keep],
                                                                         weights=w[keep], m_threshold=m)
    assert np.array_equal(res["base"], want["base"]) and np.array_equal(res["w_icp"], want["w_icp"])
    st[22] = (st[22][0], st[22][1], np.array([30.0], np.float32))              # every weight 1: nothing to drop, the tail's limit stands
    with pytest.raises(ValueError, match="lr_dgr_refine takes at most 32768"):
        dgr.DGR(fcgf_model(), dgr.InlierNet.from_stages(st), voxel_size=0.3).register(raw0, raw1)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_device_memory():
    L = _ext.lib()
    m = model(THIN)
    n = 65
    cells = torch.from_numpy(np.array(CASES["clusters65"])).cuda()
    w8 = (ctypes.c_int32 * 8)(*THIN)
    need = L.lr_dgr_inlier_scratch_bytes(n, ctypes.byref(w8))
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    res = torch.zeros(16, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    p = _ext.DgrInlierParams(widths=THIN)
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()
    wp, wb = m.weights_blob.data_ptr(), m.weights_blob.numel() * 4

    def call(coords=cells.data_ptr(), rows=n, w=wp, wbytes=wb, r=res.data_ptr(), o=out.data_ptr(), ptr=None, nbytes=need):
        return L.lr_dgr_inlier(coords, rows, w, wbytes, ctypes.byref(p), r, o, None, scratch.data_ptr() if ptr is None else ptr, nbytes, st)
    assert call() == 0
    assert call(rows=131073) == -1 and "n must lie" in err()
    assert call(coords=None) == -1 and "null coords" in err()
    assert call(o=None) == -1 and "null coords or logit_out" in err()
    assert call(r=None) == -1 and "null result" in err()
    assert call(w=None) == -1 and "null weights" in err()
    assert call(nbytes=need - 1) == -1 and "scratch too small" in err()
    assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
    assert call(w=wp + 4) == -1 and "16-byte" in err()
    assert call(wbytes=wb - 4) == -1 and "weights_bytes" in err()
    hostbuf = np.zeros(need + 256, np.uint8)
    assert call(ptr=(hostbuf.ctypes.data + 255) & ~255) == -1 and "not device memory" in err()
    assert call() == 0
    torch.cuda.synchronize()
    want = dgr6_cpu.run(CASES["clusters65"], stages(THIN), mode="chain")["logit"]
    assert np.array_equal(bits(host(out)), bits(want)) and L.lr_version() == 103
