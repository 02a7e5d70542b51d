"""lr_fcgf_extract_batch on the GPU (contract n2: csrc/lr_fcgf_batch.h through fcgf.FCGF.features_batch).

The contract is B2: every cloud of a batch comes out with the BYTES of lr_fcgf_extract on that cloud alone, which tests/test_gpu_fcgf.py
holds to the fmaf-chain restatement bit for bit; the four smallest cases are compared with that restatement here as well, so this file
does not rest on the device alone.  No tolerance anywhere.  The shapes are the smallest at which each mechanism can go wrong: a cloud
boundary inside and on a 64- and a 128-row tile, the sort's 2 048-key chunk, equal cells under different tags, the 19-bit field's edge."""
import ctypes
import os

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, fcgf, harness, io_lists, synth
from tests import fcgf_cases, fcgf_cpu
from tests.test_gpu_fcgf import CASES, bits, host, model, scan_cells, stages

pytestmark = pytest.mark.gpu
LIMIT = (1 << 18) - 2                # the batch entry's range limit (B2)
_SINGLE = {}


def single(cells, k1=5, feat_in=None):
    """(rows, result block) of lr_fcgf_extract on this cloud alone: computed once per input, shared and read-only."""
    cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 3)
    key = (cells.tobytes(), k1, None if feat_in is None else np.asarray(feat_in, np.float32).tobytes())
    if key not in _SINGLE:
        m = model(k1)
        out = host(m.features(cells, feat_in))
        out.setflags(write=False)
        _SINGLE[key] = (out, dict(m.last_info))
    return _SINGLE[key]


def run_batch(clouds, k1=5, feat_in=None, poison=None):
    m = model(k1)
    outs = [host(o) for o in m.features_batch([np.ascontiguousarray(c) for c in clouds], feat_in, poison)]      # (a reversed view has negative strides)
    return outs, [dict(i) for i in m.last_info]


def assert_equals_single(clouds, k1=5, feat_in=None, poison=None):
    outs, infos = run_batch(clouds, k1, feat_in, poison)
    assert len(outs) == len(infos) == len(clouds)
    for b, cells in enumerate(clouds):
        want, info = single(cells, k1, None if feat_in is None else feat_in[b])
        assert infos[b] == info, (b, infos[b], info)
        assert outs[b].shape == want.shape == (len(cells), 32), (b, outs[b].shape)
        bad = np.nonzero((bits(outs[b]) != bits(want)).any(1))[0]
        assert bad.size == 0, (b, len(cells), bad[:8])
    return outs


def clouds_of(sizes, box=12, seed=500):
    """Random clouds of these sizes in overlapping boxes (the same cells occur in several of them), rows shuffled."""
    return [fcgf_cases.random_cells(n, box, seed + 17 * b, lo=-(box // 2) + (b % 3)) if n else np.zeros((0, 3), np.int32) for b, n in enumerate(sizes)]


# ---- single entries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k1", [(n, 5) for n in CASES] + [(n, 3) for n in fcgf_cases.K3_CASES], ids=lambda v: str(v))
def test_a_batch_of_one_is_the_single_call(name, k1):
    out = assert_equals_single([CASES[name]], k1)[0]
    if k1 == 5 and name in ("one", "two_adjacent", "block3_origin", "random65"):
        want = fcgf_cpu.run(CASES[name], stages(5), 5, mode="chain")["out"]
        assert np.array_equal(bits(out), bits(want)), name


# ---- tile edges across clouds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(63, 1, 64, 65), (127, 129), (128, 128), (0, 40, 1), (1, 40, 0), (40, 0, 1, 0, 40), (0, 0, 5), (0,), (1,)],
                         ids=lambda s: "-".join(map(str, s)))
def test_cloud_boundaries_inside_and_on_the_row_tiles(sizes):
    assert_equals_single(clouds_of(sizes))


# ---- the sort's chunk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(1500, 547), (1500, 548), (1500, 549), (1500, 1000, 1597)], ids=lambda s: str(sum(s)))
def test_totals_around_the_sort_chunk_with_a_cloud_across_it(sizes):
    """The second cloud ends one row before the chunk's edge, on it, and lies across it (2 049 and 4 097: two and four chunks)."""
    assert sum(sizes) in (2047, 2048, 2049, 4097) and sizes[0] < 2047 <= sizes[0] + sizes[1] and (sum(sizes) <= 2048 or sizes[0] + sizes[1] > 2048)
    assert_equals_single(clouds_of(sizes, box=24, seed=900))


# ---- tags -------------------------------------------------------------------------------------------------------------------------------
def test_equal_cells_in_different_clouds_are_not_duplicates():
    a = CASES["random129"]
    assert_equals_single([a, a.copy()])                                           # the same cells twice
    b = np.concatenate([a[:64], fcgf_cases.random_cells(70, 12, 77, lo=40)])       # half of a's cells and others
    assert_equals_single([a, b, a[::-1]])
    cell = np.array([[3, -2, 5]], np.int32)
    outs = assert_equals_single([cell] * 64)                                       # 64 one-cell clouds at one cell
    assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs)


# ---- order ------------------------------------------------------------------------------------------------------------------------------
def test_batch_order_and_row_order_change_no_bit():
    clouds = clouds_of((63, 1, 64, 65, 130))
    outs = assert_equals_single(clouds)
    rev = assert_equals_single(clouds[::-1])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs, rev[::-1]))
    rng = np.random.default_rng(4)
    perms = [rng.permutation(len(c)) for c in clouds]
    shuffled, _ = run_batch([c[p] for c, p in zip(clouds, perms)])
    assert all(np.array_equal(bits(o[p]), bits(s)) for o, p, s in zip(outs, perms, shuffled))


# ---- range ------------------------------------------------------------------------------------------------------------------------------
def test_range_limit_of_the_19_bit_fields_and_a_shift_by_8192():
    base = np.array(CASES["random65"])
    edge = base.copy()
    edge[0] = [LIMIT - 1, -(LIMIT - 1), LIMIT - 1]; edge[1] = [-(LIMIT - 1), LIMIT - 1, -(LIMIT - 1)]          # +-(2^18 - 3): the last admitted cells
    other = CASES["random64"]
    outs = assert_equals_single([other, edge, base])
    assert single(edge)[1]["status"] == 0
    for axis in range(3):
        for v in (LIMIT, -LIMIT):
            far = base.copy(); far[5, axis] = v
            got, infos = run_batch([other, far, base])
            assert infos[1] == dict(status=3, n=65, n_tap=0) and got[1].shape == (65, 32) and not got[1].any(), (axis, v)
            assert infos[0]["status"] == 0 and infos[2]["status"] == 0
            assert np.array_equal(bits(got[0]), bits(outs[0])) and np.array_equal(bits(got[2]), bits(outs[2])), (axis, v)
    for axis in range(3):
        moved = base.copy(); moved[:, axis] += 8192
        got, infos = run_batch([moved, other, (base + 8192).astype(np.int32)])
        assert all(i["status"] == 0 for i in infos)
        assert np.array_equal(bits(got[0]), bits(outs[2])) and np.array_equal(bits(got[2]), bits(outs[2])) and np.array_equal(bits(got[1]), bits(outs[0]))


# ---- duplicates -------------------------------------------------------------------------------------------------------------------------
def test_status_is_per_cloud_and_refused_clouds_leave_the_others_alone():
    a, b = np.array(CASES["random65"]), np.array(CASES["random129"])
    dup = a.copy(); dup[-1] = dup[7]
    both = dup.copy(); both[0, 2] = LIMIT                                          # a duplicate and a cell past the range: 3 wins
    want_a, want_b = single(a)[0], single(b)[0]
    got, infos = run_batch([a, dup, b, both, a])
    assert [i["status"] for i in infos] == [0, 2, 0, 3, 0]
    assert infos[1] == dict(status=2, n=65, n_tap=0) and infos[3] == dict(status=3, n=65, n_tap=0)
    assert not got[1].any() and not got[3].any() and got[1].shape == got[3].shape == (65, 32)
    assert np.array_equal(bits(got[0]), bits(want_a)) and np.array_equal(bits(got[4]), bits(want_a)) and np.array_equal(bits(got[2]), bits(want_b))
    assert single(dup)[1] == infos[1]                                              # the single call's block for the same cloud
    got, infos = run_batch([dup, both, dup[::-1]], poison=0xFF)                    # every cloud refused: rows of zeros, LR_OK
    assert [i["status"] for i in infos] == [2, 3, 2] and not any(g.any() for g in got)


# ---- feature inputs -----------------------------------------------------------------------------------------------------------------------
def test_feat_in_entries_may_be_null_values_or_carry_a_nan():
    a, b, c = np.array(CASES["random65"]), np.array(CASES["random33"]), np.array(CASES["random129"])
    rng = np.random.default_rng(2)
    fb = rng.uniform(0.5, 2.0, len(b)).astype(np.float32)
    fc = rng.uniform(0.5, 2.0, len(c)).astype(np.float32); fc[5] = np.nan
    outs = assert_equals_single([a, b, c, b], feat_in=[None, fb, fc, None])
    assert np.isnan(outs[2]).any() and np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all() and np.isfinite(outs[3]).all()
    assert not np.array_equal(bits(outs[1]), bits(outs[3]))
    want = fcgf_cpu.run(b, stages(5), 5, feat_in=fb, mode="chain")["out"]
    assert np.array_equal(bits(outs[1]), bits(want))
    ones = assert_equals_single([a, b], feat_in=[np.ones(len(a), np.float32), None])      # explicit ones = NULL
    assert np.array_equal(bits(ones[0]), bits(outs[0]))
    assert_equals_single([a, b])                                                    # the whole array NULL


# ---- scratch ------------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_whatever_the_scratch_held():
    clouds = clouds_of((63, 1, 64, 65, 0, 300), box=14)
    dup = clouds[3].copy(); dup[3] = dup[9]
    clouds[3] = dup
    a, ia = run_batch(clouds, poison=0xFF)
    b, ib = run_batch(clouds, poison=0x00)
    assert ia == ib and [i["status"] for i in ia] == [0, 0, 0, 2, 0, 0]
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert_equals_single(clouds, poison=0xFF)


# ---- size limits and the refusals that need a device ------------------------------------------------------------------------------------------
def test_size_limits_and_refusals_leave_the_outputs_untouched():
    L = _ext.lib()
    m = model()
    B = 65
    cells = torch.from_numpy(np.tile(np.array([[3, -2, 5]], np.int32), (B, 1))).cuda()
    out = torch.full((B, 32), 7.0, dtype=torch.float32, device="cuda")
    res = torch.full((B * 16,), 0x55, dtype=torch.uint8, device="cuda")
    need = L.lr_fcgf_batch_scratch_bytes(64, 64)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()

    def call(nclouds, ns=None, tap=0, nbytes=need, ptr=None):
        ns = [1] * nclouds if ns is None else ns
        vp = lambda t: (ctypes.c_void_p * len(ns))(*[t[k:].data_ptr() for k in range(len(ns))])
        p = _ext.FcgfParams(tap=tap)
        return L.lr_fcgf_extract_batch(nclouds, vp(cells), None, (ctypes.c_int32 * len(ns))(*ns), m.weights.data_ptr(), m.weights.numel() * 4, ctypes.byref(p),
                                       res.data_ptr(), vp(out), scratch.data_ptr() if ptr is None else ptr, nbytes, st)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 7.0).all()) and bool((res == 0x55).all())
    assert call(65) == -1 and "nclouds" in err() and untouched()
    assert call(2, ns=[1 << 20, 1]) == -1 and "sum of n" in err() and untouched()        # refused before any launch: nothing is read or written
    assert call(3, tap=1) == -1 and "tap" in err() and untouched()
    assert call(64, nbytes=need - 1) == -1 and "scratch too small" in err() and untouched()
    assert call(64, ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err() and untouched()
    hostbuf = np.zeros(need + 256, np.uint8)
    assert call(64, ptr=(hostbuf.ctypes.data + 255) & ~255) == -1 and "not device memory" in err() and untouched()
    assert call(64) == 0                                                                  # 64 clouds are accepted
    torch.cuda.synchronize()
    want = single(np.array([[3, -2, 5]], np.int32))[0]
    got = host(out)
    assert np.array_equal(bits(got[:64]), bits(np.tile(want, (64, 1)))) and (got[64] == 7.0).all()
    blocks = host(res).view(np.int32).reshape(B, 4)
    assert blocks[:64].tolist() == [[0, 1, 1, 0]] * 64 and (host(res)[64 * 16:] == 0x55).all()
    assert L.lr_version() == 103


# ---- graph replay -------------------------------------------------------------------------------------------------------------------------
def test_a_three_cloud_batch_can_be_captured_into_a_graph():
    L = _ext.lib()
    m = model()
    sizes = (63, 130, 65)
    sets = [clouds_of(sizes, seed=s) for s in (31, 32)]
    dev = [torch.empty((n, 3), dtype=torch.int32, device="cuda") for n in sizes]
    outs = [torch.empty((n, 32), dtype=torch.float32, device="cuda") for n in sizes]
    res = torch.empty(3 * 16, dtype=torch.uint8, device="cuda")
    sc = torch.empty(L.lr_fcgf_batch_scratch_bytes(3, sum(sizes)), dtype=torch.uint8, device="cuda")
    p = _ext.FcgfParams()
    s = torch.cuda.Stream()
    vp = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])

    def call():
        _ext.check(L.lr_fcgf_extract_batch(3, vp(dev), None, (ctypes.c_int32 * 3)(*sizes), m.weights.data_ptr(), m.weights.numel() * 4, ctypes.byref(p),
                                           res.data_ptr(), vp(outs), sc.data_ptr(), sc.numel(), s.cuda_stream))

    def load(clouds, poison):
        for t, c in zip(dev, clouds):
            t.copy_(torch.from_numpy(c))
        for o in outs:
            o.fill_(7.0)
        res.fill_(0x55); sc.fill_(poison)
        torch.cuda.synchronize()

    def outputs():
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in outs + [res]]
    eager = []
    for clouds in sets:
        load(clouds, 0x00); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k in (1, 0, 1):
        load(sets[k], 0xFF if k else 0x00); g.replay()
        assert outputs() == eager[k], k
    assert eager[0] != eager[1]
    for clouds, e in zip(sets, eager):
        for b, c in enumerate(clouds):
            assert e[b] == single(c)[0].tobytes()


# ---- the bench hook -------------------------------------------------------------------------------------------------------------------------
def test_bench_hook_ends_a_call_behind_conv1_and_is_undone_by_zero():
    """lr_debug_fcgf_batch_stop_after(1): the call returns LR_OK and writes the result blocks but no features (the wrapper's zeros stay);
    stage 0 restores the contract."""
    L = _ext.lib()
    clouds = clouds_of((63, 65))
    want = assert_equals_single(clouds)
    L.lr_debug_fcgf_batch_stop_after(1)
    try:
        cut, infos = run_batch(clouds)
    finally:
        L.lr_debug_fcgf_batch_stop_after(0)
    assert [i["status"] for i in infos] == [0, 0] and not any(c.any() for c in cut) and any(w.any() for w in want)
    assert_equals_single(clouds)


# ---- a frame-sized batch ------------------------------------------------------------------------------------------------------------------
def test_two_small_frames_and_a_30000_voxel_frame_in_one_batch():
    small, big = np.array(scan_cells(4400)), np.array(scan_cells(40000))
    assert 3000 < len(small) < 5000 and 24000 < len(big) < 36000
    outs = assert_equals_single([small, big, small[::-1]], poison=0xFF)
    assert np.isfinite(outs[1]).all() and np.allclose(np.linalg.norm(outs[1], axis=1), 1.0, atol=1e-5)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def same_tensor(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and np.array_equal(host(a).view(np.uint8), host(b).view(np.uint8))


def test_extract_batch_and_extract_pairs_equal_extract_and_extract_pair():
    m = model()
    raws = [synth.make_scan_pair(n0=3000, seed=5), synth.make_scan_pair(n0=2000, seed=6)]
    scans = [raws[0][0], raws[0][1], raws[1][0]]
    got = m.extract_batch(scans, 0.3)
    assert [i["status"] for i in m.last_info] == [0, 0, 0]
    for raw, (xyz, feats, sel) in zip(scans, got):
        x1, f1, s1 = m.extract(raw, 0.3)
        assert same_tensor(xyz, x1) and same_tensor(feats, f1) and same_tensor(sel, s1)
    pairs = m.extract_pairs([(r[0], r[1]) for r in raws], 0.3)
    for r, got4 in zip(raws, pairs):
        want4 = m.extract_pair(r[0], r[1], 0.3)
        assert len(got4) == 4 and all(same_tensor(a, b) for a, b in zip(got4, want4))
    far = scans[1].copy(); far[0] = [0.3 * (LIMIT + 5), 0.0, 0.0]
    with pytest.raises(_ext.LidarRegError, match="cloud 1: status 3"):
        m.extract_batch([scans[0], far], 0.3)


def test_eval_pairs_through_finish_window_equals_the_per_cloud_path(tmp_path, monkeypatch):
    """A cloud directory built as tests/test_gpu_fcgf_cli.py builds its own (raw scans, a balanced list, no feature cache): the window path
    (one batched extraction per window, device tensors) against the per-cloud path (finish per row), every non-time column and the motions."""
    from tests.conftest import Args
    name = io_lists.DATASET_NAMES["A"]
    clouds, sets = tmp_path / "clouds", tmp_path / "sets"
    os.makedirs(sets / name)
    rows = []
    for k, seed in enumerate((8, 9)):
        raw0, raw1, T = synth.make_scan_pair(n0=5000, seed=seed)
        io_lists.save_ref_cloud(str(clouds / name), 4, 10 + 2 * k, raw0); io_lists.save_ref_cloud(str(clouds / name), 4, 11 + 2 * k, raw1)
        rows += [(10 + 2 * k, 11 + 2 * k, T), (11 + 2 * k, 10 + 2 * k, np.linalg.inv(T))]
    with open(sets / name / "test.txt", "w") as f:
        f.write("session_ind i j " + " ".join(f"mot{k}" for k in range(16)) + "\n")
        for i, j, M in rows:
            f.write(f"4 {i} {j} " + " ".join("%.17g" % v for v in M.reshape(-1)) + "\n")
    src = harness.RefCloudSource(io_lists.read_pair_list(str(sets / name / "test.txt")), str(clouds / name), None, extractor=model())
    a = Args(mode="MNN", codebase="GC", iters=2000, prosac=True, icp=False)
    calls = []
    real = fcgf.FCGF.extract_batch

    def counted(self, raws, voxel_size=0.3):
        calls.append(len(raws))
        return real(self, raws, voxel_size)
    monkeypatch.setattr(fcgf.FCGF, "extract_batch", counted)
    s1, T1 = harness.eval_pairs(src, [0, 1, 2, 3], a, batch=2, in_flight=2, workers=2)
    assert calls == [4]                                                             # four pairs over four distinct scans: each extracted once
    monkeypatch.delattr(harness.RefCloudSource, "finish_window")
    s0, T0 = harness.eval_pairs(src, [0, 1, 2, 3], a, batch=2, in_flight=2, workers=2)
    assert calls == [4]
    for c in (0, 1, 2, 15, 16, 17, 18, 19, 20, 21):
        assert np.array_equal(s1[:, c], s0[:, c], equal_nan=True), (c, s1[:, c], s0[:, c])
    assert np.array_equal(T1, T0) and np.isfinite(T1).all() and s1[:, 19:22].tolist() == [[4, i, j] for i, j, _ in rows]
