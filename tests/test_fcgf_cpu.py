"""The yardsticks of the FCGF extractor, without a GPU: the fmaf emulation of tests/fcgf_cpu.py against libm, the conventions of the
restatement (levels, kernel maps, offset order, stage order, epilogues) against torch's DENSE conv3d / conv_transpose3d -- the check that
stands in for MinkowskiEngine, which neither the reference tree nor this project ships --, the three arithmetic modes against each other,
the state-dict packing, and the size functions and host-side refusals of the C ABI."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, fcgf
from tests import fcgf_cases, fcgf_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the fmaf emulation -----------------------------------------------------------------------------------------------------------
def _libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def test_fmaf32_equals_libm_including_half_ulp_ties():
    rng = np.random.default_rng(1)
    n = 30000
    a = rng.standard_normal(n).astype(np.float32); b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    # constructed ties: (1 + i 2^-12)(1 + j 2^-12) = 1 + (i + j) 2^-12 + i j 2^-24 lies exactly between two floats when i j is odd; an
    # addend far below the fp64 sum's last place decides the rounding, which (a * b + c) evaluated in fp64 and cast cannot see
    i = 2 * rng.integers(0, 600, n) + 1; j = 2 * rng.integers(0, 600, n) + 1
    ta = (1 + i * 2.0 ** -12).astype(np.float32); tb = (1 + j * 2.0 ** -12).astype(np.float32)
    tc = (rng.choice([-1.0, 1.0], n) * 2.0 ** -rng.integers(56, 100, n).astype(np.float64)).astype(np.float32)
    # ... and near-cancellation, where the sum's exponent drops
    ca = rng.standard_normal(n).astype(np.float32); cb = rng.standard_normal(n).astype(np.float32)
    cc = (-(ca.astype(np.float64) * cb.astype(np.float64)) * (1 + rng.integers(-3, 4, n) * 2.0 ** -24)).astype(np.float32)
    A, B, C = np.concatenate([a, ta, ca]), np.concatenate([b, tb, cb]), np.concatenate([c, tc, cc])
    f = _libm_fmaf()
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(A, B, C)], np.float32)
    got = fcgf_cpu.fmaf32(A, B, C)
    naive = (A.astype(np.float64) * B.astype(np.float64) + C.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (naive.view(np.uint32) != want.view(np.uint32)).sum() > 1000, "the constructed ties do not separate fmaf from a double rounding"


# ---- 2. the conventions, against torch's dense convolutions ----------------------------------------------------------------------------
def _dense_run(coords, stages, k1):
    """Stages 1..23 on dense [1, C, z, y, x] float64 grids of the 16^3 box -8..7 (level l: (16 >> l)^3, index (cell + 8) >> l)."""
    F = torch.nn.functional
    L = fcgf_cpu.levels(coords)
    idx = [((c + 8) >> l) for l, c in enumerate(L)]
    mask = []
    for l in range(4):
        S = 16 >> l
        m = torch.zeros((1, 1, S, S, S), dtype=torch.float64)
        m[0, 0, idx[l][:, 2], idx[l][:, 1], idx[l][:, 0]] = 1.0
        mask.append(m)
    t64 = lambda v: torch.from_numpy(np.asarray(v, np.float64))
    acts = {}

    def stage(s, x, kind, lvl, res=None, relu=0):
        W, sc, of = stages[s - 1]
        K = round(W.shape[0] ** (1 / 3))
        w5 = t64(W).reshape(K, K, K, W.shape[1], W.shape[2])              # [z][y][x]: idx(o) has x fastest
        if kind == "same":
            y = F.conv3d(x, w5.permute(4, 3, 0, 1, 2).contiguous(), padding=K // 2)
        elif kind == "down":
            y = F.conv3d(x, w5.permute(4, 3, 0, 1, 2).contiguous(), stride=2, padding=1)
        else:
            y = F.conv_transpose3d(x, w5.permute(3, 4, 0, 1, 2).contiguous(), stride=2, padding=1, output_padding=1)
        y = y * t64(sc).reshape(1, -1, 1, 1, 1) + t64(of).reshape(1, -1, 1, 1, 1)
        if res is not None:
            y = y + res
        if relu:
            y = torch.relu(y)
        y = y * mask[lvl]
        acts[s] = y[0][:, idx[lvl][:, 2], idx[lvl][:, 1], idx[lvl][:, 0]].T.numpy()
        return y

    def block(s, x, lvl):
        return stage(s + 1, stage(s, x, "same", lvl, None, 1), "same", lvl, x, 1)

    x = stage(1, mask[0].clone(), "same", 0)
    s1 = block(2, x, 0)
    s2 = block(5, stage(4, s1, "down", 1), 1)
    s4 = block(8, stage(7, s2, "down", 2), 2)
    s8 = block(11, stage(10, s4, "down", 3), 3)
    u = block(14, stage(13, s8, "up", 2), 2)
    u = block(17, stage(16, torch.cat([u, s4], 1), "up", 1), 1)
    u = block(20, stage(19, torch.cat([u, s2], 1), "up", 0), 0)
    x = stage(22, torch.cat([u, s1], 1), "same", 0, None, 1)
    stage(23, x, "same", 0)
    return acts


@pytest.mark.parametrize("n,k1,seed", [(300, 5, 1), (40, 5, 2), (300, 3, 3), (4096, 5, 4)], ids=["n300_k5", "n40_k5", "n300_k3", "full_box_k5"])
def test_restatement_fp64_equals_dense_torch_convolutions(n, k1, seed):
    """Both sides are fp64 and differ by summation order only: 27 x 256 terms x 2^-53 ~ 1e-12, so 1e-11 relative to the stage's largest
    magnitude leaves one decade of room."""
    coords = fcgf_cases.random_cells(n, 16, seed)                           # cells -8 .. 7: negative floor division included
    assert coords.min() < 0
    stages = fcgf.fold(fcgf_cases.make_state_dict(seed, k1), k1)
    want = _dense_run(coords, stages, k1)
    got = fcgf_cpu.run(coords, stages, k1, mode="f64")["acts"]
    for s in range(1, 24):
        d = np.abs(got[s] - want[s]).max() / np.abs(want[s]).max()
        assert got[s].shape == want[s].shape and d <= 1e-11, (s, d)


def test_levels_floor_negative_cells_and_sort_by_x_then_y_then_z():
    L = fcgf_cpu.levels(np.array([[-1, 0, 5], [3, -3, 0], [-1, 1, 4], [2, -4, 1]]))
    assert L[1].tolist() == [[-2, 0, 4], [2, -4, 0]] and L[2].tolist() == [[-4, 0, 4], [0, -4, 0]] and L[3].tolist() == [[-8, 0, 0], [0, -8, 0]]
    assert fcgf_cpu.status_of([[0, 0, 0], [1, 0, 0], [0, 0, 0]]) == 2 and fcgf_cpu.status_of([[0, 0, (1 << 20) - 2], [0, 0, 0], [0, 0, 0]]) == 3
    assert fcgf_cpu.status_of([[0, 0, (1 << 20) - 3], [0, -(1 << 20) + 3, 0]]) == 0


def test_transposed_map_is_the_transpose_of_the_strided_map():
    """F4 by hand: per axis a fine cell on the coarse lattice takes o = 0 only, any other o = +1 from the coarse cell below and o = -1 from
    the one above -- and the pairs are those of F3's map, read the other way."""
    L = fcgf_cpu.levels(fcgf_cases.random_cells(200, 12, 9))
    for l in range(3):
        t = 1 << l
        dn = {(k, int(a), int(b)) for k, ro, ri in fcgf_cpu.kernel_map(L[l + 1], L[l], 3, t) for a, b in zip(ro, ri)}       # (o, coarse, fine)
        up = {(k, int(b), int(a)) for k, ro, ri in fcgf_cpu.kernel_map(L[l], L[l + 1], 3, -t) for a, b in zip(ro, ri)}      # (o, coarse, fine)
        assert dn == up and len({u for _, _, u in dn}) == len(L[l])        # every fine cell is reached, at least from its own coarse cell
        for k, v, u in dn:
            o = np.array([k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1])
            fine, coarse = L[l][u], L[l + 1][v]
            on = fine % (2 * t) == 0
            below = coarse == (fine // (2 * t)) * (2 * t)
            assert (o[on] == 0).all() and below[on].all() and (o[~on] == np.where(below[~on], 1, -1)).all()


def test_the_three_arithmetics_agree_and_the_chain_differs_from_a_matmul_in_the_last_bits():
    coords = fcgf_cases.random_cells(60, 10, 5)
    stages = fcgf.fold(fcgf_cases.make_state_dict(5), 5)
    r64, rmm, rch = (fcgf_cpu.run(coords, stages, 5, mode=m) for m in ("f64", "f32mm", "chain"))
    assert rch["out"].dtype == np.float32 and rch["out"].shape == (60, 32)
    assert np.allclose(np.linalg.norm(r64["out"], axis=1), 1.0, atol=1e-6)
    d_mm, d_ch = np.abs(rmm["out"] - r64["out"]).max(), np.abs(rch["out"] - r64["out"]).max()
    assert 0 < d_mm < 1e-4 and 0 < d_ch < 1e-4
    f = np.random.default_rng(0).standard_normal(60).astype(np.float32)
    assert np.array_equal(fcgf_cpu.run(coords, stages, 5, feat_in=np.ones(60), upto=3)["acts"][3], rch["acts"][3])
    assert not np.array_equal(fcgf_cpu.run(coords, stages, 5, feat_in=f, upto=1)["acts"][1], rch["acts"][1])


# ---- 3. packing, sizes, refusals --------------------------------------------------------------------------------------------------------
def test_fold_rounds_once_and_the_blob_has_the_documented_layout():
    sd = fcgf_cases.make_state_dict(2)
    st32, st64 = fcgf.fold(sd, 5), fcgf.fold(sd, 5, np.float64)
    plan = fcgf.stage_plan(5)
    assert [(p[2], p[3], p[4]) for p in plan][:4] == [(125, 1, 32), (27, 32, 32), (27, 32, 32), (27, 32, 64)] and plan[21][2:] == (1, 96, 64)
    g, b, m, v = (np.asarray(sd["block3_tr.norm2.bn." + k], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + 1e-5)
    i = [p[0] for p in plan].index("block3_tr.conv2")
    assert np.array_equal(st64[i][1], s) and np.array_equal(st64[i][2], (0.0 - m) * s + b)
    assert np.array_equal(st32[i][1], s.astype(np.float32)) and np.array_equal(st32[i][2], ((0.0 - m) * s + b).astype(np.float32))
    assert np.array_equal(st32[21][1], np.ones(64, np.float32)) and not st32[21][2].any()                  # conv1_tr: no norm, no bias
    assert np.array_equal(st32[22][2], sd["final.bias"].reshape(-1)) and np.array_equal(st32[22][1], np.ones(32, np.float32))
    blob = fcgf.pack(sd, 5)
    assert blob.dtype == np.float32 and blob.size == fcgf.packed_floats(5) and blob.nbytes == _ext.lib().lr_fcgf_weights_bytes(5)
    assert np.array_equal(blob[:125 * 32], st32[0][0].reshape(-1)) and np.array_equal(blob[125 * 32:125 * 32 + 32], st32[0][1])
    assert np.array_equal(blob[-32:], st32[22][2]) and np.array_equal(blob[-64 - 64 * 32:-64], np.asarray(sd["final.kernel"]).reshape(-1))
    for (W, s_, o), (W2, s2, o2) in zip(fcgf.unpack(blob, 5), st32):
        assert np.array_equal(W, W2) and np.array_equal(s_, s2) and np.array_equal(o, o2)
    assert all((fcgf.packed_floats(k) * 4) % 16 == 0 for k in (3, 5)) and 34e6 < blob.nbytes < 37e6


def test_weights_bytes_and_one_by_one_kernel_forms():
    L = _ext.lib()
    assert [L.lr_fcgf_weights_bytes(k) for k in (0, 1, 4, 7)] == [0, 0, 0, 0]
    assert L.lr_fcgf_weights_bytes(5) - L.lr_fcgf_weights_bytes(3) == (125 - 27) * 32 * 4 and L.lr_fcgf_weights_bytes(3) == fcgf.packed_floats(3) * 4
    a, b = fcgf_cases.make_state_dict(3, 3, lead_one=False), fcgf_cases.make_state_dict(3, 3, lead_one=True)
    assert a["conv1_tr.kernel"].shape == (96, 64) and b["conv1_tr.kernel"].shape == (1, 96, 64) and b["final.kernel"].shape == (1, 64, 32)
    assert np.array_equal(fcgf.pack(a, 3), fcgf.pack(b, 3))
    a["final.bias"] = a["final.bias"].reshape(-1)                                                          # [32] as well as [1,32]
    assert np.array_equal(fcgf.pack(a, 3), fcgf.pack(b, 3))


def test_the_size_functions_keep_their_values():
    """Literal values, read from the library of the commit before the maps, the convolution and the layout moved into csrc/lr_sparse.h
    (built from that commit with the Makefile's flags): the layout function is shared now and must size every call as before."""
    L = _ext.lib()
    ns = (0, 1, 64, 65, 1 << 20)
    assert [L.lr_fcgf_scratch_bytes(n) for n in ns] == [65792, 436480, 436480, 807168, 6073417984]
    assert [L.lr_fcgf_batch_scratch_bytes(3, n) for n in ns] == [66048, 436736, 436736, 807424, 6073418240]
    assert [L.lr_fcgf_weights_bytes(k) for k in (3, 5)] == [35001728, 35014272]


def test_state_dict_refusals_name_the_key():
    sd = fcgf_cases.make_state_dict(4, 3)
    for key in ("conv1.kernel", "block2.norm1.bn.running_var", "final.bias", "conv3_tr.kernel", "norm4_tr.bn.weight"):
        bad = dict(sd); del bad[key]
        with pytest.raises(ValueError, match=re.escape(key)):
            fcgf.pack(bad, 3)
        bad = dict(sd); bad[key] = np.asarray(sd[key])[..., :-1]
        with pytest.raises(ValueError, match=re.escape(key) + " has shape"):
            fcgf.pack(bad, 3)
        bad = dict(sd); v = np.array(sd[key], np.float32); v.reshape(-1)[3] = np.nan; bad[key] = v
        with pytest.raises(ValueError, match=re.escape(key) + " holds a non-finite"):
            fcgf.pack(bad, 3)
    with pytest.raises(ValueError, match="conv1.kernel has shape"):
        fcgf.pack(sd, 5)                                                                                   # a K = 3 checkpoint read as K = 5
    with pytest.raises(ValueError, match="conv1_kernel_size"):
        fcgf.stage_plan(4)
    bad = dict(sd); bad["norm1.bn.running_var"] = np.full(32, -1.0, np.float32)
    with pytest.raises(ValueError, match="norm1.bn.running_var"):
        fcgf.pack(bad, 3)


def test_cli_flag_without_a_cloud_cache_is_a_parser_error_that_says_so(tmp_path, monkeypatch, capsys):
    import importlib
    import sys
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "Experiments"))
    for v in ("LIDARREG_CLOUD_CACHE", "LIDARREG_BALANCED_SETS", "LIDARREG_FEATURE_CACHE"):
        monkeypatch.delenv(v, raising=False)
    cli = importlib.import_module("test")
    assert cli.get_args(["--dataset", "synthetic", "--num_pairs", "1"]).fcgf_weights_file is None              # the default: nothing changes
    for argv in (["--dataset", "A"], ["--dataset", "synthetic"]):
        with pytest.raises(SystemExit):
            cli.get_args(argv + ["--fcgf_weights_file", "w.pth"])
        assert "cloud cache" in capsys.readouterr().err
    monkeypatch.setenv("LIDARREG_CLOUD_CACHE", str(tmp_path)); monkeypatch.setenv("LIDARREG_BALANCED_SETS", str(tmp_path))
    assert cli.get_args(["--dataset", "A", "--fcgf_weights_file", "w.pth"]).fcgf_weights_file == "w.pth"
    with pytest.raises(SystemExit):
        cli.get_args(["--dataset", "synthetic", "--fcgf_weights_file", "w.pth"])
    sys.modules.pop("test", None)


def test_scratch_bytes_is_linear_and_closed_outside_the_range():
    L = _ext.lib()
    f = L.lr_fcgf_scratch_bytes
    assert f(-1) == 0 and f((1 << 20) + 1) == 0 and f(0) > 0 and f(1 << 20) > 0
    per = f(128) - f(64)
    assert per > 0 and all(f(64 * k) == f(0) + per * k for k in (1, 2, 3, 100, 4097, 1 << 14))
    assert all(f(64 * k + r) == f(64 * (k + 1)) for k in (0, 5) for r in (1, 63))                           # rows are rounded up to 64
    assert f(0) % 256 == 0 and per % 256 == 0
    assert per // 64 >= 3 * 256 * 4 + (32 + 64 + 128) * 4 + 125 * 4 + 10 * 27 * 4                            # three 256-channel buffers, the skips, the maps


def test_refusals_before_any_launch_name_the_argument():
    """F12 without a device: every pointer below is a made-up address that a refused call never reads."""
    L = _ext.lib()
    need_w, need_s = L.lr_fcgf_weights_bytes(5), L.lr_fcgf_scratch_bytes(100)
    ok = dict(coords=0x10000, feat_in=None, n=100, w=0x20000, wb=need_w, p=_ext.FcgfParams(), res=0x30000, out=0x40000, tc=None, s=None, sb=need_s)

    def call(**kw):
        a = {**ok, **kw}
        rc = L.lr_fcgf_extract(a["coords"], a["feat_in"], a["n"], a["w"], a["wb"], ctypes.byref(a["p"]) if a["p"] is not None else None, a["res"],
                               a["out"], a["tc"], a["s"], a["sb"], None)
        return rc, L.lr_last_error().decode()
    p = _ext.FcgfParams(); p.struct_size = 8
    cases = [(dict(p=p), "struct_size"), (dict(p=None), "null params"), (dict(p=_ext.FcgfParams(conv1_kernel_size=4)), "conv1_kernel_size"),
             (dict(p=_ext.FcgfParams(tap=24)), "tap"), (dict(p=_ext.FcgfParams(tap=-1)), "tap"), (dict(n=-1), "n must"), (dict(n=(1 << 20) + 1), "n must"),
             (dict(w=None), "null weights"), (dict(w=0x20008), "16-byte aligned"), (dict(wb=need_w - 4), "weights_bytes"),
             (dict(p=_ext.FcgfParams(conv1_kernel_size=5), wb=L.lr_fcgf_weights_bytes(3)), "weights_bytes"), (dict(res=None), "null result"),
             (dict(coords=None), "null coords"), (dict(out=None), "feat_out"), (dict(), "null scratch"),
             (dict(s=0x50000, sb=need_s - 1), "scratch too small"), (dict(s=0x50010), "256-byte aligned")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("lr_fcgf_extract"), (kw, rc, msg)
    assert L.lr_version() == 103                                                                           # new entry points only: no ABI of an existing one moved
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    assert all(re.search(r"LR_API\s+\w+\s+" + s + r"\(", hdr) for s in ("lr_fcgf_weights_bytes", "lr_fcgf_scratch_bytes", "lr_fcgf_extract"))
