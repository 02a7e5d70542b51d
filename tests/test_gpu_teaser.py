"""lr_teaser / lr_teaser_batch on the MI355X against the contract restated in tests/teaser_cpu.py."""
import ctypes
import glob
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import teaser_cpu as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    from lidarregistration_amd import _ext, teaser
    _ext.build()
    assert torch.cuda.is_available()
    return teaser


def _adjacency_dev(a, b):
    """lr_teaser on one pair, then the graph read back from the scratch (layout documented in include/lidarreg.h)."""
    import torch
    from lidarregistration_amd import _ext
    m = a.shape[0]
    A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    nbytes = _ext.lib().lr_teaser_scratch_bytes(m)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.zeros(176, dtype=torch.uint8, device="cuda")
    p = _ext.TeaserParams()
    _ext.check(_ext.lib().lr_teaser(A.data_ptr(), B.data_ptr(), m, None, ctypes.byref(p), res.data_ptr(), None, scratch.data_ptr(),
                                     nbytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    W = (m + 63) // 64
    words = scratch[256:256 + m * W * 8].cpu().numpy().view(np.uint64).reshape(m, W)
    bits = np.unpackbits(words.view(np.uint8).reshape(m, W, 8)[:, :, ::-1], axis=2, bitorder="big")   # per word: bit 63..0
    bits = bits.reshape(m, W, 64)[:, :, ::-1].reshape(m, W * 64)
    return bits[:, :m].astype(bool)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 1000, 4097])
def test_adjacency_bit_identical(T, m):
    rng = np.random.default_rng(m)
    a = rng.uniform(-20, 20, (m, 3)).astype(np.float32)
    b = (a + rng.normal(0, 0.2, (m, 3))).astype(np.float32)
    if m >= 8:
        # exactly on the 2 beta boundary (|a| = 1, |b| = 1.6 along an axis) and just inside the fp32 guard band
        a[0], a[1], b[0], b[1] = (0, 0, 0), (1, 0, 0), (0, 0, 0), (1.6, 0, 0)
        a[2], a[3], b[2], b[3] = (5, 5, 5), (5, 5, 6), (5, 5, 5), (5, 5, np.float32(6.6) + np.float32(1e-6))
        a[4], a[5], b[4], b[5] = (3, 0, 0), (3, 0.5, 0), (3, 0, 0), (3, np.nextafter(np.float32(1.1), np.float32(2)), 0)
    G = _adjacency_dev(a, b)
    assert np.array_equal(G, tc.graph(a, b))


def _random_planted(seed, m):
    rng = np.random.default_rng(seed)
    n_in = int(rng.integers(5, max(6, m // 3)))
    return tc.planted(m, n_in, seed, noise=0.35, outlier_scale=3.0)[:2]    # noise above beta: the planted set is not itself a clique


def _is_clique(A, c):
    sub = A[np.ix_(c, c)]
    return bool(np.all(sub | np.eye(len(c), dtype=bool)))


def test_clique_size_equals_networkx(T):
    import networkx as nx
    for seed in range(50):
        m = 40 + (seed * 53) % 260
        a, b = _random_planted(seed, m)
        A = tc.graph(a, b)
        om = len(nx.max_weight_clique(tc.to_nx(A), None)[0])
        _, info, c = T.teaser_dev(a, b, kcore_threshold=1.0)
        _, info2, c2 = T.teaser_dev(a, b, kcore_threshold=1.0)
        assert info["exact"] == 1 and info["K"] == om == len(c), (seed, info, om)
        assert np.all(np.diff(c) > 0) and _is_clique(A, c)
        assert np.array_equal(c, c2)


def test_kcore_shortcut_set(T):
    import networkx as nx
    a, b, _, _ = tc.planted(60, 48, 7, noise=0.02)
    A = tc.graph(a, b)
    core = nx.core_number(tc.to_nx(A))
    mc = max(core.values())
    assert mc > 0.5 * 60
    _, info, c = T.teaser_dev(a, b)
    assert info["max_core"] == mc
    assert list(c) == sorted(v for v, k in core.items() if k == mc)


def _margin_ok(out):
    for r, th1, th2 in out["trace"]:
        for th in (th1, th2):
            if np.any(np.abs(r - th) <= 1e-9 * th):
                return False
    return np.all(np.abs(out["w"] - 0.5) > 1e-9)


def test_rotation_translation_match_restatement(T):
    checked = 0
    for seed in range(12):
        a, b, _, _ = tc.planted(200, 60, 100 + seed, noise=0.12)
        Tg, info, c = T.teaser_dev(a, b)
        out = tc.solve_from_clique(a, b, c)
        if not _margin_ok(out):
            continue
        X = out["X"]
        if np.any(np.abs(np.abs(X - out["t"]) - 0.3) < 1e-9):
            continue
        checked += 1
        assert info["status"] == 0 and out["status"] == 0
        dR = 2 * np.arcsin(min(1.0, np.linalg.norm(Tg[:3, :3] - out["T"][:3, :3]) / (2 * np.sqrt(2))))
        assert dR < 1e-9 and np.linalg.norm(Tg[:3, 3] - out["T"][:3, 3]) < 1e-8, (seed, dR)
        assert info["n_rot_inliers"] == out["n_rot"] and info["n_trans_inliers"] == out["n_trans"]
        assert info["gnc_iters"] == out["iters"]
    assert checked >= 6


@pytest.mark.parametrize("rho", [0.5, 0.2])
def test_full_size_surrogate(T, rho):
    import torch
    from lidarregistration_amd import _ext, metrics, synth

    class Args:
        GPF_grid_wid = 10; GPF_max_matches = 10 ** 9

    p = synth.make_pair(N=30000, rho=rho, seed=51)
    x0, x1 = torch.from_numpy(p["xyz0"]).cuda(), torch.from_numpy(p["xyz1"]).cuda()
    F0, F1 = torch.from_numpy(p["feats0"]).cuda(), torch.from_numpy(p["feats1"]).cuda()
    ws = _ext.Workspace(30000, 30000, F0.shape[1], 1)
    o0, o1, cnt = T.correspondences_dev(x0, x1, F0, F1, Args, ws, torch.cuda.current_stream().cuda_stream)
    m = int(cnt[0].item())
    src, tgt = x0[o0[:m].long()], x1[o1[:m].long()]
    Tg, info, c = T.teaser_dev(src, tgt)
    torch.cuda.synchronize(); ws.close()
    a, b = src.cpu().numpy(), tgt.cpu().numpy()
    assert info["exact"] == 1 and info["K"] == len(c) and np.all(np.diff(c) > 0)
    for i0 in range(0, len(c), 1024):                           # a clique, checked in chunks
        blk = tc.graph(np.concatenate([a[c[i0:i0 + 1024]], a[c]]), np.concatenate([b[c[i0:i0 + 1024]], b[c]]))[:len(c[i0:i0 + 1024]), len(c[i0:i0 + 1024]):]
        sub = blk | (np.arange(len(c))[None, :] == np.arange(i0, i0 + blk.shape[0])[:, None])
        assert sub.all()
    Tgt = p["T_gt"]
    true_res = np.linalg.norm(a.astype(np.float64) @ Tgt[:3, :3].T + Tgt[:3, 3] - b, axis=1)
    assert info["K"] >= int((true_res < 0.15).sum())
    assert metrics.rotation_error_deg(Tg, Tgt) < metrics.RE_THRE_DEG and metrics.translation_error_cm(Tg, Tgt) < metrics.TE_THRE_CM
    print(f"rho {rho}: M {m} K {info['K']} max_core {info['max_core']} lb {info['lb']} nodes {info['nodes']} gnc {info['gnc_iters']}")


def test_batch_equals_single_ragged(T):
    import torch
    sets = [tc.planted(m, min(m, max(3, m // 3)), 300 + m, noise=0.1)[:2] if m else (np.zeros((0, 3), np.float32),) * 2
            for m in (0, 1, 2, 150, 700, 64, 333)]
    srcs, tgts = [s for s, _ in sets], [t for _, t in sets]
    out, _ = T.teaser_batch_dev(srcs, tgts)
    for k, (s, t) in enumerate(sets):
        Ts, info, c = T.teaser_dev(s, t) if len(s) else (np.eye(4), None, None)
        Tb, ib, cb = out[k]
        if len(s) < 3:
            assert ib["status"] == 1 and np.array_equal(Tb, np.eye(4))
            continue
        assert np.array_equal(Tb, Ts) and ib == info and np.array_equal(cb, c)
    # live count below m: the first 100 of 333
    live = torch.tensor([100], dtype=torch.int32, device="cuda")
    T1, i1, c1 = T.teaser_dev(srcs[-1], tgts[-1], m_dev=live)
    T2, i2, c2 = T.teaser_dev(srcs[-1][:100], tgts[-1][:100])
    assert np.array_equal(T1, T2) and i1 == i2 and np.array_equal(c1, c2)


def test_search_budget_returns_promptly(T):
    a, b = _random_planted(11, 300)
    G = tc.graph(a, b)
    for kw in (dict(node_budget=1), dict(time_budget_ms=1e-6)):
        t0 = time.time()
        _, info, c = T.teaser_dev(a, b, kcore_threshold=1.0, **kw)
        assert time.time() - t0 < 30
        assert _is_clique(G, c) and len(c) >= info["lb"] and info["nodes"] <= 1


def test_search_budget_reports_inexact(T):
    # a planted set whose greedy bound is not tight (the full search needs several nodes), cut at one node
    found = False
    for seed in range(40):
        a, b = _random_planted(1000 + seed, 300)
        _, full, _ = T.teaser_dev(a, b, kcore_threshold=1.0)
        if full["nodes"] >= 3:
            _, info, c = T.teaser_dev(a, b, kcore_threshold=1.0, node_budget=1)
            assert info["exact"] == 0 and len(c) >= info["lb"] and _is_clique(tc.graph(a, b), c)
            found = True
            break
    assert found


def test_scratch_poisoning(T):
    a, b, _, _ = tc.planted(500, 120, 77, noise=0.1)
    r0 = T.teaser_dev(a, b, poison=0x00)
    r1 = T.teaser_dev(a, b, poison=0xFF)
    assert np.array_equal(r0[0], r1[0]) and r0[1] == r1[1] and np.array_equal(r0[2], r1[2])


def test_refusals_not_faults(T):
    """A bad call is refused with its code before anything is launched, and a good call still works afterwards (the mirror of
    test_gpu_sm.py's test).  m = 257: four full 64-bit words of bitset and a ragged fifth."""
    import torch
    from lidarregistration_amd import _ext
    L = _ext.lib()
    m = 257
    a, b = tc.planted(m, 80, 5, noise=0.1)[:2]
    A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    need = L.lr_teaser_scratch_bytes(m)
    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda")
    res = torch.zeros(ctypes.sizeof(_ext.TeaserResult), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    EINVAL, ESIZE = -1, -4

    def call(p, m=m, nbytes=need):
        return L.lr_teaser(A.data_ptr(), B.data_ptr(), m, None, ctypes.byref(p), res.data_ptr(), None, scratch.data_ptr(), nbytes, st)
    assert call(_ext.TeaserParams()) == 0
    assert call(_ext.TeaserParams(), nbytes=need - 1) == ESIZE and b"scratch too small" in L.lr_last_error()
    p = _ext.TeaserParams(); p.struct_size -= 4
    assert call(p) == EINVAL and b"struct_size" in L.lr_last_error()
    assert call(_ext.TeaserParams(), m=32769, nbytes=1 << 40) == ESIZE and b"32768" in L.lr_last_error()
    L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)          # (the hook only: no memory or stream of another device)
    try:
        assert call(_ext.TeaserParams()) == EINVAL and b"device" in L.lr_last_error()
    finally:
        L.lr_debug_fake_current_device(-1)
    assert call(_ext.TeaserParams()) == 0
    torch.cuda.synchronize()


def _cli(args, cwd, env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([sys.executable, "-m", "test"] + args, cwd=cwd, env=e, capture_output=True, text=True, timeout=900)


def test_cli_teaser(tmp_path):
    exp = os.path.join(ROOT, "Experiments")
    flags = ["--dataset", "synthetic", "--num_pairs", "6", "--synthetic_n", "6000", "--algo", "TEASER", "--mode", "FAIL_TOLERANT"]
    env = {"PYTHONPATH": exp + os.pathsep + ROOT}
    r = _cli(flags, str(tmp_path), env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = sorted(glob.glob(str(tmp_path / "outputs" / "*")))[-1]
    stats = np.load(os.path.join(out, "raw_stats.npy"))
    assert stats.shape == (6, 22) and stats[:, 0].mean() == 1.0
    assert open(os.path.join(out, "TEASER_success_or_failure.txt")).read().split() == ["1"] * 6
    assert len(open(os.path.join(out, "coarse_motions.txt")).read().strip().splitlines()) >= 6
    two = tmp_path / "two"; two.mkdir()
    r2 = _cli(["launch"] + flags, str(two), dict(env, LIDARREG_GPUS="0 0"))
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    s2 = np.load(os.path.join(sorted(glob.glob(str(two / "outputs" / "*")))[-1], "raw_stats.npy"))
    keep = [0, 1, 2, 15, 17, 19, 20, 21]
    assert np.array_equal(s2[:, keep], stats[:, keep])
