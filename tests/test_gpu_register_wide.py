"""The wide workspace (lr_workspace_create_wide, descriptors of 33..128 numbers) through the C ABI and the Python surface, against the
oracle: forward NN bit for bit, reverse / mutual, strip independence, batch == single pair under poisoned scratch, GPF and the ratio,
the whole pair in every mode, FR(), a hipGraph replay and the refusals."""
import ctypes

import numpy as np
import pytest

from tests import wide_cases
from tests.conftest import Args, gc_oracle_kwargs

pytestmark = pytest.mark.gpu

RESULT_BYTES = 496


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, matching, metrics
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.matching = matching; ns.FR = FR; ns.metrics = metrics; ns.L = _ext.lib()
    return ns


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(lr, a, dtype=np.float32):
    return host(lr, a, dtype).cuda()


def host(lr, a, dtype=None):
    return lr.torch.from_numpy(np.array(a, dtype))          # (a copy: the shared cases are read-only)


def stream(lr):
    return lr.torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def nn_on_workspace(lr, ws, F0, F1, second=True):
    torch = lr.torch
    n0, n1, d = len(F0), len(F1), F0.shape[1]
    t0, t1 = dev(lr, F0), dev(lr, F1)
    idx1 = torch.full((n0,), -7, dtype=torch.int32, device="cuda")
    idx2 = torch.full((n0,), -7, dtype=torch.int32, device="cuda") if second else None
    s1 = torch.full((n0,), -7.0, dtype=torch.float32, device="cuda")
    s2 = torch.full((n0,), -7.0, dtype=torch.float32, device="cuda") if second else None
    lr.ext.check(lr.L.lr_nn_top2(ws.handle, t0.data_ptr(), n0, t1.data_ptr(), n1, d, idx1.data_ptr(), ptr(idx2), s1.data_ptr(), ptr(s2), stream(lr)))
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (idx1, idx2, s1, s2))


# ----------------------------------------------------------------------------- forward NN
@pytest.mark.parametrize("d", [33, 34, 64, 127, 128])
@pytest.mark.parametrize("n0,n1", [(1, 2), (129, 33), (2049, 4097)])
def test_forward_nn_bit_exact(lr, oracle, d, n0, n1):
    F0, F1 = wide_cases.descriptors(n0, n1, d, 100 * d + n0)
    o1, o2, os1, os2 = oracle.nn_top2(F0, F1)
    ws = lr.ext.Workspace.wide(n0, n1, d, 1)
    i1, i2, s1, s2 = nn_on_workspace(lr, ws, F0, F1)
    assert np.array_equal(i1, o1) and np.array_equal(i2, o2)
    assert np.array_equal(bits(s1), bits(os1)) and np.array_equal(bits(s2), bits(os2))
    j1, none, t1, _ = nn_on_workspace(lr, ws, F0, F1, second=False)          # the top-1 form
    assert none is None and np.array_equal(j1, o1) and np.array_equal(bits(t1), bits(os1))
    ws.close()


# ----------------------------------------------------------------------------- reverse / mutual
def mutual_on_workspace(lr, ws, F0, F1, idx1, idx2):
    torch = lr.torch
    n0, n1, d = len(F0), len(F1), F0.shape[1]
    t0, t1, a1, a2 = dev(lr, F0), dev(lr, F1), dev(lr, idx1, np.int32), dev(lr, idx2, np.int32)
    is_bb = torch.full((n0,), 9, dtype=torch.uint8, device="cuda")
    o = [torch.full((n0,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr.ext.check(lr.L.lr_nn_to_mutual(ws.handle, t0.data_ptr(), n0, t1.data_ptr(), n1, d, a1.data_ptr(), a2.data_ptr(), is_bb.data_ptr(),
                                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), cnt.data_ptr(), stream(lr)))
    m = int(cnt.item())
    return is_bb.cpu().numpy().astype(bool), [x[:m].cpu().numpy() for x in o]


def rev_of(lr, ws, pair, n1):
    """The reverse-NN list of `pair` as the last call left it in the arena (the library's test hook)."""
    rev = lr.torch.full((n1,), -7, dtype=lr.torch.int32, device="cuda")
    lr.ext.check(lr.L.lr_debug_workspace_rev(ws.handle, pair, n1, rev.data_ptr(), stream(lr)))
    lr.torch.cuda.synchronize()
    return rev.cpu().numpy()


@pytest.mark.parametrize("d", [33, 128])
@pytest.mark.parametrize("n0,n1", [(2049, 1777), (33, 700)])
def test_mutual_equals_oracle_and_rev_is_minus_one_off_target(lr, oracle, d, n0, n1):
    F0, F1 = wide_cases.descriptors(n0, n1, d, 7 * d + n1)
    i0, i1, i2, _ = oracle.find_2nn(F0, F1)
    e0, e1, e2 = oracle.nn_to_mutual(F0, F1, i0, i1, i2)
    ebb, _ = oracle.mark_best_buddies(F0, F1, i0, i1)
    ws = lr.ext.Workspace.wide(n0, n1, d, 1)
    targeted = np.zeros(n1, bool); targeted[i1] = True
    want_rev = np.where(targeted, oracle.nn_top2(F1, F0)[0], -1)          # the oracle's reverse NN on the targeted rows, -1 elsewhere
    assert 0 < targeted.sum() < n1
    for byte in (0x00, 0xFF):          # (a poisoned arena: every -1 and every index below was written by this call)
        ws.poison(byte, stream(lr))
        is_bb, (o0, o1, o2) = mutual_on_workspace(lr, ws, F0, F1, i1, i2)
        assert np.array_equal(o0, e0) and np.array_equal(o1, e1) and np.array_equal(o2, e2)
        assert np.array_equal(is_bb, ebb)
        rev = rev_of(lr, ws, 0, n1)          # the workspace's own list
        assert (rev[~targeted] == -1).all() and (rev[targeted] >= 0).all()
        assert np.array_equal(rev, want_rev)
    ws.close()


# ----------------------------------------------------------------------------- pairs: single and batched
def params_of(lr, **kw):
    p = lr.FR.pair_params(Args(**kw))
    p.icp = 0
    return p


def register_pair(lr, ws, p, params):
    torch = lr.torch
    x0, x1, f0, f1 = dev(lr, p["xyz0"]), dev(lr, p["xyz1"]), dev(lr, p["feats0"]), dev(lr, p["feats1"])
    out = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device="cuda")
    lr.FR.register_pair_dev(x0, x1, f0, f1, params, out=out, ws=ws)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), lists_at(lr, ws, 0, len(p["feats0"]))


def lists_at(lr, ws, k, n0):
    torch = lr.torch
    L4 = [torch.full((n0,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    lr.ext.check(lr.L.lr_workspace_lists_at(ws.handle, k, n0, *[t.data_ptr() for t in L4], stream(lr)))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in L4]


def live(result_bytes, lists):
    """The lists of a pair cut to what the call defines: nn_idx1 / nn_idx2 over n0, the filtered pairs over n_corr."""
    r = _result(result_bytes)
    return [lists[0].tobytes(), lists[1].tobytes(), lists[2][:r.n_corr].tobytes(), lists[3][:r.n_corr].tobytes()]


def _result(b):
    from lidarregistration_amd import _ext
    return _ext.PairResult.from_buffer_copy(b)


@pytest.mark.parametrize("d", [33, 96])
def test_batch_equals_single_pairs_under_poison(lr, d):
    torch = lr.torch
    pairs = wide_cases.batch_pairs(d)
    params = params_of(lr, mode="GPF", codebase="GC", iters=1000, prosac=True, GPF_factor=0.5)
    mx0 = max(len(p["feats0"]) for p in pairs); mx1 = max(len(p["feats1"]) for p in pairs)
    ws1 = lr.ext.Workspace.wide(mx0, mx1, d, 1000)
    single = [register_pair(lr, ws1, p, params) for p in pairs]
    wsb = lr.ext.Workspace.wide(mx0, mx1, d, 1000, max_pairs=len(pairs))
    T = [(dev(lr, p["xyz0"]), dev(lr, p["xyz1"]), dev(lr, p["feats0"]), dev(lr, p["feats1"])) for p in pairs]
    runs = []
    for byte in (0x00, 0xFF):
        wsb.poison(byte, stream(lr))
        out = torch.zeros((len(pairs), RESULT_BYTES), dtype=torch.uint8, device="cuda")
        lr.FR.register_batch_dev(T, params, out=out, ws=wsb)
        torch.cuda.synchronize()
        res = out.cpu().numpy()
        runs.append([(res[k].tobytes(), lists_at(lr, wsb, k, len(p["feats0"]))) for k, p in enumerate(pairs)])
    for k in range(len(pairs)):
        for run in runs:
            assert run[k][0] == single[k][0], k                                  # the 496-byte result block
            assert live(*run[k]) == live(*single[k]), k
    assert any(_result(s[0]).status == 0 for s in single)
    ws1.close(); wsb.close()


def test_strip_count_does_not_change_a_result(lr, oracle):
    """One pair alone (few row blocks: many strips) and the same pair eight times in one batched call (an eighth of the strips)."""
    torch = lr.torch
    d, n0, n1 = 33, 700, 1500
    F0, F1 = wide_cases.descriptors(n0, n1, d, 5)
    rng = np.random.default_rng(5)
    p = dict(xyz0=rng.standard_normal((n0, 3)).astype(np.float32), xyz1=rng.standard_normal((n1, 3)).astype(np.float32), feats0=F0, feats1=F1)
    params = params_of(lr, mode="MNN", codebase="open3D", iters=64)
    ws1 = lr.ext.Workspace.wide(n0, n1, d, 64)
    one = register_pair(lr, ws1, p, params)
    wsb = lr.ext.Workspace.wide(n0, n1, d, 64, max_pairs=8)
    t = (dev(lr, p["xyz0"]), dev(lr, p["xyz1"]), dev(lr, F0), dev(lr, F1))
    lr.FR.register_batch_dev([t] * 8, params, ws=wsb)
    torch.cuda.synchronize()
    o1, o2, _, _ = oracle.nn_top2(F0, F1)
    assert np.array_equal(one[1][0], o1) and np.array_equal(one[1][1], o2)
    e0, e1 = oracle.nn_to_mutual(F0, F1, np.arange(n0), o1)
    for k in range(8):
        got = lists_at(lr, wsb, k, n0)
        assert np.array_equal(got[0], o1) and np.array_equal(got[1], o2)
        assert np.array_equal(got[2][:len(e0)], e0) and np.array_equal(got[3][:len(e1)], e1)
    assert np.array_equal(one[1][2][:len(e0)], e0) and _result(one[0]).n_corr == len(e0)
    ws1.close(); wsb.close()


# ----------------------------------------------------------------------------- GPF and the ratio
@pytest.mark.parametrize("d", [33, 64])
def test_gpf_and_ratio_equal_the_oracle(lr, oracle, d):
    p = wide_cases.reg_pair(2000, d, 71)
    F0, F1 = p["feats0"], p["feats1"]
    i0, i1, i2, _ = oracle.find_2nn(F0, F1)
    t = lambda x: host(lr, x)      # noqa: E731
    ratio = lr.matching.calc_distance_ratio_in_feature_space(t(F0), t(F1), t(i0), t(i1), t(i2)).cpu().numpy()
    assert np.array_equal(bits(ratio), bits(oracle.calc_distance_ratio_in_feature_space(F0, F1, i0, i1, i2)))
    for bb_first in (False, True):
        a = Args(GPF_factor=0.5, GPF_max_matches=300)
        e = oracle.Grid_Prioritized_Filter(F0, F1, i0, i1, i2, p["xyz0"], a, BB_first=bb_first)
        g = lr.matching.Grid_Prioritized_Filter(t(F0), t(F1), t(i0), t(i1), t(i2), t(p["xyz0"]), a, BB_first=bb_first)
        for k in range(3):
            assert np.array_equal(g[k].numpy(), e[k]), (bb_first, k)
        assert len(e[0]) > 50
        assert (g[6] is None) == (e[6] is None)
        if e[6] is not None:
            assert np.array_equal(bits(g[6].cpu().numpy()), bits(e[6]))


# ----------------------------------------------------------------------------- the whole pair
@pytest.mark.parametrize("d", [33, 128])
@pytest.mark.parametrize("mode", ["MNN", "GPF", "no_filter"])
@pytest.mark.parametrize("codebase", ["GC", "open3D"])
def test_whole_pair_equals_oracle(lr, oracle, d, mode, codebase):
    p = wide_cases.reg_pair(2000, d, 51)
    iters = 2000
    a = Args(mode=mode, codebase=codebase, iters=iters, GPF_factor=0.5, prosac=(codebase == "GC"))
    params = params_of(lr, **a.__dict__)
    assert params.refit == (0 if codebase == "GC" else 1)
    ws = lr.ext.Workspace.wide(2000, 2000, d, iters)
    res, lists = register_pair(lr, ws, p, params)
    r = _result(res)
    kw = gc_oracle_kwargs(a) if codebase == "GC" else dict(sample_size=4, use_elc=True, confidence=a.o3d_conf, refit_on_orig=1, scoring=0)
    e = oracle.register_pair(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], mode=mode, iters=iters, seed=51, args=a, **kw)
    assert np.array_equal(lists[0], e["idx1_orig"])
    assert r.n_corr == len(e["idx0"]) and np.array_equal(lists[2][:r.n_corr], e["idx0"]) and np.array_equal(lists[3][:r.n_corr], e["idx1"])
    T = np.array(r.T[:], np.float64).reshape(4, 4)
    assert r.status == 0
    # the tolerance tests/test_gpu_parity.py applies to this comparison at D = 32
    assert np.radians(oracle.rotation_error_deg(T, e["T"])) <= 1e-4 and oracle.translation_error_cm(T, e["T"]) / 100 <= 1e-3
    np.testing.assert_allclose(T, e["T"], rtol=0, atol=1e-9)
    assert oracle.rotation_error_deg(T, p["T_gt"]) < 1.0 and oracle.translation_error_cm(T, p["T_gt"]) < 30
    ws.close()


# ----------------------------------------------------------------------------- Python surface
def test_FR_at_33_recovers_the_planted_motion(lr):
    p = wide_cases.reg_pair(2000, 33, 51)
    t = lambda x: host(lr, x)      # noqa: E731
    a = Args(mode="GPF", codebase="GC", iters=2000, GPF_factor=0.5, prosac=True)
    out = lr.FR.FR(t(p["xyz0"]), t(p["xyz1"]), t(p["feats0"]), t(p["feats1"]), a, p["T_gt"])
    assert len(out) == 8
    T = out[0]
    assert T.shape == (4, 4) and np.isfinite(T).all() and out[1] > 0
    assert lr.metrics.is_success(T, p["T_gt"])
    assert out[4] == 2000 and 0 < out[6] <= 2000 and 0.0 <= out[7] <= 1.0


def test_python_workspace_kinds(lr):
    with pytest.raises(lr.ext.LidarRegError):
        lr.ext.Workspace(100, 100, 33, 10)
    with pytest.raises(lr.ext.LidarRegError):
        lr.ext.Workspace.wide(100, 100, 32, 10)
    ws = lr.ext.Workspace.for_dim(100, 100, 40, 10)
    assert ws.is_wide and ws.nbytes > 0 and ws.fits(100, 100, 40, 10) and not ws.fits(100, 100, 32, 10)
    narrow = lr.ext.Workspace(30000, 30000, 32, 10); wide = lr.ext.Workspace.wide(30000, 30000, 33, 10)
    assert wide.nbytes < narrow.nbytes          # none of the f16 operand copies / candidate stores
    ws.close(); narrow.close(); wide.close()


# ----------------------------------------------------------------------------- graph capture
def test_graph_replay_equals_eager(lr):
    torch = lr.torch
    d = 33
    p = wide_cases.reg_pair(2000, d, 51)
    params = params_of(lr, mode="GPF", codebase="GC", iters=500, prosac=True, GPF_factor=0.5)
    ws = lr.ext.Workspace.wide(2000, 2000, d, 500)
    eager, eager_lists = register_pair(lr, ws, p, params)
    x0, x1, f0, f1 = dev(lr, p["xyz0"]), dev(lr, p["xyz1"]), dev(lr, p["feats0"]), dev(lr, p["feats1"])
    out = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lr.FR.register_pair_dev(x0, x1, f0, f1, params, out=out, ws=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        lr.FR.register_pair_dev(x0, x1, f0, f1, params, out=out, ws=ws)
    out.zero_(); ws.poison(0xFF, stream(lr)); torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == eager
    assert live(eager, lists_at(lr, ws, 0, 2000)) == live(eager, eager_lists)
    ws.close()


# ----------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(lr):
    torch = lr.torch
    d, n = 33, 300
    p = wide_cases.reg_pair(n, d, 3)
    x0, x1, f0, f1 = dev(lr, p["xyz0"]), dev(lr, p["xyz1"]), dev(lr, p["feats0"]), dev(lr, p["feats1"])
    ws = lr.ext.Workspace.wide(n, n, d, 100, max_pairs=2)
    out = torch.full((2, RESULT_BYTES), 0xAB, dtype=torch.uint8, device="cuda")
    i1 = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def pair(params, n1=n, dim=d):
        return lr.L.lr_register_pair(ws.handle, x0.data_ptr(), x1.data_ptr(), f0.data_ptr(), f1.data_ptr(), n, n1, dim, ctypes.byref(params), out.data_ptr(), None)

    def batch(params, n1s):
        VP, IP = ctypes.c_void_p * 2, ctypes.c_int32 * 2
        return lr.L.lr_register_batch(ws.handle, 2, VP(x0.data_ptr(), x0.data_ptr()), VP(x1.data_ptr(), x1.data_ptr()), VP(f0.data_ptr(), f0.data_ptr()),
                                      VP(f1.data_ptr(), f1.data_ptr()), IP(n, n), IP(*n1s), d, ctypes.byref(params), out.data_ptr(), None)

    weighted = params_of(lr, mode="MNN", codebase="open3D", iters=100, refit=3)
    assert pair(weighted) == -1 and b"refit == 3" in lr.L.lr_last_error()
    assert batch(weighted, (n, n)) == -1 and b"refit == 3" in lr.L.lr_last_error()
    plain = params_of(lr, mode="MNN", codebase="open3D", iters=100)
    assert pair(plain, dim=34) == -1 and b"dim 34 != workspace dim 33" in lr.L.lr_last_error()
    assert lr.L.lr_nn_top2(ws.handle, f0.data_ptr(), n, f1.data_ptr(), n, 32, i1.data_ptr(), None, None, None, None) == -1
    # n1 < 2 where the second neighbour is read: GPF, the PROSAC sampler, lr_gpf / lr_gpf_bb_first
    gpf = params_of(lr, mode="GPF", codebase="open3D", iters=100)
    prosac = params_of(lr, mode="MNN", codebase="GC", iters=100, prosac=True)
    for params in (gpf, prosac):
        assert pair(params, n1=1) == -1 and b"n1 < 2" in lr.L.lr_last_error()
        assert batch(params, (n, 1)) == -1 and b"n1 < 2" in lr.L.lr_last_error()
    o = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cnt2 = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    assert lr.L.lr_gpf(ws.handle, f0.data_ptr(), n, f1.data_ptr(), 1, d, i1.data_ptr(), i1.data_ptr(), x0.data_ptr(), 10, 2.0,
                       o.data_ptr(), o.data_ptr(), o.data_ptr(), None, None, None) == -1 and b"n1 < 2" in lr.L.lr_last_error()
    assert lr.L.lr_gpf_bb_first(ws.handle, f0.data_ptr(), n, f1.data_ptr(), 1, d, i1.data_ptr(), i1.data_ptr(), x0.data_ptr(), 10, 300.0,
                                o.data_ptr(), o.data_ptr(), o.data_ptr(), None, cnt2.data_ptr(), cnt2[1:].data_ptr(), None) == -1 and b"n1 < 2" in lr.L.lr_last_error()
    # the wrong device
    lr.L.lr_debug_fake_current_device(3)
    try:
        assert pair(plain) == -1 and b"device" in lr.L.lr_last_error()
        assert lr.L.lr_nn_top2(ws.handle, f0.data_ptr(), n, f1.data_ptr(), n, d, i1.data_ptr(), None, None, None, None) == -1
        assert lr.L.lr_workspace_poison(ws.handle, 0, None) == -1
    finally:
        lr.L.lr_debug_fake_current_device(-1)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all() and (i1.cpu().numpy() == -7).all() and (o.cpu().numpy() == -7).all() and (cnt2.cpu().numpy() == -7).all()
    ws.close()
