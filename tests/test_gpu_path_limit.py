"""The registration path between 100 000 points and its limit of 2^22 - 1 -- lr_nn_top2, lr_nn_to_mutual, lr_register_pair, lr_register_batch,
the filters, lr_ransac, lr_refit, lr_inlier_mask and lr_icp -- on the cases of tests/path_limit_cases.py: one long side and one short side, so
that the exhaustive oracle is the reference on EVERY row, bit for bit (ICP: the bounds of tests/test_gpu_icp_ref.py).  What each case reaches
and the conditions that make the oracle's answer decisive are in tests/path_limit_cases.py and tests/test_path_limit_cpu.py.  One workspace
per shape, closed in a finally, poisoned before the first call and with another byte before the second.  Needs an MI355X."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import path_limit_cases as C
from tests.conftest import Args, gc_oracle_kwargs
from tests.test_gpu_icp_ref import _same

pytestmark = pytest.mark.gpu

NMAX, SHORT, STRIP0 = C.NMAX, C.SHORT, C.STRIP0
ONE_STRIP = {"nn_blocks": 1}             # LR_OPT_NN_BLOCKS = 1: every row block takes one strip of all column tiles
ESIZE = -4


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, matching, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.torch = torch; ns.ext = _ext; ns.matching = matching; ns.ransac = ransac
    ns.dev = torch.device("cuda", 0)
    return ns


@contextlib.contextmanager
def workspace(lr, n0, n1, options=None, max_pairs=1, install=False):
    """A workspace of its own for one shape (max_iters = 256); install: also what matching.workspace() -- and with it nn_top2_dev,
    nn_to_mutual, the filters, ransac_dev and icp_dev -- hands out meanwhile.  Closed, and the device cache emptied, on the way out."""
    idx = lr.torch.cuda.current_device()
    old = lr.matching._WS.pop(idx, None)
    if old is not None:
        lr.torch.cuda.synchronize(); old.close()
    ws = lr.ext.Workspace(n0, n1, 32, C.RANSAC_ITERS, max_pairs=max_pairs)
    try:
        for k, v in (options or {}).items():
            ws.set_option(k, v)
        if install:
            lr.matching._WS[idx] = ws
        yield ws
    finally:
        lr.torch.cuda.synchronize()
        if lr.matching._WS.get(idx) is ws:
            lr.matching._WS.pop(idx)
        ws.close()
        lr.torch.cuda.empty_cache()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _dev(lr, a):
    return lr.torch.from_numpy(np.ascontiguousarray(a)).to(lr.dev)


def _lists(lr, ws, pair, n0):
    bufs = [lr.torch.empty(n0, dtype=lr.torch.int32, device=lr.dev) for _ in range(4)]
    lr.ext.check(lr.ext.lib().lr_workspace_lists_at(ws.handle, pair, n0, *[b.data_ptr() for b in bufs], None))
    return [b.cpu().numpy() for b in bufs]


def _mnn_params(lr):
    return lr.FR.pair_params(Args(mode="MNN", codebase="open3D", iters=C.RANSAC_ITERS, ransac_n=3, o3d_conf=1.0))


# ---- 1. the entry points ----------------------------------------------------------------------------------------------------------------------
def check_entry_points(lr, oracle, name, options):
    """nn_top2_dev with and without the second neighbour and nn_to_mutual with and without the second list: indices and distance bits of
    the oracle on all rows, and the planted rows name the planted columns."""
    p, ref = C.feature_case(name), C.nn_ref(oracle, name)
    n0, n1 = len(p["F0"]), len(p["F1"])
    t = lr.torch.from_numpy
    with workspace(lr, n0, n1, options, install=True) as ws:
        f0, f1 = _dev(lr, p["F0"]), _dev(lr, p["F1"])
        ws.poison(0xA5)
        i1, i2, s1, s2 = (x.cpu().numpy() for x in lr.matching.nn_top2_dev(f0, f1, want_2nd=True, want_dist=True))
        assert np.array_equal(i1, ref["i1"]) and np.array_equal(i2, ref["i2"])
        assert np.array_equal(_bits(s1), _bits(ref["s1"])) and np.array_equal(_bits(s2), _bits(ref["s2"]))
        assert np.array_equal(i1[p["rows"]], p["cols"])
        ws.poison(0x3C)
        j1, j2, r1, r2 = lr.matching.nn_top2_dev(f0, f1, want_2nd=False, want_dist=True)
        assert j2 is None and r2 is None and np.array_equal(j1.cpu().numpy(), ref["i1"]) and np.array_equal(_bits(r1.cpu().numpy()), _bits(ref["s1"]))
        rows, o1, o2 = t(np.arange(n0)), t(ref["i1"].astype(np.int64)), t(ref["i2"].astype(np.int64))
        ws.poison(0xA5)
        g = lr.matching.nn_to_mutual(f0, f1, rows, o1, o2)
        assert len(g) == 3 and all(np.array_equal(a.numpy(), b) for a, b in zip(g, ref["m"]))
        ws.poison(0x3C)
        g1 = lr.matching.nn_to_mutual(f0, f1, rows, o1)
        assert len(g1) == 2 and all(np.array_equal(a.numpy(), b) for a, b in zip(g1, ref["m1"]))
        assert np.isin(p["rows"], g[0].numpy()).all()
        del f0, f1
    return ref


@pytest.mark.parametrize("name,options", [("cols_limit", {}), ("cols_limit", ONE_STRIP), ("rows_limit", {})], ids=["cols_limit", "cols_limit_one_strip", "rows_limit"])
def test_entry_points_at_the_limit(lr, oracle, name, options):
    ref = check_entry_points(lr, oracle, name, options)
    if name == "cols_limit":
        assert (ref["i1"] == NMAX - 1).any() and (ref["i1"] >> 21 & 1).any()


# ---- 2. through lr_register_pair -----------------------------------------------------------------------------------------------------------------
def check_register_pair(lr, oracle, name, options):
    """lr_register_pair (MNN, open3D scoring, 256 iterations, random coordinates), one warm-up call and one checked call: the lists of the
    oracle, no row re-done by the exact scan of all columns (n_nn_fixed == 0) and no form miss -- the filter pass itself kept the
    neighbours --, and the oracle's number of pairs."""
    p, ref = C.feature_case(name), C.nn_ref(oracle, name)
    n0, n1 = len(p["F0"]), len(p["F1"])
    params = _mnn_params(lr)
    with workspace(lr, n0, n1, options) as ws:
        dp = (_dev(lr, C.coordinates(n0, 1)), _dev(lr, C.coordinates(n1, 2)), _dev(lr, p["F0"]), _dev(lr, p["F1"]))
        for poison in (0xA5, 0x5A):
            ws.poison(poison)
            r = lr.FR.read_result(lr.FR.register_pair_dev(*dp, params, ws=ws))
        assert r.n_nn_fixed == 0 and r.reserved[2] == 0, (r.n_nn_fixed, r.reserved[2])
        nn1, nn2, c0, c1 = _lists(lr, ws, 0, n0)
        m = ref["m"]
        assert np.array_equal(nn1, ref["i1"]) and np.array_equal(nn2, ref["i2"]) and np.array_equal(nn1[p["rows"]], p["cols"])
        assert r.n_corr == len(m[0]) and np.array_equal(c0[:r.n_corr], m[0]) and np.array_equal(c1[:r.n_corr], m[1])
        nbytes = ws.nbytes
        del dp
    return nbytes


@pytest.mark.parametrize("name,options", [("cols_limit", {}), ("cols_limit", ONE_STRIP), ("rows_limit", {})], ids=["cols_limit", "cols_limit_one_strip", "rows_limit"])
def test_register_pair_at_the_limit(lr, oracle, name, options):
    nbytes = check_register_pair(lr, oracle, name, options)
    print(f"{name}: lr_workspace_bytes {nbytes} ({nbytes / 2 ** 30:.2f} GiB)")
    # the candidate store alone is 2^31 bytes; about 830 bytes per row of the long side in all (the carve list of lr_api.hip)
    assert 1 << 31 < nbytes < 5 << 30


# ---- 3. the filters at 4 194 303 rows ----------------------------------------------------------------------------------------------------------------
def test_filters_over_the_rows_limit(lr, oracle):
    """The feature-distance ratio on the mutual list and on all 4 194 303 forward pairs, and the grid filter at factors 0.5 and 2.0 over a
    clustered cloud: indices and score bits of the oracle."""
    p, ref = C.feature_case("rows_limit"), C.nn_ref(oracle, "rows_limit")
    xyz0, _ = C.clustered_sources()
    t = lr.torch.from_numpy
    rows, i1, i2 = np.arange(NMAX), ref["i1"].astype(np.int64), ref["i2"].astype(np.int64)
    with workspace(lr, NMAX, SHORT, install=True) as ws:
        f0, f1 = _dev(lr, p["F0"]), _dev(lr, p["F1"])
        for a0, a1, a2 in (ref["m"], (rows, i1, i2)):
            got = lr.matching.calc_distance_ratio_in_feature_space(f0, f1, t(a0), t(a1.astype(np.int64)), t(a2.astype(np.int64))).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(oracle.calc_distance_ratio_in_feature_space(p["F0"], p["F1"], a0, a1, a2)))
        for factor, poison in ((0.5, 0xA5), (2.0, 0x3C)):
            a = Args(GPF_factor=factor)
            e = oracle.Grid_Prioritized_Filter(p["F0"], p["F1"], rows, i1, i2, xyz0, a)
            ws.poison(poison)
            out = lr.matching.Grid_Prioritized_Filter(f0, f1, t(rows), t(i1), t(i2), t(xyz0), a)
            assert all(np.array_equal(out[k].numpy(), e[k]) for k in range(3)) and 0 < len(e[0]) < NMAX
            assert np.array_equal(_bits(out[6].cpu().numpy()), _bits(e[6]))
        del f0, f1


def test_prosac_order_over_the_rows_limit(lr, oracle):
    """PROSAC over all 4 194 303 forward pairs (no filter, so the order kernels see every row): lr_register_pair with prosac against
    oracle.register_pair, as tests/test_gpu_gc.py::test_prosac_order_with_tied_qualities reads it -- the transform to 1e-9 -- and the
    winner's id and count exactly: the sampler draws from the head of the order, so another order is another winner."""
    p = C.feature_case("rows_limit")
    xyz0, xyz1 = C.clustered_sources()
    a = Args(mode="no_filter", codebase="GC", iters=C.RANSAC_ITERS, prosac=True, fast_rejection="NONE")
    e = oracle.register_pair(xyz0, xyz1, p["F0"], p["F1"], mode="no_filter", iters=C.RANSAC_ITERS, seed=51, args=a, **gc_oracle_kwargs(a))
    params = lr.FR.pair_params(a)
    with workspace(lr, NMAX, SHORT) as ws:
        dp = (_dev(lr, xyz0), _dev(lr, xyz1), _dev(lr, p["F0"]), _dev(lr, p["F1"]))
        for poison in (0xA5, 0x5A):
            ws.poison(poison)
            r = lr.FR.read_result(lr.FR.register_pair_dev(*dp, params, ws=ws))
        assert r.n_corr == NMAX == len(e["idx0"]) and r.n_nn_fixed == 0
        assert (r.ransac.best_h, r.ransac.best_count, r.ransac.n_valid) == (e["ransac"]["best_h"], e["ransac"]["best_count"], e["ransac"]["n_valid"])
        np.testing.assert_allclose(np.array(r.T[:]).reshape(4, 4), e["T"], rtol=0, atol=1e-9)
        del dp


# ---- 4. the strip clamp ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1], ids=["196609", "196608"])
def test_strip_clamp_both_sizes(lr, oracle, k):
    """769 row blocks (768 / 769 = 0 strips, clamped to 1) and 768 (a true quotient of 1): NN and mutual lists of the oracle through the
    entry points and through lr_register_pair, which re-does no row."""
    name = f"strip_clamp_{k}"
    assert len(C.feature_case(name)["F0"]) == STRIP0 - k
    check_entry_points(lr, oracle, name, {})
    check_register_pair(lr, oracle, name, {})


# ---- 5. the batch ------------------------------------------------------------------------------------------------------------------------------
def test_batch_with_two_large_pairs(lr, oracle):
    """One lr_register_batch of (STRIP0, 300), (300, 2^21 + 33), (3 000, 2 500): every pair's result block (but the diagnostic bytes
    312..315) and lists equal the same pair through lr_register_pair on a single-pair workspace; the two large pairs' NN lists are the
    oracle's."""
    host = C.batch_pairs()
    params = _mnn_params(lr)
    devp = [tuple(_dev(lr, p[key]) for key in ("xyz0", "xyz1", "feats0", "feats1")) for p in host]
    with workspace(lr, STRIP0, C.BATCH_LONG, max_pairs=3) as wsb, workspace(lr, STRIP0, C.BATCH_LONG) as ws1:
        wsb.poison(0xA5)
        outb = lr.FR.register_batch_dev(devp, params, ws=wsb).cpu().numpy().copy()
        for k, p in enumerate(host):
            n0 = len(p["feats0"])
            ws1.poison(0x3C + k)
            single = lr.FR.register_pair_dev(*devp[k], params, ws=ws1).cpu().numpy().copy()
            b, s = outb[k].copy(), single.copy()
            b[312:316] = 0; s[312:316] = 0
            print(f"pair {k}: n_nn_fixed batched {lr.ext.PairResult.from_buffer_copy(b.tobytes()).n_nn_fixed}, alone {lr.ext.PairResult.from_buffer_copy(s.tobytes()).n_nn_fixed}")
            assert b.tobytes() == s.tobytes() and len(b) == ctypes.sizeof(lr.ext.PairResult), f"pair {k}: the batched block differs from the single-pair one"
            r = lr.ext.PairResult.from_buffer_copy(b.tobytes())
            lb, ls = _lists(lr, wsb, k, n0), _lists(lr, ws1, 0, n0)
            assert np.array_equal(lb[0], ls[0]) and np.array_equal(lb[1], ls[1]), k
            assert np.array_equal(lb[2][:r.n_corr], ls[2][:r.n_corr]) and np.array_equal(lb[3][:r.n_corr], ls[3][:r.n_corr]), k
            assert r.n_nn_fixed == 0 and r.n_corr > 0
            if k < 2:
                ref = C.nn_ref(oracle, ("batch_rows", "batch_cols")[k])
                assert np.array_equal(lb[0], ref["i1"]) and np.array_equal(lb[1], ref["i2"])
                assert r.n_corr == len(ref["m"][0]) and np.array_equal(lb[2][:r.n_corr], ref["m"][0]) and np.array_equal(lb[3][:r.n_corr], ref["m"][1])
    del devp


# ---- 6. RANSAC, refit, mask --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ransac_ws(lr):
    with workspace(lr, NMAX, 1, install=True) as ws:
        yield ws


@pytest.mark.parametrize("config", sorted(C.RANSAC_CONFIGS))
@pytest.mark.parametrize("m", C.RANSAC_M)
def test_ransac_against_the_oracle(lr, oracle, ransac_ws, m, config):
    """lr_ransac at the limit and on both sides of the scoring chunk switch: the record and every bit of the transform are the oracle's,
    whatever the workspace held."""
    c = C.ransac_case(m)
    Te, einfo = C.ransac_ref(oracle, m, config)
    kw = C.ransac_kwargs(config)
    src, tgt = _dev(lr, c["src"]), _dev(lr, c["tgt"])
    for poison in (0xA5, 0x5A):
        ransac_ws.poison(poison)
        T, info = lr.ransac.ransac_dev(src, tgt, **kw)
        assert info == einfo and np.array_equal(T, Te), (info, einfo)
    assert lr.matching._WS[lr.torch.cuda.current_device()] is ransac_ws          # (the calls ran on this workspace, not on a grown one)
    assert einfo["best_h"] >= 0
    del src, tgt


def test_ransac_refuses_one_record_more_than_the_workspace(lr, oracle, ransac_ws):
    """m = max_n0 + 1 = 2^22: LR_ESIZE, nothing launched (the outputs keep what they held), and the good call that follows returns the
    oracle's answer."""
    c = C.ransac_case(NMAX)
    t = lr.torch
    src = t.zeros((NMAX + 1, 3), dtype=t.float32, device=lr.dev); tgt = t.zeros_like(src)
    src[:NMAX] = _dev(lr, c["src"]); tgt[:NMAX] = _dev(lr, c["tgt"])
    kw = C.ransac_kwargs("count")
    p = lr.ransac.ransac_params(kw["iters"], use_elc=kw["use_elc"], thr=kw["thr"], scoring=kw["scoring"])
    T = t.full((16,), 7.0, dtype=t.float64, device=lr.dev)
    res = t.full((ctypes.sizeof(lr.ext.RansacResult),), 0x55, dtype=t.uint8, device=lr.dev)
    L = lr.ext.lib()
    st = t.cuda.current_stream().cuda_stream
    assert L.lr_ransac(ransac_ws.handle, src.data_ptr(), tgt.data_ptr(), NMAX + 1, None, ctypes.byref(p), T.data_ptr(), res.data_ptr(), st) == ESIZE
    assert L.lr_last_error() == b"lr_ransac: m exceeds the workspace"
    t.cuda.synchronize()
    assert np.all(T.cpu().numpy() == 7.0) and np.all(res.cpu().numpy() == 0x55)
    Tg, info = lr.ransac.ransac_dev(src[:NMAX], tgt[:NMAX], **kw)
    Te, einfo = C.ransac_ref(oracle, NMAX, "count")
    assert info == einfo and np.array_equal(Tg, Te)
    del src, tgt


def test_refit_at_the_limit(lr, oracle, ransac_ws):
    """lr_refit over 4 194 303 pairs -- 16 384 blocks of partials -- with the assertions of tests/test_gpu_refit.py::test_lr_refit_cases: the
    same bits under 0x00, under 0xFF and on the call that follows at once, the oracle's inlier count, its transform to 1e-10."""
    c = C.refit_case()
    x0, x1, i1 = _dev(lr, c["xyz0"]), _dev(lr, c["xyz1"]), _dev(lr, c["idx1"])
    runs = []
    for poison in (0x00, 0xFF, None):
        if poison is not None:
            ransac_ws.poison(poison)
        runs.append(lr.ransac.refit_dev(x0, x1, i1, c["T"], thr2=c["thr2"], ws=ransac_ws))
    T, n = runs[0]
    assert all(np.array_equal(Tk, T) and nk == n for Tk, nk in runs[1:]), "the result depends on what the scratch held"
    Te, ne = oracle.refit(c["xyz0"], c["xyz1"], c["idx1"], c["T"], thr2=c["thr2"])
    print(f"refit at {NMAX}: n {n} (oracle {ne}), |T - Te| {np.abs(T - Te).max():.2e}")
    assert n == ne and np.abs(T - Te).max() <= 1e-10, np.abs(T - Te).max()
    del x0, x1, i1


def test_inlier_mask_at_the_limit(lr, oracle, ransac_ws):
    """lr_inlier_mask over 4 194 303 pairs: the oracle's mask and count; the bytes behind m keep their 0x55."""
    c, r = C.ransac_case(NMAX), C.refit_case()
    src, tgt = _dev(lr, c["src"]), _dev(lr, c["tgt"])
    buf, n = lr.ransac.inlier_mask_dev(src, tgt, r["T"], r["thr2"], fill=0x55, room=NMAX + 300)
    want, ne = oracle.inlier_mask(c["src"], c["tgt"], r["T"], r["thr2"])
    assert np.all(buf[NMAX:] == 0x55) and set(np.unique(buf[:NMAX])) <= {0, 1}
    assert n == ne == int(buf[:NMAX].sum()) and np.array_equal(buf[:NMAX].astype(bool), want) and want[-1024:].mean() > 0.9
    del src, tgt


# ---- 7. ICP --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many_sources", "many_targets"])
def test_icp_at_the_limit(lr, name):
    c = C.icp_case(name)
    Tr, ref = C.icp_reference(name)
    with workspace(lr, len(c["src"]), len(c["tgt"]), install=True) as ws:
        ws.poison(0xA5)
        T, info = lr.ransac.icp_dev(c["src"], c["tgt"], c["T0"], max_dist=c["max_dist"], max_iter=c["max_iter"])
        print(name, info, ref)
        _same(info, ref, T, Tr)
        ws.poison(0x3C)
        T2, info2 = lr.ransac.icp_dev(c["src"], c["tgt"], c["T0"], max_dist=c["max_dist"], max_iter=c["max_iter"])
        assert info2 == info and np.array_equal(T2, T)
    assert ref["n_corr"] > (2_000_000 if name == "many_sources" else 290)


# ---- 8. the limit ----------------------------------------------------------------------------------------------------------------------------------
def test_the_limit_itself(lr):
    """2^22 points on either side are refused by both constructors with LR_ESIZE and the limit's words, 2^22 - 1 are accepted, and a good
    call works on the workspace that was created after the refusals."""
    L = lr.ext.lib()
    for n0, n1 in ((1 << 22, SHORT), (SHORT, 1 << 22)):
        h = ctypes.c_void_p()
        assert L.lr_workspace_create(ctypes.byref(h), n0, n1, 32, 256) == ESIZE and b"clouds are limited to 2^22 points" in L.lr_last_error() and not h
        assert L.lr_workspace_create_batch(ctypes.byref(h), 2, n0, n1, 32, 256) == ESIZE and b"clouds are limited to 2^22 points" in L.lr_last_error() and not h
    for n0, n1, pairs in ((NMAX, NMAX, 1), (NMAX, SHORT, 2), (SHORT, NMAX, 2)):
        with workspace(lr, n0, n1, max_pairs=pairs) as ws:
            assert ws.handle and ws.nbytes > pairs * (1 << 31)
            if pairs == 1:
                h = ctypes.c_void_p()
                assert L.lr_workspace_create(ctypes.byref(h), 1 << 22, 1 << 22, 32, 256) == ESIZE and not h
                c = C.ransac_case(C.CHUNKS)
                ws.poison(0xA5)
                lr.matching._WS[lr.torch.cuda.current_device()] = ws
                T, info = lr.ransac.ransac_dev(c["src"], c["tgt"], **C.ransac_kwargs("count"))
                assert info["best_count"] > 200000 and lr.matching._WS[lr.torch.cuda.current_device()] is ws
