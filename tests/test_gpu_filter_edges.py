"""The filter kernels (csrc/lr_filter.hip) on the clouds of tests/filter_edges.py: pairs ON the cell edges, a cell that does not exist,
the branches and the summation order of the water-filling, PROSAC's order at the strides of its scan kernel, and the mutual compaction
at its block boundaries.  Every expected value is an index list or a bit pattern: exact comparisons only.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

from tests import filter_edges as fe
from tests.conftest import Args, gc_oracle_kwargs, golden

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(fe.all_clouds())


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, matching
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.matching = matching; ns.torch = torch; ns.ext = _ext
    return ns


@pytest.fixture(scope="module")
def g15():
    return golden("g15_filter_edges.npz")


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _gpf(lr, c, a, bb_first=False):
    t = lr.torch.from_numpy
    out = lr.matching.Grid_Prioritized_Filter(t(c["F0"]), t(c["F1"]), t(c["i0"]), t(c["i1"]), t(c["i2"]), t(c["xyz0"]), a, BB_first=bb_first)
    return out[0].numpy(), out[1].numpy(), out[2].numpy(), (None if out[6] is None else out[6].cpu().numpy())


# ----------------------------------------------------------------------------- GPF, one pair
@pytest.mark.parametrize("bb_first", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_gpf_on_the_edges_equals_reference_and_oracle(lr, oracle, g15, name, bb_first):
    c = fe.all_clouds()[name]()
    a = Args(GPF_grid_wid=c["G"], GPF_factor=c["factor"], GPF_max_matches=c["cap"])
    tag = "bbf" if bb_first else "gpf"
    k = _gpf(lr, c, a, bb_first)
    e = oracle.Grid_Prioritized_Filter(c["F0"], c["F1"], c["i0"], c["i1"], c["i2"], c["xyz0"], a, BB_first=bb_first)
    for j in range(3):
        assert np.array_equal(k[j], g15[f"{name}_{tag}_idx{j}"]), (name, tag, j, len(k[j]), len(g15[f"{name}_{tag}_idx{j}"]))
        assert np.array_equal(k[j], e[j])
    assert np.array_equal(_bits(k[3]), _bits(e[6])) and np.array_equal(_bits(k[3]), g15[f"{name}_{tag}_score"])


# ----------------------------------------------------------------------------- GPF, batched (z.descs paths of the same kernels)
def _groups():
    by = {}
    for name in NAMES:
        c = fe.all_clouds()[name]()
        by.setdefault((c["G"], c["F0"].shape[1]), []).append(name)
    return by


def _prefix(oracle, c, k):
    """The first k points of cloud 0 against the whole of cloud 1: the neighbours of those points stay what they were; the best buddies
    are recomputed (a guest whose host is cut off becomes one)."""
    d = dict(c)
    for key in ("xyz0", "F0", "i0", "i1", "i2"):
        d[key] = np.ascontiguousarray(c[key][:k])
    d["is_bb"] = np.asarray(oracle.mark_best_buddies(d["F0"], d["F1"], d["i0"], d["i1"])[0], bool)
    return d


def _lists(lr, ws, pair, n0, n_corr):
    dev = lr.torch.device("cuda", 0)
    bufs = [lr.torch.empty(n0, dtype=lr.torch.int32, device=dev) for _ in range(4)]
    lr.ext.check(lr.ext.lib().lr_workspace_lists_at(ws.handle, pair, n0, *[b.data_ptr() for b in bufs], None))
    nn1, nn2, c0, c1 = [b.cpu().numpy() for b in bufs]
    return nn1, nn2, c0[:n_corr], c1[:n_corr]


@pytest.mark.parametrize("name", NAMES)
def test_gpf_batched_calls_equal_the_single_pair_lists(lr, oracle, g15, name):
    """The cloud in a call of 2 and in a call of 6 pairs with different n0 (other clouds of the same grid width, or prefixes of this one),
    all at this cloud's factor: every pair's lists equal the restatement at that factor, this cloud's equal the fixture and the
    single-pair call."""
    c = fe.all_clouds()[name]()
    G, dim = c["G"], c["F0"].shape[1]
    group = [n for n in _groups()[(G, dim)] if n != name]
    others = [fe.all_clouds()[n]() for n in group[:5]]
    n0 = len(c["i1"])
    k = 0
    while len(others) < 5 and n0 > 8:
        k += 1
        others.append(_prefix(oracle, c, n0 - max(1, n0 // 12) * k))
    a = Args(mode="GPF", codebase="open3D", iters=64, ransac_n=3, o3d_conf=1.0, GPF_grid_wid=G, GPF_factor=c["factor"])
    params = lr.FR.pair_params(a)
    dev = lr.torch.device("cuda", 0)
    up = lambda d: tuple(lr.torch.from_numpy(d[key]).to(dev) for key in ("xyz0", "xyz1", "F0", "F1"))
    want = {id(d): fe.gpf_ref(d, G, factor=c["factor"]) for d in [c] + others}
    assert np.array_equal(want[id(c)]["idx0"], g15[f"{name}_gpf_idx0"])
    mx0 = max(len(d["i1"]) for d in [c] + others); mx1 = max(len(d["F1"]) for d in [c] + others)
    ws1 = lr.ext.Workspace(mx0, mx1, dim, a.iters)
    ws1.poison(0x3C)
    out1 = lr.FR.register_pair_dev(*up(c), params, ws=ws1)
    lr.torch.cuda.synchronize()
    r1 = lr.ext.PairResult.from_buffer_copy(out1.cpu().numpy().tobytes())
    single = _lists(lr, ws1, 0, n0, r1.n_corr)
    assert np.array_equal(single[0], c["i1"]) and np.array_equal(single[1], c["i2"])          # the lists of the builder are the true neighbours
    assert np.array_equal(single[2], g15[f"{name}_gpf_idx0"]) and np.array_equal(single[3], g15[f"{name}_gpf_idx1"])
    for call in ([others[0], c], [c if k == 3 else others[k % len(others)] for k in range(6)]):
        P = len(call)
        ws = lr.ext.Workspace(mx0, mx1, dim, a.iters, max_pairs=P)
        ws.poison(0xA5)
        out = lr.FR.register_batch_dev([up(d) for d in call], params, ws=ws).cpu().numpy()
        lr.torch.cuda.synchronize()
        for k, d in enumerate(call):
            r = lr.ext.PairResult.from_buffer_copy(out[k].tobytes())
            got = _lists(lr, ws, k, len(d["i1"]), r.n_corr)
            w = want[id(d)]
            assert r.n_corr == len(w["idx0"]), (name, P, k)
            assert np.array_equal(got[2], w["idx0"]) and np.array_equal(got[3], w["idx1"]), (name, P, k)
            if d is c:
                for x, y in zip(got, single):
                    assert np.array_equal(x, y), (name, P, k)
        ws.close()
    ws1.close()


# ----------------------------------------------------------------------------- PROSAC order
PROSAC_GPU = [n for n, q in fe.prosac_lists().items() if np.isfinite(q).all()]


@pytest.mark.parametrize("name", PROSAC_GPU)
def test_prosac_order_scan_scatter_and_fused_forms(lr, oracle, name):
    """Every finite list of prosac_lists() as the feature-distance ratios of a cloud, all pairs kept (no_filter): RANSAC with the PROSAC
    sampler draws by position in the sorted list, so the model, its hypothesis id and its count are the oracle's on the stable order only
    if the device's order is that order.  Once alone (scan + scatter kernels) and five times in one call (fused scan).  The lists with
    +-inf or NaN cannot be fed through the ABI (no entry takes a quality vector): they are checked on the CPU only."""
    q = fe.prosac_lists()[name]
    c = fe.prosac_cloud(q)
    n = len(q)
    ratio = fe.ratio_ref(c["F0"], c["F1"], c["i0"], c["i1"], c["i2"])
    order = fe.prosac_expected(ratio)
    assert np.array_equal(order, oracle.prosac_order(ratio))
    # the cloud has the order and the ties of the list
    fq = fe.prosac_expected(q)
    assert (np.diff(ratio[fq]) >= 0).all()
    a = Args(mode="no_filter", codebase="GC", iters=1500, prosac=True)
    params = lr.FR.pair_params(a)
    e = oracle.register_pair(c["xyz0"], c["xyz1"], c["F0"], c["F1"], mode="no_filter", iters=1500, seed=51, args=a, **gc_oracle_kwargs(a))
    dev = lr.torch.device("cuda", 0)
    up = tuple(lr.torch.from_numpy(c[key]).to(dev) for key in ("xyz0", "xyz1", "F0", "F1"))
    res = []
    for P in (1, 5):
        ws = lr.ext.Workspace(n, 2 * n, 32, a.iters, max_pairs=P)
        ws.poison(0x5A)
        out = (lr.FR.register_pair_dev(*up, params, ws=ws)[None] if P == 1 else lr.FR.register_batch_dev([up] * P, params, ws=ws)).cpu().numpy()
        for k in range(P):
            r = lr.ext.PairResult.from_buffer_copy(out[k].tobytes())
            assert r.n_corr == n
            assert (r.ransac.best_h, r.ransac.best_count) == (e["ransac"]["best_h"], e["ransac"]["best_count"]), (name, P, k)
            if e["ransac"]["best_h"] >= 0:
                np.testing.assert_allclose(np.array(r.T).reshape(4, 4), e["T"], rtol=0, atol=1e-9)
            mask = lr.torch.empty(n, dtype=lr.torch.uint8, device=dev); cnt = lr.torch.zeros(1, dtype=lr.torch.int32, device=dev)
            lr.ext.check(lr.ext.lib().lr_workspace_mask_at(ws.handle, k, up[0].data_ptr(), up[1].data_ptr(), n, ctypes.c_float(params.ransac.effective_thr2()),
                                                           mask.data_ptr(), cnt.data_ptr(), None))
            res.append((bytes(r.T), bytes(r.T_ransac), r.ransac.best_h, r.ransac.best_count, r.ransac.best_ssq, mask.cpu().numpy().tobytes()))
        ws.close()
    assert all(x == res[0] for x in res[1:]), name          # scan + scatter == fused, pair for pair, bit for bit
    if n > 100:
        assert e["ransac"]["best_h"] >= 0 and oracle.rotation_error_deg(e["T"], c["T_gt"]) < 1.0


# ----------------------------------------------------------------------------- mutual compaction
@pytest.mark.parametrize("n0,pattern", [(1, "all")] + [(n, p) for n in (255, 256, 257, 1024, 65537) for p in ("first", "last", "none", "all")])
def test_mutual_compaction_through_gpf_total(lr, n0, pattern):
    """Best buddies only in the first 256-pair block, only in the last, nowhere, everywhere: the flags and their count (LR_CNT_NBB) are
    GPF's best-buddy shift and TOTAL = factor * count, so the kept list and the score bits equal the restatement's only if both are right;
    the compacted lists themselves come back from nn_to_mutual."""
    c = fe.compaction_cloud(n0, pattern)
    G = 4
    factor = 2.0 if n0 == 1 else 0.5
    a = Args(GPF_grid_wid=G, GPF_factor=factor)
    k = _gpf(lr, c, a)
    w = fe.gpf_ref(c, G, factor=factor)
    assert np.array_equal(k[0], w["idx0"]) and np.array_equal(k[1], w["idx1"]) and np.array_equal(k[2], w["idx2"])
    if n0 > 1:
        assert np.array_equal(_bits(k[3]), _bits(w["score"]))
    nbb = int(c["is_bb"].sum())
    t = lr.torch.from_numpy
    m = lr.matching.nn_to_mutual(t(c["F0"]), t(c["F1"]), t(c["i0"]), t(c["i1"]), t(c["i2"]))
    sel = np.flatnonzero(c["is_bb"])
    assert np.array_equal(m[0].numpy(), sel) and np.array_equal(m[1].numpy(), c["i1"][sel]) and np.array_equal(m[2].numpy(), c["i2"][sel])
    is_bb, num = lr.matching.mark_best_buddies(t(c["F0"]), t(c["F1"]), t(c["i0"]), t(c["i1"]))
    assert np.array_equal(is_bb, c["is_bb"]) and int(num) == nbb
