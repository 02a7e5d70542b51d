"""The stage after RANSAC on the device (csrc/lr_refit.hip): refit_moments_kernel with its solve, inlier_mask_kernel and the result
block they fill, against the exact restatement of tests/refit_cpu.py on the cases of tests/refit_cases.py -- the thread, block and
64-block staging edges, the slots of the kernel's layout, the strict fp64 threshold, listed pairs with a live count (refit = 2), weights
(refit = 3), the gates, every field of every result block of ragged batches, and the refusals.  Counts and masks are exact; transforms
are held to rigid_hp.check's bound and to the 1e-10 (one stage) / 1e-9 (whole pipeline) of the existing oracle comparisons.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest

from lidarregistration_amd import synth
from tests import refit_cases as cases
from tests import refit_cpu as rc
from tests.conftest import Args

pytestmark = pytest.mark.gpu

PLAIN = [cases.plain_case(n, p) for n, p in cases.plain_specs()] + [cases.skip_case(), cases.boundary_case("at"), cases.boundary_case("next64")]


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, matching, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.torch = torch; ns.ext = _ext; ns.ransac = ransac; ns.matching = matching
    ns.dev = torch.device("cuda", 0)
    return ns


@pytest.fixture(scope="module")
def big_ws(lr):
    ws = lr.ext.Workspace(66561, 1, 32, 1)
    yield ws
    ws.close()


def _bits(T, n):
    return np.asarray(T, np.float64).tobytes() + int(n).to_bytes(4, "little", signed=True)


# ------------------------------------------------------------------------------------------------------------ lr_refit
@pytest.mark.parametrize("c", PLAIN, ids=[c["name"] for c in PLAIN])
def test_lr_refit_cases(lr, oracle, big_ws, c):
    """Plain refit on every size x pattern case: the inlier count is the restatement's, T passes rigid_hp.check against it and lies
    within 1e-10 of the oracle's.  The scratch is poisoned with 0x00 and with 0xFF before a call and a third call follows at once on the
    same workspace: the same bits every time, so nothing is read before it is written.  (That the last block puts the ticket back to 0
    cannot be observed through the ABI: lr_refit clears the ticket before every launch and lr_register_pair starts from cleared
    counters, so a kernel that left it set would give the same bits here, and no entry point reads the counter.)"""
    t = lr.torch
    x0, x1, i1 = (t.from_numpy(c[k]).to(lr.dev) for k in ("xyz0", "xyz1", "idx1"))
    runs = []
    for poison in (0x00, 0xFF, None):
        if poison is not None:
            big_ws.poison(poison)
        runs.append(lr.ransac.refit_dev(x0, x1, i1, c["T"], thr2=c["thr2"], ws=big_ws))
    T, n = runs[0]
    assert _bits(*runs[1]) == _bits(T, n) and _bits(*runs[2]) == _bits(T, n), "the result depends on what the scratch held"
    ref = cases.reference(c)
    print(f"{c['name']}: n {n} (restatement {ref['n_refit']})")
    bad = cases.problems(T, n, ref, c)
    assert not bad, "\n".join(bad)
    Te, ne = cases.oracle_refit(oracle, c)
    assert n == ne and np.abs(T - Te).max() <= 1e-10, np.abs(T - Te).max()


def test_lr_refit_on_a_small_workspace_and_after_a_larger_call(lr):
    """The count partials sit behind the moment partials of the call's own grid: a 1-row workspace has room for them, and a short call
    after a long one on the same workspace does not pick up the long one's."""
    t = lr.torch
    ws1 = lr.ext.Workspace(1, 1, 32, 1)
    c = cases.plain_case(1, "all")
    T, n = lr.ransac.refit_dev(*(t.from_numpy(c[k]).to(lr.dev) for k in ("xyz0", "xyz1", "idx1")), c["T"], thr2=c["thr2"], ws=ws1)
    assert n == 1 and np.array_equal(T, c["T"])
    ws1.close()
    ws = lr.ext.Workspace(2049, 1, 32, 1)
    for size, pat in ((2049, "all"), (1023, "three"), (2049, "u3"), (4, "all")):
        c = cases.plain_case(size, pat)
        T, n = lr.ransac.refit_dev(*(t.from_numpy(c[k]).to(lr.dev) for k in ("xyz0", "xyz1", "idx1")), c["T"], thr2=c["thr2"], ws=ws)
        assert not cases.problems(T, n, cases.reference(c), c), c["name"]
    ws.close()


# ------------------------------------------------------------------------------------------------------------ refit = 1, 2, 3 in the pipeline
SIZES = [(1023, 1100), (1025, 990), (5, 7), (2049, 2049), (1, 3), (4100, 4000)]
#        refit, mode, PROSAC, descriptor width
MODES = [(1, "MNN", False, 32), (2, "MNN", False, 32), (2, "MNN", True, 32), (2, "no_filter", False, 32), (3, "no_filter", False, 32),
         (3, "MNN", False, 5), (1, "no_filter", False, 5)]
ITERS = 1000
_PAIRS = {}


def _pairs(lr, dim):
    if dim not in _PAIRS:
        host = [synth.make_pair(N=n0, N1=n1, D=dim, rho=0.5, s=0.9 if dim == 32 else 0.15, seed=4200 + k) for k, (n0, n1) in enumerate(SIZES)]
        devp = [tuple(lr.torch.from_numpy(p[key]).to(lr.dev) for key in ("xyz0", "xyz1", "feats0", "feats1")) for p in host]
        _PAIRS[dim] = (host, devp)
    return _PAIRS[dim]


def _params(lr, refit, mode, prosac, sampler=None):
    p = lr.FR.pair_params(Args(mode=mode, codebase="open3D", iters=ITERS, ransac_n=3, o3d_conf=1.0, refit=refit))
    # distinct indices by default: a pair with fewer than three correspondences has no hypothesis then
    p.ransac.sampler = (1 if prosac else 2) if sampler is None else sampler
    return p


def _lists(lr, ws, pair, n0):
    bufs = [lr.torch.empty(n0, dtype=lr.torch.int32, device=lr.dev) for _ in range(3)]
    lr.ext.check(lr.ext.lib().lr_workspace_lists_at(ws.handle, pair, n0, bufs[0].data_ptr(), None, bufs[1].data_ptr(), bufs[2].data_ptr(), None))
    return [b.cpu().numpy() for b in bufs]


def _block(raw):
    raw = raw.copy()
    raw[312:316] = 0          # reserved[0]: a diagnostic that may differ between runs (lidarreg.h)
    return raw.tobytes()


def _restate(p, r, lists, refit, thr2):
    nn1, c0, c1 = lists
    have = r.ransac.best_h >= 0
    T_ransac = np.array(r.T_ransac[:]).reshape(4, 4)
    kw = dict(have_model=have)
    if refit == 2:
        return rc.refit(p["xyz0"], p["xyz1"], c1, T_ransac, thr2, idx0=c0, m=r.n_corr, **kw)        # (the buffers whole: rows past n_corr are the scratch's)
    if refit == 3:
        kw.update(F0=p["feats0"], F1=p["feats1"])
    return rc.refit(p["xyz0"], p["xyz1"], nn1, T_ransac, thr2, **kw)


@pytest.mark.parametrize("refit,mode,prosac,dim", MODES)
def test_result_blocks_of_a_ragged_batch(lr, refit, mode, prosac, dim):
    """lr_register_batch over six ragged pairs, two of them too small for a hypothesis, and lr_register_pair on each: every field of
    every result block against the restatement fed the device's own T_ransac and the lists read back from the workspace."""
    host, devp = _pairs(lr, dim)
    P = len(devp)
    params, plain = _params(lr, refit, mode, prosac), _params(lr, 0, mode, prosac)
    wsb = lr.ext.Workspace(4100, 4100, dim, ITERS, max_pairs=P)
    # 0xFF makes the list rows past n_corr read as -1, which the kernel skips with or without the live count; under the single-pair
    # workspace's 0x5A + k they would be out-of-range indices.  So a refit = 2 kernel that read past *m_dev is caught here by the byte
    # comparison of the two paths (and by the restatement, which stops at n_corr), not by a poisoned row changing a sum.
    wsb.poison(0xFF)
    outb = lr.FR.register_batch_dev(devp, params, ws=wsb).cpu().numpy().copy()
    ws1 = lr.ext.Workspace(4100, 4100, dim, ITERS)
    fitted, failed = 0, []
    for k in range(P):
        p, n0 = host[k], SIZES[k][0]
        ws1.poison(0x00)
        base = lr.ext.PairResult.from_buffer_copy(lr.FR.register_pair_dev(*devp[k], plain, ws=ws1).cpu().numpy().tobytes())      # refit = 0
        ws1.poison(0x5A + k)
        single = lr.FR.register_pair_dev(*devp[k], params, ws=ws1).cpu().numpy().copy()
        assert _block(outb[k]) == _block(single), f"pair {k}: the batched block differs from the single-pair one"
        r = lr.ext.PairResult.from_buffer_copy(outb[k].tobytes())
        lists = _lists(lr, wsb, k, n0)
        alone = _lists(lr, ws1, 0, n0)
        assert np.array_equal(lists[0], alone[0]) and all(np.array_equal(x[:r.n_corr], y[:r.n_corr]) for x, y in zip(lists[1:], alone[1:])), k
        T, T_ransac, T_icp = (np.array(a[:]).reshape(4, 4) for a in (r.T, r.T_ransac, r.T_icp))
        # the RANSAC model and its record are those of the same call without a refit stage: the stage leaves them alone
        assert np.array_equal(T_ransac, np.array(base.T[:]).reshape(4, 4)) and np.array_equal(T_ransac, np.array(base.T_ransac[:]).reshape(4, 4))
        assert bytes(r.ransac) == bytes(base.ransac) and r.n_corr == base.n_corr and base.n_refit == 0
        assert r.n_corr == n0 if mode == "no_filter" else 0 <= r.n_corr <= n0
        have = r.ransac.best_h >= 0
        assert r.status == (0 if have else 1)
        if not have:
            failed.append(k)
            assert np.array_equal(T, np.eye(4)) and r.n_refit == 0
        # ICP did not run: T_icp is T and the icp record is zero
        assert np.array_equal(T_icp, T) and (r.icp.fitness, r.icp.inlier_rmse, r.icp.n_corr, r.icp.iterations) == (0.0, 0.0, 0, 0)
        assert list(r.reserved[3:]) == [0] * 5
        ref = _restate(p, r, lists, refit, params.refit_thr2)
        assert np.all(np.abs(ref["gap"]) > rc.SAFETY * rc.d2_bound(ref["d2"], ref["M"], rc.U64, 7)), "a pair too close to the threshold to call"
        print(f"refit {refit} {mode} pair {k}: n_corr {r.n_corr} n_refit {r.n_refit} (restatement {ref['n_refit']}) status {r.status}")
        assert r.status == ref["status"]
        bad = cases.problems(T, r.n_refit, ref, dict(name=f"pair {k}", T=T_ransac))
        assert not bad, "\n".join(bad)
        fitted += ref["ref"] is not None
    assert fitted >= 3 and failed and set(failed) <= {2, 4}, (fitted, failed)          # ordinary pairs around the ones with no hypothesis
    wsb.close(); ws1.close()


@pytest.mark.parametrize("refit,mode,prosac", [(2, "MNN", False), (2, "MNN", True), (3, "no_filter", False), (2, "no_filter", False)])
def test_pipeline_refit_modes_match_the_oracle(lr, oracle, refit, mode, prosac):
    """refit = 2 and 3 end to end against oracle.register_pair's refit_on_orig 2 and 3 (1e-9, as every pipeline comparison)."""
    host, devp = _pairs(lr, 32)
    params = _params(lr, refit, mode, prosac)
    for k in (0, 3):
        p = host[k]
        r = lr.FR.read_result(lr.FR.register_pair_dev(*devp[k], params))
        e = oracle.register_pair(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], mode=mode, iters=ITERS, sample_size=3, seed=51,
                                 refit_on_orig=refit, prosac=prosac, unique=not prosac)
        assert r.status == 0 and r.ransac.best_h == e["ransac"]["best_h"] and r.n_corr == len(e["idx0"]) and r.n_refit == e["n_refit"]
        assert np.abs(np.array(r.T[:]).reshape(4, 4) - e["T"]).max() <= 1e-9


def test_listed_refit_with_a_live_count_of_65537(lr):
    """refit = 2 past the first staging chunk: 65 537 rows, no filter, so the lists are all live (the count equals the allocated
    length) and 65 blocks report."""
    n0 = 65537
    p = synth.make_pair(N=n0, N1=n0, rho=0.5, s=0.5, seed=4300)
    # the one row of block 64 is a sure inlier of the planted motion: the descriptor and the pre-image of a cloud-1 point
    Tg = p["T_gt"]
    p["feats0"][-1] = p["feats1"][7]
    p["xyz0"][-1] = ((p["xyz1"][7].astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    devp = tuple(lr.torch.from_numpy(p[key]).to(lr.dev) for key in ("xyz0", "xyz1", "feats0", "feats1"))
    params = _params(lr, 2, "no_filter", False)
    ws = lr.ext.Workspace(n0, n0, 32, ITERS)
    ws.poison(0xFF)
    r = lr.FR.read_result(lr.FR.register_pair_dev(*devp, params, ws=ws))
    lists = _lists(lr, ws, 0, n0)
    assert r.n_corr == n0 and np.array_equal(lists[1], np.arange(n0)) and np.array_equal(lists[2], lists[0])
    ref = _restate(p, r, lists, 2, params.refit_thr2)
    assert np.all(np.abs(ref["gap"]) > rc.SAFETY * rc.d2_bound(ref["d2"], ref["M"], rc.U64, 7))
    print(f"n_refit {r.n_refit} (restatement {ref['n_refit']}), inliers in block 64: {int(ref['inlier'][65536:].sum())}")
    bad = cases.problems(np.array(r.T[:]).reshape(4, 4), r.n_refit, ref, dict(name="65537 listed", T=np.array(r.T_ransac[:]).reshape(4, 4)))
    assert not bad and r.status == 0 and ref["ref"] is not None and ref["inlier"][65536] and lists[0][65536] == 7, "\n".join(bad)
    ws.close()


WEIGHT_EDGES = [(how, dim) for how in ("identical", "dominant", "below_one", "one", "two") for dim in (32, 5)]


@pytest.mark.parametrize("how,dim", WEIGHT_EDGES)
def test_weight_edges_reach_the_kernel(lr, how, dim):
    """refit = 3 at the edges of its weights, through lr_register_pair without a filter: the descriptors of cloud 1 are copies or
    perturbations of cloud 0's, so the device's own NN pairs them up.  Identical descriptors (every weight is the clamp's 1e12 and their
    sum is far beyond an int32), one pair 10^6 times heavier than the rest, weights that sum to less than 1 over more than 100 inliers, and
    one or two inliers (a single- or two-row cloud 0; sampling with replacement gives those a model), which under weights are fitted all
    the same.  T, n_refit and status against the restatement fed the device's own T_ransac and NN list."""
    few = {"one": 1, "two": 2}.get(how)
    c = cases.weighted_case("ordinary" if few else how, dim, r_in=0.05)
    n0 = few or len(c["idx1"])
    p = dict(xyz0=c["xyz0"][:n0], xyz1=c["xyz1"], feats0=c["F0"][:n0], feats1=c["F1"])
    devp = tuple(lr.torch.from_numpy(np.ascontiguousarray(p[key])).to(lr.dev) for key in ("xyz0", "xyz1", "feats0", "feats1"))
    params = _params(lr, 3, "no_filter", False, sampler=0)
    ws = lr.ext.Workspace(257, 257, dim, ITERS)
    ws.poison(0xFF)
    r = lr.FR.read_result(lr.FR.register_pair_dev(*devp, params, ws=ws))
    lists = _lists(lr, ws, 0, n0)
    ref = _restate(p, r, lists, 3, params.refit_thr2)
    assert np.all(np.abs(ref["gap"]) > rc.SAFETY * rc.d2_bound(ref["d2"], ref["M"], rc.U64, 7))
    w = ref.get("w", np.zeros(0))
    print(f"{how} dim {dim}: n_refit {r.n_refit} (restatement {ref['n_refit']}) status {r.status} weight sum {w.sum():.6g} max {w.max() if w.size else 0:.6g}")
    assert r.status == 0 == ref["status"] and r.n_corr == n0 and ref["ref"] is not None
    # the case is what it is meant to be under the model RANSAC found
    if how == "identical":
        assert np.array_equal(lists[0], c["idx1"]) and ref["n_refit"] > 100 and np.all(w == 1.0 / float(np.float32(1e-12))) and w.sum() > 2.0 ** 31
    elif how == "dominant":
        ws_ = np.sort(w)
        assert ws_[-1] == 2.0 ** 20 and ws_[-2] < 2.0 ** 10 and ref["n_refit"] > 100
    elif how == "below_one":
        assert 0.0 < w.sum() < 1.0 and ref["n_refit"] > 100
    else:
        assert 1 <= ref["n_refit"] <= few
    T, T_ransac = (np.array(a[:]).reshape(4, 4) for a in (r.T, r.T_ransac))
    bad = cases.problems(T, r.n_refit, ref, dict(name=f"weights {how} dim={dim}", T=T_ransac))
    assert not bad, "\n".join(bad)
    ws.close()


# ------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("m", cases.MASK_SIZES)
def test_inlier_mask_sizes(lr, oracle, m):
    """lr_inlier_mask with a model given and, after an lr_ransac, with the model that call left on the workspace: bytes at and beyond m
    keep their 0x55, the count is the popcount (summed from wave ballots: sizes across the wave edges) and the restatement's."""
    c = cases.mask_case(m)
    ref = rc.mask(c["src"], c["tgt"], c["T"], c["thr2"])
    assert np.all(np.abs(ref["gap"]) > rc.SAFETY * ref["bound"])
    buf, n = lr.ransac.inlier_mask_dev(c["src"], c["tgt"], c["T"], c["thr2"], fill=0x55, room=m + 300)
    assert np.all(buf[m:] == 0x55) and set(np.unique(buf[:m])) <= {0, 1}
    assert n == int(buf[:m].sum()) == int(ref["inlier"].sum()) and np.array_equal(buf[:m].astype(bool), ref["inlier"])
    got, ne = oracle.inlier_mask(c["src"], c["tgt"], c["T"], c["thr2"])
    assert np.array_equal(buf[:m].astype(bool), got) and n == ne
    # T = NULL: the model of the last lr_ransac on the workspace
    T, info = lr.ransac.ransac_dev(c["src"], c["tgt"], 200, sample_size=3, use_elc=False)
    ws = lr.matching.workspace(max(m, 1), 1, 200)
    buf0, n0 = lr.ransac.inlier_mask_dev(c["src"], c["tgt"], None, c["thr2"], ws=ws, fill=0x55, room=m + 300)
    buf1, n1 = lr.ransac.inlier_mask_dev(c["src"], c["tgt"], T, c["thr2"], fill=0x55, room=m + 300)
    assert np.array_equal(buf0, buf1) and n0 == n1 and np.all(buf0[m:] == 0x55)
    if info["best_h"] >= 0:
        assert n0 == info["best_count"] == oracle.inlier_mask(c["src"], c["tgt"], T, c["thr2"])[1]


@pytest.mark.parametrize("which", ["at", "next32"])
def test_inlier_mask_on_the_exact_boundary(lr, which):
    c = cases.boundary_case(which)
    buf, n = lr.ransac.inlier_mask_dev(c["xyz0"], c["xyz1"], c["T"], c["thr2"], fill=0x55, room=64)
    assert np.array_equal(buf[:8].astype(bool), c["planted"]) and n == int(c["planted"].sum()) and np.all(buf[8:] == 0x55)


def test_workspace_mask_at_for_every_pair_of_a_ragged_batch(lr, oracle):
    """lr_workspace_mask_at, the m_dev form of the mask kernel: the live count n_corr is below the n0 bytes the buffer holds."""
    host, devp = _pairs(lr, 32)
    params = _params(lr, 2, "MNN", False)
    ws = lr.ext.Workspace(4100, 4100, 32, ITERS, max_pairs=len(devp))
    out = lr.FR.register_batch_dev(devp, params, ws=ws).cpu().numpy()
    thr2 = params.ransac.effective_thr2()
    for k, p in enumerate(host):
        r = lr.ext.PairResult.from_buffer_copy(out[k].tobytes())
        n0 = SIZES[k][0]
        _, c0, c1 = _lists(lr, ws, k, n0)
        buf, n = lr.ransac.mask_at_dev(ws, k, devp[k][0], devp[k][1], thr2, fill=0x55)
        m = r.n_corr
        assert m < n0 or n0 <= 5
        assert np.all(buf[m:] == 0x55) and set(np.unique(buf[:m])) <= {0, 1} and n == int(buf[:m].sum())
        T_ransac = np.array(r.T_ransac[:]).reshape(4, 4)
        ref = rc.mask(p["xyz0"][c0[:m]], p["xyz1"][c1[:m]], T_ransac, thr2)
        sure = np.abs(ref["gap"]) > rc.SAFETY * ref["bound"]
        assert np.array_equal(buf[:m].astype(bool)[sure], ref["inlier"][sure]), k
        got, ne = oracle.inlier_mask(p["xyz0"][c0[:m]], p["xyz1"][c1[:m]], T_ransac, thr2)
        assert np.array_equal(buf[:m].astype(bool), got) and n == ne
        if r.status == 0:
            assert n == r.ransac.best_count
    ws.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_stay_refusals(lr):
    """Each bad call returns its error code and writes nothing."""
    t, L = lr.torch, lr.ext.lib()
    c = cases.plain_case(255, "all")
    x0, x1, i1 = (t.from_numpy(c[k]).to(lr.dev) for k in ("xyz0", "xyz1", "idx1"))
    Tin = t.from_numpy(c["T"].reshape(16).copy()).to(lr.dev)
    Tout = t.full((16,), 7.0, dtype=t.float64, device=lr.dev)
    nin = t.full((1,), -5, dtype=t.int32, device=lr.dev)
    mask = t.full((255,), 0x55, dtype=t.uint8, device=lr.dev)
    ws = lr.ext.Workspace(255, 255, 32, ITERS, max_pairs=2)
    EINVAL, ESIZE = -1, -4
    refit = lambda ws_, x0_, n0, x1_, i1_, Ti, To: L.lr_refit(ws_, x0_, n0, x1_, i1_, Ti, 0.36, To, nin.data_ptr(), None)
    ok = (ws.handle, x0.data_ptr(), 255, x1.data_ptr(), i1.data_ptr(), Tin.data_ptr(), Tout.data_ptr())
    assert refit(*ok[:2], 0, *ok[3:]) == ESIZE and refit(*ok[:2], -1, *ok[3:]) == ESIZE and refit(*ok[:2], 256, *ok[3:]) == ESIZE
    for k in (0, 1, 3, 4, 5, 6):
        bad = list(ok); bad[k] = None
        assert refit(*bad) == EINVAL, k
    th = ctypes.c_float(0.36)
    assert L.lr_inlier_mask(None, None, x1.data_ptr(), 255, Tin.data_ptr(), th, mask.data_ptr(), nin.data_ptr(), None) == EINVAL
    assert L.lr_inlier_mask(None, x0.data_ptr(), None, 255, Tin.data_ptr(), th, mask.data_ptr(), nin.data_ptr(), None) == EINVAL
    assert L.lr_inlier_mask(None, x0.data_ptr(), x1.data_ptr(), 255, Tin.data_ptr(), th, None, nin.data_ptr(), None) == EINVAL
    assert L.lr_inlier_mask(None, x0.data_ptr(), x1.data_ptr(), -1, Tin.data_ptr(), th, mask.data_ptr(), nin.data_ptr(), None) == EINVAL
    assert L.lr_inlier_mask(None, x0.data_ptr(), x1.data_ptr(), 255, None, th, mask.data_ptr(), nin.data_ptr(), None) == EINVAL          # no model, no workspace
    assert L.lr_inlier_mask(ws.handle, x0.data_ptr(), x1.data_ptr(), 255, Tin.data_ptr(), ctypes.c_float(0.0), mask.data_ptr(), nin.data_ptr(), None) == EINVAL
    # pair beyond the last call: nothing registered yet, then a single-pair call on a two-pair workspace
    at = lambda pair, n0: L.lr_workspace_mask_at(ws.handle, pair, x0.data_ptr(), x1.data_ptr(), n0, th, mask.data_ptr(), nin.data_ptr(), None)
    lists = lambda pair, n0: L.lr_workspace_lists_at(ws.handle, pair, n0, i1.data_ptr(), None, None, None, None)
    p = synth.make_pair(N=255, N1=255, rho=0.5, s=0.9, seed=4400)
    devp = tuple(t.from_numpy(p[key]).to(lr.dev) for key in ("xyz0", "xyz1", "feats0", "feats1"))
    before = i1.cpu().numpy().copy()
    lr.FR.register_pair_dev(*devp, _params(lr, 1, "MNN", False), ws=ws)
    assert at(1, 255) == EINVAL and at(2, 255) == EINVAL and at(-1, 255) == EINVAL and lists(1, 255) == EINVAL and lists(2, 255) == EINVAL
    assert at(0, 0) == ESIZE and at(0, 256) == ESIZE and lists(0, 0) == ESIZE
    assert L.lr_workspace_mask_at(ws.handle, 0, None, x1.data_ptr(), 255, th, mask.data_ptr(), nin.data_ptr(), None) == EINVAL
    assert L.lr_workspace_mask_at(ws.handle, 0, x0.data_ptr(), x1.data_ptr(), 255, th, None, nin.data_ptr(), None) == EINVAL
    t.cuda.synchronize()
    assert np.all(Tout.cpu().numpy() == 7.0) and int(nin.item()) == -5 and np.all(mask.cpu().numpy() == 0x55)
    assert np.array_equal(i1.cpu().numpy(), before)
    ws.close()
