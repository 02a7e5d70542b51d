"""lr_ransac across its whole threshold range: bit-exact against the oracle, and within the fp32 band of independent fp64 scoring
(tests/ransac_hp.py).  Several kernel branches are chosen by the threshold (csrc/lr_ransac.hip, lr_score.hip, lr_lo.hip); every row restates the predicate
that picks its branch and asserts it, so the row is known to reach that branch.  Needs an MI355X."""
import numpy as np
import pytest

from tests import ransac_hp as hp
from tests.conftest import Args

pytestmark = pytest.mark.gpu

TWO32 = 2.0 ** 32
SC_MIN_V, SC_MIN_PAIRS, SC_MIN_M, SC_REACH = 128, 4, 2048, 128 * 0.0625      # LR_SC_MIN_V, LR_SC_MIN_PAIRS, LR_SC_MIN_M, LR_SC_NB * LR_SC_W
LO_THREADS, LO_CHUNK_REC = 1024, 384


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.ransac = ransac; ns.torch = torch; ns.ext = _ext
    return ns


# ----------------------------------------------------------------------------- the threshold predicates of lr_ransac.hip, lr_score.hip and lr_lo.hip

def f32_thr2(thr):
    return float(np.float32(float(thr) * float(thr)))           # what ransac_params / oracle._params store


def eff_thr2(thr2, scoring):
    return float(np.float32(np.float32(thr2) * np.float32(2.25))) if scoring == 2 else thr2       # eff_params / ransac_resolve


def sub_len(thr2):
    """lr_score_run: sub-block length of the 32-bit error sums of lr_score_stream."""
    sub = int(4095.0 / (thr2 * 1.0000001 + 1e-6))
    sub = min(sub, 4096) & ~1
    return max(sub, 2)


def lo_narrow(m, thr2):
    """lo_score: one model scored with 32-bit per-thread sums (lo_score_one) or 64-bit ones (lo_score_wide)."""
    return (m // LO_THREADS + 2) * float(np.float32(thr2)) * 1048576.0 < 4.0e9


def reach_clamped(thr2):
    """ransac_order_kernel: cut = thr + eps + slack, slack >= 0.01, eps >= 0 -- every model's reach is the whole list when this holds."""
    return float(np.sqrt(np.float32(thr2))) + 0.01 >= SC_REACH


# thr2 -> expected sub (the effective, i.e. after the 2.25 of scoring 2, squared threshold decides)
SUB = {1e-6: 4096, 0.36: 4096, 0.9997: 4096, 1.0003: 4092, 2.25: 1818, 49.0: 82, 64.1: 62, 100.0: 40, 1023.0: 4, 1025.0: 2,
       1907.0: 2, 1908.0: 2, 2047.9: 2}


def _scene(m, thr2, seed, offset=0.0, inlier=0.4):
    thr = float(np.sqrt(thr2))
    return hp.scaled_scene(m, thr, inlier=inlier, rng=np.random.default_rng(seed), offset=offset if thr >= 0.5 else 0.0)


def _mask_matches_oracle(oracle, src, tgt, T, thr2, mask):
    """The device mask is the oracle's decision per correspondence: scored on the mask every one is an inlier, off it none is."""
    c_in, _ = oracle.score(src[mask], tgt[mask], T, thr2=thr2) if mask.any() else (0, 0)
    c_out, _ = oracle.score(src[~mask], tgt[~mask], T, thr2=thr2) if (~mask).any() else (0, 0)
    assert c_in == int(mask.sum()) and c_out == 0


def _fp64_consistent(oracle, src, tgt, T, thr2, n_mask):
    """The fp32 count / error sum of T against fp64 scoring: within the band."""
    ref = hp.score_fp64(src, tgt, T, thr2)
    c32, q32 = oracle.score(src, tgt, T, thr2=thr2)
    nb = int(ref["band"].sum())
    assert abs(n_mask - ref["count"]) <= nb and abs(c32 - ref["count"]) <= nb
    assert abs(q32 / hp.SCALE - ref["ssq"]) <= hp.ssq_tolerance(ref, c32)
    return ref


def _rows():
    rows = []
    for thr2 in SUB:
        big = 2.25 * thr2 >= 2048.0
        rows.append(dict(thr2=thr2, scoring=0, local_opt=0, use_elc=1, m=2047, ns=3))
        rows.append(dict(thr2=thr2, scoring=1, local_opt=1, use_elc=1, m=2049, ns=4))
        if not big:
            rows.append(dict(thr2=thr2, scoring=2, local_opt=2, use_elc=1, m=1001, ns=3))
        rows.append(dict(thr2=thr2, scoring=1, local_opt=2, use_elc=2 if thr2 in (0.36, 100.0, 2047.9) else 0, m=1001, ns=3))
    return rows


@pytest.mark.parametrize("row", _rows(), ids=lambda r: "thr2={thr2}-sc{scoring}-lo{local_opt}-pre{use_elc}-m{m}".format(**r))
def test_single_pair_sweep(lr, oracle, row):
    thr2, m = row["thr2"], row["m"]
    thr = float(np.sqrt(thr2))
    t2 = eff_thr2(f32_thr2(thr), row["scoring"])
    # the branches this row reaches
    assert sub_len(t2) == SUB[thr2] if row["scoring"] != 2 else t2 < 2048.0
    if row["local_opt"] and m == 1001:
        assert lo_narrow(m, t2) == (t2 <= 1907.0)                        # the polish: lo_score_one, or lo_score_wide from 1908 on
    if row["local_opt"] == 1:
        assert m >= 4 * LO_CHUNK_REC                                      # single pair: the helper-block scoring jobs run
    src, tgt, T_gt = _scene(m, thr2, seed=int(thr2 * 10) + m, offset=1e3 if m == 2049 else 0.0)
    kw = dict(sample_size=row["ns"], use_elc=row["use_elc"], thr=thr, seed=17, scoring=row["scoring"], local_opt=row["local_opt"])
    iters = 1500
    T, info = lr.ransac.ransac_dev(src, tgt, iters, want_mask=True, **kw)
    Te, einfo = oracle.ransac(src, tgt, iters, **kw)
    mask = info.pop("mask"); n_mask = info.pop("n_inliers")
    assert info == einfo, (info, einfo)
    assert np.array_equal(T, Te)
    if info["best_h"] < 0:
        assert row["use_elc"] == 2 or thr2 < 1e-3
        return
    _mask_matches_oracle(oracle, src, tgt, T, t2, mask)
    ref = _fp64_consistent(oracle, src, tgt, T, t2, n_mask)
    if row["local_opt"] == 0:
        c32, q32 = oracle.score(src, tgt, T, thr2=t2)
        assert info["best_count"] == c32 and info["best_ssq"] == q32
        assert abs(info["best_count"] - ref["count"]) <= int(ref["band"].sum())


def test_thresholds_out_of_range_are_refused(lr):
    src, tgt, _ = _scene(500, 1.0, seed=1)
    for thr, scoring in [(np.sqrt(2048.0), 0), (np.sqrt(2048.0 / 2.25) * 1.0001, 2), (np.sqrt(1000.0), 2)]:
        with pytest.raises(lr.ext.LidarRegError) as e:
            lr.ransac.ransac_dev(src, tgt, 100, thr=thr, scoring=scoring)
        assert "error -1:" in str(e.value) and "thr2" in str(e.value)         # LR_EINVAL, from the argument checks before any launch
    lr.ransac.ransac_dev(src, tgt, 100, thr=np.sqrt(2047.9))                # the largest admissible one runs


# ----------------------------------------------------------------------------- batched calls: the pilot-ordered scoring

def _batch(lr, clouds, thr2, scoring=0, use_elc=1, local_opt=0, iters=2048, ns=3):
    dev = lr.torch.device("cuda", 0)
    a = Args(mode="no_filter", codebase="open3D", iters=iters, ransac_n=ns, o3d_conf=1.0, refit=0)
    p = lr.FR.pair_params(a)
    p.ransac.thr2 = f32_thr2(np.sqrt(thr2)); p.ransac.scoring = scoring; p.ransac.use_elc = use_elc; p.ransac.local_opt = local_opt
    p.ransac.seed = 23
    pairs = []
    for k, (src, tgt) in enumerate(clouds):
        # identical descriptors on both sides: every row's nearest neighbour is itself, the correspondences are (i, i)
        F = np.random.default_rng(k).normal(size=(len(src), 16)).astype(np.float32)
        t = lambda x: lr.torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        pairs.append((t(src), t(tgt), t(F), t(F)))
    out = lr.FR.register_batch_dev(pairs, p)
    lr.torch.cuda.synchronize()
    return [lr.ext.PairResult.from_buffer_copy(out[k].cpu().numpy().tobytes()) for k in range(len(clouds))]


@pytest.mark.parametrize("thr2,scoring,inlier,iters", [(0.36, 0, 0.4, 4096), (49.0, 1, 0.4, 4096), (64.1, 0, 0.4, 4096), (100.0, 2, 0.4, 4096),
                                                       (1023.0, 0, 0.4, 4096), (1025.0, 1, 0.4, 4096), (2047.9, 0, 0.4, 4096), (2.25, 0, 0.01, 2048)])
def test_batched_sweep_pilot_ordered(lr, oracle, thr2, scoring, inlier, iters):
    """More than LR_SC_MIN_PAIRS pairs of >= LR_SC_MIN_M correspondences and 2048 ids: the pilot-ordered scoring runs wherever a
    batch has >= LR_SC_MIN_V valid models (inlier 0.01 gives the ELC too few survivors: the plain pass over everything)."""
    assert iters >= 2048
    t2 = eff_thr2(f32_thr2(np.sqrt(thr2)), scoring)
    assert t2 < 2048.0
    ms = [2049, 2047, 2051, 3001, 2049, 2063]
    assert len(ms) > SC_MIN_PAIRS and min(ms) <= SC_MIN_M + 3
    clouds = []
    for k, m in enumerate(ms):
        src, tgt, _ = _scene(m, thr2, seed=100 * k + int(thr2), offset=1e3 if k == 3 else 0.0, inlier=inlier)
        clouds.append((src, tgt))
    res = _batch(lr, clouds, thr2, scoring=scoring, iters=iters)
    clamped = reach_clamped(t2)
    assert clamped == (t2 >= 64.0)                       # 49 (7 m) keeps a per-model reach, 64.1 and above reach everything
    for k, (src, tgt) in enumerate(clouds):
        r = res[k]
        assert r.n_corr == len(src)
        Te, einfo = oracle.ransac(src, tgt, iters, sample_size=3, use_elc=1, thr=float(np.sqrt(thr2)), seed=23, scoring=scoring)
        got = dict(best_h=r.ransac.best_h, best_count=r.ransac.best_count, best_ssq=r.ransac.best_ssq, n_valid=r.ransac.n_valid,
                   n_ids=r.ransac.n_ids)
        assert got == einfo, (k, got, einfo)
        assert np.array_equal(np.array(r.T[:]).reshape(4, 4), Te)
        if inlier < 0.05:
            assert got["n_valid"] < SC_MIN_V
        else:
            assert got["n_valid"] >= SC_MIN_V
        if got["best_h"] >= 0:
            _fp64_consistent(oracle, src, tgt, Te, t2, oracle.score(src, tgt, Te, thr2=t2)[0])


# ----------------------------------------------------------------------------- error-sum capacity

def _window_max(d2, inl, sub):
    """Largest 32-bit partial the main scoring can form: the fixed-point terms of `sub` consecutive correspondences."""
    v = np.where(inl, np.floor(np.float32(d2) * np.float32(1048576.0)), 0.0)
    c = np.concatenate([[0.0], np.cumsum(v)])
    sub = min(sub, len(v))
    return float(np.max(c[sub:] - c[:-sub]))


def _thread_max(d2, inl):
    """Largest per-thread 32-bit sum of lo_score_one: thread t takes the records (pairs of correspondences) t, t + 1024, ..."""
    v = np.where(inl, np.floor(np.float32(d2) * np.float32(1048576.0)), 0.0)
    v = np.concatenate([v, [0.0] * (len(v) % 2)]).reshape(-1, 2).sum(1)
    pad = (-len(v)) % LO_THREADS
    return float(np.concatenate([v, np.zeros(pad)]).reshape(-1, LO_THREADS).sum(0).max())


def _chunk_len(L, V):
    """ransac_score_kernel<0> on a single pair: the records one work item scans (its sub-blocks start at the item's first record)."""
    hb = (V + 63) // 64
    chunks = max(1, min(2048 // hb, max(L // 256, 1)))
    return ((L + chunks - 1) // chunks + 1) & ~1


@pytest.mark.parametrize("case", ["sub4096", "sub4092", "sub1818", "sub4", "sub2", "lo_one", "lo_wide", "lo_wide_overflow", "lo_helpers"])
def test_error_sum_capacity(lr, oracle, case):
    """Every non-exact correspondence sits at 0.99 thr: the 32-bit partial sums of the scoring come within 10 % of 2^32, next to
    the guards that keep them from overflowing (the sub-block length of lr_score_stream; lo_score's choice of lo_score_one).
    Bit-exact against the oracle."""
    thr2 = {"sub4096": 0.9997, "sub4092": 1.0003, "sub1818": 2.25, "sub4": 1023.0, "sub2": 2047.9, "lo_one": 119.0, "lo_wide": 121.0,
            "lo_wide_overflow": 200.0, "lo_helpers": 100.0}[case]
    sub_case = case.startswith("sub")
    # sub-block cases: 8192 models make every work item of the main pass 4098 records long, so a full sub-block is scanned
    m, iters, local_opt = (65537, 8192, 0) if sub_case else (31000, 3000, 1 if case == "lo_helpers" else 2)
    thr = float(np.sqrt(thr2))
    t2 = f32_thr2(thr)
    k = int(0.15 * m)
    src, tgt, T_gt = hp.near_threshold_set(m, k, thr, eta=0.01, rng=np.random.default_rng(m + int(thr2)), below=True, shuffle=False)
    if not sub_case:
        # the exact inliers go to records that threads 512..1023 of lo_score_one take: threads 0..139 see near-threshold ones only
        rec = np.arange((m + 1) // 2)
        slots = np.concatenate([2 * r + np.arange(2) for r in rec[(rec % LO_THREADS) >= 512]])
        slots = slots[slots < m][:k]
        rest = np.setdiff1d(np.arange(m), slots)
        order = np.empty(m, np.int64); order[slots] = np.arange(k); order[rest] = np.arange(k, m)
        src, tgt = src[order], tgt[order]
    kw = dict(sample_size=3, use_elc=0, thr=thr, seed=29, local_opt=local_opt)
    T, info = lr.ransac.ransac_dev(src, tgt, iters, **kw)
    Te, einfo = oracle.ransac(src, tgt, iters, **kw)
    assert info == einfo and np.array_equal(T, Te)
    ref = hp.score_fp64(src, tgt, T, t2)
    assert ref["count"] > 0.95 * m                                          # the planted motion was found: nearly all are inliers
    if sub_case:
        sub = sub_len(t2)
        assert sub == {"sub4096": 4096, "sub4092": 4092, "sub1818": 1818, "sub4": 4, "sub2": 2}[case]
        assert _chunk_len(m, info["n_valid"]) >= 4096
        w = _window_max(ref["d2"], ref["inlier"], sub)
        assert 0.9 * TWO32 < w < TWO32                                      # a sub-block's sum: within 10 % of 2^32, below it
        if case in ("sub1818", "sub4", "sub2"):
            assert _window_max(ref["d2"], ref["inlier"], 4096) > TWO32      # ... which a 4096-long block would overflow
    else:
        assert lo_narrow(m, t2) == (case in ("lo_one", "lo_helpers"))      # (lo_helpers: its final polish scores one model)
        tm = _thread_max(ref["d2"], ref["inlier"])
        if case == "lo_one":
            assert 0.9 * TWO32 < tm < TWO32
        if case == "lo_wide_overflow":
            assert tm > TWO32                                               # 32-bit per-thread sums would wrap
        if case == "lo_helpers":
            assert m >= 4 * LO_CHUNK_REC                                    # single pair: helper blocks take the scoring jobs


# ----------------------------------------------------------------------------- independent selection

@pytest.mark.parametrize("kind", ["near", "scene", "far"])
def test_selection_against_fp64_hypotheses(lr, oracle, kind):
    """Open3D semantics (count, then error sum; ELC; uniform sampler; no LO / SPRT): every numpy hypothesis is scored in fp64.
    With lo_h = count_h - band_h and hi_h = count_h + band_h (band: correspondences whose fp32 decision may differ), the kernel's
    winner w satisfies hi_w >= lo_h for every valid h; and among the h with band_h = band_w = 0 and count_h = count_w,
    ssq_w <= ssq_h + tol_w + tol_h (tol: ssq_tolerance, the truncation and rounding of the fixed-point sums).  Hypotheses whose
    sample is degenerate (sigma_1 / sigma_2 > 1e4 of its cross-covariance: the fit is not unique) are left out; there are few."""
    rng = np.random.default_rng({"near": 1, "scene": 2, "far": 3}[kind])
    m, iters, thr = 6000, 2000, 0.6
    if kind == "near":
        src, tgt, _ = hp.near_threshold_set(m, 900, thr, eta=1e-4, n_band=60, rng=rng)
    else:
        src, tgt, _ = hp.scaled_scene(m, thr, inlier=0.3, rng=rng, offset=1e3 if kind == "far" else 0.0)
    T, info = lr.ransac.ransac_dev(src, tgt, iters, sample_size=3, use_elc=True, thr=thr, seed=41)
    H = hp.hypotheses(src, tgt, np.arange(iters), ns=3, use_elc=True, seed=41)
    assert info["n_valid"] == int(H["valid"].sum())
    w = info["best_h"]
    assert w >= 0 and H["valid"][w]
    good = H["valid"] & (H["sv"][:, 1] > 1e-4 * H["sv"][:, 0])
    assert good[w] and good.sum() >= H["valid"].sum() - max(3, H["valid"].sum() // 100)
    np.testing.assert_allclose(T[:3, :3], H["T"][w][:3, :3], rtol=0, atol=1e-12)
    t2 = f32_thr2(thr)
    scale = float(np.abs(np.r_[src, tgt]).max())
    cnt, band, ssq, tol = {}, {}, {}, {}
    for h in np.nonzero(good)[0]:
        r = hp.score_fp64(src, tgt, H["T"][h], t2, t_err=1e-11 * (1 + scale))     # (the numpy fit vs the kernel's: within 1e-12 (1 + |c|))
        cnt[h], band[h], ssq[h] = r["count"], int(r["band"].sum()), r["ssq"]
        tol[h] = hp.ssq_tolerance(r, r["count"])
    hi_w = cnt[w] + band[w]
    for h in cnt:
        assert hi_w >= cnt[h] - band[h], (h, cnt[h], band[h], w, cnt[w], band[w])
        if band[h] == 0 and band[w] == 0 and cnt[h] == cnt[w]:
            assert ssq[w] <= ssq[h] + tol[w] + tol[h], (h, w)
    assert info["best_count"] <= hi_w and info["best_count"] >= cnt[w] - band[w]
