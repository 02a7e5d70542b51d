"""CPU checks of tests/ransac_hp.py: the numpy restatements agree with the oracle, and the fp32 decision band holds."""
import numpy as np
import pytest

from tests import ransac_hp as hp


def test_philox_known_answers(oracle):
    # Random123 known-answer vectors of philox4x32_10 (kat_vectors: counter, key -> output)
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, out in kat:
        assert tuple(int(x) for x in hp.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))) == out
    ids = np.array([0, 1, 7, 2 ** 31 + 5, 2 ** 33 + 3], np.uint64)
    for seed in (0, 51, 2 ** 40 + 7):
        w = hp.philox_words(seed, ids)
        for k, h in enumerate(ids):
            assert np.array_equal(w[k], oracle.philox(seed, int(h)))


@pytest.mark.parametrize("m", [3, 4, 7, 2049, 5001])
@pytest.mark.parametrize("ns", [3, 4])
def test_hypotheses_match_the_oracle(oracle, m, ns):
    """Same sample indices and ELC verdicts as oracle.hypothesis for every id; the SVD fit equals the oracle's model within
    1e-12 (rotation) and 1e-12 (1 + |coordinates|) (translation) where the sample's cross-covariance has sigma_1 / sigma_2 <= 1e4;
    on the degenerate samples (repeated indices) the two fits reach the same least-squares residual."""
    rng = np.random.default_rng(m * 10 + ns)
    src = rng.uniform(-40, 40, (m, 3)).astype(np.float32)
    T = hp.motion(rng)
    tgt = (src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.3, (m, 3))).astype(np.float32)
    ids = np.arange(1500)
    H = hp.hypotheses(src, tgt, ids, ns=ns, seed=9)
    n_cmp = 0
    for h in ids:
        ok, To, s = oracle.hypothesis(src, tgt, int(h), sample_size=ns, use_elc=True, seed=9)
        assert np.array_equal(s, H["sample"][h]) and ok == H["valid"][h], h
        if not ok:
            continue                      # (the oracle fits only samples that pass)
        P = src[s].astype(np.float64); Q = tgt[s].astype(np.float64)
        sv = H["sv"][h]
        if sv[1] > 1e-4 * sv[0]:
            n_cmp += 1
            assert np.abs(To[:3, :3] - H["T"][h][:3, :3]).max() <= 1e-12, h
            assert np.abs(To[:3, 3] - H["T"][h][:3, 3]).max() <= 1e-12 * (1 + np.abs(np.r_[P, Q]).max()), h
        else:
            res = [np.sum((P @ X[:3, :3].T + X[:3, 3] - Q) ** 2) for X in (To, H["T"][h])]
            assert abs(res[0] - res[1]) <= 1e-9 * (1 + res[1]), h
    assert n_cmp > (300 if m > 7 else 20)


@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1e-3, 0.0), (30.0, 0.0), (1.0, 1e3), (45.0, 1e3), (0.02, -1e3)])
def test_band_bound_holds_against_the_oracle(oracle, scale, offset):
    """Over many random models: outside the band, the oracle's fp32 decisions are the fp64 ones (scored on the non-band subset the
    counts are equal); its count is within the band size and its error sum within ssq_tolerance of the fp64 ones."""
    rng = np.random.default_rng(int(scale * 1000) + int(abs(offset)))
    for trial in range(25):
        thr = scale * rng.uniform(0.3, 1.0)
        src, tgt, T = hp.near_threshold_set(3000, 300, thr, eta=10 ** rng.uniform(-7, -2), n_band=30, rng=rng, offset=offset)
        Tm = T.copy()
        if trial % 2:                                    # a model a little off the planted motion
            if trial % 5 == 0:
                Tm[:3, :3] = hp.motion(rng)[:3, :3]       # (a wrong model: nearly everything is an outlier)
            Tm[:3, 3] += rng.normal(0, thr / 50, 3)
        thr2 = np.float32(thr * thr)
        ref = hp.score_fp64(src, tgt, Tm, thr2)
        c32, q32 = oracle.score(src, tgt, Tm, thr2=thr2)
        out = ~ref["band"]
        c_out, _ = oracle.score(src[out], tgt[out], Tm, thr2=thr2)
        assert c_out == int(ref["inlier"][out].sum())
        assert abs(c32 - ref["count"]) <= int(ref["band"].sum())
        assert abs(q32 / hp.SCALE - ref["ssq"]) <= hp.ssq_tolerance(ref, c32)


def test_band_is_narrow_and_catches_planted_members():
    """The band is a rounding-sized sliver: near-threshold points at 1 +- 1e-3 lie outside it, points planted at the threshold
    itself (up to the fp32 rounding of their target) lie in it."""
    rng = np.random.default_rng(3)
    src, tgt, T = hp.near_threshold_set(2000, 200, 0.6, eta=1e-3, n_band=25, rng=rng)
    ref = hp.score_fp64(src, tgt, T, np.float32(0.36))
    near = np.abs(ref["d2"] - 0.36) < 1e-5 * 0.36          # the planted ones (|d2 / thr2 - 1| ~ 1e-7 from the rounding of tgt)
    assert near.sum() == 25 and np.array_equal(ref["band"], near)
    assert np.max(ref["delta"]) < 1e-3 * 0.36               # well inside the 2 eta = 2e-3 gap to the other near-threshold points


def test_scaled_scene_keeps_the_planted_motion():
    for thr, off in [(45.0, 0.0), (45.0, 1e3), (0.6, 1e3), (1e-3, 0.0)]:
        src, tgt, T = hp.scaled_scene(2000, thr, rng=np.random.default_rng(1), offset=off)
        ref = hp.score_fp64(src, tgt, T, np.float32(thr * thr))
        assert ref["count"] > 0.35 * 2000
        assert np.ptp(src, axis=0).max() > 30 * thr or thr < 2
