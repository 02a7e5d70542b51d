"""Fixture G29 (tests/golden/make_golden_gpf_wide.py): the reference's own matching.py -- find_2nn, nn_to_mutual, the feature-distance
ratio and Grid_Prioritized_Filter in both forms -- at 33 numbers per descriptor, against the oracle, with the comparison and the
tolerances tests/test_oracle_golden.py applies to the 32-wide fixtures G2 .. G5.  The wide workspace is held to the oracle on the GPU
(tests/test_gpu_register_wide.py); this test holds the oracle to the reference at that width."""
import numpy as np
import pytest

from tests import wide_cases
from tests.conftest import Args, golden


@pytest.fixture(scope="module")
def case(oracle):
    g = golden("g29_gpf_wide.npz")
    n, d, seed = [int(v) for v in g["shape"]]
    p = wide_cases.reg_pair(n, d, seed)
    i0, i1, i2, _ = oracle.find_2nn(p["feats0"], p["feats1"])
    return dict(g=g, F0=p["feats0"], F1=p["feats1"], xyz0=p["xyz0"], i0=i0, i1=i1, i2=i2)


def test_g29_nn_mutual_and_ratio(oracle, case):
    g = case["g"]
    assert case["F0"].shape[1] == 33
    assert np.array_equal(case["i1"], g["idx1"]) and np.array_equal(case["i2"], g["idx2"])
    m0, m1, m2 = oracle.nn_to_mutual(case["F0"], case["F1"], case["i0"], case["i1"], case["i2"])
    assert np.array_equal(m0, g["mnn_idx0"]) and np.array_equal(m1, g["mnn_idx1"]) and np.array_equal(m2, g["mnn_idx2"])
    r = oracle.calc_distance_ratio_in_feature_space(case["F0"], case["F1"], case["i0"], case["i1"], case["i2"])
    np.testing.assert_allclose(r, g["ratio_nn"], rtol=2e-6, atol=0)
    r = oracle.calc_distance_ratio_in_feature_space(case["F0"], case["F1"], g["mnn_idx0"], g["mnn_idx1"], g["mnn_idx2"])
    np.testing.assert_allclose(r, g["ratio_mnn"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("k", [0, 1])
def test_g29_gpf(oracle, case, k):
    g = case["g"]
    factor, wid = g[f"gpf{k}_cfg"]
    out = oracle.Grid_Prioritized_Filter(case["F0"], case["F1"], case["i0"], case["i1"], case["i2"], case["xyz0"],
                                         Args(GPF_grid_wid=int(wid), GPF_factor=float(factor)))
    assert np.array_equal(out[0], g[f"gpf{k}_idx0"]) and np.array_equal(out[1], g[f"gpf{k}_idx1"]) and np.array_equal(out[2], g[f"gpf{k}_idx2"])
    np.testing.assert_allclose(out[6], g[f"gpf{k}_score"], rtol=0, atol=3e-6)


@pytest.mark.parametrize("k", [0, 1])
def test_g29_gpf_bb_first(oracle, case, k):
    g = case["g"]
    out = oracle.Grid_Prioritized_Filter(case["F0"], case["F1"], case["i0"], case["i1"], case["i2"], case["xyz0"],
                                         Args(GPF_max_matches=int(g[f"gpfbb{k}_cap"])), BB_first=True)
    assert np.array_equal(out[0], g[f"gpfbb{k}_idx0"]) and np.array_equal(out[1], g[f"gpfbb{k}_idx1"])
    assert (out[6] is not None) == bool(g[f"gpfbb{k}_has_score"])
    if out[6] is not None:
        np.testing.assert_allclose(out[6], g[f"gpfbb{k}_score"], rtol=0, atol=3e-6)
