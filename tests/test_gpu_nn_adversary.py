"""The NN kernel's f16 filter pass against inputs that use up its safety margins (tests/nn_adversary.py): lists and distances
bit-identical to the oracle, the planted neighbours confirmed by exact integer distances, and proof that the filter pass decided
them (no row re-done by the exact scan of all columns).  Needs an MI355X."""

import numpy as np
import pytest

from tests import nn_adversary as A
from tests.conftest import Args

pytestmark = pytest.mark.gpu

CASES = list(A.CASES)


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, matching
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.matching = matching; ns.torch = torch; ns.ext = _ext
    return ns


_ORACLE = {}


def _oracle(oracle, name):
    """(idx1, idx2, s1, s2, mutual idx0, mutual idx1) of the oracle for case `name`, once per process."""
    if name not in _ORACLE:
        p = A.make(name)
        o1, o2, s1, s2 = oracle.nn_top2(p.F0, p.F1)
        m = oracle.nn_to_mutual(p.F0, p.F1, np.arange(len(p.F0)), o1, o2)
        m1 = oracle.nn_to_mutual(p.F0, p.F1, np.arange(len(p.F0)), o1)
        _ORACLE[name] = (o1, o2, s1, s2, m, m1)
    return _ORACLE[name]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _witness(p, idx1, rev_pairs_mutual):
    """The exact integer distances agree with what the kernel returned for the planted rows / groups."""
    if len(p.rows):
        assert np.array_equal(idx1[p.rows], p.true)
        for r, i in enumerate(p.rows[:8]):
            ex = A.exact_d2_int(p.F0, p.F1, [(i, p.true[r])] + [(i, j) for j in p.decoys[r]])
            assert ex[0] < min(ex[1:])
    if len(p.jrow):
        assert np.array_equal(idx1[p.istar], p.jrow) and np.array_equal(idx1[p.iprime], p.j1)
        for g in range(min(8, len(p.jrow))):
            a, b = A.exact_d2_int(p.F0, p.F1, [(p.iprime[g], p.jrow[g]), (p.istar[g], p.jrow[g])])
            assert a < b
        assert not np.isin(p.istar, rev_pairs_mutual).any()        # i* is not mutual: j's reverse neighbour is i'


@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_nn_top2_and_mutual_bit_exact_on_adversarial_rounding(lr, oracle, name, stride):
    """nn_top2_dev and nn_to_mutual (single pair: several strips with pooled thresholds) at the default sampling stride and at 1
    (every tile sampled: the start thresholds are the tightest the sample can give)."""
    p = A.make(name)
    o1, o2, os1, os2, m, m1 = _oracle(oracle, name)
    t = lr.torch.from_numpy
    n0, n1, d = p.F0.shape[0], p.F1.shape[0], p.F0.shape[1]
    ws = lr.matching.workspace(n0, n1, dim=d)
    ws.set_option("nn_sample_stride", stride)
    try:
        for want_2nd in ((True, False) if p.need == 1 else (True,)):
            i1, i2, s1, s2 = lr.matching.nn_top2_dev(p.F0, p.F1, want_2nd=want_2nd, want_dist=True)
            assert np.array_equal(i1.cpu().numpy(), o1) and np.array_equal(_bits(s1.cpu().numpy()), _bits(os1))
            if want_2nd:
                assert np.array_equal(i2.cpu().numpy(), o2) and np.array_equal(_bits(s2.cpu().numpy()), _bits(os2))
        g = lr.matching.nn_to_mutual(t(p.F0), t(p.F1), t(np.arange(n0)), t(o1.astype(np.int64)), t(o2.astype(np.int64)))
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(g, m))
        g1 = lr.matching.nn_to_mutual(t(p.F0), t(p.F1), t(np.arange(n0)), t(o1.astype(np.int64)))
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(g1, m1))
        _witness(p, i1.cpu().numpy(), g[0].numpy())
    finally:
        ws.set_option("nn_sample_stride", 0)


def _params(lr):
    return lr.FR.pair_params(Args(mode="MNN", codebase="open3D", iters=200, ransac_n=3, o3d_conf=1.0))


def _lists(lr, ws, pair, n0, dev):
    bufs = [lr.torch.empty(n0, dtype=lr.torch.int32, device=dev) for _ in range(4)]
    lr.ext.check(lr.ext.lib().lr_workspace_lists_at(ws.handle, pair, n0, *[b.data_ptr() for b in bufs], None))
    return [b.cpu().numpy() for b in bufs]


@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_register_pair_decides_adversarial_rows_in_the_filter_pass(lr, oracle, name, stride):
    """lr_register_pair (MNN): NN and mutual lists equal the oracle's, and no row went to the exact-scan fallback
    (n_nn_fixed == 0, no form miss) -- the margins themselves kept the planted neighbours.  The first call warms the form hint on
    the same norms.  Top-1 cases run with the second neighbour switched off (need = 1, reverse ordered by s1)."""
    p = A.make(name)
    o1, o2, _, _, m, m1 = _oracle(oracle, name)
    t = lr.torch.from_numpy
    dev = lr.torch.device("cuda", 0)
    n0, n1, d = p.F0.shape[0], p.F1.shape[0], p.F0.shape[1]
    rng = np.random.default_rng(3)
    xyz0 = t(rng.random((n0, 3), np.float32)).to(dev); xyz1 = t(rng.random((n1, 3), np.float32)).to(dev)
    f0, f1 = t(p.F0).to(dev), t(p.F1).to(dev)
    params = _params(lr)
    ws = lr.ext.Workspace(n0, n1, d, params.ransac.iters)
    try:
        ws.set_option("nn_sample_stride", stride)
        if p.need == 1:
            ws.set_option("nn_second_auto", 1)
        for _ in range(2):
            ws.poison(0x5A)
            out = lr.FR.register_pair_dev(xyz0, xyz1, f0, f1, params, ws=ws)
            r = lr.ext.PairResult.from_buffer_copy(out.cpu().numpy().tobytes())
        assert r.n_nn_fixed == 0 and r.reserved[2] == 0, (r.n_nn_fixed, r.reserved[2])
        nn1, nn2, c0, c1 = _lists(lr, ws, 0, n0, dev)
        mm = m if p.need == 2 else m1
        assert np.array_equal(nn1, o1)
        if p.need == 2:
            assert np.array_equal(nn2, o2)
        assert r.n_corr == len(mm[0]) and np.array_equal(c0[:r.n_corr], mm[0]) and np.array_equal(c1[:r.n_corr], mm[1])
        _witness(p, nn1, c0[:r.n_corr])
    finally:
        ws.close()


@pytest.mark.parametrize("name", CASES)
def test_register_batch_adversarial_pair_among_ordinary_ones(lr, oracle, name):
    """lr_register_batch with the adversarial pair between two ordinary ones (one strip per row block, joint tightening rounds):
    its lists equal the oracle's and it was decided without the exact-scan fallback."""
    from lidarregistration_amd import synth
    p = A.make(name)
    o1, o2, _, _, m, _ = _oracle(oracle, name)
    t = lr.torch.from_numpy
    dev = lr.torch.device("cuda", 0)
    n0, n1, d = p.F0.shape[0], p.F1.shape[0], p.F0.shape[1]
    others = [synth.make_features(3000 + 700 * k, 3500, d, 0.5, 1.0, 40 + k) for k in range(2)]
    feats = [others[0], (p.F0, p.F1), others[1]]
    pairs = [(lr.torch.rand(A_.shape[0], 3, device=dev), lr.torch.rand(B_.shape[0], 3, device=dev), t(A_).to(dev), t(B_).to(dev))
             for A_, B_ in feats]
    params = _params(lr)
    ws = lr.ext.Workspace(max(n0, 5000), max(n1, 5000), d, params.ransac.iters, max_pairs=3)
    try:
        ws.poison(0xA5)
        out = lr.FR.register_batch_dev(pairs, params, ws=ws).cpu().numpy()
        r = lr.ext.PairResult.from_buffer_copy(out[1].tobytes())
        assert r.n_nn_fixed == 0, r.n_nn_fixed
        nn1, nn2, c0, c1 = _lists(lr, ws, 1, n0, dev)
        assert np.array_equal(nn1, o1) and np.array_equal(nn2, o2)
        assert r.n_corr == len(m[0]) and np.array_equal(c0[:r.n_corr], m[0]) and np.array_equal(c1[:r.n_corr], m[1])
        _witness(p, nn1, c0[:r.n_corr])
        # the ordinary pairs of the batch are still the oracle's
        for k, (F0, F1) in ((0, others[0]), (2, others[1])):
            e1, e2, _, _ = oracle.nn_top2(F0, F1)
            g1, g2, _, _ = _lists(lr, ws, k, F0.shape[0], dev)
            assert np.array_equal(g1, e1) and np.array_equal(g2, e2), k
    finally:
        ws.close()
