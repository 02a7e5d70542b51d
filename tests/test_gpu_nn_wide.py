"""lr_nn_wide through the C ABI, bit for bit against the oracle's orc_nn_top2 (indices and the bits of s1 / s2): every width class, sizes
below one tile and past one strip, duplicate columns across every boundary, non-finite and zero rows, the optional outputs, poisoned
scratch, a hipGraph replay, fixture G28 and matching.py's routing of descriptors wider than 32."""
import ctypes
import itertools

import numpy as np
import pytest

from lidarregistration_amd import synth
from tests.conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, devmem, matching
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.matching = matching; ns.devmem = devmem; ns.L = _ext.lib()
    return ns


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(lr, F0, F1, want=(True, True, True), poison=None):
    """(idx1, idx2, s1, s2) as numpy (None where not asked for) from one lr_nn_wide call."""
    torch = lr.torch
    n0 = len(F0)
    t0, t1 = torch.from_numpy(np.ascontiguousarray(F0, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(F1, np.float32)).cuda()
    idx1 = torch.full((n0,), -7, dtype=torch.int32, device="cuda")
    idx2 = torch.full((n0,), -7, dtype=torch.int32, device="cuda") if want[0] else None
    s1 = torch.full((n0,), -7.0, dtype=torch.float32, device="cuda") if want[1] else None
    s2 = torch.full((n0,), -7.0, dtype=torch.float32, device="cuda") if want[2] else None
    lr.matching.nn_wide_into(t0, t1, idx1, idx2, s1, s2, poison=poison)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (idx1, idx2, s1, s2))


def assert_equal(got, want):
    assert np.array_equal(got[0], want[0])
    if got[1] is not None: assert np.array_equal(got[1], want[1])
    if got[2] is not None: assert np.array_equal(bits(got[2]), bits(want[2]))
    if got[3] is not None: assert np.array_equal(bits(got[3]), bits(want[3]))


def feats(n0, n1, d, seed):
    rng = np.random.default_rng(seed)
    F0 = (rng.standard_normal((n0, d)) * rng.uniform(0.5, 2.0, (n0, 1))).astype(np.float32)      # not unit norm
    F1 = rng.standard_normal((n1, d)).astype(np.float32)
    k = min(n0, n1) // 2
    F1[:k] = F0[:k] + 0.3 * rng.standard_normal((k, d)).astype(np.float32)
    return F0, F1


@pytest.mark.parametrize("d", [33, 34, 64, 127, 128])
@pytest.mark.parametrize("n0,n1", [(1, 1), (33, 31), (2049, 4097)])
def test_bit_exact(lr, oracle, d, n0, n1):
    F0, F1 = feats(n0, n1, d, 100 * d + n0)
    want = oracle.nn_top2(F0, F1)
    assert_equal(run(lr, F0, F1), want)
    if n1 == 1:
        assert want[1][0] == -1 and np.isinf(want[3][0])


@pytest.mark.parametrize("d", [33, 48, 96, 128])
def test_duplicate_columns_lowest_index_wins(lr, oracle, d):
    """Every row of F1 is one of 7 vectors, laid out so that the copies of a row's nearest vector sit inside one 32-column tile, across
    tile boundaries and across every strip boundary the launch can have (all of them: the pattern repeats through the whole cloud)."""
    rng = np.random.default_rng(d)
    n0, n1 = 300, 4097
    pool = rng.standard_normal((7, d)).astype(np.float32)
    which = rng.integers(0, 7, n1)
    which[:200] = 1                                  # vector 1: its first two copies inside one tile (columns 0, 1)
    which[31] = which[32] = 2                        # vector 2: across a tile boundary
    which[95] = which[96] = 0                        # vector 0: across a strip boundary (300 rows: strips of 3 tiles)
    which[5] = which[100] = 3                        # vector 3: first copy in strip 0, second in strip 1
    which[97] = which[130] = 4                       # vector 4: two tiles of strip 1
    which[150] = 5                                   # vector 5: the second copy far away; vector 6: both past column 200
    F1 = pool[which]
    F0 = (pool[rng.integers(0, 7, n0)] + 0.05 * rng.standard_normal((n0, d))).astype(np.float32)
    want = oracle.nn_top2(F0, F1)
    got = run(lr, F0, F1)
    assert_equal(got, want)
    first = np.array([np.nonzero(which == v)[0][:2] for v in range(7)])
    near = np.array([np.argmin(((F0[i].astype(np.float64) - pool.astype(np.float64)) ** 2).sum(1)) for i in range(n0)])
    assert np.array_equal(got[0], first[near, 0]) and np.array_equal(got[1], first[near, 1])
    assert np.array_equal(bits(got[2]), bits(got[3]))
    # ... and with the copies of every vector only in the last columns of the cloud (the last strip, a partial tile)
    F1b = rng.standard_normal((n1, d)).astype(np.float32) * 3.0
    F1b[-9:-2] = pool; F1b[-2:] = pool[:2]; F1b[31] = pool[6]; F1b[32] = pool[6]
    assert_equal(run(lr, F0, F1b), oracle.nn_top2(F0, F1b))


def test_non_finite_and_zero_rows(lr, oracle):
    d = 33
    F0, F1 = feats(500, 700, d, 9)
    F0[3] = 0.0; F0[17, 5] = np.nan; F0[18, 32] = np.inf
    assert_equal(run(lr, F0, F1), oracle.nn_top2(F0, F1))
    F1[40] = 0.0; F1[333, 32] = np.nan; F1[650] = -np.inf; F1[651] = 3e19
    want = oracle.nn_top2(F0, F1)
    got = run(lr, F0, F1)
    assert_equal(got, want)
    assert not np.isnan(got[2]).any() and not np.isnan(got[3]).any()              # no NaN distance is ever returned: fmaxf drops it


def test_optional_outputs_and_poisoned_scratch(lr, oracle):
    F0, F1 = feats(777, 2100, 64, 3)
    want = oracle.nn_top2(F0, F1)
    for combo in itertools.product((False, True), repeat=3):
        assert_equal(run(lr, F0, F1, want=combo, poison=0xFF if combo[0] else 0x00), want)
    a, b = run(lr, F0, F1, poison=0x00), run(lr, F0, F1, poison=0xFF)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_graph_replay(lr, oracle):
    torch = lr.torch
    d, n0, n1 = 33, 700, 1500
    inputs = [feats(n0, n1, d, 40 + k) for k in range(3)]
    A = torch.empty((n0, d), dtype=torch.float32, device="cuda"); B = torch.empty((n1, d), dtype=torch.float32, device="cuda")
    idx1 = torch.empty(n0, dtype=torch.int32, device="cuda"); idx2 = torch.empty_like(idx1)
    s1 = torch.empty(n0, dtype=torch.float32, device="cuda"); s2 = torch.empty_like(s1)
    need = lr.L.lr_nn_wide_scratch_bytes(n0, n1, d)
    sc = lr.devmem.scratch(need, A.device)
    s = torch.cuda.Stream()

    def call():
        lr.ext.check(lr.L.lr_nn_wide(A.data_ptr(), n0, B.data_ptr(), n1, d, idx1.data_ptr(), idx2.data_ptr(), s1.data_ptr(), s2.data_ptr(),
                                     sc.data_ptr(), need, torch.cuda.current_stream().cuda_stream))

    def load(x):
        A.copy_(torch.from_numpy(x[0])); B.copy_(torch.from_numpy(x[1])); torch.cuda.synchronize()

    def outputs():
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (idx1, idx2, s1, s2)]
    load(inputs[0])
    with torch.cuda.stream(s):
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k, x in list(enumerate(inputs))[::-1]:
        load(x); sc.fill_(0xFF if k & 1 else 0x00); idx1.fill_(-5); s2.fill_(-5.0); g.replay()
        want = oracle.nn_top2(*x)
        assert outputs() == [np.ascontiguousarray(w).tobytes() for w in want]


@pytest.mark.parametrize("tag", ["d33", "d64", "d128"])
def test_golden_and_matching_routing(lr, oracle, tag):
    g = golden("g28_nn_wide.npz")
    n0, n1, d, seed = [int(v) for v in g[f"{tag}_shape"]]
    F0, F1 = synth.make_features(n0, n1, d, 0.5, 0.5, seed)
    t = lr.torch.from_numpy
    i0, i1, i2, extra = lr.matching.find_2nn(t(F0), t(F1))
    assert extra == 0.0 and np.array_equal(i0.numpy(), np.arange(n0))
    assert np.array_equal(i1.numpy(), g[f"{tag}_idx1"]) and np.array_equal(i2.numpy(), g[f"{tag}_idx2"])
    j0, j1, none = lr.matching.find_nn(t(F0), t(F1))
    assert none is None and np.array_equal(j1.numpy(), i1.numpy())
    m = lr.matching.nn_to_mutual(t(F0), t(F1), i0, i1, i2)
    for ours, key in zip(m, ("m0", "m1", "m2")):
        assert ours.dtype == lr.torch.int64 and np.array_equal(ours.numpy(), g[f"{tag}_{key}"])
    m2 = lr.matching.nn_to_mutual(t(F0), t(F1), i0, i1)
    assert len(m2) == 2 and np.array_equal(m2[0].numpy(), g[f"{tag}_m0"])


def test_nn_to_mutual_at_33_against_the_oracle(lr, oracle):
    F0, F1 = feats(2049, 1777, 33, 12)
    F1[5] = F1[4]                                    # a duplicate pair among the targets
    t = lr.torch.from_numpy
    i0, i1, i2, _ = lr.matching.find_2nn(t(F0), t(F1))
    e0, e1, e2, _ = oracle.find_2nn(F0, F1)
    assert np.array_equal(i1.numpy(), e1) and np.array_equal(i2.numpy(), e2)
    m = lr.matching.nn_to_mutual(t(F0), t(F1), i0, i1, i2)
    em = oracle.nn_to_mutual(F0, F1, e0, e1, e2)
    for a, b in zip(m, em):
        assert np.array_equal(a.numpy(), b)
    is_bb, n_bb = lr.matching.mark_best_buddies(t(F0), t(F1), i0, i1)
    e_bb, e_n = oracle.mark_best_buddies(F0, F1, e0, e1)
    assert np.array_equal(is_bb, e_bb) and n_bb == e_n == len(em[0])


@pytest.mark.parametrize("d,word", [(32, "use lr_nn_top2"), (129, "33..128")])
def test_other_widths_are_refused_and_nothing_is_written(lr, d, word):
    torch = lr.torch
    F = torch.zeros((64, d), device="cuda")
    outs = [torch.full((64,), -7, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.full((64,), -7.0, device="cuda") for _ in range(2)]
    sc = lr.devmem.scratch(1 << 20, F.device, poison=0x5A)
    rc = lr.L.lr_nn_wide(F.data_ptr(), 64, F.data_ptr(), 64, d, *[o.data_ptr() for o in outs], sc.data_ptr(), 1 << 20, None)
    torch.cuda.synchronize()
    assert rc == -1 and word in lr.L.lr_last_error().decode()
    assert all(bool((o == -7).all()) for o in outs) and bool((sc == 0x5A).all())
    if d == 32:
        assert ("lr_nn_top2" in word) and lr.L.lr_nn_wide_scratch_bytes(64, 64, d) == 0
    with pytest.raises(lr.ext.LidarRegError):
        lr.matching.find_nn(torch.zeros((8, 129)), torch.zeros((8, 129)))
