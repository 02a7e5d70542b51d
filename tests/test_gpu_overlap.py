"""lr_voxel_mean / lr_overlap / lr_overlap_batch and their Python mirror (lidarregistration_amd/overlap.py) against the numpy restatement
of the contract (tests/overlap_cpu.py): centroids, counts, first indices, n_overlap, both fractions and the statuses bit for bit.
Needs an MI355X."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import icp_ref, overlap_cases, overlap_cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g17_overlap.npz"))
CLOUDS = overlap_cases.cloud_cases()
PAIRS = {**overlap_cases.golden_cases(), **overlap_cases.search_cases(), **{f"batch_{k}": p for k, p in enumerate(overlap_cases.batch_pairs())}}
KEYS = ("status", "n0_ds", "n1_ds", "n_overlap", "n0_dropped", "n1_dropped", "frac", "frac_sym")
SENT = -7


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, overlap, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.ov = overlap; ns.ransac = ransac
    return ns


@functools.lru_cache(maxsize=None)
def ref_cloud(name):
    return overlap_cpu.voxel_mean(*CLOUDS[name])


@functools.lru_cache(maxsize=None)
def ref_pair(name):
    p = PAIRS[name]
    return overlap_cpu.overlap(p["A"], p["B"], p["T"], p["voxel"], p["radius"])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def raw_voxel_mean(lr, X, voxel, T=None, poison=None):
    """lr_voxel_mean into buffers pre-filled with a sentinel: (cent, cent_f32, counts, first) in full length, info."""
    torch, L = lr.torch, lr.ext.lib()
    n = len(X)
    x = torch.from_numpy(np.ascontiguousarray(X, np.float64)).cuda()
    Td = None if T is None else torch.from_numpy(np.ascontiguousarray(T, np.float64).reshape(16)).cuda()
    m = max(n, 1)
    cent = torch.full((m, 3), float(SENT), dtype=torch.float64, device="cuda"); c32 = torch.full((m, 3), float(SENT), dtype=torch.float32, device="cuda")
    counts = torch.full((m,), SENT, dtype=torch.int32, device="cuda"); first = torch.full((m,), SENT, dtype=torch.int32, device="cuda")
    info = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lr_voxel_mean_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    if poison is not None:
        scratch.fill_(poison)
    lr.ext.check(L.lr_voxel_mean(x.data_ptr() if n else None, n, None if Td is None else Td.data_ptr(), float(voxel), cent.data_ptr(), c32.data_ptr(),
                                 counts.data_ptr(), first.data_ptr(), info.data_ptr(), scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return cent.cpu().numpy(), c32.cpu().numpy(), counts.cpu().numpy(), first.cpu().numpy(), info.cpu().numpy()


def check_cloud(out, ref):
    cent, c32, counts, first, info = out
    rows = ref["rows"]
    assert tuple(info) == (rows, ref["dropped"], ref["status"], 0)
    assert np.array_equal(bits(cent[:rows]), bits(ref["cent"]))
    with np.errstate(over="ignore"):
        assert np.array_equal(c32[:rows].view(np.uint32), ref["cent"].astype(np.float32).view(np.uint32))
    assert np.array_equal(counts[:rows], ref["counts"]) and np.array_equal(first[:rows], ref["first"])
    # nothing behind the rows is written (status 2: nothing at all)
    assert (cent[rows:] == SENT).all() and (c32[rows:] == SENT).all() and (counts[rows:] == SENT).all() and (first[rows:] == SENT).all()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_voxel_mean_equals_the_restatement(lr, name):
    X, voxel, T = CLOUDS[name]
    check_cloud(raw_voxel_mean(lr, X, voxel, T), ref_cloud(name))


def test_null_transform_equals_the_identity(lr):
    a, b = raw_voxel_mean(lr, *CLOUDS["T_identity"]), raw_voxel_mean(lr, *CLOUDS["T_none"])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["scan_20000_v0.3", "long_segment", "one_cell_20000", "dropped_many"])
def test_voxel_mean_is_reproducible_whatever_the_scratch_held(lr, name):
    X, voxel, T = CLOUDS[name]
    for poison in (0x00, 0xFF, None, None):
        check_cloud(raw_voxel_mean(lr, X, voxel, T, poison), ref_cloud(name))


def test_nullable_outputs(lr):
    torch, L = lr.torch, lr.ext.lib()
    X, voxel, _ = CLOUDS["scan_1025_v1"]
    x = torch.from_numpy(X).cuda()
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(L.lr_voxel_mean_scratch_bytes(len(X)), dtype=torch.uint8, device="cuda")
    lr.ext.check(L.lr_voxel_mean(x.data_ptr(), len(X), None, voxel, None, None, None, None, info.data_ptr(), scratch.data_ptr(), scratch.numel(), None))
    torch.cuda.synchronize()
    assert tuple(info.cpu().numpy()) == (ref_cloud("scan_1025_v1")["rows"], 0, 0, 0)


def test_two_entry_points_one_table(lr):
    """lr_voxel_dedup and lr_voxel_mean share the cell table (csrc/lr_cells.h) but not the cell rule: floor(p) in one, floor((p - vmb) /
    voxel) in the other.  777 points (3 full blocks and a partial one), coordinates multiples of 2^-8 in [0.5, 40), every axis with
    minimum exactly k + 0.5, voxel 1: vmb = min - 0.5 is an integer, so floor(p - vmb) = floor(p) - vmb exactly and both entry points see
    the same partition into cells.  Then the same with the second half a copy of the first: every cell is hit at least twice."""
    from lidarregistration_amd import voxel
    rng = np.random.default_rng(777)
    lo, hi = np.array([0.5, 3.5, 7.5]), np.array([40.0, 9.0, 10.0])
    X = np.floor((lo + rng.random((777, 3)) * (hi - lo)) * 256.0) / 256.0
    X[5, 0], X[300, 1], X[387, 2] = lo                                    # the minima, all in the first half
    assert (X.min(0) == lo).all() and (X >= 0.5).all() and (X < 40.0).all() and (X * 256.0 == np.floor(X * 256.0)).all()
    twice = np.concatenate([X[:388], X[:388], X[:1]])
    for cloud in (X, twice):
        assert cloud.shape == (777, 3) and (cloud.min(0) == lo).all()
        # the plain definition: cells in order of their first point, points per cell
        _, idx, inv = np.unique(np.floor(cloud).astype(np.int64), axis=0, return_index=True, return_inverse=True)
        order = np.argsort(idx)
        rank = np.empty_like(order); rank[order] = np.arange(len(order))
        want_first, want_counts = idx[order], np.bincount(rank[inv.reshape(-1)], minlength=len(order))
        cells, sel = voxel.sparse_quantize(cloud)
        r = lr.ov.voxel_mean_dev(cloud, 1.0)
        first, counts = r["first"].cpu().numpy(), r["counts"].cpu().numpy()
        assert (r["status"], r["dropped"]) == (0, 0)
        assert np.array_equal(first, sel.cpu().numpy()) and np.array_equal(first, want_first)
        assert r["rows"] == len(sel) == len(want_first)
        assert counts.sum() == 777 and np.array_equal(counts, want_counts)
        assert np.array_equal(cells.cpu().numpy(), np.floor(cloud[want_first]).astype(np.int32))
    assert (counts >= 2).all() and (first < 388).all()                     # (the doubled cloud)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_overlap_equals_the_restatement(lr, name):
    p, ref = PAIRS[name], ref_pair(name)
    r = lr.ov.overlap_dev(p["A"], p["B"], p["T"], p["voxel"], p["radius"])
    assert {k: r[k] for k in KEYS} == ref
    if "expect" in p:
        assert r["n_overlap"] == p["expect"]
    if name in overlap_cases.golden_cases():
        assert r["frac"] == float(GOLD[name + "/frac"]) and r["frac_sym"] == float(GOLD[name + "/frac_sym"])


def test_radius_range(lr):
    """Served: 0.5 and 3 voxel (among the pair cases above) and the ends of the range; refused: outside voxel / 16 .. 4 voxel."""
    p = PAIRS["g_none_257"]
    for radius in (0.0625, 4.0):
        r = lr.ov.overlap_dev(p["A"], p["B"], None, 1.0, radius)
        assert {k: r[k] for k in KEYS} == overlap_cpu.overlap(p["A"], p["B"], None, 1.0, radius)
    for radius in (0.06, 4.01, -1.0, float("nan")):
        with pytest.raises(lr.ext.LidarRegError, match="radius"):
            lr.ov.overlap_dev(p["A"], p["B"], None, 1.0, radius)


def test_statuses_of_a_pair(lr):
    X, voxel, _ = CLOUDS["extent_at"]
    ok = CLOUDS["scan_257_v1"][0]
    for A, B, want in ((X, ok, (2, 0, ref_cloud("scan_257_v1")["rows"])), (ok, X, (2, ref_cloud("scan_257_v1")["rows"], 0)),
                       (CLOUDS["dropped_all"][0], ok, (1, 0, ref_cloud("scan_257_v1")["rows"])), (X, np.zeros((0, 3)), (2, 0, 0))):
        r = lr.ov.overlap_dev(A, B)
        assert (r["status"], r["n0_ds"], r["n1_ds"]) == want and (r["n_overlap"], r["frac"], r["frac_sym"]) == (0, 0.0, 0.0)
        assert {k: r[k] for k in KEYS} == overlap_cpu.overlap(A, B)


def test_batch_equals_the_single_calls(lr):
    pairs = overlap_cases.batch_pairs()
    assert [len(p["A"]) for p in pairs] == [0, 1, 257, 5000, 20000] and any(p["T"] is None for p in pairs) and any(p["T"] is not None for p in pairs)
    want = [ref_pair(f"batch_{k}") for k in range(len(pairs))]
    args = [(p["A"], p["B"], p["T"]) for p in pairs]
    for poison in (None, None, 0x00, 0xFF):
        got = lr.ov.overlap_batch_dev(args, 1.0, 0.0, poison=poison)
        assert [{k: r[k] for k in KEYS} for r in got] == want
    single = [lr.ov.overlap_dev(p["A"], p["B"], p["T"], 1.0, 0.0, poison=0xFF) for p in pairs]
    assert single == got
    rev = lr.ov.overlap_batch_dev(args[::-1], 1.0, 0.0)                # the pair's place in the batch does not matter
    assert rev[::-1] == got


def test_batch_of_64(lr):
    names = [n for n in sorted(overlap_cases.search_cases()) if PAIRS[n]["radius"] == 0.0][:58] + ["g_none_5000", "batch_3"] + ["g_none_257", "g_rot90_1025", "batch_0", "batch_2"]
    assert len(names) == 64 and all(PAIRS[n]["radius"] == 0.0 and PAIRS[n]["voxel"] == 1.0 for n in names)
    got = lr.ov.overlap_batch_dev([(PAIRS[n]["A"], PAIRS[n]["B"], PAIRS[n]["T"]) for n in names])
    assert [{k: r[k] for k in KEYS} for r in got] == [ref_pair(n) for n in names]
    with pytest.raises(lr.ext.LidarRegError, match="npairs"):
        lr.ov.overlap_batch_dev([(PAIRS[names[0]]["A"], PAIRS[names[0]]["B"])] * 65)


def test_refusals_on_the_device(lr):
    """C5's device-side half: short, misaligned and foreign scratch; nothing is launched, a good call still works afterwards."""
    torch, L = lr.torch, lr.ext.lib()
    p = PAIRS["g_none_257"]
    a, b = torch.from_numpy(p["A"]).cuda(), torch.from_numpy(p["B"]).cuda()
    need = L.lr_overlap_scratch_bytes(len(p["A"]), len(p["B"]))
    scratch = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    res = torch.zeros(ctypes.sizeof(lr.ext.OverlapResult), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    prm = lr.ext.OverlapParams()
    err = lambda: L.lr_last_error().decode()

    def call(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_overlap(a.data_ptr(), len(p["A"]), b.data_ptr(), len(p["B"]), None, ctypes.byref(prm), res.data_ptr(), ptr, nbytes, st)
    assert call() == 0
    assert call(nbytes=need - 1) == -1 and "scratch too small" in err()
    assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
    host = np.zeros(need + 256, np.uint8)
    hp = (host.ctypes.data + 255) & ~255
    assert call(ptr=hp) == -1 and "not device memory" in err()
    L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)
    try:
        assert call() == -1 and "device" in err()
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        assert L.lr_voxel_mean(a.data_ptr(), len(p["A"]), None, 1.0, None, None, None, None, info.data_ptr(), scratch.data_ptr(), need, st) == -1 and "device" in err()
    finally:
        L.lr_debug_fake_current_device(-1)
    assert call() == 0
    torch.cuda.synchronize()
    r = lr.ext.OverlapResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert (r.status, r.n_overlap, r.frac) == (0, ref_pair("g_none_257")["n_overlap"], ref_pair("g_none_257")["frac"])


def test_python_mirror_against_the_reference(lr):
    """overlap_fraction / calc_GT_overlap with the reference's call shapes against what the reference's own functions returned."""
    for name, p in overlap_cases.golden_cases().items():
        want = (float(GOLD[name + "/frac"]), float(GOLD[name + "/frac_sym"]))
        if p["T"] is None:
            assert lr.ov.overlap_fraction(p["A"], p["B"]) == want
        else:
            assert lr.ov.calc_GT_overlap(p["A"], p["B"], p["T"], return_both=True) == want
            assert lr.ov.calc_GT_overlap(p["A"], p["B"], p["T"]) == want[1]
            assert lr.ov.calc_GT_overlap(p["A"], p["B"], p["T"], overlap_measure="src_to_tgt") == want[0]
    X, voxel, T = CLOUDS["T_rigid"]
    cent, counts = lr.ov.voxel_down_sample(X, voxel, T, return_counts=True)
    ref = ref_cloud("T_rigid")
    assert cent.dtype == lr.torch.float64 and cent.is_cuda and np.array_equal(bits(cent.cpu().numpy()), bits(ref["cent"]))
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])
    with pytest.raises(lr.ext.LidarRegError):
        lr.ov.voxel_down_sample(*CLOUDS["extent_at"][:2])


def test_refine_motion_on_a_planted_pair(lr):
    """GenerateBalancedSet.py:220-246: icp_mot @ GT_mot_orig.  Equal, bit for bit, to lr_icp run by hand on the same down-sampled float32
    clouds; the ICP part agrees with the independent fp64 ICP of tests/icp_ref.py inside the band tests/test_gpu_icp_ref.py asserts for
    lr_icp (1e-9 on the rotation, 1e-9 + 1e-12 |t| on the translation), and the result lies as close to the planted motion as that
    independent ICP gets, up to the same band."""
    A = overlap_cases.scan(6000, 77)
    a = np.radians(1.0)
    T_true = np.eye(4)
    T_true[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T_true[:3, 3] = [0.2, -0.1, 0.05]
    B = overlap_cpu.transform(A, T_true)
    off = np.eye(4)
    b = np.radians(0.3)
    off[:3, :3] = [[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]]
    off[:3, 3] = [0.1, -0.05, 0.03]
    GT_orig = off @ T_true
    got = lr.ov.refine_motion(GT_orig, A, B, downsample=True, voxel_size=0.3)
    a_corr, bb = lr.ov.refine_inputs(GT_orig, A, B, True, 0.3)
    assert a_corr.dtype == lr.torch.float32 and 3000 < len(a_corr) <= 6000
    ra, rb = overlap_cpu.voxel_mean(A, 0.3), overlap_cpu.voxel_mean(B, 0.3)
    assert np.array_equal(bb.cpu().numpy().view(np.uint32), rb["cent"].astype(np.float32).view(np.uint32))
    assert np.array_equal(a_corr.cpu().numpy().view(np.uint32), overlap_cpu.transform(ra["cent"], GT_orig).astype(np.float32).view(np.uint32))
    T_icp, info = lr.ransac.icp_dev(a_corr, bb, np.eye(4), max_dist=0.6)
    assert np.array_equal(bits(got), bits(T_icp @ GT_orig))
    Tr, ref = icp_ref.icp(a_corr.cpu().numpy(), bb.cpu().numpy(), np.eye(4), max_dist=0.6)
    assert info["n_corr"] == ref["n_corr"] and info["n_corr"] > 0.5 * len(a_corr)
    assert np.abs(T_icp[:3, :3] - Tr[:3, :3]).max() <= 1e-9 and np.abs(T_icp[:3, 3] - Tr[:3, 3]).max() <= 1e-9 + 1e-12 * np.abs(Tr[:3, 3]).max()
    want = Tr @ GT_orig
    err = lambda T: (np.abs(T[:3, :3] - T_true[:3, :3]).max(), np.abs(T[:3, 3] - T_true[:3, 3]).max())
    print("refine_motion: |dR|, |dt| to the planted motion", err(got), "independent ICP", err(want), "before", err(GT_orig))
    assert err(got)[0] <= err(want)[0] + 1e-9 and err(got)[1] <= err(want)[1] + 1e-9 + 1e-12 * 30.0
    assert err(want)[1] < err(GT_orig)[1]                                  # (the independent ICP does move towards the planted motion)
