"""lr_nn3 / lr_refine_z and their Python mirror (lidarregistration_amd/overlap.py) against the numpy restatement of the contract
(tests/refine_z_cpu.py): idx, dist and every field of the result block bit for bit.  Needs an MI355X."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import overlap_cpu, refine_z_cases, refine_z_cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g18_refine_z.npz"))
GOLDEN = refine_z_cases.golden_cases()
NN = refine_z_cases.nn_cases()
RZ = refine_z_cases.refine_cases()
KEYS = ("status", "repeats", "n_valid", "n0_dropped", "n1_dropped", "reserved", "dz", "last_step")
GROUPS = {"ties": ("ties", "dup", "same"), "edges": ("far", "outside", "one_cell", "single", "line", "plane", "faces", "offset"),
          "nonfinite": ("nonfinite", "all_targets"), "scan": ("scan",)}
GROUPS.update({f"size_n0_{n}": (f"size_{n}_",) for n in refine_z_cases.SIZES})


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, overlap
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.ov = overlap
    return ns


@functools.lru_cache(maxsize=None)
def ref_nn(name):
    return refine_z_cpu.nn(NN[name]["A"], NN[name]["B"])


@functools.lru_cache(maxsize=None)
def ref_rz(name):
    p = RZ[name]
    return refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], p["max_repeats"], p["min_change"])


@functools.lru_cache(maxsize=None)
def ref_scan_20000():
    p = GOLDEN["g_scan_20000"]
    return refine_z_cpu.nn(refine_z_cpu.transform(p["A"], p["T"]), p["B"])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def exact(r):
    """The result block with its doubles as bit patterns."""
    return {k: (float(r[k]).hex() if isinstance(r[k], float) else r[k]) for k in KEYS}


def check_nn(lr, A, B, ref, cell=0.0, poison=None):
    d, ind, info = ref
    r = lr.ov.nearest_neighbour_dev(A, B, cell=cell, poison=poison)
    assert (r["status"], r["n0_dropped"], r["n1_dropped"]) == (info["status"], info["n0_dropped"], info["n1_dropped"])
    assert np.array_equal(r["idx"].cpu().numpy(), ind.astype(np.int32))
    assert np.array_equal(bits(r["dist"].cpu().numpy()), bits(d))
    assert 0 <= r["n_far"] <= len(A)
    return r


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_nn_equals_the_restatement(lr, group):
    """Every case under the automatic cell, a quarter of it and four times it, and under the case's own cell where it names one: the
    same bits each time."""
    names = [n for n in sorted(NN) if n.startswith(GROUPS[group])]
    assert names
    far = 0
    for name in names:
        p = NN[name]
        auto = refine_z_cases.auto_cell(p["B"])
        for cell in dict.fromkeys((p.get("cell", 0.0), 0.0, 0.25 * auto, 4.0 * auto)):
            r = check_nn(lr, p["A"], p["B"], ref_nn(name), cell)
            far += r["n_far"]
        if "expect" in p:
            assert r["idx"].cpu().numpy().tolist() == p["expect"]
    if group == "edges":
        assert far > 0                                  # the second phase did run


def test_nn_at_the_20000_point_pair(lr):
    p = GOLDEN["g_scan_20000"]
    A = refine_z_cpu.transform(p["A"], p["T"])
    auto = refine_z_cases.auto_cell(p["B"])
    shares = []
    for cell, poison in ((0.0, 0x00), (0.25 * auto, 0xFF), (4.0 * auto, None)):
        r = check_nn(lr, A, p["B"], ref_scan_20000(), cell, poison)
        shares.append(r["n_far"] / len(A))
    print("share of queries resolved by the second phase at cell auto, auto / 4, 4 auto:", shares)
    assert np.array_equal(ref_scan_20000()[1], GOLD["g_scan_20000/ind0"])


def test_nn_is_reproducible_whatever_the_scratch_held(lr):
    for name in ("scan_3000", "far_queries", "ties_lattice_cell1.0", "nonfinite"):
        p = NN[name]
        for poison in (0x00, 0xFF, None, None):
            check_nn(lr, p["A"], p["B"], ref_nn(name), p.get("cell", 0.0), poison)


def test_far_queries_go_through_the_second_phase(lr):
    p = NN["far_queries"]
    r = check_nn(lr, p["A"], p["B"], ref_nn("far_queries"))
    assert 70 <= r["n_far"] <= 140                 # (a far query beside the box can be settled by the box term of the bound)
    one = NN["single_point"]
    assert check_nn(lr, one["A"], one["B"], ref_nn("single_point"))["n_far"] == 0          # one cell: the first shell covers the grid


@pytest.mark.parametrize("name", sorted(RZ))
def test_refine_z_equals_the_restatement(lr, name):
    p, ref = RZ[name], ref_rz(name)
    auto = refine_z_cases.auto_cell(np.asarray(p["B"]).reshape(-1, 3)) if len(p["B"]) else 1.0
    for cell, poison in ((0.0, None), (0.25 * auto, 0x00), (4.0 * auto, 0xFF)):
        r = lr.ov.refine_z_dev(p["A"], p["B"], p["T"], p["gate"], p["max_repeats"], p["min_change"], cell=cell, poison=poison)
        assert exact(r) == exact(ref), (cell, r, ref)
    for k, v in p.get("expect", {}).items():
        assert r[k] == v


def test_loop_behaviour(lr):
    r = lambda name: lr.ov.refine_z_dev(RZ[name]["A"], RZ[name]["B"], RZ[name]["T"], RZ[name]["gate"], RZ[name]["max_repeats"], RZ[name]["min_change"])
    lifted = r("lifted_1025")
    assert (lifted["status"], lifted["repeats"], lifted["dz"], lifted["last_step"]) == (2, 2, -0.25, 0.0)
    assert (r("lifted_1e-7")["repeats"], r("no_valid_pair")["status"], r("coincide_most")["status"], r("coincide_few")["status"]) == (1, 1, 2, 0)
    assert [r(f"scan_3000_reps{k}")["repeats"] for k in (1, 2, 10)] == [1, 2, 10]
    a, b = r("T_identity"), r("T_null")
    assert a == b and a["repeats"] == 10
    full = r("scan_3000_reps10")
    assert abs(full["dz"] + 0.38) < 1e-3                                   # the 0.37 m error of the raw motion is found


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases_through_the_device(lr, name):
    """Against what the reference's own refine_motion_Z_only returned: |dz - dz_ref| <= 40 n 2^-53 Zmax (summation order only)."""
    p = GOLDEN[name]
    bound = 40.0 * len(p["A"]) * 2.0 ** -53 * float(GOLD[name + "/zmax"])
    M, info = lr.ov.refine_motion_Z_only(p["T"], p["A"], p["B"], p["gate"], return_info=True)
    means, nvalid = GOLD[name + "/means"], GOLD[name + "/nvalid"]
    print(f"{name}: |dz - dz_ref| = {abs(info['dz'] - float(GOLD[name + '/dz'])):.3e}, bound {bound:.3e}")
    assert abs(info["dz"] - float(GOLD[name + "/dz"])) <= bound
    assert (info["status"], info["repeats"], info["n_valid"]) == (0, len(means), int(nvalid[-1]))
    assert abs(info["last_step"] - means[-1]) <= bound * len(means) / 10.0
    assert M[2, 3] == p["T"][2, 3] + info["dz"] and np.array_equal(np.delete(M.ravel(), 11), np.delete(np.asarray(p["T"]).ravel(), 11))
    d, ind = lr.ov.nearest_neighbour(refine_z_cpu.transform(p["A"], p["T"]), p["B"])
    assert ind.dtype == np.int64 and d.dtype == np.float64 and np.array_equal(ind, GOLD[name + "/ind0"])
    first = lr.ov.refine_z_dev(p["A"], p["B"], p["T"], p["gate"], max_repeats=1)
    assert first["n_valid"] == int(nvalid[0]) and abs(first["last_step"] - means[0]) <= bound / 10.0


def test_refusals_on_the_device(lr):
    """The device-side half of the refusals: short, misaligned and foreign scratch, a stream of another device; nothing is launched, a
    good call still works afterwards."""
    torch, L = lr.torch, lr.ext.lib()
    p = NN["size_257_257"]
    a, b = torch.from_numpy(p["A"]).cuda(), torch.from_numpy(p["B"]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()
    idx = torch.zeros(257, dtype=torch.int32, device="cuda"); dist = torch.zeros(257, dtype=torch.float64, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = torch.zeros(ctypes.sizeof(lr.ext.RefineZResult), dtype=torch.uint8, device="cuda")
    need = max(L.lr_nn3_scratch_bytes(257, 257), L.lr_refine_z_scratch_bytes(257, 257))
    scratch = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    pn, pz = lr.ext.Nn3Params(), lr.ext.RefineZParams()

    def nn3(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_nn3(a.data_ptr(), 257, b.data_ptr(), 257, ctypes.byref(pn), idx.data_ptr(), dist.data_ptr(), info.data_ptr(), ptr, nbytes, st)

    def rz(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_refine_z(a.data_ptr(), 257, b.data_ptr(), 257, None, ctypes.byref(pz), res.data_ptr(), ptr, nbytes, st)
    host = np.zeros(need + 256, np.uint8)
    hp = (host.ctypes.data + 255) & ~255
    for call, fn in ((nn3, L.lr_nn3_scratch_bytes), (rz, L.lr_refine_z_scratch_bytes)):
        assert call() == 0
        assert call(nbytes=fn(257, 257) - 1) == -1 and "scratch too small" in err()
        assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
        assert call(ptr=hp) == -1 and "not device memory" in err()
        L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)
        try:
            assert call() == -1 and "device" in err()
        finally:
            L.lr_debug_fake_current_device(-1)
        assert call() == 0
    torch.cuda.synchronize()
    d, ind, _ = ref_nn("size_257_257")
    assert np.array_equal(idx.cpu().numpy(), ind.astype(np.int32)) and np.array_equal(bits(dist.cpu().numpy()), bits(d))
    r = lr.ext.RefineZResult.from_buffer_copy(res.cpu().numpy().tobytes())
    want = refine_z_cpu.refine_z(p["A"], p["B"])
    assert (r.status, r.repeats, r.n_valid, r.dz) == (want["status"], want["repeats"], want["n_valid"], want["dz"])


def test_python_mirror(lr):
    a, b, raw = refine_z_cases.scan_pair(3000)
    d, ind = lr.ov.nearest_neighbour(refine_z_cpu.transform(a, raw), b)
    rd, rind, _ = ref_nn("scan_3000")
    assert np.array_equal(ind, rind) and np.array_equal(bits(d), bits(rd))
    # refine_motion_Z_only returns a new matrix and leaves its argument alone
    keep = raw.copy()
    M = lr.ov.refine_motion_Z_only(raw, a, b, 0.3)
    want = ref_rz("scan_3000_reps10")
    assert np.array_equal(bits(raw), bits(keep)) and M is not raw and M.dtype == np.float64 and M.shape == (4, 4)
    assert M[2, 3] == raw[2, 3] + want["dz"] and np.array_equal(np.delete(M.ravel(), 11), np.delete(raw.ravel(), 11))
    # refine_GT: the Z-only branch works on the float64 centroids of both clouds, the other one is refine_motion
    from lidarregistration_amd import synth
    A, B, T = synth.make_scan_pair(3000, 3000)
    G = lr.ov.refine_GT(raw, A, B, downsample=True, voxel_size=0.3, z_only=True)
    assert np.array_equal(bits(G), bits(M))
    assert np.array_equal(bits(lr.ov.refine_GT(raw, a, b, downsample=False, voxel_size=0.3, z_only=True)), bits(M))
    icp = lr.ov.refine_GT(raw, A, B, downsample=True, voxel_size=0.3, z_only=False)
    assert np.array_equal(bits(icp), bits(lr.ov.refine_motion(raw, A, B, True, 0.3)))
    a32, _ = lr.ov.refine_inputs(raw, A, B, True, 0.3)
    assert a32.dtype == lr.torch.float32                                   # (what refine_inputs returns has not changed)
    # refine_session on three frames: every frame down-sampled once, positions chained as mot @ previous
    A2, B2, T2 = synth.make_scan_pair(3000, 3000, seed=52)
    clouds, raws = [A, B, B2], [raw, T2]
    ds = [overlap_cpu.voxel_mean(c, 0.3)["cent"] for c in clouds]
    for z_only in (True, False):
        pos = lr.ov.refine_session(clouds, raws, voxel_size=0.3, z_only=z_only)
        assert len(pos) == 3 and np.array_equal(pos[0], np.eye(4))
        m01 = lr.ov.refine_GT(raws[0], ds[0], ds[1], downsample=False, voxel_size=0.3, z_only=z_only)
        m12 = lr.ov.refine_GT(raws[1], ds[1], ds[2], downsample=False, voxel_size=0.3, z_only=z_only)
        assert np.array_equal(bits(pos[1]), bits(m01 @ np.eye(4))) and np.array_equal(bits(pos[2]), bits(m12 @ pos[1]))
    with pytest.raises(NotImplementedError, match="refine_GT"):
        lr.ov.refine_motion(raw, a, b, refine_GT_Z_only=True)


def test_calls_can_be_captured_into_a_graph(lr):
    """No host synchronisation, no allocation, the loop never driven from the host: lr_nn3 and lr_refine_z recorded once on a side stream
    and replayed on other contents of the same buffers give what the eager calls give, bit for bit."""
    torch, L = lr.torch, lr.ext.lib()
    a, b, raw = refine_z_cases.scan_pair(3000)
    inputs = [refine_z_cpu.transform(a, raw), refine_z_cpu.transform(a, raw) + np.array([0.0, 0.0, 0.125]), b[: len(a)] + np.array([0.0, 0.0, 0.25])]
    n0, n1 = len(a), len(b)
    A = torch.empty((n0, 3), dtype=torch.float64, device="cuda"); B = torch.from_numpy(b).cuda()
    idx = torch.empty(n0, dtype=torch.int32, device="cuda"); dist = torch.empty(n0, dtype=torch.float64, device="cuda")
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    res = torch.zeros(ctypes.sizeof(lr.ext.RefineZResult), dtype=torch.uint8, device="cuda")
    s1 = torch.empty(L.lr_nn3_scratch_bytes(n0, n1), dtype=torch.uint8, device="cuda")
    s2 = torch.empty(L.lr_refine_z_scratch_bytes(n0, n1), dtype=torch.uint8, device="cuda")
    pn, pz = lr.ext.Nn3Params(), lr.ext.RefineZParams()
    s = torch.cuda.Stream()

    def call():
        lr.ext.check(L.lr_nn3(A.data_ptr(), n0, B.data_ptr(), n1, ctypes.byref(pn), idx.data_ptr(), dist.data_ptr(), info.data_ptr(), s1.data_ptr(), s1.numel(), s.cuda_stream))
        lr.ext.check(L.lr_refine_z(A.data_ptr(), n0, B.data_ptr(), n1, None, ctypes.byref(pz), res.data_ptr(), s2.data_ptr(), s2.numel(), s.cuda_stream))

    def outputs():
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (idx, dist, info, res)]

    def load(x):
        A.copy_(torch.from_numpy(np.ascontiguousarray(x))); torch.cuda.synchronize()
    eager = []
    for x in inputs:
        load(x); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for x, want in list(zip(inputs, eager))[::-1]:
        load(x); s1.fill_(0xFF); s2.fill_(0x00); g.replay()
        assert outputs() == want
    reps = [lr.ext.RefineZResult.from_buffer_copy(e[3]).repeats for e in eager]
    assert reps[0] == 10 and len(set(e[3] for e in eager)) == 3              # the replays took different numbers of live repeats / steps
    want = refine_z_cpu.refine_z(inputs[1], b)
    r = lr.ext.RefineZResult.from_buffer_copy(eager[1][3])
    assert (r.status, r.repeats, r.n_valid, r.dz) == (want["status"], want["repeats"], want["n_valid"], want["dz"])
