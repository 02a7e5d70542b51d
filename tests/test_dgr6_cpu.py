"""The yardsticks of the 6-D inlier network, without a GPU: the conventions of tests/dgr6_cpu.py (levels, the 729-offset maps, offset order,
stage order, epilogues) against the pinned 3-D restatement tests/fcgf_cpu.py on clouds that are flat in three of the six axes and against
a brute-force loop over the 729 offsets on a dense array; the arithmetic modes against each other; the decomposition of a cloud of far
motifs; the state-dict packing and its refusals; the size functions and the host-side refusals of the C ABI."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, dgr
from tests import dgr6_cases, dgr6_cpu, fcgf_cases, fcgf_cpu

THIN = dgr6_cpu.THIN
MIXED = (32, 64, 96, 128, 64, 32, 64, 32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the conventions, against the pinned 3-D restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("flat_first", [False, True], ids=["last_three_constant", "first_three_constant"])
@pytest.mark.parametrize("widths", [THIN, MIXED], ids=["thin", "mixed"])
def test_restatement_fp64_equals_the_3d_restatement_on_flat_clouds(flat_first, widths):
    """On a cloud that is constant in three axes only the offsets that are 0 there meet a cell, and the network is the 3-D one whose
    kernels are those slices: idx = idx3(o) + 351 (last three constant: 351 = 27 + 81 + 243) or 13 + 27 idx3(o) (first three: 13 = 1 + 3 + 9).
    The constants are multiples of 8: a constant off the lattice would meet its coarse cell at o = +1 in F3 / F4 and leave the slices.
    Both sides fp64, the tolerance of test_restatement_fp64_equals_dense_torch_convolutions: 1e-11 of the stage's largest magnitude."""
    c3 = fcgf_cases.random_cells(300, 16, 6)                                  # cells -8 .. 7: negative floor division included
    const = np.tile(np.array([8, -16, 0], np.int32), (len(c3), 1))
    c6 = np.concatenate([const, c3] if flat_first else [c3, const], 1)
    stages = dgr6_cpu.random_stages(widths, seed=3)
    sl = 13 + 27 * np.arange(27) if flat_first else np.arange(27) + 351
    stages3 = [(W[sl] if W.shape[0] == 729 else W, sc, of) for W, sc, of in stages]
    got = dgr6_cpu.run(c6, stages, mode="f64")
    want = fcgf_cpu.run(c3, stages3, 3, mode="f64")
    for lvl in range(4):
        keep = slice(3, 6) if flat_first else slice(0, 3)
        assert np.array_equal(got["levels"][lvl][:, keep], want["levels"][lvl])
    for s in range(1, 24):
        d = np.abs(got["acts"][s] - want["acts"][s]).max() / np.abs(want["acts"][s]).max()
        assert got["acts"][s].shape == want["acts"][s].shape and d <= 1e-11, (s, d)
    assert np.array_equal(got["logit"], got["acts"][23][:, 0])


# ---- 2. brute force on a dense array ---------------------------------------------------------------------------------------------------
def test_restatement_fp64_equals_a_dense_loop_over_the_729_offsets_on_the_full_box():
    """The full box {-2..1}^6 (4 096 cells, level 1 = {-2, 0}^6), stages 1 - 4: out[u] = sum_o in[u + o] W[idx(o)] written as 729 shifted
    slices of a zero-padded dense array, the offset order spelt out here (axis 0 fastest) and not taken from dgr6_cpu."""
    coords = dgr6_cases.box(4, (-2,) * 6)
    stages = dgr6_cpu.random_stages(THIN, seed=4)
    got = dgr6_cpu.run(coords, stages, mode="f64", upto=4)["acts"]
    offs = [o[::-1] for o in itertools.product((-1, 0, 1), repeat=6)]          # product's last factor is fastest: reversed, axis 0 is

    def dense(x, s, stride):
        W, sc, of = stages[s - 1]
        xp = np.pad(x, [(1, 1)] * 6 + [(0, 0)])
        acc = 0.0
        for k, o in enumerate(offs):
            sl = tuple(slice(1 + oa, 1 + oa + 4, stride) for oa in o)          # u + o for u = 0 .. 3 (stride 2: the even cells, v = -2, 0)
            acc = acc + xp[sl] @ W[k].astype(np.float64)
        return acc * sc.astype(np.float64) + of.astype(np.float64)

    x1 = dense(np.ones((4,) * 6 + (1,)), 1, 1)
    t = np.maximum(dense(x1, 2, 1), 0)
    x3 = np.maximum(dense(t, 3, 1) + x1, 0)
    x4 = dense(x3, 4, 2)
    for s, want in ((1, x1), (2, t), (3, x3), (4, x4)):
        want = want.reshape(-1, want.shape[-1])                                # C order = lexicographic, axis 0 slowest: the rows of box() and of level 1
        d = np.abs(got[s] - want).max() / np.abs(want).max()
        assert got[s].shape == want.shape and d <= 1e-11, (s, d)


# ---- 3. arithmetic modes ----------------------------------------------------------------------------------------------------------------
def test_chain_and_fp64_agree_to_fp32_rounding_and_lockstep_equals_offset_major():
    """100 rows of a 3^6 block.  A chain of N terms of magnitude m errs by at most N 2^-24 m, typically sqrt(N) 2^-24 m; the longest chain is
    729 x 64 terms and there are 23 stages: 1e-4 of the largest magnitude is two decades above the typical error and far below a wrong
    term, which shows at order 1."""
    coords = dgr6_cases.random_cells(100, 3, 8, lo=(-1, 0, 7, -9, 3, 4))
    stages = dgr6_cpu.random_stages(THIN, seed=5)
    ch = dgr6_cpu.run(coords, stages, mode="chain")
    r64 = dgr6_cpu.run(coords, stages, mode="f64")
    mm = dgr6_cpu.run(coords, stages, mode="f32mm")
    for s in range(1, 24):
        m = np.abs(r64["acts"][s]).max()
        assert np.abs(ch["acts"][s] - r64["acts"][s]).max() <= 1e-4 * m and np.abs(mm["acts"][s] - r64["acts"][s]).max() <= 1e-4 * m, s
    assert ch["logit"].dtype == np.float32 and (bits(ch["logit"]) != bits(mm["logit"])).any()       # the order of summation matters in the last bits
    org = dgr6_cpu.origin(coords)
    maps = dgr6_cpu.kernel_map(coords.astype(np.int64), coords, 1, org)
    x = np.random.default_rng(1).standard_normal((100, 32)).astype(np.float32)
    W = stages[1][0]
    assert len(maps) > 300
    assert np.array_equal(bits(dgr6_cpu._conv(x, maps, W, 100, "chain")), bits(fcgf_cpu._conv(x, maps, W, 100, "chain")))


# ---- 4. levels, keys, statuses ------------------------------------------------------------------------------------------------------
def test_levels_are_lexicographic_axis0_first_and_independent_of_the_row_order():
    c = np.array([[-1, 0, 5, 0, 0, 0], [3, -3, 0, 0, 0, 9], [-1, 1, 4, 0, 0, 0], [2, -4, 1, 7, 0, 0], [3, -3, 0, 0, 0, 1]])
    L = dgr6_cpu.levels(c)
    assert L[1].tolist() == [[-2, 0, 4, 0, 0, 0], [2, -4, 0, 0, 0, 0], [2, -4, 0, 0, 0, 8], [2, -4, 0, 6, 0, 0]]
    assert L[3].tolist() == [[-8, 0, 0, 0, 0, 0], [0, -8, 0, 0, 0, 0], [0, -8, 0, 0, 0, 8]]
    cells = dgr6_cases.clusters(129, 1)
    perm = np.random.default_rng(0).permutation(len(cells))
    for a, b in zip(dgr6_cpu.levels(cells)[1:], dgr6_cpu.levels(cells[perm])[1:]):
        assert np.array_equal(a, b)
        keys = dgr6_cpu.pack_keys(a, dgr6_cpu.origin(cells))
        assert (np.diff(keys) > 0).all()                                       # ascending packed keys = ascending lexicographic cells
    assert dgr6_cpu.origin([[-1, 8, 15, 16, -8, -9]]).tolist() == [-8, 8, 8, 16, -8, -16]
    assert [dgr6_cpu.index_of(o) for o in ([-1] * 6, [0] * 6, [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], [1] * 6)] == [0, 364, 365, 607, 728]
    assert np.array_equal(dgr6_cpu.OFFSETS, dgr6_cases.motif_offsets())
    assert np.array_equal(dgr.offset_index(dgr6_cpu.OFFSETS), np.arange(729))


def test_statuses_of_the_restatement():
    base = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]])
    assert dgr6_cpu.status_of(base) == 0 and dgr6_cpu.status_of(np.zeros((0, 6))) == 0
    assert dgr6_cpu.status_of(np.concatenate([base, base[:1]])) == 2
    for a in range(6):
        far = base.copy(); far[1, a] = 1007
        assert dgr6_cpu.status_of(far) == 0                                    # the last admitted extent: 1 008 cells from a minimum on the lattice
        far[1, a] = 1008
        assert dgr6_cpu.status_of(far) == 3 and dgr6_cpu.status_of(np.concatenate([far, far[:1]])) == 3
        low = base.copy(); low[0, a] = -1; low[1, a] = 1000                    # a minimum off the lattice: origin -8, 1 002 cells are one too many
        assert dgr6_cpu.status_of(low) == 3
        low[1, a] = 999                                                        # an extent of 1 001 cells is admitted wherever it lies
        assert dgr6_cpu.status_of(low) == 0


# ---- 5. the decomposition of far motifs -------------------------------------------------------------------------------------------------
def test_a_cloud_of_far_motifs_is_its_motifs_alone_bit_for_bit():
    """DESIGN.md §18.3's argument in six dimensions, in the restatement itself: motifs on a lattice of pitch 64 share no map entry at any
    level, so a composite's rows are the motifs' rows computed alone (F10: the shift to the motif's site changes no bit) and a level's
    rows are the motifs' rows in ascending key order.  8 of the 729 two-cell motifs, every stage."""
    which = [0, 1, 121, 364, 365, 500, 607, 728]
    cloud = dgr6_cases.motifs(which)
    stages = dgr6_cpu.random_stages(THIN, seed=6)
    whole = dgr6_cpu.run(cloud, stages, mode="chain")
    parts = [dgr6_cpu.run(dgr6_cases.motifs([k]), stages, mode="chain") for k in which]
    assert np.array_equal(bits(whole["logit"]), bits(np.concatenate([p["logit"] for p in parts])))
    for s in range(1, 24):
        lvl = whole["level_of"][s]
        cells = np.concatenate([p["levels"][lvl] for p in parts])
        acts = np.concatenate([p["acts"][s] for p in parts])
        order = np.arange(len(cells)) if lvl == 0 else np.lexsort(cells.T[::-1])
        assert np.array_equal(cells[order], whole["levels"][lvl]) and np.array_equal(bits(acts[order]), bits(whole["acts"][s])), s
    # what the motifs are for: at level 0 -> 1 coarse cell v receives offset o from v + o, and v + o receives offset o from coarse v
    o, v = dgr6_cases.motif_offsets(), dgr6_cases.motif_sites()
    full = dgr6_cases.motifs().astype(np.int64)
    L = dgr6_cpu.levels(full); org = dgr6_cpu.origin(full)
    site = {tuple(c): r for r, c in enumerate(L[1])}
    dn = {(k, int(a), int(b)) for k, ro, ri in dgr6_cpu.kernel_map(L[1], L[0], 1, org) for a, b in zip(ro, ri)}
    up = {(k, int(a), int(b)) for k, ro, ri in dgr6_cpu.kernel_map(L[0], L[1], -1, org) for a, b in zip(ro, ri)}
    for k in range(729):
        if k != 364:
            assert (k, site[tuple(v[k])], 2 * k + 1) in dn and (k, 2 * k + 1, site[tuple(v[k])]) in up, k
    assert {k for k, _, _ in dn} == set(range(729)) == {k for k, _, _ in up}
    assert len(full) == 1458 and dgr6_cpu.status_of(full) == 0


# ---- 6. the packer -------------------------------------------------------------------------------------------------------------------
def test_fold_reads_the_widths_and_pack_is_the_blob_layout():
    sd = dgr6_cases.make_state_dict(MIXED, seed=2)
    assert dgr.widths_of(sd) == MIXED
    stages = dgr.inlier_fold(sd)
    assert [(W.shape, s.shape, o.shape) for W, s, o in stages] == [((k, ci, co), (co,), (co,)) for k, ci, co in dgr6_cpu.stage_shapes(MIXED)]
    assert dgr6_cpu.widths_of(stages) == MIXED == dgr.widths_of_stages(stages)
    blob = dgr.inlier_pack(stages)
    assert blob.dtype == np.float32 and blob.size == dgr.inlier_packed_floats(MIXED)
    assert np.array_equal(blob[:729 * 32], stages[0][0].reshape(-1)) and blob[-1] == stages[22][2][0] == np.float32(sd["final.bias"][0, 0])
    assert blob[-2] == 1.0 and (stages[21][1] == 1).all() and not stages[21][2].any()               # no BatchNorm: scale 1, offset 0 / bias
    g, b, mu, var = (sd[f"norm2.bn.{f}"].astype(np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
    sc = g / np.sqrt(var + 1e-5)
    assert np.array_equal(stages[3][1], sc.astype(np.float32)) and np.array_equal(stages[3][2], ((0 - mu) * sc + b).astype(np.float32))
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}                                  # tensors as torch.load gives them
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(stages, dgr.inlier_fold(t)))


def test_the_packer_refuses_by_key():
    sd = dgr6_cases.make_state_dict(THIN, seed=1)

    def refused(change, text):
        bad = dict(sd); change(bad)
        with pytest.raises(ValueError, match=text):
            dgr.inlier_fold(bad)

    refused(lambda d: d.pop("block3.conv2.kernel"), "missing key 'block3.conv2.kernel'")
    refused(lambda d: d.pop("norm4_tr.bn.running_var"), "missing key 'norm4_tr.bn.running_var'")
    refused(lambda d: d.pop("final.bias"), "missing key 'final.bias'")
    refused(lambda d: d.update({"block1_tr.conv1.kernel": d["conv2.kernel"]}), "unexpected key 'block1_tr.conv1.kernel'")
    refused(lambda d: d.update({"conv3.kernel": d["conv3.kernel"][:27]}), "conv3.kernel has shape")
    refused(lambda d: d.update({"norm2.bn.weight": d["norm2.bn.weight"][:5]}), "norm2.bn.weight has shape")
    refused(lambda d: d.update({"final.bias": np.zeros((1, 2), np.float32)}), "final.bias has shape")

    def poison(key, v):
        def f(d):
            a = np.array(d[key]); a.reshape(-1)[3] = v; d[key] = a
        return f
    refused(poison("block2.conv1.kernel", np.nan), "block2.conv1.kernel holds a non-finite")
    refused(poison("norm3.bn.bias", np.inf), "norm3.bn.bias holds a non-finite")
    refused(poison("norm3.bn.running_var", -1.0), "norm3.bn.running_var does not fold")
    # I1: K = 3 and one input feature, read from conv1.kernel; I5: the widths
    refused(lambda d: d.update({"conv1.kernel": np.zeros((15625, 1, 32), np.float32)}), r"conv1.kernel has shape \(15625, 1, 32\), expected \[729, 1, C\]")
    refused(lambda d: d.update({"conv1.kernel": np.zeros((729, 6, 32), np.float32)}), "conv1.kernel has shape")
    refused(lambda d: d.update({"conv2.kernel": np.zeros((729, 32, 48), np.float32)}), "conv2.kernel: width 48")
    refused(lambda d: d.update({"conv4.kernel": np.zeros((729, 32, 288), np.float32)}), "conv4.kernel: width 288")
    with pytest.raises(ValueError, match="conv1_tr.kernel: width 16"):
        dgr.inlier_stage_plan((32,) * 7 + (16,))


def test_a_checkpoint_with_another_inlier_feature_or_model_is_refused_by_name(tmp_path):
    sd = dgr6_cases.make_state_dict(THIN, seed=1)
    for cfg, text in ((dict(inlier_model="ResUNetBN2C", inlier_feature_type="feats"), "inlier_feature_type 'feats'"),
                      (dict(inlier_model="ResUNetBN2C", inlier_feature_type="coords"), "inlier_feature_type 'coords'"),
                      (dict(inlier_model="ResUNetBN2D", inlier_feature_type="ones"), "inlier_model 'ResUNetBN2D'")):
        path = tmp_path / "ck.pth"
        torch.save({"state_dict_inlier": sd, "config": cfg}, path)
        with pytest.raises(ValueError, match=text):
            dgr.InlierNet.from_checkpoint(path)
    torch.save({"state_dict": sd}, tmp_path / "ck.pth")
    with pytest.raises(ValueError, match="state_dict_inlier"):
        dgr.InlierNet.from_checkpoint(tmp_path / "ck.pth")


# ---- 7. sizes and host-side refusals of the C ABI ---------------------------------------------------------------------------------------
def _w8(widths):
    return ctypes.byref((ctypes.c_int32 * 8)(*widths))


def test_weights_and_scratch_sizes():
    L = _ext.lib()
    for widths in (dgr6_cpu.WIDTHS, THIN, MIXED):
        floats = sum(k * ci * co + 2 * co for k, ci, co in dgr6_cpu.stage_shapes(widths))
        assert L.lr_dgr_inlier_weights_bytes(_w8(widths)) == 4 * floats == 4 * dgr.inlier_packed_floats(widths)
        # per row (of max_n rounded up to 64): four tables of 4 slots (12 bytes each), four levels of row keys, the sort buffer, ten gather
        # tables of 729 entries, three activation buffers of the largest width, the three skips
        per_row = 4 * 4 * 12 + 4 * 8 + 2 * 8 + 10 * 729 * 4 + 3 * max(widths) * 4 + (widths[0] + widths[1] + widths[2]) * 4
        base = L.lr_dgr_inlier_scratch_bytes(0, _w8(widths))
        assert base == 256 + 4 * 1024 * 12 + 2048 * 8
        for n in (1, 64, 65, 4000, 131072):
            assert L.lr_dgr_inlier_scratch_bytes(n, _w8(widths)) == base + per_row * ((n + 63) // 64 * 64), (widths, n)
    assert L.lr_dgr_inlier_weights_bytes(_w8(dgr6_cpu.WIDTHS)) == 4 * 235926818                    # "about 236 M weights"
    assert 10 * 729 * 4 * 131072 == 3822059520 < L.lr_dgr_inlier_scratch_bytes(131072, _w8(dgr6_cpu.WIDTHS)) < 4.5e9
    for bad in ((16,) + THIN[1:], THIN[:7] + (288,), THIN[:3] + (48,) + THIN[4:], (0,) * 8):
        assert L.lr_dgr_inlier_weights_bytes(_w8(bad)) == 0 and L.lr_dgr_inlier_scratch_bytes(10, _w8(bad)) == 0
    assert L.lr_dgr_inlier_weights_bytes(None) == 0
    assert L.lr_dgr_inlier_scratch_bytes(131073, _w8(THIN)) == 0 and L.lr_dgr_inlier_scratch_bytes(-1, _w8(THIN)) == 0


def test_the_size_functions_keep_their_values():
    """Literal values, read from the library of the commit before the maps, the convolution and the layout moved into csrc/lr_sparse.h
    (built from that commit with the Makefile's flags): the layout function is shared now and must size every call as before."""
    L = _ext.lib()
    ns = (0, 1, 64, 65, 131072)
    assert [L.lr_dgr_inlier_scratch_bytes(n, _w8(dgr6_cpu.WIDTHS)) for n in ns] == [65792, 2201344, 2201344, 4336896, 4373676288]
    assert [L.lr_dgr_inlier_scratch_bytes(n, _w8(THIN)) for n in ns] == [65792, 1996544, 1996544, 3927296, 3954245888]
    assert [L.lr_dgr_inlier_weights_bytes(_w8(w)) for w in (dgr6_cpu.WIDTHS, THIN)] == [943707272, 65798920]


def test_refusals_before_any_launch():
    """n above the limit, null pointers, struct_size, widths, tap: LR_EINVAL naming the argument; none of these calls reaches a device."""
    L = _ext.lib()
    err = lambda: L.lr_last_error().decode()
    p = _ext.DgrInlierParams(widths=THIN)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) & ~15 | 16                                       # a 16-byte aligned non-null address; never read
    wb = L.lr_dgr_inlier_weights_bytes(_w8(THIN))

    def call(coords=a, n=4, w=a, wbytes=wb, params=p, res=a, out=a, scratch=a, sbytes=1 << 40):
        return L.lr_dgr_inlier(coords, n, w, wbytes, ctypes.byref(params) if params is not None else None, res, out, None, scratch, sbytes, None)

    assert call(n=131073) == -1 and "n must lie in 0 .. 131072" in err()
    assert call(n=-1) == -1 and "n must lie" in err()
    assert call(coords=None) == -1 and "null coords or logit_out" in err()
    assert call(out=None) == -1 and "null coords or logit_out" in err()
    assert call(res=None) == -1 and "null result" in err()
    assert call(w=None) == -1 and "null weights" in err()
    assert call(w=a + 4) == -1 and "16-byte" in err()
    assert call(wbytes=wb - 4) == -1 and "weights_bytes" in err()
    assert call(scratch=None) == -1 and "null scratch" in err()
    assert call(sbytes=1024) == -1 and "scratch too small" in err()
    assert call(params=None) == -1 and "null params" in err()
    q = _ext.DgrInlierParams(widths=THIN); q.struct_size = 36
    assert call(params=q) == -1 and "struct_size" in err()
    assert call(params=_ext.DgrInlierParams(widths=THIN, tap=24)) == -1 and "tap" in err()
    assert call(params=_ext.DgrInlierParams(widths=THIN[:7] + (40,))) == -1 and "width" in err()
    assert _ext.DgrInlierParams().widths[:] == list(dgr6_cpu.WIDTHS) and L.lr_version() == 103
