"""The cloud-level kernels past 65 536 points per cloud -- lr_voxel_mean / lr_overlap / lr_overlap_batch, lr_nn3, lr_refine_z, lr_bbrf,
lr_normals -- against the numpy restatements of their contracts, bit for bit in every output, on the cases of tests/large_cases.py: the
third radix pass and its live third digit, the second round of lr_blocks_before, of nn_init_kernel, of nn_far_kernel and of the step
kernels' sum over more than 64 runs.  The assertions and the plumbing are those of tests/test_gpu_overlap.py, tests/test_gpu_refine_z.py
and tests/test_gpu_bbrf.py; where brute force is out of reach the nearest neighbour of the restatement is nn_tree, proven equal to it in
tests/test_large_cpu.py.  Needs an MI355X."""
import functools
import os

import numpy as np
import pytest

from tests import bbrf_cpu, large_cases, overlap_cpu, refine_z_cases, refine_z_cpu
from tests import test_gpu_bbrf as t_bbrf, test_gpu_overlap as t_overlap, test_gpu_refine_z as t_refine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g20_refine_z_large.npz"))
G = large_cases.GOLDEN_NAME
CLOUDS = large_cases.cloud_cases()
PAIRS = large_cases.pair_cases()
NN = large_cases.nn_cases()
RZ = large_cases.refine_cases()
BB = large_cases.bbrf_cases_large()
POISONS = (0x00, 0xFF, None)
CLOUD_GROUPS = {"own_cell": ("own_cell_6",), "own_cell_nan": ("own_cell_nan",), "one_cell": ("one_cell",), "few_cells": ("few_cells",), "scan": ("scan",)}
bits = t_refine.bits


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, bbrf, overlap
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.ov = overlap; ns.bb = bbrf
    return ns


@functools.lru_cache(maxsize=None)
def ref_cloud(name):
    return overlap_cpu.voxel_mean(*CLOUDS[name])


@functools.lru_cache(maxsize=None)
def ref_pair(name):
    p = PAIRS[name]
    return overlap_cpu.overlap(p["A"], p["B"], p["T"], p["voxel"], p["radius"])


@functools.lru_cache(maxsize=None)
def ref_batch():
    return tuple(overlap_cpu.overlap(p["A"], p["B"], p["T"], p["voxel"], p["radius"]) for p in large_cases.batch_pairs())


@functools.lru_cache(maxsize=None)
def ref_nn(name):
    p = NN[name]
    return (refine_z_cpu.nn_tree if p.get("tree") else refine_z_cpu.nn)(p["A"], p["B"])


@functools.lru_cache(maxsize=None)
def ref_bbrf(name):
    p = BB[name]
    return bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], search=refine_z_cpu.nn_tree, **p["params"])


@pytest.mark.parametrize("group", sorted(CLOUD_GROUPS))
def test_voxel_mean_equals_the_restatement(lr, group):
    """Centroids, float32 centroids, counts, first and info, and nothing written behind the rows; the scratch poisoned both ways and
    left as it is."""
    names = [n for n in sorted(CLOUDS) if n.startswith(CLOUD_GROUPS[group])]
    assert len(names) == (4 if group == "scan" else 1 if group == "few_cells" else 3)
    for name in names:
        X, voxel, T = CLOUDS[name]
        for poison in POISONS:
            t_overlap.check_cloud(t_overlap.raw_voxel_mean(lr, X, voxel, T, poison), ref_cloud(name))


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_overlap_equals_the_restatement(lr, name):
    p, ref = PAIRS[name], ref_pair(name)
    for poison in POISONS:
        r = lr.ov.overlap_dev(p["A"], p["B"], p["T"], p["voxel"], p["radius"], poison=poison)
        assert {k: r[k] for k in t_overlap.KEYS} == ref


def test_batch_sorted_in_three_passes_equals_the_single_calls(lr):
    """passes comes from the call's largest cloud: inside this batch the (257, 257) pair is sorted in three passes, alone in two -- and
    every pair equals its single call and the restatement, whatever the scratch held and wherever the pair stands in the batch."""
    pairs = large_cases.batch_pairs()
    args = [(p["A"], p["B"], p["T"]) for p in pairs]
    want = list(ref_batch())
    single = {poison: [lr.ov.overlap_dev(p["A"], p["B"], p["T"], 1.0, 0.0, poison=poison) for p in pairs] for poison in (0x00, 0xFF)}
    for poison in POISONS:
        got = lr.ov.overlap_batch_dev(args, 1.0, 0.0, poison=poison)
        assert [{k: r[k] for k in t_overlap.KEYS} for r in got] == want
        assert got == single[0x00] == single[0xFF]
    assert lr.ov.overlap_batch_dev(args[::-1], 1.0, 0.0, poison=0xFF)[::-1] == got
    assert lr.ov.overlap_batch_dev(args[3:], 1.0, 0.0) == got[3:]                           # the small pair in a batch of its own: two passes


@pytest.mark.parametrize("name", sorted(NN))
def test_nn_equals_the_restatement(lr, name):
    """idx, the bits of dist and info under the automatic cell, a quarter of it and four times it."""
    p, ref = NN[name], ref_nn(name)
    auto = refine_z_cases.auto_cell(p["B"])
    far = []
    for cell, poison in ((0.0, 0x00), (0.25 * auto, 0xFF), (4.0 * auto, None)):
        far.append(t_refine.check_nn(lr, p["A"], p["B"], ref, cell, poison)["n_far"])
    print(name, "queries resolved by the second phase at cell auto, auto / 4, 4 auto:", far)
    if "middle" in p:                                    # these stay open at the first two cells (tests/test_large_cpu.py: the geometry)
        assert far[0] >= len(p["middle"]) and far[1] >= len(p["middle"])
    if name == "far_rounds":                             # more open queries than nn_far_kernel has waves
        assert len(p["middle"]) >= 8193


@pytest.mark.parametrize("name", sorted(RZ))
def test_refine_z_equals_the_restatement(lr, name):
    """Every field of the result block; more than 64 runs in the step kernel's sum."""
    p, ref = RZ[name], large_cases.refine_trace(name)[0]
    auto = refine_z_cases.auto_cell(p["B"])
    for cell, poison in ((0.0, None), (0.25 * auto, 0x00), (4.0 * auto, 0xFF)):
        r = lr.ov.refine_z_dev(p["A"], p["B"], p["T"], p["gate"], p["max_repeats"], p["min_change"], cell=cell, poison=poison)
        assert t_refine.exact(r) == t_refine.exact(ref), (cell, r, ref)
    for k, v in p.get("expect", {}).items():
        assert r[k] == v


@pytest.mark.parametrize("name", sorted(BB))
def test_bbrf_equals_the_restatement(lr, name):
    """Every log row and every field of the result block over three iterations, at three cells and under poisoned scratch."""
    t_bbrf.check(lr, BB[name], ref=ref_bbrf(name))


def test_normals_equal_the_restatement(lr):
    p = large_cases.normals_case()
    want, winfo = bbrf_cpu.normals(p["X"], p["radius"], p["max_nn"], nbrs=large_cases.ball_neighbours(p["X"], p["radius"], p["max_nn"]))
    for poison in POISONS:
        got, info = lr.bb.normals_dev(p["X"], p["radius"], p["max_nn"], poison=poison)
        assert info == winfo
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert 0 < winfo["n_default"] < len(p["X"]) // 2


def test_golden_case_at_full_size_through_the_device(lr):
    """Against what the reference's own refine_motion_Z_only returned on the 75 199 x 74 958 pair: |dz - dz_ref| <= 40 n 2^-53 Zmax, the
    bound of tests/test_gpu_refine_z.py; equal valid counts; the first repeat's indices equal by their hash."""
    p = large_cases.golden_case()
    bound = 40.0 * len(p["A"]) * 2.0 ** -53 * float(GOLD[G + "/zmax"])
    M, info = lr.ov.refine_motion_Z_only(p["T"], p["A"], p["B"], p["gate"], return_info=True)
    means, nvalid = GOLD[G + "/means"], GOLD[G + "/nvalid"]
    print(f"{G}: |dz - dz_ref| = {abs(info['dz'] - float(GOLD[G + '/dz'])):.3e}, bound {bound:.3e}")
    assert abs(info["dz"] - float(GOLD[G + "/dz"])) <= bound
    assert (info["status"], info["repeats"], info["n_valid"]) == (0, len(means), int(nvalid[-1]))
    assert abs(info["last_step"] - means[-1]) <= bound * len(means) / 10.0
    assert M[2, 3] == p["T"][2, 3] + info["dz"] and np.array_equal(np.delete(M.ravel(), 11), np.delete(np.asarray(p["T"]).ravel(), 11))
    d, ind = lr.ov.nearest_neighbour(refine_z_cpu.transform(p["A"], p["T"]), p["B"])
    assert ind.dtype == np.int64 and large_cases.index_hash(ind) == str(GOLD[G + "/ind0_sha256"])
    for reps in range(1, len(means)):                    # the valid count of every repeat
        r = lr.ov.refine_z_dev(p["A"], p["B"], p["T"], p["gate"], max_repeats=reps)
        assert r["n_valid"] == int(nvalid[reps - 1]) and abs(r["last_step"] - means[reps - 1]) <= bound * reps / 10.0
