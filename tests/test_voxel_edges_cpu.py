"""The voxel-hash builders of tests/voxel_edges.py do what they claim under the restated hash, and oracle.sparse_quantize is held to the
plain definition (a Python dict over tuples) on all of them.  No GPU."""
import numpy as np
import pytest

from tests import voxel_edges as ve


def _held(oracle, coords):
    cells, sel = ve.dedup_ref(coords)
    oc, osel = oracle.sparse_quantize(coords, return_index=True)
    assert np.array_equal(osel, sel) and np.array_equal(oc, cells)
    return cells, sel


def test_hash_restatement_inverts():
    rng = np.random.default_rng(1)
    for _ in range(200):
        c = tuple(int(v) for v in rng.integers(-ve.BIAS + 1, ve.BIAS, 3))
        k = ve.key_of(c)
        assert ve.cell_of(k) == c and k < (1 << 63)
        h = int(rng.integers(0, 1 << 62))
        u = ve._unmix(h)
        x = u ^ (u >> 33); x = (x * ve.C1) & ve.M64; x ^= x >> 33; x = (x * ve.C2) & ve.M64; x ^= x >> 33
        assert x == h
    assert ve.capacity(15000) == 32768 and ve.capacity(1) == 1024 and ve.capacity(512) == 1024 and ve.capacity(513) == 2048


def test_probe_chain_cloud_builds_one_long_merged_chain(oracle):
    p = ve.probe_chain_cloud()
    coords = p["coords"]
    assert len(coords) == 15000 and ve.capacity(len(coords)) == p["cap"]
    cells = [tuple(int(v) for v in np.floor(r)) for r in coords]
    steps = ve.probe_lengths(cells, p["cap"])
    # 1 500 keys on one slot probe 0, 1, ..., 1 499 slots; the second group starts inside the first chain and runs past its end
    assert max(steps) >= 2400 and sum(s >= 700 for s in steps) >= 1700, (max(steps), sum(s >= 700 for s in steps))
    # an ordinary cloud of this size never comes close
    rng = np.random.default_rng(2)
    plain = [tuple(int(v) for v in r) for r in np.floor(rng.normal(0, 100, (15000, 3)))]
    assert max(ve.probe_lengths(plain, p["cap"])) < 50
    c, sel = _held(oracle, coords)
    assert len(sel) >= 2500 and sel.max() < 12500           # every repeat at the end is dropped


def test_contention_limit_and_stride_clouds(oracle):
    cl = ve.contention_clouds()
    assert _held(oracle, cl["first_is_0"])[1].tolist() == [0]
    assert _held(oracle, cl["first_is_49999"])[1].tolist() == list(range(50000))
    L = ve.BIAS
    pts = ve.limit_cloud()
    cells, sel = _held(oracle, pts)
    half = len(pts) // 2
    assert sel.max() < half                                  # the mirrored second half repeats the first
    kept = {tuple(c) for c in cells.tolist()}
    for a in range(3):
        for v, want in ((L - 1, True), (-(L - 1), True)):
            c = [0, 0, 0]; c[a] = v
            assert (tuple(c) in kept) == want
    assert np.abs(cells).max() == L - 1
    assert (L - 1, L - 1, L - 1) in kept and (-(L - 1),) * 3 in kept
    assert (-1, 0, 0) in kept and (0, -1, -1) in kept and (-3, -4, -5) in kept and (-4, -5, -6) in kept
    assert (4, 5, 5) in kept and (-6, -5, -5) in kept and (0, -1, -1) in kept
    dropped = set(range(half)) - set(sel.tolist())
    for i in dropped:                                        # dropped = a repeat of an earlier cell, out of the grid, or not finite
        fl = np.floor(pts[i])
        out = (not np.isfinite(fl).all()) or (np.abs(fl) >= L).any()
        assert out or any(np.array_equal(np.floor(pts[j]), fl) for j in range(i))
    assert sum(1 for i in dropped if not np.isfinite(pts[i]).all() or (np.abs(np.floor(pts[i])) >= L).any()) >= 3 * 7 + 3
    for name, pts in ve.stride_clouds().items():
        cells, sel = _held(oracle, pts)
        n = len(pts)
        if name.startswith("tail_"):
            assert sel.tolist() == [n - 3, n - 2, n - 1]
        if name.startswith("first_and_last_"):
            assert sel.tolist() == [0, n - 1]
