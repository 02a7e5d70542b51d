"""What tests/test_gpu_fcgf_large.py stands on, without a GPU: the network of a cloud of isolated copies IS the copies' networks (checked
in the fmaf-chain restatement itself, every stage), tests/fcgf_large_cases.py builds such clouds at every size the GPU tests use, and the
refusals at the 2^20 limit that are made before the first HIP call."""
import ctypes
import functools

import numpy as np
import pytest

from lidarregistration_amd import _ext, fcgf
from tests import fcgf_cases, fcgf_cpu, fcgf_large_cases as lc

SMALL_MIX = ("random33", "line", "one", "block3_origin")
SMALL_N = 150


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def stages(k1):
    return fcgf.fold(fcgf_cases.make_state_dict(0, k1), k1)


# ---- 1. the decomposition, in the restatement itself --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k1,feat", [(5, False), (3, False), (5, True)], ids=["k5", "k3", "k5_feat"])
def test_a_composite_of_isolated_copies_is_its_parts_bit_for_bit_at_every_stage(k1, feat):
    comp = lc.composite(SMALL_N, seed=1, order="shuffled", mix=SMALL_MIX)
    present = {lc.NAMES[j] for j in np.unique(comp.motif_id)}
    assert present == set(SMALL_MIX) and len(comp.cells) == SMALL_N
    assert not np.array_equal(np.sort(comp.motif_id), comp.motif_id)                   # shuffled: the copies' rows are interleaved
    f = lc.composite_feat(comp) if feat else None
    whole = fcgf_cpu.run(comp.cells, stages(k1), k1, feat_in=f, mode="chain")
    parts = lc.chain_parts(stages(k1), k1, feat_seed=2 if feat else None, names=SMALL_MIX)
    if feat:
        assert not np.array_equal(bits(parts["line"]["out"]), bits(fcgf_cpu.run(lc.MOTIFS["line"], stages(k1), k1, mode="chain")["out"]))
    assert np.array_equal(bits(whole["out"]), bits(lc.expected_out(parts, comp.motif_id, comp.local_row)))
    assert whole["level_of"] == lc.LEVEL_OF
    for s in range(1, 24):
        cells, acts = lc.expected_tap(parts, comp, s)
        lvl = whole["level_of"][s]
        assert np.array_equal(cells, whole["levels"][lvl]), (s, lvl)
        assert acts.shape == whole["acts"][s].shape and np.array_equal(bits(acts), bits(whole["acts"][s])), s


# ---- 2. the builder ---------------------------------------------------------------------------------------------------------------------
def cross_copy_links(comp):
    """The number of (level-3 cell, one of its 26 neighbours at a step of 8) pairs that belong to different copies, counted from the
    cells themselves: the copy of a cell is the lattice site or range-limit corner it lies at, not what the builder says."""
    c3 = (comp.cells.astype(np.int64) >> 3) << 3
    keys, first = np.unique(fcgf_cpu.pack_keys(c3), return_index=True)
    c3 = c3[first]
    site = np.floor_divide(c3 + lc.PITCH // 2, lc.PITCH)                                # a motif's level-3 cells lie within -64 .. 63 of its shift
    out = np.abs(c3) > (1 << 19)                                                        # at the range limit: which axes it went out on, which way
    copy_key = fcgf_cpu.pack_keys(np.where(out.any(1)[:, None], np.sign(c3) * out * (1 << 19), site))
    links = 0
    for k in range(27):
        o = np.array([k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1], np.int64) * 8
        q = c3 + o
        ok = (np.abs(q) < fcgf_cpu.BIAS).all(1)
        qk = fcgf_cpu.pack_keys(np.where(ok[:, None], q, 0))
        pos = np.minimum(np.searchsorted(keys, qk), len(keys) - 1)
        hit = ok & (keys[pos] == qk)
        links += int((copy_key[pos[hit]] != copy_key[hit]).sum())
    return links


@functools.lru_cache(maxsize=None)
def built(n, order="shuffled", mix="all"):
    return lc.composite(n, seed=n % 1000, order=order, mix=mix)


@pytest.mark.parametrize("n,order,mix", [(n, "shuffled", "all") for n in lc.NETWORK_SIZES] + [(lc.MID_N, o, m) for o, m in lc.MID_CASES]
                         + [(1 << 20, "shuffled", "singles")], ids=lambda v: str(v))
def test_builder_invariants_at_every_size_the_gpu_tests_use(n, order, mix):
    comp = built(n, order, mix)
    cells = comp.cells.astype(np.int64)
    assert cells.shape == (n, 3) and comp.cells.dtype == np.int32 and len(comp.motif_id) == len(comp.local_row) == n
    keys = fcgf_cpu.pack_keys(cells)
    assert len(np.unique(keys)) == n and fcgf_cpu.status_of(cells) == 0                 # distinct, in range
    assert (comp.shifts % 8 == 0).all() and cross_copy_links(comp) == 0                  # the separation
    assert (cells.max(0) >= lc.LIMIT - 64).all() and (cells.min(0) <= -(lc.LIMIT - 64)).all() and np.abs(cells).max() < lc.LIMIT
    assert (keys.max() >> 62) == 1 and (keys.min() >> 52) == 0                           # the sorted keys use their high bits
    for j in np.unique(comp.motif_id):                                                   # every row is the cell it says it is, moved by 8k
        at = np.nonzero(comp.motif_id == j)[0][:1000]
        d = cells[at] - lc.MOTIFS[lc.NAMES[j]][comp.local_row[at]]
        assert (d % 8 == 0).all()
    if mix == "singles":
        assert set(np.unique(comp.motif_id)) == {lc.NAMES.index("one")}
    if order == "as_built":                                                              # copies contiguous
        assert (np.diff(comp.local_row) == 1).sum() == n - len(comp.copy_motif)
    if order == "descending_key":
        assert (np.diff(keys) < 0).all()
    counts = lc.level_counts(comp)                                                       # the level counts, from packed keys (np.unique(axis=0)
    for lvl in (1, 2, 3):                                                                # takes seconds at 2^20 rows)
        assert len(np.unique(fcgf_cpu.pack_keys((cells >> lvl) << lvl))) == counts[lvl], lvl
    assert counts[0] == n


def test_assembled_level_sets_equal_the_restatements_levels_at_70000_cells():
    comp = built(lc.MID_N + 4463)                                                        # 70 000
    L = fcgf_cpu.levels(comp.cells)
    for lvl in range(4):
        cells, motif, row = lc.level_rows(comp, lvl)
        assert np.array_equal(cells, L[lvl]), lvl
        pick = np.random.default_rng(lvl).integers(0, len(cells), 2000)                  # ... and each names its cell of its motif
        for i in pick:
            d = cells[i] - lc.MOTIF_LEVELS[lc.NAMES[motif[i]]][lvl][row[i]]
            assert (d % 8 == 0).all()


def test_mixes_orders_and_the_motif_library():
    assert "two_clusters" not in lc.NAMES and len(lc.NAMES) == 11 and max(len(m) for m in lc.MOTIFS.values()) <= 150
    assert {"random33", "random65", "random129", "block3_origin", "one", "two_adjacent", "line", "plane", "single_coarse", "block5"} < set(lc.NAMES)
    for m in lc.MOTIFS.values():
        assert fcgf_cpu.status_of(m) == 0
    comp = built(lc.MID_N)
    assert {lc.NAMES[j] for j in np.unique(comp.motif_id)} == set(lc.NAMES)
    tiles = comp.motif_id[:len(comp.motif_id) // 64 * 64].reshape(-1, 64)               # shuffled: a row tile mixes motifs
    assert (tiles != tiles[:, :1]).any(1).all()


# ---- 3. refusals at the limit, before any HIP call -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _ext.build()
    return _ext.lib()


def test_scratch_bytes_up_to_the_limit_and_the_refusal_past_it(L):
    sizes = sorted(set(lc.NETWORK_SIZES) | {0, 1, lc.MID_N})
    need = [L.lr_fcgf_scratch_bytes(n) for n in sizes]
    assert all(b > 0 for b in need) and all(a <= b for a, b in zip(need, need[1:]))
    assert L.lr_fcgf_scratch_bytes(1 << 20) > 5 * (1 << 30) and L.lr_fcgf_scratch_bytes((1 << 20) + 1) == 0 and L.lr_fcgf_scratch_bytes(-1) == 0
    p = _ext.FcgfParams()
    rc = L.lr_fcgf_extract(None, None, (1 << 20) + 1, None, 0, ctypes.byref(p), None, None, None, None, 0, None)      # no pointer is looked at
    assert rc == -1 and "n must lie in 0 .. 2^20" in L.lr_last_error().decode()
