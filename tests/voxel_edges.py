"""Inputs for the voxel hash (csrc/lr_voxel.hip) that random scans never produce, and the plain definition they are held to
(numpy / pure Python only): long merged probe chains, one heavily contended cell, the +-2^20 cell limit, floors of negative
coordinates, and the 256-element strides of the ordered compaction."""
import functools
import math

import numpy as np

BIAS = 1 << 20
M64 = (1 << 64) - 1
C1, C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)


def dedup_ref(coords):
    """The definition: floor, the first index of every occupied cell, ascending; a point whose cell is not inside (-2^20, 2^20) on
    every axis, or is not finite, is dropped.  A Python dict over tuples.  Returns (cells [M, 3] int32, sel [M] int64)."""
    first = {}
    for i, p in enumerate(np.asarray(coords, np.float64).tolist()):
        if not all(math.isfinite(v) for v in p):
            continue
        c = tuple(math.floor(v) for v in p)
        if any(abs(v) >= BIAS for v in c):
            continue
        if c not in first:
            first[c] = i
    sel = sorted(first.values())
    by_index = {i: c for c, i in first.items()}
    return np.array([by_index[i] for i in sel], np.int32).reshape(-1, 3), np.array(sel, np.int64)


# ----------------------------------------------------------------------------- the hash, restated
def key_of(cell):
    x, y, z = (int(v) + BIAS for v in cell)
    return (x << 42) | (y << 21) | z


def cell_of(key):
    return tuple(((key >> s) & 0x1fffff) - BIAS for s in (42, 21, 0))


def hash_of(key):
    k = key
    k ^= k >> 33; k = (k * C1) & M64; k ^= k >> 33; k = (k * C2) & M64; k ^= k >> 33
    return k & 0xffffffff


def _unmix(h):
    """The 64-bit mixing function is a bijection: x ^= x >> 33 undoes itself, the multipliers are odd."""
    k = h
    k ^= k >> 33; k = (k * C2_INV) & M64; k ^= k >> 33; k = (k * C1_INV) & M64; k ^= k >> 33
    return k


def capacity(n):
    c = 1024
    while c < 2 * max(n, 1):
        c <<= 1
    return c


def cells_on_slot(slot, cap, count, rng):
    """`count` distinct valid cells whose key hashes to table slot `slot` of a table of `cap` slots."""
    out = set()
    while len(out) < count:
        h = (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))) & M64
        h = (h & ~(cap - 1)) | slot
        k = _unmix(h)
        if k >> 63:
            continue
        c = cell_of(k)
        if all(abs(v) < BIAS for v in c) and key_of(c) == k:
            out.add(c)
    return sorted(out)


def probe_lengths(cells_in_order, cap):
    """Linear probing as the kernel does it, one point after the other: the number of steps every distinct cell took."""
    table = {}
    steps = []
    for c in cells_in_order:
        k = key_of(c)
        s = hash_of(k) & (cap - 1)
        d = 0
        while s in table and table[s] != k:
            s = (s + 1) & (cap - 1); d += 1
        if s not in table:
            table[s] = k; steps.append(d)
    return steps


@functools.lru_cache(maxsize=None)
def probe_chain_cloud():
    """1 500 distinct cells whose keys fall on ONE slot of the table the kernel sizes for this cloud (2 n rounded up to a power of two),
    1 000 more on the slot 700 places further on -- the two chains merge -- interleaved with 10 000 ordinary points; every chain cell
    occurs a second time later in the cloud.  Should the hash ever change, the assertions on the result still hold and only the stress
    is lost (tests/test_voxel_edges_cpu.py notices: it asserts the chain length under the restated hash)."""
    rng = np.random.default_rng(77)
    n = 2 * 2500 + 10000
    cap = capacity(n)
    a = cells_on_slot(1234, cap, 1500, rng); b = cells_on_slot(1234 + 700, cap, 1000, rng)
    chain = np.array(a + b, np.float64)[rng.permutation(2500)]
    ordinary = np.concatenate([rng.normal(0, 100, (10000, 2)), rng.uniform(-10, 17, (10000, 1))], 1)
    pts = np.concatenate([chain + rng.random((2500, 3)), ordinary, chain + rng.random((2500, 3))])
    where = np.concatenate([rng.permutation(12500), 12500 + np.arange(2500)])       # first occurrences interleaved, the repeats at the end
    out = np.empty_like(pts); out[where] = pts
    return dict(coords=out, cap=cap, n_chain=2500)


def contention_clouds():
    """(a) 50 000 points in one cell, the first at index 0; (b) 49 999 points in distinct cells, then the same 50 000: the cell's
    first index is 49 999, and the blocks that insert it are the last ones."""
    rng = np.random.default_rng(5)
    one = np.array([3.0, -7.0, 2.0]) + rng.random((50000, 3))
    k = np.arange(49999)
    distinct = np.stack([100 + k % 300, 50 + k // 300, np.full(49999, 9)], 1) + 0.5
    return {"first_is_0": one, "first_is_49999": np.concatenate([distinct, one])}


def limit_cloud():
    """Cells at +-(2^20 - 1) on each axis (kept), at +-2^20 (dropped), -0.0, -1e-300, exact negative integers, and the doubles on
    either side of an integer."""
    L = float(BIAS)
    rows = [[0.5, 0.5, 0.5], [-0.0, 0.0, -0.0], [-1e-300, 0.0, 0.0], [0.0, -1e-300, -1e-300], [-3.0, -4.0, -5.0], [-3.5, -4.5, -5.5],
            [np.nextafter(5.0, -np.inf), 5.0, np.nextafter(5.0, np.inf)], [np.nextafter(-5.0, -np.inf), -5.0, np.nextafter(-5.0, np.inf)],
            [np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), np.nextafter(0.0, -1.0)], [4.999, 5.0, 5.001]]
    for a in range(3):
        for v in (L - 1, L - 0.5, np.nextafter(L, 0.0), L, L + 0.5, -(L - 1), -(L - 1) - 1e-9, -L, -L - 0.5, np.nextafter(-(L - 1), 0.0), 1e9, -1e9):
            r = [0.25, 0.25, 0.25]; r[a] = v
            rows.append(r)
    rows += [[L - 1, L - 1, L - 1], [-(L - 1), -(L - 1), -(L - 1)], [L - 1, -(L - 1), L - 1], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    pts = np.array(rows, np.float64)
    return np.concatenate([pts, pts[::-1]])           # everything twice: the first occurrence wins


def stride_clouds():
    """n around the 256-point blocks of the compaction and its 256-blocks-per-round prefix loop: random cells with collisions, and
    clouds whose only survivors are the last three points."""
    out = {}
    for n in (255, 256, 257, 65536, 65537):
        rng = np.random.default_rng(n)
        out[f"random_{n}"] = rng.uniform(-40, 40, (n, 3)) * np.array([1.0, 1.0, 0.1])
        tail = np.full((n, 3), 1e9)
        tail[n - 3:] = [[1.5, 2.5, 3.5], [-1.5, 2.5, 3.5], [1.5, -2.5, 3.5]]
        out[f"tail_{n}"] = tail
        dup = np.tile(np.array([[0.5, 0.5, 0.5]]), (n, 1)); dup[n - 1] = [7.5, 0.5, 0.5]
        out[f"first_and_last_{n}"] = dup
    return out
