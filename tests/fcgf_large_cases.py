"""Large inputs of the FCGF tests with an exact reference: clouds of ISOLATED copies of the small cases of tests/fcgf_cases.py.

A sparse convolution connects cells that are neighbours at some level only.  Copies of small motifs, each moved by a multiple of 8 and
kept so far apart that no level-3 cell of one lies within two level-3 steps (16) of a level-3 cell of another, share no entry of any
gather table of any level: the network decomposes.  Every output row is then, bit for bit, the fmaf-chain restatement's row of that cell
in its motif alone (F10: a shift by 8k changes no bit), and a level's rows are the motifs' rows in F1 order, i.e. the ascending key sort
of the moved motif level sets (disjoint: no np.unique).  The reference of a 2^20-row cloud is a handful of chain runs on at most 144
cells plus fancy indexing.  tests/test_fcgf_large_cpu.py checks the decomposition in the restatement itself; `composite` asserts the
conditions it rests on."""
import collections

import numpy as np

from tests import fcgf_cases, fcgf_cpu

LIMIT = fcgf_cpu.LIMIT
PITCH = 128                                          # lattice pitch: a multiple of 64
N_EDGE = 8                                           # copies put at the range limit
ORDERS = ("shuffled", "as_built", "descending_key")
# the sizes of the whole-network test: around the sort's first global step (2 048) and its second, a hash table at a load of exactly
# one half (2^k) and right behind the doubling (2^k + 1), and the limit of the call
NETWORK_SIZES = (2047, 2048, 2049, 4096, 4097, 65536, 65537, 131073, (1 << 20) - 1, 1 << 20)
MID_N = 65537
MID_CASES = (("as_built", "all"), ("descending_key", "all"), ("shuffled", "singles"), ("shuffled", "lines"), ("as_built", "dense"))


def _library():
    small = fcgf_cases.small_cases()
    lib = {k: small[k] for k in ("random33", "random65", "random129", "block3_origin", "one", "two_adjacent", "line", "plane", "single_coarse",
                                 "block5")}                    # (two_clusters left out: its extent of 6 000 fits no lattice cell)
    lib["dense140"] = fcgf_cases.random_cells(140, 6, 9, lo=-11)      # 140 of the 216 cells of a box across the level-3 boundary at -8
    return {k: np.ascontiguousarray(v, np.int32) for k, v in lib.items()}


MOTIFS = _library()
NAMES = tuple(MOTIFS)
MOTIF_LEVELS = {k: fcgf_cpu.levels(v) for k, v in MOTIFS.items()}
MIXES = {"all": NAMES, "singles": ("one",), "lines": ("line",), "dense": ("block5", "block3_origin", "dense140")}
# the directions of the copies at the range limit: each sign of each axis, and two more on a diagonal of the xy plane.  No copy lies
# near the corner (+, -, +), where the test of the last admitted cell puts its cell.
EDGE_DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [-1, -1, 0]])

LEVEL_OF = {s: (0, 1, 2, 3, 2, 1, 0, 0)[min((s - 1) // 3, 7)] for s in range(1, 24)}      # the level a stage's rows live at (F7)

Composite = collections.namedtuple("Composite", "cells motif_id local_row copy_motif shifts")


def _lvl3_span():
    """(lo, hi) [3]: the smallest and largest level-3 coordinate any motif has on each axis."""
    lo = np.min([(m.min(0) >> 3) << 3 for m in MOTIFS.values()], 0)
    hi = np.max([(m.max(0) >> 3) << 3 for m in MOTIFS.values()], 0)
    return lo.astype(np.int64), hi.astype(np.int64)


def _copy_list(n, names, rng):
    """Motif ids of the copies: N_EDGE copies for the range limit first, then the lattice's.  The sizes add up to exactly n."""
    size = {k: len(MOTIFS[k]) for k in NAMES}
    edge, used = [], 0
    for i in range(N_EDGE):                          # the mix's motifs in turn while they leave half of n to the lattice, `one` otherwise
        k = names[i % len(names)]
        if used + size[k] + (N_EDGE - 1 - i) > n // 2:
            k = "one"
        edge.append(k); used += size[k]
    assert used <= n, (n, used)
    rest = n - used
    rounds, rest = divmod(rest, sum(size[k] for k in names))
    tail = []
    for k in sorted(names, key=lambda k: -size[k]):  # the remainder: largest first while they fit ...
        if size[k] <= rest:
            tail.append(k); rest -= size[k]
    tail += ["one"] * rest                           # ... and trimmed to exactly n with single cells
    lattice = np.array([NAMES.index(k) for k in list(names) * rounds + tail], np.int64)
    return np.array([NAMES.index(k) for k in edge], np.int64), lattice[rng.permutation(len(lattice))]


def composite(n, seed=0, order="shuffled", mix="all"):
    """n distinct cells: copies of the motifs of `mix` (a key of MIXES, or a tuple of motif names) on a lattice of pitch PITCH centred on
    the origin, N_EDGE more within 64 of the range limit +-(2^20 - 2), trimmed to n with copies of `one`.
    -> Composite(cells [n,3] int32, motif_id [n] (index into NAMES), local_row [n] (row in MOTIFS[name]), copy_motif [c], shifts [c,3])."""
    names = MIXES[mix] if isinstance(mix, str) else tuple(mix)
    assert order in ORDERS and n >= 2 * N_EDGE
    rng = np.random.default_rng(seed)
    edge, lattice = _copy_list(n, names, rng)
    # the lattice: the first sites of a g^3 cube around the origin, in a seeded order
    g = 1
    while g ** 3 < len(lattice):
        g += 1
    site = rng.permutation(g ** 3)[:len(lattice)]
    lat_shift = (np.stack([site % g, site // g % g, site // (g * g)], 1) - g // 2) * PITCH
    # the range limit: along direction d the copy's far cell lands on +-(LIMIT - 1 - (0 .. 7)), the shift a multiple of 8
    edge_shift = np.zeros((N_EDGE, 3), np.int64)
    for i, (j, d) in enumerate(zip(edge, EDGE_DIRS)):
        m = MOTIFS[NAMES[j]].astype(np.int64)
        up = (LIMIT - 1 - m.max(0)) // 8 * 8
        dn = -((LIMIT - 1 + m.min(0)) // 8 * 8)
        edge_shift[i] = np.where(d > 0, up, np.where(d < 0, dn, 0))
    copy_motif = np.concatenate([edge, lattice])
    shifts = np.concatenate([edge_shift, lat_shift]).astype(np.int64)

    # what the decomposition rests on
    assert (shifts % 8 == 0).all() and (lat_shift % 64 == 0).all() and PITCH % 64 == 0 and PITCH >= 128
    lo3, hi3 = _lvl3_span()
    assert PITCH - (hi3 - lo3).max() >= 16, "two lattice copies: their level-3 ranges are 16 apart on an axis where the sites differ"
    assert len(np.unique(site)) == len(site)
    reach = max(np.abs(lo3).max(), np.abs(hi3).max())
    far = np.abs(edge_shift).max(1)                  # an edge copy against the lattice: apart on the axis it went out on
    assert (far - reach - 16 >= np.abs(lat_shift).max(initial=0) + reach).all()
    for a in range(N_EDGE):                          # the edge copies among themselves: 28 pairs
        for b in range(a):
            gap = np.maximum(edge_shift[a] + lo3 - (edge_shift[b] + hi3), edge_shift[b] + lo3 - (edge_shift[a] + hi3))
            assert gap.max() >= 16, (a, b)

    # rows in copy order (`as_built`: the copies contiguous)
    sizes = np.array([len(MOTIFS[k]) for k in NAMES], np.int64)[copy_motif]
    start = np.cumsum(sizes) - sizes
    assert start[-1] + sizes[-1] == n
    cells = np.empty((n, 3), np.int64); motif_id = np.empty(n, np.int64); local_row = np.empty(n, np.int64)
    for j in np.unique(copy_motif):
        m = MOTIFS[NAMES[j]].astype(np.int64)
        c = np.nonzero(copy_motif == j)[0]
        rows = (start[c][:, None] + np.arange(len(m))[None, :]).reshape(-1)
        cells[rows] = (shifts[c][:, None, :] + m[None, :, :]).reshape(-1, 3)
        motif_id[rows] = j
        local_row[rows] = np.tile(np.arange(len(m)), len(c))
    if order == "shuffled":
        p = rng.permutation(n)
        single = np.nonzero(motif_id[p] == NAMES.index("one"))[0]
        if len(single):                              # the last row is a single cell: it stands for its coarse cell at every level, so at
            p[[single[-1], n - 1]] = p[[n - 1, single[-1]]]      # n = 2^k + 1 its key is the one the sort has to carry across a chunk boundary
    elif order == "descending_key":
        p = np.argsort(fcgf_cpu.pack_keys(cells))[::-1]
    else:
        p = np.arange(n)
    cells, motif_id, local_row = cells[p], motif_id[p], local_row[p]
    assert fcgf_cpu.status_of(cells) == 0
    assert np.abs(cells).max(0).min() >= LIMIT - 64 and (cells.max(0) >= LIMIT - 64).all() and (cells.min(0) <= -(LIMIT - 64)).all()
    return Composite(cells.astype(np.int32), motif_id, local_row, copy_motif, shifts)


def motif_feat(name, seed=2):
    """A non-constant feat_in of a motif, fixed per motif-local row."""
    return np.random.default_rng(seed + 17 * NAMES.index(name)).uniform(0.5, 2.0, len(MOTIFS[name])).astype(np.float32)


def composite_feat(comp, seed=2):
    f = np.empty(len(comp.cells), np.float32)
    for j in np.unique(comp.motif_id):
        at = comp.motif_id == j
        f[at] = motif_feat(NAMES[j], seed)[comp.local_row[at]]
    return f


def chain_parts(stages, k1=5, feat_seed=None, names=NAMES):
    """name -> fcgf_cpu.run(motif, mode="chain"), read-only: the parts a reference is assembled from."""
    parts = {}
    for k in names:
        r = fcgf_cpu.run(MOTIFS[k], stages, k1, feat_in=None if feat_seed is None else motif_feat(k, feat_seed), mode="chain")
        for a in list(r["acts"].values()) + [r["out"]]:
            a.setflags(write=False)
        parts[k] = r
    return parts


def _rows_of(parts, motif_id, local_row, pick):
    first = pick(parts[NAMES[motif_id[0]]])
    out = np.empty((len(motif_id), first.shape[1]), first.dtype)
    for j in np.unique(motif_id):
        at = motif_id == j
        out[at] = pick(parts[NAMES[j]])[local_row[at]]
    return out


def expected_out(parts, motif_id, local_row):
    """[n,32]: row i is the row local_row[i] of the chain result of motif motif_id[i]."""
    return _rows_of(parts, motif_id, local_row, lambda r: r["out"])


def level_rows(comp, lvl):
    """(the composite's level-lvl cells in F1 order [n_l,3] int64, the motif each comes from [n_l], its row in that motif's level [n_l])."""
    if lvl == 0:
        return comp.cells.astype(np.int64), comp.motif_id, comp.local_row
    cells, motif, row = [], [], []
    for j in np.unique(comp.copy_motif):
        L = MOTIF_LEVELS[NAMES[j]][lvl]
        sh = comp.shifts[comp.copy_motif == j]
        cells.append((sh[:, None, :] + L[None, :, :]).reshape(-1, 3))
        motif.append(np.full(len(sh) * len(L), j, np.int64))
        row.append(np.tile(np.arange(len(L)), len(sh)))
    cells = np.concatenate(cells)
    keys = fcgf_cpu.pack_keys(cells)
    order = np.argsort(keys)
    assert (np.diff(keys[order]) > 0).all(), "the copies' level sets are disjoint"
    return cells[order], np.concatenate(motif)[order], np.concatenate(row)[order]


def expected_tap(parts, comp, s):
    """(the cells of stage s's level in F1 order, the activations [n_l,Cout]) of the composite, assembled from the parts.  (comp carries
    the per-copy shifts; level 0 is in input order, which takes the rows' motif_id / local_row as well.)"""
    cells, motif, row = level_rows(comp, LEVEL_OF[s])
    return cells, _rows_of(parts, motif, row, lambda r: r["acts"][s])


def level_counts(comp):
    """[n_0 .. n_3] of the composite from the motifs' own level counts."""
    per = np.array([[len(l) for l in MOTIF_LEVELS[k]] for k in NAMES], np.int64)
    return per[comp.copy_motif].sum(0)
