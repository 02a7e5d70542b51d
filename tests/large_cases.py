"""Clouds for the tests of the cloud-level kernels past 65 536 points per cloud (lr_voxel_mean / lr_overlap, lr_nn3, lr_refine_z, lr_bbrf,
lr_normals), built from seeds: the smallest at which each path that first runs above 65 536 is reached.  Shared by
tests/test_large_cpu.py, tests/test_gpu_large.py and tests/golden/make_golden_refine_z.py.

Every case group carries the threshold it is named for as a predicate on its sizes (THRESHOLDS), computed from the sizes alone:
  three_passes   lr_overlap.hip sorts the rows in three radix passes from 65 536 points of the call's largest cloud on
  third_digit    a row index >= 65 536 is the first sort key whose third digit is not 0: rows >= 65 537
  blocks_before  lr_prims.h's lr_blocks_before takes a second round from block 257 on: cdiv(n, 256) > 257
  runs           the step kernels of lr_refine_z / lr_bbrf sum the run totals 64 at a time: cdiv(n0, 1024) > 64
  init_rounds    nn_init_kernel clears max(4096, 4 n1) cells with at most 1024 blocks of 256: 4 n1 > 262 144
  far_rounds     nn_far_kernel serves at most 8 192 open queries per round
"""
import functools

import numpy as np

from lidarregistration_amd import synth
from tests import bbrf_cases, overlap_cpu, refine_z_cases, refine_z_cpu
from tests.overlap_cases import ROT90, checksum, lattice, partner_pair, scan  # noqa: F401  (checksum: re-exported for the fixture)
from tests.refine_z_cases import VOXEL, Z_OFF, auto_cell, lifted

EDGE = (65535, 65536, 65537)        # the last two-pass size, the first three-pass size, the first with a row whose third digit is 1
RAW = 120000                        # raw points per frame of the full-size scan pair
SHELL_CAP = 3                       # nn_walk_kernel looks at the shells 0 .. 3 around the query's cell
FAR_WAVES = 8192                    # nn_far_kernel: NN_FAR_BLOCKS * 4 waves, one open query each per round


def cdiv(a, b):
    return -(-a // b)


THRESHOLDS = dict(three_passes=lambda n: n >= 65536, third_digit=lambda rows: rows >= 65537, blocks_before=lambda n: cdiv(n, 256) > 257,
                  runs=lambda n0: cdiv(n0, 1024) > 64, init_rounds=lambda n1: max(4096, 4 * n1) > 262144, far_rounds=lambda n_open: n_open > FAR_WAVES)


@functools.lru_cache(maxsize=None)
def raw_pair():
    """synth.make_scan_pair at 120 000 raw points per frame: (A, B, T)."""
    return synth.make_scan_pair(RAW, RAW)


def scan_pair():
    """The pair above down-sampled at 0.3 (75 199 / 74 958 centroids), the motion off by 0.37 m in z: (a, b, raw_mot)."""
    return refine_z_cases.scan_pair(RAW)


# ---- lr_voxel_mean ----------------------------------------------------------------------------------------------------------------------
def one_cell(n, seed):
    """n points of one cell at voxel 1 (all within 0.45 of the cloud's minimum), offsets of magnitudes 1e-8 .. 1: one n-point segment."""
    rng = np.random.default_rng(seed)
    X = 0.45 * 10.0 ** rng.uniform(-8.0, 0.0, size=(n, 3)) - 3.0
    X[n // 3] = -3.0                                                     # the cloud's minimum: the cell is [-3.5, -2.5)
    return X


def few_cells(n, cells, seed):
    """n points in `cells` cells at voxel 1, every cell hit, in shuffled order: the lattice's points (2 apart, the minimum among them) plus
    offsets in [0.1, 0.4) -- measured from the grid's origin, minimum - 0.5, every point lies in (2 j + 0.5, 2 j + 0.9)."""
    rng = np.random.default_rng(seed)
    g = lattice(cells, 2.0, seed)
    X = g[np.concatenate([np.arange(cells), rng.integers(0, cells, size=n - cells)])] + rng.uniform(0.1, 0.4, size=(n, 3))
    X[:cells][g.argmin(axis=0)] = g[g.argmin(axis=0)]                    # the three minima are lattice points themselves
    return X[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def cloud_cases():
    """name -> (X, voxel, T) like overlap_cases.cloud_cases; `expect_rows` below names the row count each is built for."""
    c = {}
    for n in EDGE:
        X = lattice(n, 2.0, n)
        c[f"own_cell_{n}"] = (X, 1.0, None)
        Y = X.copy(); Y[n // 2, 1] = np.nan; Y[n - 1, 0] = np.nan
        c[f"own_cell_nan_{n}"] = (Y, 1.0, None)
        c[f"one_cell_{n}"] = (one_cell(n, n), 1.0, None)
    c["few_cells_70001"] = (few_cells(70001, 300, 70001), 1.0, None)
    A, B, _ = raw_pair()
    for voxel in (0.3, 1.0):
        c[f"scan_a_v{voxel}"] = (A, voxel, None)
        c[f"scan_b_v{voxel}"] = (B, voxel, None)
    return c


def expect_rows(name):
    """The row count a cloud case is built for (None: whatever the scan gives)."""
    if name.startswith("scan"):
        return None
    n = int(name.rsplit("_", 1)[1])
    return n - 2 if name.startswith("own_cell_nan") else n if name.startswith("own_cell") else 1 if name.startswith("one_cell") else 300


# ---- lr_overlap / lr_overlap_batch ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_cases():
    A, B, T = raw_pair()
    return {f"scan_v{voxel}": dict(A=A, B=B, T=T, voxel=voxel, radius=0.0) for voxel in (0.3, 1.0)}


BATCH_SIZES = ((70001, 257), (257, 70001), (0, 65536), (257, 257))


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """One batch whose largest cloud asks for three passes: the (257, 257) pair is sorted in three passes inside it and in two alone."""
    return tuple(partner_pair(91 + k, n0, n1, T) for k, ((n0, n1), T) in enumerate(zip(BATCH_SIZES, (None, ROT90, None, None))))


# ---- lr_nn3 -----------------------------------------------------------------------------------------------------------------------------
def grid_of(B, cell=0.0):
    """N6 restated: (cell edge, cells per axis) of the search grid over B for the caller's `cell` -- 0: the automatic rule; otherwise that
    edge, doubled until the grid has at most max(4096, 4 n1) cells."""
    B = B[np.isfinite(B).all(axis=1)]
    ext = B.max(axis=0) - B.min(axis=0)
    cap = max(4096, 4 * len(B))
    e = auto_cell(B) if cell == 0.0 else float(cell)
    while np.prod(np.floor(ext / e) + 1.0) > cap:
        e *= 2.0
    return e, (np.floor(ext / e) + 1.0).astype(int)


def _clusters(rng, n):
    """n points in two tight clusters at opposite corners of a 100 m box."""
    return np.concatenate([rng.uniform(0.0, 0.5, size=(n - n // 2, 3)), rng.uniform(99.5, 100.0, size=(n // 2, 3))])


def _corner_target(rng):
    """1 024 points in the two clusters and one point that pins the box's upper corner (the lower one is pinned too): 1 025 points."""
    B = np.concatenate([_clusters(rng, 1024), np.full((1, 3), 100.0)])
    B[0] = 0.0
    return B[rng.permutation(len(B))]


def far_rounds_case(seed=95):
    """More than 8 192 queries that stay open after the shells, without a large cloud: the target is two tight clusters of 512 points at
    opposite corners of a 100 m box and one point that pins the box's upper corner; 8 193 + 257 queries lie within 1 m of the box's
    centre -- 49 m (Chebyshev) from every target point --, 257 more inside the clusters.  The queries are shuffled, so the open ones
    are spread over every block.  middle: the rows of the former."""
    rng = np.random.default_rng(seed)
    B = _corner_target(rng)
    middle = 50.0 + rng.uniform(-1.0, 1.0, size=(FAR_WAVES + 1 + 257, 3))
    A = np.concatenate([middle, _clusters(rng, 257)])
    perm = rng.permutation(len(A))
    return dict(A=A[perm], B=B, middle=np.flatnonzero(np.isin(perm, np.arange(len(middle)))))


def blocks_case(n0, seed):
    """n0 queries inside the clusters of the same kind of target, except the rows `middle`, which lie at the box's centre and stay open:
    a few in the first block, the others from row 65 530 on -- beyond block 256, and for n0 = 70 001 in every block from 257 on."""
    rng = np.random.default_rng(seed)
    B = _corner_target(rng)
    A = _clusters(rng, n0)[rng.permutation(n0)]
    middle = np.concatenate([np.arange(3, 9), np.arange(65530, n0 - 1, 7), [n0 - 1]])
    A[middle] = 50.0 + rng.uniform(-1.0, 1.0, size=(len(middle), 3))
    return dict(A=A, B=B, middle=middle)


@functools.lru_cache(maxsize=None)
def nn_cases():
    """name -> dict(A, B[, middle][, tree]); middle: the rows that stay open after the shells; tree: the brute-force reference is out of
    reach, the reference is nn_tree."""
    c = {}
    for n1 in (65537, 70001):
        c[f"grid_257_{n1}"] = dict(A=scan(257, 700 + n1 % 7), B=scan(n1, 701 + n1 % 7) + np.array([1.0, -0.5, 0.1]))
    for n0 in (65537, 70001):
        c[f"blocks_{n0}_1025"] = blocks_case(n0, 710 + n0 % 7)
    c["far_rounds"] = far_rounds_case()
    a, b, raw = scan_pair()
    c["scan"] = dict(A=refine_z_cpu.transform(a, raw), B=b, tree=True)
    return c


# ---- lr_refine_z ------------------------------------------------------------------------------------------------------------------------
def two_pairs(seed=96):
    """65 537 source points against 1 025 target points (one layer, at least 0.75 apart in x or in y) of which only source 0 (run 0) and source 65 536 (run 64)
    lie within the xy gate of their neighbour: every other one sits 0.36 in x beside a target point -- nearer to it than to any other
    (those are 0.39 away at the least), and beyond the gate of 0.3 from both."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(33), np.arange(32), indexing="ij"), axis=-1).reshape(-1, 2)[:1025].astype(np.float64)
    B = np.concatenate([g, np.zeros((1025, 1))], axis=1) + np.floor(rng.uniform(0, 0.25, size=(1025, 3)) * 1024.0) / 1024.0
    B = B[rng.permutation(1025)]
    n0 = 65537
    A = B[rng.integers(0, 1025, size=n0)] + np.array([0.36, 0.0, 0.0])
    A[:, 2] += np.clip(rng.normal(scale=0.05, size=n0), -0.1, 0.1)
    A[0] = B[11] + np.array([0.0625, 0.0, 0.25])
    A[n0 - 1] = B[700] + np.array([0.0, -0.125, -0.0625])
    return A, B


@functools.lru_cache(maxsize=None)
def refine_cases():
    """name -> dict(A, B, T, gate, max_repeats, min_change[, expect]) like refine_z_cases.refine_cases."""
    d = dict(T=None, gate=VOXEL, max_repeats=10, min_change=1e-6)
    c = {}
    for n in (65537, 66561):                                             # 65 and 66 runs
        A, B = lifted(n, 70 + n, 0.25)
        c[f"lifted_{n}"] = dict(d, A=A, B=B, expect=dict(status=2, repeats=2, dz=-0.25, n_valid=n))
    A, B = two_pairs()
    c["two_pairs"] = dict(d, A=A, B=B)
    a, b, raw = scan_pair()
    c["scan"] = dict(d, A=a, B=b, T=raw)
    return c


@functools.lru_cache(maxsize=None)
def refine_trace(name):
    """The restatement on a refine case over nn_tree, once per process: (result block, per-repeat trace)."""
    p, trace = refine_cases()[name], []
    return refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], p["max_repeats"], p["min_change"], trace=trace, search=refine_z_cpu.nn_tree), trace


# ---- lr_bbrf / lr_normals ---------------------------------------------------------------------------------------------------------------
def _buddies(n0, n1, seed):
    """A: a scan of n0 points; B: n1 of them, the first n1 - 1 and the last one (or all of B's first n0 when n1 > n0), each moved a
    little: best buddies in the first run and in the last."""
    base = scan(max(n0, n1), seed)
    rng = np.random.default_rng(seed + 1)
    A = base[:n0].copy()
    pick = np.arange(n1) if n1 <= 1 or n1 > n0 else np.concatenate([np.arange(n1 - 1), [n0 - 1]])
    B = base[pick] + rng.normal(scale=0.001, size=(n1, 3)) + np.array([0.002, -0.001, 0.003])
    return A, B


@functools.lru_cache(maxsize=None)
def bbrf_cases_large():
    """name -> dict(A, nA, B, nB, params) like bbrf_cases; three iterations each."""
    c = {}
    A, B = _buddies(65537, 1025, 97)
    c["bb_65537_1025"] = bbrf_cases._case(A, B, seed=97, n_iter=3)
    A, B = _buddies(1025, 65537, 98)
    c["bb_1025_65537"] = bbrf_cases._case(A, B, seed=98, n_iter=3)
    a, b, raw = scan_pair()
    T = raw.copy(); T[2, 3] -= Z_OFF
    A = overlap_cpu.transform(a, bbrf_cases.small_motion(71, 0.8, 0.05) @ T)
    c["scan_z"] = bbrf_cases._case(A, b, bbrf_cases.z_normals(len(A)), bbrf_cases.z_normals(len(b)), n_iter=3)
    c["scan_generic"] = bbrf_cases._case(A, b, bbrf_cases.unit_normals(len(A), 72), bbrf_cases.unit_normals(len(b), 73), n_iter=3)
    return c


def ball_neighbours(X, radius, max_nn):
    """bbrf_cpu.neighbours without the distance matrix: the candidates from scipy's k-d tree (a ball 1e-6 wider), then the contract's d2,
    its bound d2 <= fl(radius radius) and its (d2, index) order, cut at max_nn."""
    from scipy.spatial import cKDTree
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    live = np.flatnonzero(np.isfinite(X).all(axis=1))
    out = [np.zeros(0, np.int64)] * len(X)
    if not len(live):
        return out
    P = X[live]
    lists = cKDTree(P).query_ball_point(P, radius * (1.0 + 1e-6), workers=8)
    r2 = radius * radius
    for a, l in enumerate(lists):
        c = np.asarray(l, np.int64)
        d = P[a] - P[c]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = d2 <= r2
        c, d2 = live[c[ok]], d2[ok]
        out[live[a]] = c[np.lexsort((c, d2))][:max_nn]
    return out


def normals_case():
    """The 74 958-centroid cloud at radius 0.6 (two voxels), max_nn 13."""
    return dict(X=scan_pair()[1], radius=0.6, max_nn=13)


# ---- the golden pair at full size -------------------------------------------------------------------------------------------------------
GOLDEN_NAME = "g_scan_120000"


def golden_case():
    """The pair the reference's own refine_motion_Z_only is recorded on in tests/golden/g20_refine_z_large.npz."""
    a, b, raw = scan_pair()
    return dict(A=a, B=b, T=raw, gate=VOXEL)


def golden_trace():
    return refine_trace("scan")


def index_hash(ind):
    """SHA-256 of an index array as little-endian int32."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(ind, "<i4").tobytes()).hexdigest()
