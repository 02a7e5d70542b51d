"""Clouds for the tests of lr_nn3 / lr_refine_z (csrc/lr_nn3.hip), built from seeds: the smallest at which each kernel can go wrong.
Shared by tests/test_refine_z_cpu.py, tests/test_gpu_refine_z.py and tests/golden/make_golden_refine_z.py.

nn cases: dict name -> dict(A, B[, cell][, expect]).  refine cases: dict name -> dict(A, B, T, gate, max_repeats, min_change)."""
import functools

import numpy as np

from lidarregistration_amd import synth
from tests import overlap_cpu, refine_z_cpu
from tests.overlap_cases import checksum, lattice, rigid, scan  # noqa: F401  (checksum: re-exported for the fixture)

SIZES = (0, 1, 2, 63, 64, 65, 257, 1025)
VOXEL = 0.3
Z_OFF = 0.37
MIN_GAP = 1e-8          # what the golden inputs keep between every decision and its threshold


@functools.lru_cache(maxsize=None)
def scan_pair(n):
    """synth.make_scan_pair at n raw points, both frames down-sampled at 0.3 (the generator's refine_motion), the raw motion off by
    0.37 m in z: (a [n0,3], b [n1,3], raw_mot 4x4)."""
    A, B, T = synth.make_scan_pair(n, n)
    raw = T.copy(); raw[2, 3] += Z_OFF
    return overlap_cpu.voxel_mean(A, VOXEL)["cent"], overlap_cpu.voxel_mean(B, VOXEL)["cent"], raw


def grid_points(n, seed, step=1.0, q=1024.0):
    """n points at least 0.75 step apart, every coordinate a multiple of step / q (sums with a power of two stay exact)."""
    rng = np.random.default_rng(seed)
    return lattice(n, step, seed) + np.floor(rng.uniform(0, 0.25, size=(n, 3)) * q) / q * step


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The pairs the reference's own refine_motion_Z_only is recorded on (tests/golden/g18_refine_z.npz)."""
    c = {}
    for n in (3000, 20000):
        a, b, raw = scan_pair(n)
        c[f"g_scan_{n}"] = dict(A=a, B=b, T=raw, gate=VOXEL)
    # MIN_CHANGE fires: a copy of the target, lifted and lightly jittered in z -- the steps shrink below 1e-6 within the ten repeats
    rng = np.random.default_rng(61)
    B = overlap_cpu.voxel_mean(scan(600, 61), VOXEL)["cent"]
    A = B + np.array([0.01, -0.02, 0.05]) + rng.normal(scale=[0.0, 0.0, 0.004], size=B.shape)
    c["g_small_converges"] = dict(A=A, B=B, T=np.eye(4), gate=VOXEL)
    B = overlap_cpu.voxel_mean(scan(900, 62), VOXEL)["cent"]
    T = rigid(62, 0.2, 5.0)
    A = overlap_cpu.transform(B[: len(B) * 2 // 3] + rng.normal(scale=[0.02, 0.02, 0.05], size=(len(B) * 2 // 3, 3)), np.linalg.inv(T))
    raw = T.copy(); raw[2, 3] -= 0.21
    c["g_small_rigid"] = dict(A=A, B=B, T=raw, gate=VOXEL)
    return c


@functools.lru_cache(maxsize=None)
def golden_trace(name):
    """The restatement on a golden case: (result block, per-repeat trace)."""
    p, trace = golden_cases()[name], []
    return refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"], trace=trace), trace


def check_conditions(p, name, min_change=1e-6, trace=None):
    """In every repeat: nearest and second-nearest distance of every query, every xy distance and the gate, |mean| and MIN_CHANGE lie
    at least MIN_GAP apart -- a perturbation of 1e-10 cannot flip a decision.  Returns the three margins.  trace: the restatement's per-repeat trace where it is not golden_trace(name)'s."""
    if trace is None:
        _, trace = golden_trace(name)
    nn_gap = min(float((t["d_second"] - t["d"]).min()) for t in trace)
    gate = min(float(np.abs(t["xy"][t["ind"] >= 0] - p["gate"]).min()) for t in trace)
    stop = min(abs(abs(t["mean"]) - min_change) for t in trace)
    assert nn_gap >= MIN_GAP, f"{name}: two target points are equally near a query ({nn_gap:.2e})"
    assert gate >= MIN_GAP, f"{name}: a pair sits on the xy gate ({gate:.2e})"
    assert stop >= MIN_GAP, f"{name}: a step sits on MIN_CHANGE ({stop:.2e})"
    return nn_gap, gate, stop


def auto_cell(B):
    """N6's automatic rule, for choosing explicit cells around it (the result must not depend on the cell: nothing is pinned by this)."""
    B = B[np.isfinite(B).all(axis=1)]
    if len(B) == 0:
        return 1.0
    ext = B.max(axis=0) - B.min(axis=0)
    E, cap, cell = ext.max(), max(4096, 4 * len(B)), 1.0
    if not E > 0:
        return 1.0
    cell = E
    for k in range(1, 81):
        t = E * 2.0 ** (-k / 2)
        if np.prod(np.floor(ext / t) + 1.0) > cap:
            break
        cell = t
    return float(cell)


def _pts(*rows):
    return np.array(rows, np.float64)


@functools.lru_cache(maxsize=None)
def nn_cases():
    c = {}
    for n0 in SIZES:
        for n1 in SIZES:
            c[f"size_{n0}_{n1}"] = dict(A=scan(n0, 300 + n0), B=scan(n1, 400 + n1) + np.array([1.0, -0.5, 0.1]))
    a, b, raw = scan_pair(3000)
    c["scan_3000"] = dict(A=overlap_cpu.transform(a, raw), B=b)
    # ties: an integer lattice, queries at cell centres (8 corners at equal d2) and edge midpoints (2), target indices shuffled; with
    # cell 1 the lattice point k lies in cell k, so the equal candidates sit in different cells and shells
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    B = g[np.random.default_rng(5).permutation(len(g))]
    centres = g[(g < 5).all(axis=1)] + 0.5
    edges = np.concatenate([g[g[:, a] < 5] + 0.5 * np.eye(3)[a] for a in range(3)])
    for cell in (0.0, 1.0, 0.5, 3.0):
        c[f"ties_lattice_cell{cell}"] = dict(A=np.concatenate([centres, edges, g]), B=B, cell=cell)
    # the lowest index in the FARTHER shell: with cell 1 the query's own cell holds j = 1, the next one j = 0, at equal d2
    for cell in (0.0, 1.0):
        c[f"ties_far_shell_cell{cell}"] = dict(A=_pts((0.5, 0, 0), (0.5, 0.25, 0)), B=_pts((1, 0, 0), (0, 0, 0), (7, 7, 7)), cell=cell, expect=[0, 0])
        c[f"ties_far_shell_3_cell{cell}"] = dict(A=_pts((2.0, 0, 0)), B=_pts((4, 0, 0), (0, 0, 0), (2, 2, 0), (9, 9, 9)), cell=cell, expect=[0])
    c["duplicates"] = dict(A=scan(65, 8), B=np.concatenate([scan(65, 8)[::-1], scan(65, 8), scan(65, 8)]), expect=list(range(64, -1, -1)))
    # stragglers and the grid's edges
    B = scan(1025, 9)
    c["far_queries"] = dict(A=np.concatenate([scan(70, 10) + np.array([1000.0, 0, 0]), scan(70, 11) + np.array([0, -1000.0, 1000.0]), B[:70] + 0.01]), B=B)
    lo, hi, mid = B.min(axis=0), B.max(axis=0), 0.5 * (B.min(axis=0) + B.max(axis=0))
    out = []
    for a in range(3):
        for side, d in ((lo, -1.0), (hi, 1.0)):
            for dist in (1e-9, 0.3, 4.0, 50.0):
                p = mid.copy(); p[a] = side[a] + d * dist
                out.append(p)
    out += [lo - 3.0, hi + 3.0, lo - 1e-12, hi + 1e-12, np.array([lo[0] - 2.0, hi[1] + 2.0, mid[2]]), lo, hi]
    c["outside_the_grid"] = dict(A=np.array(out), B=B)
    c["one_cell"] = dict(A=scan(257, 12), B=np.random.default_rng(13).uniform(0.1, 0.2, size=(300, 3)), cell=8.0)
    c["single_point"] = dict(A=scan(257, 14), B=_pts((1.5, -2.5, 0.25)))
    c["same_point_twice"] = dict(A=scan(65, 14), B=_pts((1.5, -2.5, 0.25), (1.5, -2.5, 0.25)), expect=[0] * 65)
    line = np.zeros((300, 3)); line[:, 0] = np.random.default_rng(15).uniform(-40, 40, size=300); line[:, 1] = 2.0; line[:, 2] = -1.0
    c["line"] = dict(A=scan(257, 16), B=line)
    plane = scan(700, 17); plane[:, 2] = 0.5
    c["plane"] = dict(A=scan(257, 18), B=plane)
    # queries exactly on the faces of the cells (cell 0.5 from the target's minimum, the origin), each with its neighbour one ulp below
    B = np.concatenate([np.zeros((1, 3)), np.random.default_rng(19).uniform(0, 6, size=(400, 3))])
    f = []
    for a in range(3):
        for k in range(1, 12):
            p = np.array([2.2, 3.1, 1.7]); p[a] = 0.5 * k
            q = p.copy(); q[a] = np.nextafter(p[a], -np.inf)
            f += [p, q]
    for cell in (0.0, 0.5):
        c[f"faces_cell{cell}"] = dict(A=np.array(f), B=B, cell=cell)
    for off in (-4.0e5, 4.0e5):
        c[f"offset{off:+.0e}"] = dict(A=scan(1025, 20) + off, B=scan(1025, 21) + off)
    # non-finite input
    A, B = scan(300, 22), scan(300, 23)
    for r, (col, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf))):
        A[10 + 70 * r, col] = v; B[5 + 90 * r, col] = v
    B[299] = np.nan
    c["nonfinite"] = dict(A=A, B=B)
    # a dropped target would have been the nearest of every query
    B = scan(65, 24); B[0] = [0.0, 0.0, np.nan]
    c["nonfinite_nearest"] = dict(A=np.zeros((3, 3)) + B[1] * 1e-3, B=B)
    c["all_targets_nonfinite"] = dict(A=scan(65, 25), B=np.full((7, 3), np.inf))
    return c


def lifted(n, seed, c):
    B = grid_points(n, seed)
    return B + np.array([0.0, 0.0, c]), B


@functools.lru_cache(maxsize=None)
def refine_cases():
    d = dict(T=None, gate=VOXEL, max_repeats=10, min_change=1e-6)
    c = {}
    a, b, raw = scan_pair(3000)
    for reps in (1, 2, 10):
        c[f"scan_3000_reps{reps}"] = dict(d, A=a, B=b, T=raw, max_repeats=reps)
    c["scan_3000_min_change_0"] = dict(d, A=a, B=b, T=raw, min_change=0.0)
    c["scan_3000_wide_gate"] = dict(d, A=a, B=b, T=raw, gate=1.0)
    for n in (1, 2, 64, 257, 1025, 2049):
        A, B = lifted(n, 70 + n, 0.25)
        c[f"lifted_{n}"] = dict(d, A=A, B=B, expect=dict(status=2, repeats=2, dz=-0.25, n_valid=n))
    A, B = lifted(1025, 80, 1e-7)
    c["lifted_1e-7"] = dict(d, A=A, B=B, expect=dict(status=0, repeats=1, n_valid=1025))
    A, B = lifted(257, 81, 0.125)
    c["no_valid_pair"] = dict(d, A=A + np.array([0.4, 0.0, 0.0]), B=B, expect=dict(status=1, repeats=1, dz=0.0, n_valid=0))
    c["empty_source"] = dict(d, A=np.zeros((0, 3)), B=B, expect=dict(status=1, repeats=1, dz=0.0, n_valid=0))
    c["empty_target"] = dict(d, A=A, B=np.zeros((0, 3)), expect=dict(status=1, repeats=1, dz=0.0, n_valid=0))
    rng = np.random.default_rng(82)
    B = grid_points(1025, 82)
    for tag, share, status in (("most", 0.6, 2), ("half_even", None, 2), ("few", 0.1, 0)):
        m = len(B) - 1 if share is None else len(B)                      # half_even: 1024 pairs, exactly 512 of them coincide
        z = rng.normal(scale=0.05, size=m) + 0.1
        z[rng.permutation(m)[: m // 2 if share is None else int(share * m)]] = 0.0
        A = B[:m].copy(); A[:, 2] = A[:, 2] + z
        c[f"coincide_{tag}"] = dict(d, A=A, B=B, expect=dict(status=status))
    # the valid pairs valid by a hair: xy distance exactly the gate (3-4-5 scaled), one ulp more
    B = grid_points(64, 83, step=4.0)
    A = B + np.array([0.1875, 0.25, 0.5]); A[::2, 1] = np.nextafter(A[::2, 1], np.inf)
    c["on_the_gate"] = dict(d, A=A, B=B, gate=0.3125)
    a2, b2, raw2 = scan_pair(3000)
    c["T_identity"] = dict(d, A=overlap_cpu.transform(a2, raw2), B=b2, T=np.eye(4))
    c["T_null"] = dict(d, A=overlap_cpu.transform(a2, raw2), B=b2, T=None)
    A, B = scan(700, 84), scan(700, 85); A[3, 0] = np.nan; B[5, 2] = np.inf; B[6, 1] = np.nan
    c["nonfinite"] = dict(d, A=A, B=B, gate=1.0)
    return c
