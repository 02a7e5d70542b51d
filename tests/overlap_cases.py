"""Clouds and pairs for the tests of lr_voxel_mean / lr_overlap (csrc/lr_overlap.hip), built from seeds: the smallest at which each
kernel can go wrong.  Shared by tests/test_overlap_cpu.py, tests/test_gpu_overlap.py and tests/golden/make_golden_overlap.py.

cloud cases: dict name -> (X [n,3] float64, voxel, T or None).  pair cases: dict name -> dict(A, B, T, voxel, radius)."""
import functools
import hashlib

import numpy as np

from tests import overlap_cpu

SIZES = (0, 1, 2, 255, 256, 257, 1025, 20000)
SEARCH_EDGE = 1.0 + 2.0 ** -16          # the search grid's cells are this much wider than r (csrc/lr_overlap.hip)


def rigid(seed, angle_scale=1.0, shift=20.0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4); q[0] += 4.0 / angle_scale; q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-shift, shift, size=3)
    return T


ROT90 = np.array([[0.0, -1.0, 0.0, 3.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])     # exact entries


def scan(n, seed, radius=30.0):
    """A LiDAR-like cloud: a disc of ground with relief and a few walls, negative coordinates on every axis."""
    rng = np.random.default_rng(seed)
    rad = radius * np.sqrt(rng.uniform(size=n)); phi = rng.uniform(0, 2 * np.pi, size=n)
    x, y = rad * np.cos(phi), rad * np.sin(phi)
    z = 0.3 * np.sin(0.2 * x) * np.cos(0.15 * y) - 1.7 + rng.normal(scale=0.02, size=n)
    wall = rng.uniform(size=n) < 0.3
    z[wall] += rng.uniform(0, 4, size=int(wall.sum()))
    x[wall] = np.round(x[wall] / 7.0) * 7.0 + rng.normal(scale=0.05, size=int(wall.sum()))
    return np.stack([x, y, z], axis=1)


def lattice(n, step, seed):
    """n points, every one in a cell of its own (step >= 2 voxels apart), shuffled; the origin cell is among them."""
    m = int(np.ceil(n ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 3)[:max(n, 1)]
    g = g[np.random.default_rng(seed).permutation(len(g))][:n]
    return g.astype(np.float64) * step - 11.0 * step


def long_segment(seed=5):
    """One cell (voxel 1e6) holding 3000 points of magnitudes 1e-8 .. 4e5 among 1000 singletons in cells of their own."""
    rng = np.random.default_rng(seed)
    heavy = np.sign(rng.normal(size=(3000, 3))) * 10.0 ** rng.uniform(-8, 5.6, size=(3000, 3))
    heavy[0] = -4.0e5                                                   # the cloud's minimum: the heavy cell is [-9e5, 1e5)
    heavy = np.clip(heavy, -4.0e5, 0.9e5)
    single = (np.arange(1, 1001)[:, None] * np.array([1.0, 0.0, 0.0]) + rng.integers(1, 50, size=(1000, 3)) * np.array([0.0, 1.0, 1.0])) * 1.0e6
    X = np.concatenate([heavy, single])
    X = X[rng.permutation(len(X))]
    return X, 1.0e6


def _hash(k):
    k = np.asarray(k, np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33)); k = k * np.uint64(0xff51afd7ed558ccd); k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xc4ceb9fe1a85ec53); k = k ^ (k >> np.uint64(33))
    return k & np.uint64(0xffffffff)


def colliding(n=256):
    """n points in distinct cells whose packed keys share the low 10 bits of the table's hash: one probe chain (the table has 1024 slots)."""
    g = np.stack(np.meshgrid(np.arange(80), np.arange(80), np.arange(80), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.uint64)
    key = (g[:, 0] << np.uint64(42)) | (g[:, 1] << np.uint64(21)) | g[:, 2]
    h = _hash(key) & np.uint64(1023)
    pick = np.flatnonzero(h == h[0])[:n]                                # includes cell (0, 0, 0): lo = 0, so cell = lattice index
    assert len(pick) == n
    return g[pick].astype(np.float64)


def faces(base, voxel):
    """Points exactly on cell faces, lo + (k + 0.5) voxel on each axis, each with its neighbour one ulp below; base is the cloud's minimum."""
    base = np.asarray(base, np.float64)
    pts = [base.copy()]
    for a in range(3):
        for k in range(6):
            p = base.copy(); p[a] = base[a] + (k + 0.5) * voxel
            q = p.copy(); q[a] = np.nextafter(p[a], -np.inf)
            pts += [p, q]
    return np.array(pts)


@functools.lru_cache(maxsize=None)
def cloud_cases():
    c = {}
    for n in SIZES:
        c[f"scan_{n}_v1"] = (scan(n, 100 + n), 1.0, None)
        c[f"scan_{n}_v0.3"] = (scan(n, 200 + n), 0.3, None)
    for n in (257, 1025, 20000):
        c[f"one_cell_{n}"] = (np.random.default_rng(n).uniform(0.1, 0.4, size=(n, 3)) - 3.0, 1.0, None)
        c[f"own_cell_{n}"] = (lattice(n, 2.0, n), 1.0, None)
    c["long_segment"] = long_segment() + (None,)
    c["colliding_256"] = (colliding(), 1.0, None)
    for voxel in (1.0, 0.5, 0.25):
        for tag, base in (("origin", (0.0, 0.0, 0.0)), ("neg", (-100.25, -50.5, -7.75)), ("far_neg", (-4.0e5, -4.0e5, -4.0e5)), ("far_pos", (4.0e5, 4.0e5, 4.0e5))):
            c[f"faces_{tag}_v{voxel}"] = (faces(base, voxel), voxel, None)
    for off in (-4.0e5, 4.0e5):
        c[f"scan_1025_v0.3_off{off:+.0e}"] = (scan(1025, 7) + off, 0.3, None)
    hi = 2.0 ** 21 - 0.5
    c["extent_under"] = (np.array([[0.0, 0.0, 0.0], [np.nextafter(hi, 0.0), 1.0, 2.0], [5.0, 5.0, 5.0]]), 1.0, None)
    c["extent_at"] = (np.array([[0.0, 0.0, 0.0], [1.0, hi, 2.0], [5.0, 5.0, 5.0]]), 1.0, None)
    X = scan(300, 9)
    for tag, rows in (("first", [0]), ("last", [299]), ("middle", [150, 151]), ("many", [0, 7, 150, 298, 299])):
        Y = X.copy()
        for j, r in enumerate(rows):
            Y[r, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
        c[f"dropped_{tag}"] = (Y, 1.0, None)
    c["dropped_all"] = (np.full((5, 3), np.nan), 1.0, None)
    c["T_rot90"] = (scan(1025, 11), 1.0, ROT90)
    c["T_rigid"] = (scan(1025, 12), 0.3, rigid(12))
    c["T_identity"] = (scan(1025, 13), 0.3, np.eye(4))
    c["T_none"] = (scan(1025, 13), 0.3, None)
    c["T_inf"] = (np.abs(scan(257, 14)) * np.array([1.0e306, 1.0, 1.0]), 1.0e305, np.diag([100.0, 1.0, 1.0, 1.0]))      # the transform overflows some points
    return c


def partner_pair(seed, n0, n1, T=None, voxel=1.0, keep=0.6, noise=0.02):
    """A: a scan; B: part of A moved by T (when given) plus points elsewhere -- an overlap strictly between 0 and 1."""
    rng = np.random.default_rng(seed)
    A = scan(n0, seed)
    if n0 == 0 or n1 == 0:
        return dict(A=A, B=scan(n1, seed + 1), T=T, voxel=voxel, radius=0.0)
    src = A[rng.integers(0, n0, size=n1)]
    near = rng.uniform(size=n1) < keep
    B = overlap_cpu.transform(src, T) + rng.normal(scale=noise, size=(n1, 3))
    B[~near] += np.array([70.0, 10.0, 0.0])
    return dict(A=A, B=B, T=T, voxel=voxel, radius=0.0)


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The pairs the reference's own overlap_fraction / calc_GT_overlap are recorded on (tests/golden/g17_overlap.npz)."""
    c = {"g_none_257": partner_pair(31, 257, 300), "g_none_5000": partner_pair(32, 5000, 4000),
         "g_rot90_1025": partner_pair(33, 1025, 999, ROT90), "g_rigid_5000": partner_pair(34, 5000, 6000, rigid(34, 0.3)),
         "g_rigid_20000": partner_pair(35, 20000, 20000, rigid(35)), "g_rigid_sparse": partner_pair(36, 3000, 500, rigid(36), keep=0.9)}
    for name, p in c.items():
        if p["T"] is not None:
            check_margins(p, name)
    return c


def check_margins(p, name, rel=1e-9):
    """With T != I the reference's own transform may differ from C1 in the last bit: no cell coordinate may lie within rel of an integer
    and no centroid distance within rel of r."""
    a, b = overlap_cpu.voxel_mean(p["A"], p["voxel"], p["T"]), overlap_cpu.voxel_mean(p["B"], p["voxel"])
    P = overlap_cpu.transform(p["A"], p["T"])
    q, _, _ = overlap_cpu.cells(P, p["voxel"])
    assert (np.abs(q - np.round(q)) > rel * np.maximum(1.0, np.abs(q))).all(), f"{name}: a cell coordinate sits on a face"
    r = overlap_cpu.radius_of(p["voxel"], p["radius"])
    i, j = overlap_cpu.candidate_pairs(a["cent"], b["cent"], r)
    d = overlap_cpu.dist(a["cent"][i], b["cent"][j])
    assert (np.abs(d - r) > rel * r).all(), f"{name}: a centroid distance sits on the radius"


def _pt(*xyz):
    return np.array([xyz], np.float64)


@functools.lru_cache(maxsize=None)
def search_cases():
    """One-point-per-cell clouds at voxel 1 (the centroids are the points).  expect: n_overlap by construction."""
    c = {}
    one, tiny = np.nextafter(1.0, 0.0), 1e-200
    a = _pt(0.0, 0.0, 0.0)                                              # (the offsets below are then the partner's exact coordinates)
    for name, off, expect in (("on_radius", (1.0, 1.0, 0.0), 0), ("inside_x", (one, 1.0, 0.0), 1), ("inside_y", (1.0, one, 0.0), 1),
                              ("on_radius_tiny_z", (1.0, 1.0, tiny), 0), ("two_cells_away", (2.9, 0.0, 0.0), 0)):
        c[name] = dict(A=a, B=a + np.array(off), T=None, voxel=1.0, radius=0.0, expect=expect)
    a = _pt(0.25, -3.5, 7.0)
    r = overlap_cpu.radius_of(1.0)
    g = r * SEARCH_EDGE
    k = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) == (0, 0, 0):
                    continue
                d = np.array([dx, dy, dz], np.float64)
                # lone partner: the source lies below the target's origin on the axes with d > 0 (negative grid indices)
                c[f"lone_{k}"] = dict(A=a, B=a + 0.8 * d, T=None, voxel=1.0, radius=0.0, expect=1, d=(dx, dy, dz))
                # anchored target: its origin is the anchor's; the source sits in the middle of grid cell 35 on every axis
                anchor = np.array([-50.0, -50.0, -50.0])
                mid = anchor - 0.5 + 35.5 * g
                c[f"anchored_{k}"] = dict(A=mid[None, :], B=np.array([anchor, mid + 0.8 * d]), T=None, voxel=1.0, radius=0.0, expect=1, d=(dx, dy, dz), g=g)
                k += 1
    c["radius_half"] = dict(A=a, B=np.concatenate([a + np.array([0.49, 0, 0]), a + np.array([0, 20.0, 0])]), T=None, voxel=1.0, radius=0.5, expect=1)
    c["radius_half_out"] = dict(A=a, B=a + np.array([0.5, 0, 0]), T=None, voxel=1.0, radius=0.5, expect=0)
    c["radius_three"] = dict(A=np.concatenate([a, a + np.array([0, 40.0, 0])]), B=a + np.array([2.0, 2.0, 1.0 - 1e-9]), T=None, voxel=1.0, radius=3.0, expect=1)
    ring = np.array([[0.9, 0, 0], [-0.9, 0, 0], [0, 0.9, 0], [0, -0.9, 0]])
    c["fewer_targets_than_hits"] = dict(A=a + ring, B=a.copy(), T=None, voxel=1.0, radius=0.0, expect=4)                 # n / |B_| = 4 > frac = 1
    c["more_targets"] = dict(A=a + ring, B=np.concatenate([a, a + 30.0 + 3.0 * np.arange(9)[:, None]]), T=None, voxel=1.0, radius=0.0, expect=4)   # frac_sym = 4 / 10
    return c


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """5 ragged pairs, T null for some."""
    return (partner_pair(41, 0, 300), partner_pair(42, 1, 1), partner_pair(43, 257, 255, ROT90),
            partner_pair(44, 5000, 4097, rigid(44, 0.3), voxel=1.0), partner_pair(45, 20000, 19999))


def checksum(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        x = np.zeros(0) if x is None else np.ascontiguousarray(x, np.float64)
        h.update(str(x.shape).encode()); h.update(x.tobytes())
    return h.hexdigest()
