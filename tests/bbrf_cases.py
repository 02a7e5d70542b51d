"""Clouds for the tests of lr_bbrf / lr_normals (csrc/lr_bbrf.hip), built from seeds: the smallest at which each kernel can go wrong.
Shared by tests/test_bbrf_cpu.py, tests/test_gpu_bbrf.py and tests/golden/make_golden_bbrf.py.

bbrf cases: dict name -> dict(A, nA, B, nB, params[, expect]).  normals cases: dict name -> dict(X, radius, max_nn)."""
import functools

import numpy as np

from tests import bbrf_cpu, overlap_cpu, refine_z_cases, refine_z_cpu
from tests.overlap_cases import checksum, scan  # noqa: F401  (checksum: re-exported for the fixture)
from tests.refine_z_cases import grid_points

SIZES = (0, 1, 2, 63, 64, 65, 257, 1025)
VOXEL = 0.3
MIN_GAP = 1e-8          # between the nearest and the second-nearest distance of every query of a golden case at iteration 0
LOSS_GAP = 1e-5         # between the two lowest losses of a golden case


def small_motion(seed, deg, shift):
    """A rigid motion of `deg` degrees about a seeded axis with a seeded shift of length `shift`."""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    a = np.radians(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    t = rng.normal(size=3); T[:3, 3] = shift * t / np.linalg.norm(t)
    return T


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def z_normals(n):
    v = np.zeros((n, 3)); v[:, 2] = 1.0
    return v


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The pairs the reference's own BBR_F_step is recorded on (tests/golden/g19_bbrf.npz)."""
    a, b, raw = refine_z_cases.scan_pair(3000)
    T = raw.copy(); T[2, 3] -= refine_z_cases.Z_OFF
    A = overlap_cpu.transform(a, small_motion(71, 0.8, 0.05) @ T)
    c = {"g_scan_z": dict(A=A, nA=z_normals(len(A)), B=b, nB=z_normals(len(b))),
         "g_scan_generic": dict(A=A, nA=unit_normals(len(A), 72), B=b, nB=unit_normals(len(b), 73))}
    B = overlap_cpu.voxel_mean(scan(500, 74), VOXEL)["cent"]
    rng = np.random.default_rng(74)
    keep = rng.permutation(len(B))[: len(B) * 3 // 4]
    A = overlap_cpu.transform(B[keep] + rng.normal(scale=0.01, size=(len(keep), 3)), small_motion(75, 0.5, 0.04))
    c["g_small"] = dict(A=A, nA=unit_normals(len(A), 76), B=B, nB=unit_normals(len(B), 77))
    for p in c.values():
        p["params"] = {}
    return c


@functools.lru_cache(maxsize=None)
def golden_run(name):
    """The restatement on a golden case, once per process: (result, log, trace)."""
    p, trace = golden_cases()[name], []
    r, log = bbrf_cpu.bbrf(p["A"], p["nA"], p["B"], p["nB"], trace=trace)
    return r, log, trace


def check_conditions(p):
    """At iteration 0 the nearest and the second-nearest distance of every query lie at least MIN_GAP apart, in both directions: the
    reference's expanded-form distance cannot flip a neighbour.  Returns the least gap."""
    gaps = []
    for q, t in ((p["A"], p["B"]), (p["B"], p["A"])):
        d, _, _, d2 = refine_z_cpu.nn(q, t, second=True)
        gaps.append(float((d2 - d).min()))
    assert min(gaps) >= MIN_GAP, f"two points are equally near a query ({min(gaps):.2e})"
    return min(gaps)


def _near_pair(n0, n1, seed, noise=0.01):
    base = scan(max(n0, n1, 1), seed)
    rng = np.random.default_rng(seed + 1)
    A = base[:n0].copy()
    B = base[:n1] + rng.normal(scale=noise, size=(n1, 3)) + np.array([0.02, -0.01, 0.03])
    return A, B


def _case(A, B, nA=None, nB=None, seed=0, **params):
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
    return dict(A=A, B=B, nA=unit_normals(len(A), seed + 11) if nA is None else nA, nB=unit_normals(len(B), seed + 12) if nB is None else nB,
                params=params)


@functools.lru_cache(maxsize=None)
def size_cases():
    return {f"size_{n0}_{n1}": _case(*_near_pair(n0, n1, 400 + 16 * n0 + n1), seed=n0 + n1, n_iter=3) for n0 in SIZES for n1 in SIZES}


@functools.lru_cache(maxsize=None)
def loop_cases():
    c = {}
    # the two-level sum: pairs on both sides of the 1024 boundary; a run without a pair (its points lie far from every target point)
    A, B = _near_pair(1025, 1025, 501, noise=0.001)
    c["run_1025"] = _case(A, B, seed=1, n_iter=3)
    A, B = _near_pair(2049, 2049, 502, noise=0.001)
    A[1024:2048] += np.array([1000.0, 0.0, 0.0])
    c["run_2049_gap"] = _case(A, B, seed=2, n_iter=3)
    A, B = _near_pair(257, 300, 503)
    c["z_normals"] = _case(A, B, z_normals(257), z_normals(300), n_iter=3)
    nB = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])[np.arange(300) % 3]
    c["normal_signs"] = _case(A, B, z_normals(257), nB, n_iter=3)
    G = grid_points(300, 504)
    c["same"] = _case(G, G.copy(), z_normals(300), z_normals(300), n_iter=3)
    c["quarter"] = _case(G + np.array([0.0, 0.0, 0.25]), G, z_normals(300), z_normals(300), n_iter=1)
    # ties: B's points sit in the middle between lattice points of A -- the lowest index decides every buddy
    m = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    perm = np.random.default_rng(505).permutation(len(m))
    c["ties_lattice"] = _case(m[perm], m[::2] + 0.5, seed=5, n_iter=2)
    A, B = _near_pair(130, 140, 506)
    A[[3, 64, 129]] = [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0, 2.0, -np.inf]]
    B[[0, 77]] = [[np.inf, np.nan, 0.0], [0.0, 0.0, np.nan]]
    c["nonfinite"] = _case(A, B, seed=6, n_iter=3)
    # A lies 1.5e308 above B and every step is 0.9e308 long (beta 0): the second step overflows B'z -- no finite B', no pair
    A, B = _near_pair(65, 65, 507)
    A[:, 2] = 1.7e308; B[:, 2] = 0.2e308
    q = np.zeros((65, 3)); q[:, 2] = 0.25
    c["no_pair_at_2"] = _case(A, B, q, q.copy(), n_iter=5, trans_lr=0.9e308, beta1=0.0, beta2=0.0)
    c["no_pair_at_2"]["expect"] = dict(status=1, iters_run=3, best_iter=1)
    A, B = _near_pair(257, 257, 508)
    c["angle_leaves"] = _case(A, B, seed=8, n_iter=10, angles_lr=0.3)
    c["angle_leaves"]["expect"] = dict(status=3, iters_run=2)
    for k in (1, 2):
        c[f"iters_{k}"] = _case(A, B, seed=9, n_iter=k)
    return c


@functools.lru_cache(maxsize=None)
def normals_cases():
    c = {}
    for n in (0, 1, 2, 3, 64, 65, 1025):
        c[f"size_{n}"] = dict(X=scan(n, 600 + n), radius=1.5, max_nn=13)
    X = scan(300, 610)
    c["all_default"] = dict(X=X, radius=0.01, max_nn=13)
    # exactly 2 and exactly 3 neighbours: triples (and couples) 0.125 apart, the groups 10 apart
    g = np.arange(40)[:, None] * np.array([10.0, 0.0, 0.0])
    two = np.concatenate([g, g + np.array([0.0, 0.125, 0.0])])
    c["exactly_2"] = dict(X=two, radius=0.25, max_nn=13)
    c["exactly_3"] = dict(X=np.concatenate([two, g + np.array([0.0, 0.0, 0.125])]), radius=0.25, max_nn=13)
    # more candidates than max_nn, ties at the cut: an integer lattice, radius 1 admits the point and its 6 neighbours, max_nn 4
    m = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    c["ties_at_cut"] = dict(X=m[np.random.default_rng(611).permutation(len(m))], radius=1.0, max_nn=4)
    c["many_candidates"] = dict(X=np.random.default_rng(612).uniform(0, 2, size=(400, 3)), radius=0.5, max_nn=32)
    rng = np.random.default_rng(613)
    uv = rng.uniform(-2, 2, size=(500, 2))
    e1, e2 = np.array([1.0, 2.0, 2.0]) / 3.0, np.array([2.0, 1.0, -2.0]) / 3.0
    c["plane"] = dict(X=uv[:, :1] * e1 + uv[:, 1:] * e2 + np.array([3.0, -1.0, 0.5]), radius=0.6, max_nn=13, plane=np.array([2.0, -2.0, 1.0]) / 3.0)
    X = scan(200, 614)
    X[[0, 50, 199]] = [[np.nan, 0.0, 0.0], [0.0, -np.inf, 0.0], [np.inf, np.inf, np.inf]]
    c["nonfinite"] = dict(X=X, radius=2.0, max_nn=13)
    c["all_nonfinite"] = dict(X=np.full((5, 3), np.nan), radius=1.0, max_nn=13)
    return c
