"""Clouds for the tests of lr_symicp / lr_normals2 (csrc/lr_symicp.hip), built from seeds: the smallest at which each kernel can go
wrong.  Shared by tests/test_symicp_cpu.py and tests/test_gpu_symicp.py.

symicp cases: dict name -> dict(A, nA, B, nB, params[, expect]); expect holds fields of the result block and `pairs0`, the accepted pairs
of iteration 0."""
import functools

import numpy as np

from tests.bbrf_cases import _near_pair, small_motion, unit_normals, z_normals
from tests.overlap_cases import scan
from tests.refine_z_cases import grid_points

SIZES = (0, 1, 5, 6, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049)       # the 16-term segment, the 64-lane fold, the run of 1024
PARTNERS = (17, 1025)                                                      # every size against itself, these two, and these two against it
TIGHT = dict(eps_rot=1e-300, eps_trans=1e-300)                             # never converges unless the step is exactly zero


def size_pairs():
    out = []
    for n in SIZES:
        for pair in [(n, n)] + [(n, m) for m in PARTNERS] + [(m, n) for m in PARTNERS]:
            if pair not in out:
                out.append(pair)
    return out


def _case(A, B, nA, nB, **params):
    f = lambda X: np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    return dict(A=f(A), B=f(B), nA=f(nA), nB=f(nB), params=params)


def _index_normals(n0, n1, seed, tilt=0.02):
    """Generic unit normals by index: point k of either cloud has (nearly) the same one, so the pairs (k, k) pass min_cos."""
    base = unit_normals(max(n0, n1, 1), seed)
    nb = base[:n1] + tilt * unit_normals(max(n1, 1), seed + 1)[:n1]
    return base[:n0].copy(), nb / np.linalg.norm(nb, axis=1)[:, None] if n1 else nb


def near_case(n0, n1, seed, noise=0.01, **params):
    A, B = _near_pair(n0, n1, seed, noise)
    nA, nB = _index_normals(n0, n1, seed + 7)
    return _case(A, B, nA, nB, **params)


@functools.lru_cache(maxsize=None)
def size_cases():
    return {f"size_{n0}_{n1}": near_case(n0, n1, 900 + 16 * n0 + n1, n_iter=3, **TIGHT) for n0, n1 in size_pairs()}


def _regular(k, seed):
    """k well-separated pairs (A on a lattice of step 4 of multiples of 1/1024, B a small generic offset away) with common generic
    normals: a regular 6 x 6 system on their own."""
    A = grid_points(k, seed, step=4.0)
    rng = np.random.default_rng(seed + 1)
    B = A + np.floor(rng.uniform(-0.05, 0.05, size=(k, 3)) * 1024.0) / 1024.0
    n = unit_normals(k, seed + 2)
    return A, B, n, n.copy()


def _with(base, A=(), B=(), nA=(), nB=()):
    """The regular pairs of `base` followed by extra points."""
    cat = lambda X, Y: np.concatenate([X, np.asarray(Y, np.float64).reshape(-1, 3)])
    return cat(base[0], A), cat(base[1], B), cat(base[2], nA), cat(base[3], nB)


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """One iteration from the identity: B' = B exactly, so every decision of Y3 is made on the numbers written here."""
    c = {}
    reg = _regular(12, 700)
    far = np.array([400.0, 0.0, 0.0])
    up = np.array([0.0, 0.0, 1.0])
    # d.d == fl(max_dist max_dist) = 0.25 is accepted; 0.25 + 2^-54, one ulp above, is rejected
    for name, off, pairs in (("dist_equal", [0.5, 0.0, 0.0], 13), ("dist_ulp_above", [0.5, 2.0 ** -27, 0.0], 12)):
        c[name] = _case(*_with(reg, A=[far], B=[far + off], nA=[up], nB=[up]), n_iter=1, max_dist=0.5)
        c[name]["expect"] = dict(pairs0=pairs)
    # |dot| == min_cos = 0.75 is accepted, either sign; one ulp below is rejected
    for name, nz, pairs in (("cos_equal", 0.75, 13), ("cos_equal_negative", -0.75, 13), ("cos_ulp_below", np.nextafter(0.75, 0.0), 12),
                            ("cos_ulp_below_negative", -np.nextafter(0.75, 0.0), 12)):
        c[name] = _case(*_with(reg, A=[far], B=[far + [0.125, 0.0, 0.0]], nA=[up], nB=[[0.0, 0.5, nz]]), n_iter=1, min_cos=0.75)
        c[name]["expect"] = dict(pairs0=pairs)
    # dot > 0, < 0 and == 0 (s = +1), all accepted at min_cos 0
    ex = np.array([[400.0, 0.0, 0.0], [400.0, 8.0, 0.0], [400.0, 16.0, 0.0]])
    c["dot_signs"] = _case(*_with(reg, A=ex, B=ex + [0.125, 0.0, 0.0625], nA=[up, up, up], nB=[up, -up, [1.0, 0.0, 0.0]]), n_iter=1, min_cos=0.0)
    c["dot_signs"]["expect"] = dict(pairs0=15)
    # a backward-only pair: B_12 is the second-nearest B of A_0, so r_12 = 0 and f_0 = 0 != 12; the 12 mutual pairs count once
    A, B, nA, nB = _with(reg, B=[reg[0][0] + [0.25, 0.0, 0.0]], nB=[reg[2][0]])
    c["backward_only"] = _case(A, B, nA, nB, n_iter=1)
    c["backward_only"]["expect"] = dict(pairs0=13)
    c["mutual_once"] = _case(*reg, n_iter=1)
    c["mutual_once"]["expect"] = dict(pairs0=12)
    return c


def three_planes(n, seed):
    """n points on the planes x = 0, y = 0, z = 0 (a corner), their analytic normals."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.5, 6.0, size=(n, 3))
    k = np.arange(n) % 3
    P[np.arange(n), k] = 0.0
    N = np.zeros((n, 3)); N[np.arange(n), k] = 1.0
    return P, N


@functools.lru_cache(maxsize=None)
def loop_cases():
    c = {}
    # the tree: accepted pairs on both sides of 15 / 16 and 1023 / 1024, a run without an accepted pair in either index space
    c["run_1025"] = near_case(1025, 1025, 801, noise=0.001, n_iter=3, **TIGHT)
    p = near_case(2049, 2049, 802, noise=0.001, n_iter=3, **TIGHT)
    p["A"][1024:2048] += np.array([1000.0, 0.0, 0.0])
    c["run_2049_gap_forward"] = p
    p = near_case(2049, 2049, 803, noise=0.001, n_iter=3, **TIGHT)
    p["B"][1024:2048] += np.array([1000.0, 0.0, 0.0])
    c["run_2049_gap_backward"] = p
    # more B than A around the boundaries: backward-only candidates at j >= n0
    c["backward_many"] = near_case(300, 1100, 804, n_iter=3, min_cos=0.0, max_dist=3.0, **TIGHT)
    # ties: B's points sit in the middle between lattice points of A -- the lowest index decides every candidate
    m = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    perm = np.random.default_rng(805).permutation(len(m))
    Bm = m[::2] + 0.5
    c["ties_lattice"] = _case(m[perm], Bm, unit_normals(len(m), 806), unit_normals(len(Bm), 807), n_iter=2, max_dist=1.0, min_cos=0.0, **TIGHT)
    p = near_case(130, 140, 808, n_iter=3, **TIGHT)
    p["A"][[3, 64, 129]] = [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0, 2.0, -np.inf]]
    p["B"][[0, 77]] = [[np.inf, np.nan, 0.0], [0.0, 0.0, np.nan]]
    p["nA"][[5, 17]] = [[np.nan, 0.0, 1.0], [0.0, -np.inf, 0.0]]
    p["nB"][[9, 100]] = [[np.inf, 0.0, 0.0], [0.0, np.nan, 1.0]]
    c["nonfinite"] = p
    # status 1: five pairs; six pairs of a plane with vertical normals and all-(0, 0, 1) normals on a plane: status 2, pivots exactly 0
    c["five_pairs"] = near_case(5, 5, 809, n_iter=3)
    c["five_pairs"]["expect"] = dict(status=1, iters_run=1, pairs0=5)
    k = np.arange(300)
    G = np.stack([k % 20, k // 20, 0 * k], axis=1) + np.floor(np.random.default_rng(810).uniform(0, 0.25, size=(300, 3)) * 1024.0) / 1024.0
    G[:, 2] = 0.0
    c["plane_z_normals"] = _case(G, G + np.array([0.0625, 0.0, 0.03125]), z_normals(300), z_normals(300), n_iter=3)
    c["plane_z_normals"]["expect"] = dict(status=2, iters_run=1, pairs0=300)
    # status 3: g overflows while H stays finite.  A_0 = 0 with the normal (0, 0, 1e120); its forward candidate B_0 is rejected (normal
    # (1, 0, 0): dot 0); B_last = (0, 0, 1e80) with the normal (0, 0, 1e120) is equally far from every A, so r = 0: the row is
    # (0, 0, 0, 0, 0, 2e120) with b = -2e200, c_5 c_5 = 4e240, c_5 b = -inf
    A, B, nA, nB = _regular(40, 811)
    A[0] = 0.0; B[0] = [0.03125, 0.0, 0.0]; nA[0] = [0.0, 0.0, 1e120]; nB[0] = [1.0, 0.0, 0.0]
    A, B, nA, nB = _with((A, B, nA, nB), B=[[0.0, 0.0, 1e80]], nB=[[0.0, 0.0, 1e120]])
    c["step_overflows"] = _case(A, B, nA, nB, n_iter=3, max_dist=1e100)
    c["step_overflows"]["expect"] = dict(status=3, iters_run=1, pairs0=40)
    # convergence at iteration 0: A == B', a step of exactly zero
    A, _, nA, _ = _regular(60, 812)
    c["same"] = _case(A, A.copy(), nA, nA.copy(), n_iter=5)
    c["same"]["expect"] = dict(status=0, iters_run=1, converged=1, pairs0=60)
    # convergence in the middle of a run: a planted motion of a corner, analytic normals
    P, N = three_planes(300, 813)
    M = small_motion(814, 1.0, 0.05)
    c["planted"] = _case(P @ M[:3, :3].T + M[:3, 3], P, N @ M[:3, :3].T, N, n_iter=20, max_dist=2.0, eps_rot=1e-12, eps_trans=1e-12)
    c["planted"]["expect"] = dict(status=0, converged=1)
    c["planted"]["truth"] = M
    for k in (1, 2, 50):
        c[f"iters_{k}"] = near_case(257, 257, 815, n_iter=k, **TIGHT)
    # T_init against a pre-moved B
    p = near_case(257, 300, 816, n_iter=3, **TIGHT)
    p["T_init"] = small_motion(817, 0.3, 0.02)
    c["t_init"] = p
    return c


@functools.lru_cache(maxsize=None)
def normals_cases():
    """lr_normals2's counts: the inputs of tests/bbrf_cases.normals_cases and one cloud whose counts reach max_nn."""
    from tests import bbrf_cases
    c = dict(bbrf_cases.normals_cases())
    c["scan_counts"] = dict(X=scan(700, 820), radius=2.5, max_nn=9)
    return c
