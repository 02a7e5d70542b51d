"""Correspondence sets for the spectral-matching tests (lr_sm, csrc/lr_sm.hip), built from seeds: the smallest at which each kernel can
go wrong.  Shared by tests/test_sm_cpu.py, tests/test_gpu_sm.py and tests/golden/make_golden_sm.py.

A case is a dict: name, a / b ([M,3] float32: src / tgt of the M correspondences), ratio (top_ratio), thr (inlier_threshold 0.6), kind:
    ragged   sizes around the 64-row blocks and the 4-column groups of the matvec
    kcut     K = int(M * ratio) at its rounding boundaries
    gap      the inlier count equals K: a clear gap in v at the cut (labels must equal the reference's)
    cluster  the cut runs inside the inlier cluster (labels may differ only at entries within the tolerance of the cut)
    planted  hand-made structure (see each builder)
unique_fit: the selected points determine the rotation.  golden: the reference's SM() is recorded for it (finite input, M <= 3000,
unique_fit: the hand-made collinear sets leave ties and the rotation to torch's argsort and SVD).

large_cases() (tests/test_sm_large_cpu.py, tests/test_gpu_sm_large.py, tests/golden/make_golden_sm_large.py) continues the list above
one selection pass and up to M = 32 768; cases() itself and g16_sm.npz stay as they were.
"""
import functools
import hashlib

import numpy as np

THR = 0.6


def _rigid(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, rng.uniform(-20, 20, size=3)


def synth(M, n_inl, seed, noise=0.05, extent=50.0):
    """M correspondences at LiDAR scale (100 m baselines), the first n_inl (then shuffled) follow one rigid motion up to `noise`."""
    rng = np.random.default_rng(seed)
    R, t = _rigid(rng)
    a = rng.uniform(-extent, extent, size=(M, 3))
    b = rng.uniform(-extent, extent, size=(M, 3))
    b[:n_inl] = a[:n_inl] @ R.T + t + rng.normal(scale=noise, size=(n_inl, 3))
    p = rng.permutation(M)
    inl = np.zeros(M, bool); inl[:n_inl] = True
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return a[p].astype(np.float32), b[p].astype(np.float32), inl[p], T


def _case(name, kind, a, b, ratio, golden=None, unique_fit=True, **extra):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    finite = bool(np.isfinite(a).all() and np.isfinite(b).all())
    return dict(name=name, kind=kind, a=a, b=b, ratio=float(ratio), thr=THR, unique_fit=unique_fit,
                golden=(finite and unique_fit and 0 < len(a) <= 3000) if golden is None else golden, **extra)


def line(M):
    """No two correspondences compatible: a_i = (10 i, 0, 0), b_i = (12 i, 0, 0), so d(i,j) = 2 |i - j| >= 2 > thr.  Integers: every
    operation of the compatibility chain is exact in fp32."""
    a = np.zeros((M, 3), np.float32); b = np.zeros((M, 3), np.float32)
    a[:, 0] = 10.0 * np.arange(M); b[:, 0] = 12.0 * np.arange(M)
    return a, b


def plant_neighbours(b, p):
    """Makes (p, p + 1) of line() compatible with d = 0 exactly (c = 4.5) and leaves every other d at >= 2."""
    b[p + 1, 0] = 12.0 * p + 10.0


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for M in (3, 60, 63, 64, 65, 257, 999, 1537, 2049, 4096):
        a, b, _, _ = synth(M, max(1, (3 * M) // 10), 1000 + M)
        out.append(_case(f"ragged_{M}", "ragged", a, b, 0.1))
    for M, ratio, K in ((100, 0.29, 28), (60, 0.05, 3), (30, 0.1, 3), (59, 0.05, 2), (20, 0.1, 2)):
        a, b, _, _ = synth(M, M // 2, 2000 + M)
        out.append(_case(f"kcut_{M}_{ratio}", "kcut", a, b, ratio, K=K))
    for M, n_inl, ratio in ((500, 25, 0.05), (1000, 50, 0.05), (2000, 100, 0.05)):
        a, b, _, _ = synth(M, n_inl, 3000 + M)
        out.append(_case(f"gap_{M}_{n_inl}", "gap", a, b, ratio))
    for M, n_inl, ratio in ((1000, 300, 0.1), (2000, 600, 0.05), (3000, 1200, 0.05), (1537, 700, 0.1), (4096, 2000, 0.1)):
        a, b, _, _ = synth(M, n_inl, 4000 + M)
        out.append(_case(f"cluster_{M}_{n_inl}", "cluster", a, b, ratio))
    # the only compatible partner of row 0 sits in the last column, that of the last row in the first: M = 257 is one row past four
    # row blocks and one column past 64 groups of four
    a, b = line(257); b[256, 0] = 2560.0
    out.append(_case("planted_last_column_257", "planted", a, b, 0.02, unique_fit=False, partners=(0, 256)))
    a, b = line(65); plant_neighbours(b, 63)
    out.append(_case("planted_last_row_65", "planted", a, b, 0.05, unique_fit=False, partners=(63, 64)))
    # nothing compatible at all: v stays 0, the K ties are resolved by index, status 1
    a, b = line(100)
    out.append(_case("planted_all_outliers", "planted", a, b, 0.1, unique_fit=False))
    # ten disjoint compatible pairs with c = 4.5 exactly: 20 equal v, K = 10 cuts through them
    a, b = line(100)
    for p in range(0, 100, 10):
        plant_neighbours(b, p)
    out.append(_case("planted_equal_at_cut", "planted", a, b, 0.1, unique_fit=False, expect_sel=(0, 1, 10, 11, 20, 21, 30, 31, 40, 41)))
    # a duplicated correspondence: c = 4.5 between the copies (the diagonal is decided by index, not by d = 0)
    a, b, _, _ = synth(200, 60, 5001)
    a[7] = a[3]; b[7] = b[3]
    out.append(_case("planted_duplicate", "planted", a, b, 0.1, dup=(3, 7)))
    # non-finite rows: compatibility 0 with everything (the reference propagates NaN: no golden)
    a, b, _, _ = synth(200, 60, 5002)
    a[5, 0] = np.nan; b[9, 2] = np.inf; a[77, 1] = -np.inf
    out.append(_case("planted_nonfinite", "planted", a, b, 0.1, bad=(5, 9, 77)))
    return tuple(out)


def plant_pair(b, p, q):
    """Makes (p, q), p < q, of line() compatible with d = 0 exactly by moving b_q: b_q - b_p = a_q - a_p."""
    b[q, 0] = b[p, 0] + 10.0 * (q - p)


def _planted(name, M, pairs, ratio):
    """line(M) with the disjoint partner pairs planted: 2 len(pairs) equal non-zero v (sm_cpu.planted_v), everything else exactly 0;
    expect_sel: the first K planted indices (K <= their number), else the lowest K indices."""
    a, b = line(M)
    for p, q in pairs:
        plant_pair(b, p, q)
    idx = sorted(i for pq in pairs for i in pq)
    assert len(set(idx)) == len(idx), "the planted pairs must be disjoint"
    K = int(M * ratio)
    sel = tuple(idx[:K]) if pairs else tuple(range(K))
    assert len(sel) == K
    return _case(name, "planted", a, b, ratio, golden=False, unique_fit=False, pairs=tuple(pairs), expect_sel=sel, K=K)


# the seed of each golden-backed case: the first from 6000 + M on that met the conditions tests/golden/make_golden_sm_large.py asserts
LARGE_SEEDS = {"gap_8193_409": 14193, "full_20001": 26001, "full_32768": 38768}


@functools.lru_cache(maxsize=None)
def large_cases():
    """Above one 1 024-entry selection pass and up to the accepted maximum (M = 32 768).  The planted ones have an analytic reference
    (sm_cpu.planted_v); the random ones (`large`: True) are too large to restate in a test: tests/golden/g23_sm_large.npz holds their
    fp64 eigenvector (tests/golden/make_golden_sm_large.py)."""
    out = []
    # 620 equal values; K = 310 falls inside the second selection pass, K = 465 (odd: it separates a pair) inside the third
    ties = [(p, p + 1) for p in range(0, 3100, 10)]
    out.append(_planted("planted_ties_3100_k310", 3100, ties, 0.1))
    out.append(_planted("planted_ties_3100_k465", 3100, ties, 0.15))
    # nothing compatible over three passes: the lowest 1 500 indices
    out.append(_planted("planted_zeros_2500", 2500, [], 0.6))
    # M = 3 mod 4 at the limit: the only partner of row 0 is the last row, that of row 32 765 is row 1; K = half of the planted entries
    far = [(0, 32766), (1, 32765)] + [(p, p + 1) for p in range(1000, 32767, 1000)]
    out.append(_planted("planted_limit_32767", 32767, far, (len(far) + 0.5) / 32767))
    for name, M, n_inl in (("gap_8193_409", 8193, 409), ("full_20001", 20001, 6000), ("full_32768", 32768, 9830)):
        a, b, _, _ = synth(M, n_inl, LARGE_SEEDS[name])
        out.append(_case(name, "gap" if name.startswith("gap") else "cluster", a, b, 0.05, golden=False, large=True))
    return tuple(out)


def by_name(name):
    hit = [c for c in cases() if c["name"] == name]
    return hit[0] if hit else next(c for c in large_cases() if c["name"] == name)


def checksum(c):
    h = hashlib.sha256()
    h.update(c["a"].tobytes()); h.update(c["b"].tobytes()); h.update(np.float64([c["ratio"], c["thr"]]).tobytes())
    return h.hexdigest()
