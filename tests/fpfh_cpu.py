"""The FPFH contract F1..F6 (include/lidarreg.h) restated in numpy: what lr_fpfh must equal bit for bit in float64.  TEST
INFRASTRUCTURE ONLY.  Open3D 0.13's compute_fpfh_feature is not vendored; its algorithm is upstream-recalled, and this contract is the
specification (tests/test_fpfh_cpu.py holds a literal restatement of the recalled algorithm -- acos, atan2, repeated += -- and measures
how far the two are apart).  Every operation is a single IEEE float64 operation in a written order; no libm call beyond sqrt."""
import numpy as np

from tests import bbrf_cpu

# the ten bin edges of the angle feature, turned by pi: direction 2 pi e / 11, e = 1..10, as (cos, sin) float64 literals
EDGE_C = (0.8412535328311812, 0.41541501300188644, -0.142314838273285, -0.654860733945285, -0.9594929736144974,
          -0.9594929736144975, -0.6548607339452852, -0.14231483827328523, 0.41541501300188605, 0.8412535328311812)
EDGE_S = (0.5406408174555976, 0.9096319953545183, 0.9898214418809328, 0.7557495743542583, 0.28173255684142967,
          -0.2817325568414294, -0.7557495743542582, -0.9898214418809327, -0.9096319953545186, -0.5406408174555974)


def angle_bin(y, x):
    """F3: the bin floor(11 (atan2(y, x) + pi) / (2 pi)), clamped to 0..10, without the angle: (-x, -y) has the angle theta + pi in
    [0, 2 pi); in the upper half-plane it has passed edge e <= 5 when cross(edge, (-x, -y)) >= 0, in the lower one all of those and edge
    e >= 6 under the same test.  theta = pi exactly (y = +0, x < 0) is bin 10, -pi (y = -0) bin 0, (0, 0) and anything unordered bin 5."""
    y = np.asarray(y, np.float64); x = np.asarray(x, np.float64)
    xr, yr = -x, -y
    with np.errstate(all="ignore"):
        passed = [(EDGE_C[e] * yr - EDGE_S[e] * xr) >= 0.0 for e in range(10)]
    up = sum(p.astype(np.int64) for p in passed[:5])
    lo = 5 + sum(p.astype(np.int64) for p in passed[5:])
    flat = np.where((y == 0.0) & (x < 0.0), np.where(np.signbit(y), 0, 10), 5)
    return np.where(y < 0.0, up, np.where(y > 0.0, lo, flat))


def unit_bin(f):
    """F3: floor(11 (f + 1) 0.5) clamped to 0..10, as the number of whole steps reached (a NaN reaches none)."""
    with np.errstate(all="ignore"):
        t = (11.0 * (np.asarray(f, np.float64) + 1.0)) * 0.5
        return sum((t >= float(e)).astype(np.int64) for e in range(1, 11))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_bins(p1, n1, p2, n2):
    """F2 + F3 for arrays of pairs [m,3]: the three bins (angle, f2, f3)."""
    with np.errstate(all="ignore"):
        d = p2 - p1
        L = np.sqrt(dot3(d, d))
        a1 = dot3(n1, d) / L
        a2 = dot3(n2, d) / L
        swap = np.abs(a1) < np.abs(a2)
        s3 = swap[:, None]
        N1 = np.where(s3, n2, n1); N2 = np.where(s3, n1, n2); d = np.where(s3, -d, d)
        f3 = np.where(swap, -a2, a1)
        v = cross3(d, N1)
        vn = np.sqrt(dot3(v, v))
        v = v / vn[:, None]
        w = cross3(N1, v)
        f2 = dot3(v, N2)
        y = dot3(w, N2); x = dot3(N1, N2)
        ok = (L != 0.0) & (vn != 0.0)
    return np.where(ok, angle_bin(y, x), 5), np.where(ok, unit_bin(f2), 5), np.where(ok, unit_bin(f3), 5)


def lists(X, radius, max_nn):
    """F1: (idx int64 [n, max_nn] padded with -1, d2 float64 [n, max_nn], len int64 [n])."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    nb = bbrf_cpu.neighbours(X, radius, max_nn)
    n = len(X)
    idx = np.full((n, max_nn), -1, np.int64); d2 = np.zeros((n, max_nn)); ln = np.zeros(n, np.int64)
    for i, l in enumerate(nb):
        ln[i] = len(l)
        idx[i, :len(l)] = l
        if len(l):
            e = X[i][None, :] - X[l]
            d2[i, :len(l)] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return idx, d2, ln


def spfh(X, N, idx, ln):
    """F4: [n,33] -- integer counts per bin times 100 / k, k = len - 1."""
    n, cap = idx.shape
    rows, cols = np.nonzero((np.arange(cap)[None, :] >= 1) & (np.arange(cap)[None, :] < ln[:, None]))
    counts = np.zeros((n, 33), np.int64)
    if len(rows):
        nb = idx[rows, cols]
        b1, b2, b3 = pair_bins(X[rows], N[rows], X[nb], N[nb])
        np.add.at(counts, (rows, b1), 1); np.add.at(counts, (rows, 11 + b2), 1); np.add.at(counts, (rows, 22 + b3), 1)
    k = np.maximum(ln - 1, 1).astype(np.float64)
    return np.where((ln > 1)[:, None], counts.astype(np.float64) * (100.0 / k)[:, None], 0.0)


def scan_cloud(n_raw=40000, half=8.0, voxel=0.3, seed=51):
    """A test cloud with the density of real use: frame 0 of synth.make_scan_pair(n_raw), de-duplicated at `voxel` (the CPU restatement
    of the voxel grid), cropped to |x|, |y| < half.  (points [n,3], normals [n,3]) -- the normals by the recipe of fpfh.extract."""
    from lidarregistration_amd import synth
    from tests import overlap_cpu
    raw = synth.make_scan_pair(n_raw, seed=seed)[0]
    P = overlap_cpu.voxel_mean(raw, voxel)["cent"]
    P = np.ascontiguousarray(P[(np.abs(P[:, 0]) < half) & (np.abs(P[:, 1]) < half)])
    return P, bbrf_cpu.normals(P, 2.0 * voxel, 30)[0]


def fpfh(X, N, radius, max_nn=100):
    """(F [n,33] float64, info dict(status, dropped, zero_rows, capped))."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); N = np.ascontiguousarray(N, np.float64).reshape(-1, 3)
    n = len(X)
    idx, d2, ln = lists(X, radius, max_nn)
    S = spfh(X, N, idx, ln)
    F = np.zeros((n, 33))
    with np.errstate(all="ignore"):
        for e in range(1, int(ln.max()) if n else 0):
            use = (e < ln) & (d2[:, e] != 0.0)
            nb = np.where(use, idx[:, e], 0)
            F = np.where(use[:, None], F + S[nb] / np.where(use, d2[:, e], 1.0)[:, None], F)
        out = np.zeros((n, 33))
        for b in range(3):
            g = np.zeros(n)
            for j in range(11 * b, 11 * b + 11):
                g = g + F[:, j]
            scale = np.where(g != 0.0, 100.0 / np.where(g != 0.0, g, 1.0), 0.0)
            out[:, 11 * b:11 * b + 11] = F[:, 11 * b:11 * b + 11] * scale[:, None] + S[:, 11 * b:11 * b + 11]
    dropped = int((~np.isfinite(X).all(axis=1)).sum())
    info = dict(status=0 if n - dropped > 0 else 1, dropped=dropped, zero_rows=int((ln <= 1).sum()), capped=int((ln == max_nn).sum()))
    return out, info
