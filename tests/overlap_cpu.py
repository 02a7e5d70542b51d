"""The contract of lr_voxel_mean / lr_overlap (include/lidarreg.h C1-C4) restated in numpy: the yardstick the device
results must equal bit for bit.  fp64 throughout; numpy's elementwise products and sums are not fused."""
import numpy as np

MAX_CELLS = 2.0 ** 21


def transform(X, T):
    """C1: p_a = ((T[a,0] x + T[a,1] y) + T[a,2] z) + T[a,3]; T None = the identity, no arithmetic."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    if T is None:
        return X.copy()
    T = np.asarray(T, np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def cells(P, voxel):
    """C2 on the kept points P: (cell coordinates as float64 [m,3] before the int cast's floor, vmb, refused)."""
    lo, hi = P.min(axis=0), P.max(axis=0)
    vmb = lo - voxel * 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        refused = bool((~((hi - vmb) / voxel < MAX_CELLS)).any())
        q = (P - vmb) / voxel
    return q, vmb, refused


def voxel_mean(X, voxel, T=None):
    """C1-C3.  dict: cent [rows,3] float64, counts, first (int32), rows, dropped, status, row_of (row of every input point, -1 dropped)."""
    voxel = float(voxel)
    with np.errstate(over="ignore", invalid="ignore"):
        P = transform(X, T)
    n = len(P)
    keep = np.isfinite(P).all(axis=1) if n else np.zeros(0, bool)
    out = dict(cent=np.zeros((0, 3)), counts=np.zeros(0, np.int32), first=np.zeros(0, np.int32), rows=0, dropped=int(n - keep.sum()),
               status=0, row_of=np.full(n, -1, np.int64), vmb=np.zeros(3))
    if not keep.any():
        out["status"] = 1
        return out
    idx = np.flatnonzero(keep)
    q, vmb, refused = cells(P[idx], voxel)
    out["vmb"] = vmb
    if refused:
        out["status"] = 2
        return out
    c = np.floor(q).astype(np.int64)
    assert (c >= 0).all() and (c < 2 ** 21).all()
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first_pos, inv = np.unique(key, return_index=True, return_inverse=True)          # first occurrence of every cell
    order = np.argsort(first_pos, kind="stable")                                         # rows by ascending first point
    row_of_unique = np.empty(len(order), np.int64); row_of_unique[order] = np.arange(len(order))
    row = row_of_unique[inv]
    rows = len(order)
    counts = np.bincount(row, minlength=rows)
    # left-to-right sums in ascending point index: round k adds the k-th point of every cell that has one
    by_row = np.argsort(row, kind="stable")
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    s = np.zeros((rows, 3))
    Pk = P[idx]
    with np.errstate(over="ignore", invalid="ignore"):
        live = np.arange(rows)
        for k in range(int(counts.max())):
            live = live[counts[live] > k]
            s[live] += Pk[by_row[start[live] + k]]
        cent = s / counts[:, None].astype(np.float64)
    out.update(cent=cent, counts=counts.astype(np.int32), first=idx[first_pos[order]].astype(np.int32), rows=rows)
    out["row_of"][idx] = row
    return out


def radius_of(voxel, radius=0.0):
    return float(np.sqrt(2) * voxel) if radius == 0 else float(radius)


def dist(a, b):
    """C4's distance of centroid rows a, b (broadcast)."""
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def candidate_pairs(A_, B_, r):
    """(i, j) index arrays of every pair whose true distance can be below r (a generous superset), from a k-d tree."""
    from scipy.spatial import cKDTree
    if len(A_) == 0 or len(B_) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ok_a, ok_b = np.isfinite(A_).all(axis=1), np.isfinite(B_).all(axis=1)
    ia, ib = np.flatnonzero(ok_a), np.flatnonzero(ok_b)
    if len(ia) == 0 or len(ib) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    lists = cKDTree(B_[ib]).query_ball_point(A_[ia], r * (1 + 1e-6))
    i = np.repeat(ia, [len(l) for l in lists])
    j = ib[np.concatenate([np.asarray(l, np.int64) for l in lists])] if len(i) else np.zeros(0, np.int64)
    return i, j


def count_overlap(A_, B_, r):
    """C4: #{ a : exists b with dist(a, b) < r }, the distance in the contract's arithmetic over a superset of the close pairs."""
    i, j = candidate_pairs(A_, B_, r)
    hit = np.zeros(len(A_), bool)
    if len(i):
        hit[i[dist(A_[i], B_[j]) < r]] = True
    return int(hit.sum())


def overlap(A, B, T=None, voxel=1.0, radius=0.0):
    """C4: the lr_overlap_result as a dict."""
    a, b = voxel_mean(A, voxel, T), voxel_mean(B, voxel, None)
    status = 2 if 2 in (a["status"], b["status"]) else (1 if a["status"] or b["status"] else 0)
    out = dict(status=status, n0_ds=a["rows"], n1_ds=b["rows"], n_overlap=0, n0_dropped=a["dropped"], n1_dropped=b["dropped"], frac=0.0, frac_sym=0.0)
    if status == 0:
        n = count_overlap(a["cent"], b["cent"], radius_of(voxel, radius))
        frac = float(n) / a["rows"]
        out.update(n_overlap=n, frac=frac, frac_sym=min(frac, float(n) / b["rows"]))
    return out
