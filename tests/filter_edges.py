"""Inputs that sit ON the decision boundaries of the correspondence filters, and a plain restatement of what the
reference decides there (numpy only; no oracle, no GPU).

* ``cells_ref`` / ``waterfill_ref`` / ``select_ref`` / ``gpf_ref``: Grid_Prioritized_Filter of the reference
  (Experiments/algorithms/matching.py:100-205) written out operation by operation.  The two quadrants of a pair stay
  separate: a pair is in cell (qi, qj) only if BOTH are in [0, G).  The oracle and the kernels are held to this file and to
  the fixture ``tests/golden/g15_filter_edges.npz`` (outputs of the reference itself on the clouds built here).
* ``boundary_cloud`` / ``wide_cloud`` / ``waterfill_cases`` / ``prosac_lists``: the builders.

How the descriptors are made (``make_cloud``): every best-buddy point ``i`` of cloud 0 has a lattice code (four
coordinates, multiples of 2); cloud 1 holds two rows for it, ``A_i = code + a_i e4`` and ``B_i = code - b e4`` with
``a_i = m_i / 1024 <= 400 / 1024`` and ``b = 1023 / 1024``.  Rows of other codes are at least 2 away, so the first and second
neighbour of ``i`` are ``A_i`` and ``B_i``, ``A_i``'s neighbour in cloud 0 is ``i`` (a best buddy), and the feature-distance
ratio is ``fl(a_i / fl(b + 1e-6))``: one non-zero difference, nothing to sum, so every implementation gives the same bits and
the order of the scores inside a cell is the order of the ``m_i`` the builder hands out.  A point that is NOT a best buddy
(a "guest") sits at ``code_h + t e4`` of a host ``h`` with ``t >= 820 / 1024 > 2 a_h``: its neighbours are ``A_h`` and ``B_h``,
but ``A_h``'s neighbour is ``h``.  The NN lists are therefore the true ones (the batched entry point recomputes them).
"""
import functools
import hashlib

import numpy as np

F32 = np.float32
B_OFF = 1023            # b = B_OFF / 1024
FACTORS = (0.37, 1.0 / 3.0, 0.3, 0.7, 0.05, 1.1)


# ----------------------------------------------------------------------------- the restatement

def quads_ref(X, G):
    """matching.py:136-142 on one coordinate, every operation in float32 as torch evaluates it."""
    X = np.asarray(X, F32)
    m = X.min()
    M = X.max()
    num = (X - m).astype(F32)                       # X - m
    rng = F32(M - m)                                # M - m
    den = F32(rng + F32(1e-3))                      # M - m + EPS
    X_ = (num / den).astype(F32)                    # (X - m) / (M - m + EPS)
    prod = (F32(G) * X_).astype(F32)                # GRID_WID * X_
    return np.floor(prod)


def cells_ref(x, y, G):
    """The two quadrants of every pair (float32 arrays, NOT combined into one index)."""
    return quads_ref(x, G), quads_ref(y, G)


def sum_numpy(v):
    return v.sum()


def sum_left_to_right(v):
    return np.add.accumulate(v.ravel())[-1] if v.size else 0.0


def waterfill_ref(max_per_quad, TOTAL, sum_fn=sum_numpy, trace=None):
    """matching.py:154-179.  ``trace`` (a dict) receives which way the loop went: 'steps', 'eq' (left through the ``==``
    break), 'final' (the height before np.round)."""
    def apply_height(height):
        is_dwarf = max_per_quad < height
        return is_dwarf * max_per_quad + (~is_dwarf) * height
    max_h = TOTAL
    min_h = 0
    steps = 0
    eq = False
    cur = (max_h + min_h) / 2
    while np.abs(max_h - min_h) > 2:
        t = sum_fn(apply_height(cur))
        if t == TOTAL:
            eq = True
            break
        elif t < TOTAL:
            min_h = cur
        elif t > TOTAL:
            max_h = cur
        cur = (max_h + min_h) / 2
        steps += 1
    if trace is not None:
        trace.update(steps=steps, eq=eq, final=cur)
    return apply_height(np.round(cur))


def select_ref(qi, qj, score, G, TOTAL, sum_fn=sum_numpy):
    """matching.py:147-195: counts per cell, quota, and per cell the `quota` best scores (ties towards the lower position,
    which the builders never need).  Returns (keep mask, counts [G, G], quota [G, G])."""
    qi = np.asarray(qi); qj = np.asarray(qj)
    n = len(qi)
    valid = (qi >= 0) & (qi < G) & (qj >= 0) & (qj < G)          # range(GRID_WID) x range(GRID_WID): nothing else is ever matched
    cell = np.full(n, -1, np.int64)
    cell[valid] = qi[valid].astype(np.int64) * G + qj[valid].astype(np.int64)
    counts = np.bincount(cell[valid], minlength=G * G).astype(np.float64).reshape(G, G)
    per_quad = waterfill_ref(counts, TOTAL, sum_fn)
    extra = per_quad.astype(np.int64).ravel()                      # int(per_quad[qi, qj])
    order = np.lexsort((np.arange(n), np.asarray(score), cell))
    sc = cell[order]
    start = np.r_[0, np.flatnonzero(sc[1:] != sc[:-1]) + 1]
    run = np.repeat(start, np.diff(np.r_[start, n]))
    rank = np.arange(n) - run
    keep = np.zeros(n, bool)
    ok = sc >= 0
    keep[order[ok]] = rank[ok] < extra[sc[ok]]
    return keep, counts, per_quad


def ratio_ref(F0, F1, i0, i1, i2):
    """matching.py:89-98 in float32, the sum over the dimensions taken in order."""
    A = F0[i0]; B1 = F1[i1]; B2 = F1[i2]
    s1 = np.zeros(len(i0), F32); s2 = np.zeros(len(i0), F32)
    for k in range(F0.shape[1]):
        e1 = (A[:, k] - B1[:, k]).astype(F32); e2 = (A[:, k] - B2[:, k]).astype(F32)
        s1 = (s1 + (e1 * e1).astype(F32)).astype(F32); s2 = (s2 + (e2 * e2).astype(F32)).astype(F32)
    d1 = np.sqrt(s1).astype(F32); d2 = np.sqrt(s2).astype(F32)
    return (d1 / (d2 + F32(1e-6)).astype(F32)).astype(F32)


def gpf_ref(c, G, factor=None, cap=None, flip=None, sum_fn=sum_numpy):
    """Grid_Prioritized_Filter on a cloud of this module: BB_first=False with ``factor``, or BB_first=True with ``cap``.
    ``flip = (position, axis, new quadrant)`` overrides one quadrant of ``cells_ref``'s output (the builders' proof that a planted
    pair matters).  Returns dict(idx0, idx1, idx2, score (None when BB_first returns early), counts, quota, TOTAL)."""
    n = len(c["i1"])
    if cap is not None:
        sub = np.flatnonzero(c["is_bb"])
        TOTAL = cap
        if TOTAL >= len(sub):
            return dict(idx0=sub, idx1=c["i1"][sub], idx2=c["i2"][sub], score=None, TOTAL=TOTAL)
    else:
        sub = np.arange(n)
        TOTAL = factor * int(c["is_bb"].sum())
    ratio = ratio_ref(c["F0"], c["F1"], sub, c["i1"][sub], c["i2"][sub])
    m = ratio.min(); M = ratio.max()
    nfd = ((ratio - m).astype(F32) / F32(M - m)).astype(F32)
    if cap is None:
        nfd[c["is_bb"]] -= F32(1)
    qi, qj = cells_ref(c["xyz0"][sub, 0], c["xyz0"][sub, 1], G)
    if flip is not None:
        q = (qi, qj)[flip[1]].copy(); q[flip[0]] = flip[2]
        qi, qj = (q, qj) if flip[1] == 0 else (qi, q)
    keep, counts, quota = select_ref(qi, qj, nfd, G, TOTAL, sum_fn)
    return dict(idx0=sub[keep], idx1=c["i1"][sub][keep], idx2=c["i2"][sub][keep], score=nfd[keep], counts=counts, quota=quota,
                TOTAL=TOTAL, qi=qi, qj=qj, nfd=nfd)


# ----------------------------------------------------------------------------- descriptors with known scores

def make_cloud(xy, is_bb, m, cell, dim, seed):
    """xy [n, 2] float32 positions, is_bb [n] bool, m [n] int (a_i = m_i / 1024 of the best buddies, distinct inside a cell; ignored for
    guests), cell [n] int (only used to keep the guests' scores distinct inside a cell) -> dict(xyz0, xyz1, F0, F1, i1, i2, is_bb)."""
    rng = np.random.default_rng(seed)
    n = len(xy)
    hosts = np.flatnonzero(is_bb); guests = np.flatnonzero(~is_bb)
    H = len(hosts)
    nd = 4 if dim < 8 else 6                        # code digits: dimensions 0..3 and, when there is room, 5 and 6
    assert 1 <= H <= 8 ** nd and dim >= 5
    code_id = rng.permutation(8 ** nd)[:H]
    code = np.stack([(code_id >> (3 * k)) & 7 for k in range(4)], 1).astype(F32) * F32(2)
    extra = (rng.integers(-8, 9, (H, dim - 5)) / 8.0).astype(F32)          # the same in a point and its rows: cancels exactly
    for k in range(4, nd):
        extra[:, k - 4] = ((code_id >> (3 * k)) & 7).astype(F32) * F32(2)
    a = (np.asarray(m)[hosts] / 1024.0).astype(F32)
    assert a.min() > 0 and a.max() <= 400 / 1024.0
    F0 = np.zeros((n, dim), F32)
    F0[hosts, :4] = code; F0[hosts, 5:] = extra
    rows = rng.permutation(2 * H)                   # row of A_h = rows[2 h], of B_h = rows[2 h + 1]
    F1 = np.zeros((2 * H, dim), F32)
    F1[rows[0::2], :4] = code; F1[rows[0::2], 4] = a; F1[rows[0::2], 5:] = extra
    F1[rows[1::2], :4] = code; F1[rows[1::2], 4] = -F32(B_OFF / 1024.0); F1[rows[1::2], 5:] = extra
    i1 = np.zeros(n, np.int64); i2 = np.zeros(n, np.int64)
    i1[hosts] = rows[0::2]; i2[hosts] = rows[1::2]
    if len(guests):
        host_of = rng.integers(0, H, len(guests))
        t = rng.integers(820, 1024, len(guests))
        for _ in range(200):                        # distinct guest scores inside every cell
            r = (t / 1024.0 - a[host_of].astype(np.float64)) / (t / 1024.0 + B_OFF / 1024.0 + 1e-6)
            key = np.stack([np.asarray(cell)[guests].astype(np.float64), r.astype(F32).astype(np.float64)], 1)
            _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
            dup = cnt[inv.ravel()] > 1
            if not dup.any():
                break
            host_of[dup] = rng.integers(0, H, int(dup.sum())); t[dup] = rng.integers(820, 1024, int(dup.sum()))
        else:
            raise AssertionError("guest scores could not be made distinct")
        F0[guests, :4] = code[host_of]; F0[guests, 4] = (t / 1024.0).astype(F32); F0[guests, 5:] = extra[host_of]
        i1[guests] = rows[0::2][host_of]; i2[guests] = rows[1::2][host_of]
    xyz0 = np.concatenate([np.asarray(xy, F32), rng.uniform(-2, 3, (n, 1)).astype(F32)], 1)
    xyz1 = rng.uniform(-50, 50, (2 * H, 3)).astype(F32)
    return dict(xyz0=np.ascontiguousarray(xyz0), xyz1=xyz1, F0=F0, F1=F1, i0=np.arange(n, dtype=np.int64), i1=i1, i2=i2,
                is_bb=np.asarray(is_bb, bool).copy())


def checksum(c):
    h = hashlib.sha256()
    for k in ("xyz0", "xyz1", "F0", "F1", "i1", "i2"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


# ----------------------------------------------------------------------------- cell edges

class Axis:
    """One coordinate axis with its minimum and maximum pinned: quadrant of a float, and the floats around every cell edge."""
    def __init__(self, lo, span, G):
        self.m = F32(lo); self.M = F32(F32(lo) + F32(span)); self.G = G
        self.rng = F32(self.M - self.m)
        self.den = F32(self.rng + F32(1e-3))

    def prod(self, x):
        return F32(F32(self.G) * F32(F32(F32(x) - self.m) / self.den))

    def quad(self, x):
        return float(np.floor(self.prod(x)))

    def edge(self, k):
        """(last float32 whose quadrant is below k, first whose quadrant is k or more), or None when no float up to the maximum reaches k."""
        if self.quad(self.M) < k:
            return None
        x = F32(float(self.m) + k / self.G * float(self.den))
        while self.quad(x) < k:
            x = np.nextafter(x, F32(np.inf))
        while self.quad(x) >= k:
            x = np.nextafter(x, F32(-np.inf))
        return F32(x), F32(np.nextafter(x, F32(np.inf)))

    def inside(self, k, u):
        """A float32 well inside cell k (u in [0, 1] -> the middle 60 % of the cell)."""
        lo = float(self.m) + k / self.G * float(self.den); hi = float(self.m) + (k + 1) / self.G * float(self.den)
        hi = min(hi, float(self.M))
        return (lo + (0.2 + 0.6 * u) * (hi - lo)).astype(F32) if isinstance(u, np.ndarray) else F32(lo + (0.2 + 0.6 * u) * (hi - lo))


GRID_PLAN = {3: (300, 20, 60), 10: (30, 3, 12), 23: (9, 1, 6)}       # G -> fillers of a crowded cell, of a sparse cell, target height


def _grid_cloud(G, seed, span_x, span_y, dim=32, lo=(-37.25, 12.5)):
    """Checkerboard of crowded ((qi + qj) even) and sparse cells with a pair planted on either side of every cell edge."""
    rng = np.random.default_rng(seed)
    fill_c, fill_s, h_t = GRID_PLAN[G]
    ax = (Axis(lo[0], span_x, G), Axis(lo[1], span_y, G))
    pts = []                # (x, y, is_bb, kind, cell or None); kind: 0 filler, 1 worst of its cell, 2 best of its cell
    planted = []            # (position in pts, axis, k, side 0 = last below / 1 = first at, quadrant on the other side of the edge)
    for qi in range(G):
        for qj in range(G):
            crowded = (qi + qj) % 2 == 0
            for f in range(fill_c if crowded else fill_s):
                guest = (not crowded) and ((qi * G + qj + f) % 3 == 1)
                pts.append((ax[0].inside(qi, rng.random()), ax[1].inside(qj, rng.random()), not guest, 0))
    for axis in (0, 1):
        for k in range(1, G + 1):
            e = ax[axis].edge(k)
            if e is None:
                continue
            for other in sorted({k % G, (k + 1) % G}):
                mid = ax[1 - axis].inside(other, 0.5)
                for side in (0, 1):
                    p = (e[side], mid) if axis == 0 else (mid, e[side])
                    planted.append((len(pts), axis, k, side, float(k - 1 + (1 - side))))
                    pts.append(p + (True, 2 if k == G else 1))
    # the extrema: one point each, away from the corners (the largest y in column c < G - 1: a wrapped index would land in (c + 1, 0))
    cmax = 0 if G < 4 else 2
    anchors = [(ax[0].m, ax[1].inside(G // 2, 0.4)), (ax[0].M, ax[1].inside(G // 2, 0.6)),
               (ax[0].inside(G // 2, 0.4), ax[1].m), (ax[0].inside(cmax, 0.6), ax[1].M)]
    anchor_pos = []
    for p in anchors:
        anchor_pos.append(len(pts)); pts.append(p + (True, 2))
    n = len(pts)
    perm = rng.permutation(n)                       # pts[perm[j]] becomes point j
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    xy = np.array([[p[0], p[1]] for p in pts], F32)[perm]
    is_bb = np.array([p[2] for p in pts], bool)[perm]
    kind = np.array([p[3] for p in pts])[perm]
    qi, qj = cells_ref(xy[:, 0], xy[:, 1], G)
    cell = (qi * (G + 1) + qj).astype(np.int64)     # (only a label here: G + 1 keeps the cells that do not exist apart)
    m = np.zeros(n, np.int64)
    for cidx in np.unique(cell):
        w = np.flatnonzero(cell == cidx)
        best = w[kind[w] == 2]; worst = w[kind[w] == 1]; fill = w[kind[w] == 0]
        m[best] = 1 + np.arange(len(best)); m[worst] = 400 - np.arange(len(worst))
        m[fill] = 20 + rng.permutation(len(fill))
        assert len(best) < 19 and 20 + len(fill) < 400 - len(worst)
    c = make_cloud(xy, is_bb, m, cell, dim, seed + 1)
    num_bb = int(is_bb.sum())
    n_crowded = (G * G + 1) // 2
    sparse_total = int(sum(1 for j in range(n) if kind[j] != 2 and (qi[j] + qj[j]) % 2 == 1 and qi[j] < G and qj[j] < G))
    c["factor"] = round((n_crowded * h_t + sparse_total) / num_bb, 4)
    c["G"] = G
    c["planted"] = [(int(inv[p]), a, k, s, q) for p, a, k, s, q in planted]
    c["anchors"] = [int(inv[p]) for p in anchor_pos]          # min x, max x, min y, max y
    c["axes"] = ax
    c["cap"] = num_bb // 3
    return c


@functools.lru_cache(maxsize=None)
def boundary_cloud(G, seed=0, span=91.5, dim=32):
    """About 2 000 points on a G x G checkerboard of crowded and sparse cells.  For every interior edge k / G in x and in y it holds the
    last float32 whose quadrant is k - 1 and the first whose quadrant is k (found by walking np.nextafter under ``quads_ref``'s
    arithmetic), in two rows / columns, so that each side of each edge is once a crowded and once a sparse cell; plus the minimum and the
    maximum of either axis.  A planted pair is the worst of its cell: in a crowded cell it is dropped, in a sparse one kept, and the
    other way round in the neighbouring cell (``planted_pairs_matter`` proves it)."""
    return _grid_cloud(G, 1000 * G + seed, span, span * 0.75, dim)


@functools.lru_cache(maxsize=None)
def wide_cloud(which):
    """``which`` in 'x', 'y', 'xy': the range of that coordinate is 40 000 >= 32768, so float32 absorbs the + 1e-3 and the largest
    coordinate gets quadrant G -- a cell that does not exist.  The largest y belongs to a point of column 2 with the best score of the
    whole cloud: were its flat index allowed to wrap into cell (3, 0), it would be kept there and push another pair out."""
    G = 10
    return _grid_cloud(G, 7000 + len(which) + ord(which[0]), 40000.0 if "x" in which else 91.5, 40000.0 if "y" in which else 70.0, 32,
                       lo=(-1234.5, 777.25))


def planted_pairs_matter(c):
    """Flip every planted pair into the cell on the other side of its edge and re-run the selection: the number of pairs whose kept
    list does NOT change (must be 0)."""
    G = c["G"]
    base = gpf_ref(c, G, factor=c["factor"])
    same = 0
    for pos, axis, k, side, q_other in c["planted"]:
        alt = gpf_ref(c, G, factor=c["factor"], flip=(pos, axis, q_other))
        same += int(np.array_equal(alt["idx0"], base["idx0"]))
    return same


# ----------------------------------------------------------------------------- water-filling

def cloud_from_counts(counts, num_bb, seed, dim=32):
    """counts[qi, qj] pairs inside every cell (the corner cells (0, 0) and (G-1, G-1) hold the extrema and need one pair each),
    num_bb of them best buddies with the extrema among them."""
    counts = np.asarray(counts, np.int64)
    G = counts.shape[0]
    assert counts[0, 0] >= 1 and counts[-1, -1] >= 1
    rng = np.random.default_rng(seed)
    ax = (Axis(-20.0, 64.0, G), Axis(5.0, 48.0, G))
    qi = np.repeat(np.arange(G * G) // G, counts.ravel()); qj = np.repeat(np.arange(G * G) % G, counts.ravel())
    n = len(qi)
    lo_x = float(ax[0].m) + qi / G * float(ax[0].den); lo_y = float(ax[1].m) + qj / G * float(ax[1].den)
    wx = np.minimum(float(ax[0].den) / G, float(ax[0].M) - lo_x); wy = np.minimum(float(ax[1].den) / G, float(ax[1].M) - lo_y)
    xy = np.stack([lo_x + (0.2 + 0.6 * rng.random(n)) * wx, lo_y + (0.2 + 0.6 * rng.random(n)) * wy], 1).astype(F32)
    xy[0] = (ax[0].m, ax[1].m); xy[n - 1] = (ax[0].M, ax[1].M)
    is_bb = np.zeros(n, bool)
    assert 2 <= num_bb <= n or n == 1
    is_bb[[0, n - 1]] = True
    rest = rng.permutation(np.arange(1, n - 1))[:max(num_bb - 2, 0)]
    is_bb[rest] = True
    m = np.zeros(n, np.int64)
    cell = qi * G + qj
    start = np.r_[0, np.cumsum(counts.ravel())]
    for cidx in range(G * G):
        k = int(counts.ravel()[cidx])
        assert k < 380
        m[start[cidx]:start[cidx] + k] = 10 + rng.permutation(k)
    perm = rng.permutation(n)
    c = make_cloud(xy[perm], is_bb[perm], m[perm], cell[perm], dim, seed + 1)
    c["G"] = G
    return c


def _final_height(counts, TOTAL, sum_fn):
    tr = {}
    waterfill_ref(counts, TOTAL, sum_fn, tr)
    return tr


def _bisect_batch(counts, TOTAL, seq):
    """The bisection of ``waterfill_ref`` for many (counts row, TOTAL) at once; only a sieve: what it finds is re-run one by one."""
    max_h = TOTAL.copy(); min_h = np.zeros_like(TOTAL); cur = (max_h + min_h) / 2
    active = np.ones(len(TOTAL), bool)
    while True:
        active &= np.abs(max_h - min_h) > 2
        if not active.any():
            return cur
        v = np.minimum(counts, cur[:, None])
        t = np.cumsum(v, axis=1)[:, -1] if seq else v.sum(axis=1)
        active &= t != TOTAL
        lt = active & (t < TOTAL); gt = active & (t > TOTAL)
        min_h[lt] = cur[lt]; max_h[gt] = cur[gt]
        cur[active] = (max_h[active] + min_h[active]) / 2


def _search_order_sensitive(G, want=3, trials=20000):
    """Seeded search for (counts, num_bb, factor) whose bisection ends at another rounded height when the sum runs left to right
    instead of numpy's pairwise order.  Returns up to ``want`` cases (possibly none: say so in DESIGN.md, do not force one)."""
    rng = np.random.default_rng(900 + G)
    C = G * G
    found = []
    batch = max(16, min(2000, 400000 // C))
    for _ in range(0, trials, batch):
        f = np.array(FACTORS)[rng.integers(len(FACTORS), size=batch)]
        cmax = max(2, min(12, 9500 // C - 1))
        c0 = rng.integers(1, cmax + 1, batch)
        crowded = rng.random(batch) < 0.5
        counts = np.where(crowded[:, None], c0[:, None] + (rng.random((batch, C)) < 0.3),
                          (rng.random((batch, C)) * (2 * c0[:, None] + 2)).astype(np.int64)).astype(np.int64)
        counts[:, 0] = np.maximum(counts[:, 0], 1); counts[:, -1] = np.maximum(counts[:, -1], 1)
        n = counts.sum(axis=1)
        B = (n // 2 + (rng.random(batch) * (n - n // 2 + 1)).astype(np.int64)).clip(2, n)
        TOTAL = f * B
        cf = counts.astype(np.float64)
        a = _bisect_batch(cf, TOTAL, False); b = _bisect_batch(cf, TOTAL, True)
        for k in np.flatnonzero((np.round(a) != np.round(b)) & (n >= 4) & (n <= 10500)):
            m = cf[k].reshape(G, G)
            ta = _final_height(m, float(TOTAL[k]), sum_numpy); tb = _final_height(m, float(TOTAL[k]), sum_left_to_right)
            if np.round(ta["final"]) != np.round(tb["final"]) and float(f[k]) * int(B[k]) == TOTAL[k]:
                found.append(dict(counts=counts[k].reshape(G, G), num_bb=int(B[k]), factor=float(f[k])))
                if len(found) == want:
                    return found
    return found


def _search_small(pred, seed, G=3, trials=20000):
    """Seeded search over small count matrices and TOTAL = factor * 64 for a branch of the bisection."""
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        counts = rng.integers(0, 9, (G, G)); counts[0, 0] = max(counts[0, 0], 1); counts[-1, -1] = max(counts[-1, -1], 1)
        counts[rng.integers(G), rng.integers(G)] += 70           # room for 64 best buddies
        factor = int(rng.integers(1, 160)) / 128.0               # TOTAL = factor * 64: every multiple of 0.5 up to 79.5
        tr = {}
        quota = waterfill_ref(counts.astype(np.float64), factor * 64, sum_numpy, tr)
        if pred(counts, quota, tr, factor * 64):
            return dict(counts=counts, num_bb=64, factor=factor)
    raise AssertionError("no case found")


@functools.lru_cache(maxsize=None)
def waterfill_cases():
    """List of dict(name, counts [G, G], num_bb, factor, why): TOTAL = factor * num_bb.  See the module docstring of the CPU test for
    the branch each one takes."""
    base = np.array([[3, 0, 5], [70, 2, 0], [1, 4, 2]])
    cases = []
    for name, factor in (("total0", 0.0), ("total1", 1 / 64), ("total2", 2 / 64), ("total3", 3 / 64), ("total1.5", 1.5 / 64)):
        cases.append(dict(name=name, counts=base, num_bb=64, factor=factor))
    frac = lambda tr: tr["final"] - np.floor(tr["final"])
    cases.append(dict(name="eq_break", **_search_small(lambda c, q, tr, T: tr["eq"] and tr["steps"] >= 2, 11)))
    cases.append(dict(name="half_even", **_search_small(lambda c, q, tr, T: frac(tr) == 0.5 and np.floor(tr["final"]) % 2 == 0 and tr["final"] > 1 and tr["steps"] >= 1, 12)))
    cases.append(dict(name="half_odd", **_search_small(lambda c, q, tr, T: frac(tr) == 0.5 and np.floor(tr["final"]) % 2 == 1 and tr["steps"] >= 1, 13)))
    def neighbours(c, q, tr, T):
        cf = c.ravel(); qf = q.ravel()
        return tr["steps"] >= 1 and any(cf[k] >= 2 and qf[k] == cf[k] and qf[k + 1] == cf[k + 1] - 1 for k in range(len(cf) - 1))
    cases.append(dict(name="quota_eq_count", **_search_small(neighbours, 14)))
    cases.append(dict(name="total_above_sum", counts=np.array([[2, 3], [4, 60]]), num_bb=69, factor=1.1))
    for G in (2, 8, 11, 12, 16, 64):
        for k, f in enumerate(_search_order_sensitive(G)):
            cases.append(dict(name=f"order_g{G}_{k}", counts=f["counts"], num_bb=f["num_bb"], factor=f["factor"]))
    return cases


@functools.lru_cache(maxsize=None)
def waterfill_cloud(name):
    k, case = next((k, c) for k, c in enumerate(waterfill_cases()) if c["name"] == name)
    c = cloud_from_counts(case["counts"], case["num_bb"], 5000 + k)
    c["factor"] = case["factor"]
    c["cap"] = max(case["num_bb"] // 3, 1)
    return c


def all_clouds():
    """name -> builder of every cloud the fixture covers."""
    d = {"b3": lambda: boundary_cloud(3), "b10": lambda: boundary_cloud(10), "b23": lambda: boundary_cloud(23),
         "b10d5": lambda: boundary_cloud(10, 1, 57.0, 5),
         "wide_x": lambda: wide_cloud("x"), "wide_y": lambda: wide_cloud("y"), "wide_xy": lambda: wide_cloud("xy")}
    for case in waterfill_cases():
        d["wf_" + case["name"]] = functools.partial(waterfill_cloud, case["name"])
    return d


# ----------------------------------------------------------------------------- PROSAC order

def prosac_expected(q):
    q = np.asarray(q, F32)
    return np.argsort(np.where(np.isnan(q), F32(np.inf), q), kind="stable")


@functools.lru_cache(maxsize=None)
def prosac_lists():
    """name -> float32 quality vector.  Lengths around the 1 024 threads and the 8 x 1 024 elements of a round of the scan kernel."""
    rng = np.random.default_rng(321)
    out = {}
    for n in (1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 9217):
        out[f"uniform_{n}"] = rng.random(n).astype(F32)
    out["all_equal"] = np.full(3000, 0.25, F32)
    out["two_values"] = rng.choice(np.array([0.125, 0.75], F32), 5000)
    g = rng.random(9217).astype(F32)
    pile = rng.random(9217) < 0.1
    g[pile] = np.nextafter(F32(1), F32(0)) - (rng.integers(0, 3, int(pile.sum())) * np.spacing(F32(0.5))).astype(F32)
    bb = rng.random(9217) < 0.3
    g[bb] -= F32(1)
    out["gpf_shape"] = g.astype(F32)
    s = rng.random(4000).astype(F32)
    s[17] = np.inf; s[2900] = -np.inf; s[1024] = np.nan
    out["inf_nan"] = s
    t = rng.random(8193).astype(F32)
    t[rng.random(8193) < 0.4] = np.nan
    out["many_nan"] = t
    return out


def prosac_cloud(q, seed=0):
    """A pair of clouds whose feature-distance ratios have the order and the ties of the finite quality vector ``q`` (quantised to the
    400 levels ``make_cloud`` has), every pair a best buddy, and a rigid motion planted on half of the pairs.  Non-finite qualities cannot
    be produced through the descriptors (the ratio of two finite distances is finite and not negative)."""
    q = np.asarray(q, F32)
    assert np.isfinite(q).all()
    n = len(q)
    rng = np.random.default_rng(4000 + seed + n)
    lo, hi = float(q.min()), float(q.max())
    m = 1 + (np.floor((q.astype(np.float64) - lo) / (hi - lo) * 399.0).astype(np.int64) if hi > lo else np.zeros(n, np.int64))
    c = make_cloud(rng.uniform(-40, 40, (n, 2)).astype(F32), np.ones(n, bool), m, np.arange(n), 32, 4100 + seed + n)
    ang = 0.4
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = [1.5, -2.0, 0.3]
    inl = rng.random(n) < 0.5
    c["xyz1"][c["i1"][inl]] = (c["xyz0"][inl].astype(np.float64) @ R.T + T[:3, 3]).astype(F32)
    c["T_gt"] = T
    return c


def compaction_cloud(n0, pattern, seed=0):
    """Every point of cloud 0 has its own two rows in cloud 1; the pairs outside ``pattern`` ('first': the first 256-pair block,
    'last': the last block, 'none', 'all') point at the NEXT point's row instead, whose neighbour in cloud 0 is that next point: they are
    no best buddies.  The lists are handed to the filter as they are (not the true neighbours)."""
    rng = np.random.default_rng(6000 + n0 + seed)
    xy = rng.uniform(-30, 30, (n0, 2)).astype(F32)
    c = make_cloud(xy, np.ones(n0, bool), rng.integers(1, 401, n0), np.arange(n0), 32, 6100 + n0 + seed)
    i = np.arange(n0)
    keep = {"first": i < 256, "last": i >= 256 * ((n0 - 1) // 256), "none": np.zeros(n0, bool), "all": np.ones(n0, bool)}[pattern]
    if n0 == 1:
        keep[:] = True
    own = c["i1"].copy()
    c["i1"] = np.where(keep, own, own[(i + 1) % n0])
    c["is_bb"] = keep
    return c
