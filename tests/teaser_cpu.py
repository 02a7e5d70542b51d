"""numpy / networkx restatement of the TEASER++ contract of include/lidarreg.h (lr_teaser) and DESIGN.md §10.

TEASER++ is not vendored, so this is the yardstick of the device solver, not a copy of upstream.  Inputs a, b: [M,3] float32.
"""
import networkx as nx
import numpy as np

PARAMS = dict(noise_bound=0.3, cbar2=1.0, kcore_threshold=0.5, gnc_factor=1.4, max_iterations=10000, cost_threshold=1e-16)


def _dist(p, i0, i1):
    d = p[i0:i1, None, :] - p[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def graph(a, b, noise_bound=0.3, cbar2=1.0, chunk=1024):
    """Boolean adjacency [M,M]: | |a_i-a_j| - |b_i-b_j| | <= 2 beta sqrt(cbar2), i != j, fp64 on the promoted inputs."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    m = a.shape[0]
    thr = 2.0 * noise_bound * np.sqrt(cbar2)
    A = np.zeros((m, m), bool)
    for i0 in range(0, m, chunk):
        i1 = min(m, i0 + chunk)
        A[i0:i1] = np.abs(_dist(a, i0, i1) - _dist(b, i0, i1)) <= thr
    np.fill_diagonal(A, False)
    return A


def graph_naive(a, b, noise_bound=0.3, cbar2=1.0):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    m = a.shape[0]
    thr = 2.0 * noise_bound * np.sqrt(cbar2)
    A = np.zeros((m, m), bool)
    for i in range(m):
        for j in range(m):
            if i == j:
                continue
            da = [float(a[i, k]) - float(a[j, k]) for k in range(3)]
            db = [float(b[i, k]) - float(b[j, k]) for k in range(3)]
            la = np.sqrt((da[0] * da[0] + da[1] * da[1]) + da[2] * da[2])
            lb = np.sqrt((db[0] * db[0] + db[1] * db[1]) + db[2] * db[2])
            A[i, j] = abs(la - lb) <= thr
    return A


def to_nx(A):
    G = nx.Graph()
    G.add_nodes_from(range(A.shape[0]))
    ii, jj = np.nonzero(np.triu(A, 1))
    G.add_edges_from(zip(ii.tolist(), jj.tolist()))
    return G


def max_clique(A, kcore_threshold=0.5):
    """(clique ascending, shortcut fired?, max core number)."""
    m = A.shape[0]
    if m == 0:
        return np.zeros(0, np.int64), False, 0
    G = to_nx(A)
    core = nx.core_number(G)
    maxcore = max(core.values())
    if maxcore > kcore_threshold * m:
        return np.array(sorted(v for v, c in core.items() if c == maxcore), np.int64), True, maxcore
    c, _ = nx.max_weight_clique(G, None)
    return np.array(sorted(c), np.int64), False, maxcore


def svd_rot(A, B, w):
    H = (A * w[:, None]).T @ B
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, np.linalg.det(V @ U.T)])
    return V @ D @ U.T


def rotation(a, b, clique, noise_bound=0.3, cbar2=1.0, gnc_factor=1.4, max_iterations=10000, cost_threshold=1e-16):
    """GNC-TLS on the chain TIMs: (R, final weights, iterations, residuals of the last evaluation, mu at each threshold test)."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(clique)
    A, B = a[np.roll(c, -1)] - a[c], b[np.roll(c, -1)] - b[c]
    nb2 = (2.0 * noise_bound) ** 2 * cbar2
    w = np.ones(len(c))
    R = svd_rot(A, B, w)
    r = np.sum((B - A @ R.T) ** 2, 1)
    mu = 1.0 / (2.0 * r.max() / nb2 - 1.0)
    trace = []
    if mu <= 0:
        return R, w, 0, r, trace
    prev, it = 0.0, 0
    for it in range(1, max_iterations + 1):
        r = np.sum((B - A @ R.T) ** 2, 1)
        th1, th2 = (mu + 1) / mu * nb2, mu / (mu + 1) * nb2
        trace.append((r.copy(), th1, th2))
        cost = float(np.sum(w * r))
        with np.errstate(divide="ignore"):
            mid = np.sqrt(nb2 * mu * (mu + 1) / np.where(r > 0, r, 1.0)) - mu
        w = np.where(r >= th1, 0.0, np.where(r <= th2, 1.0, mid))
        mu *= gnc_factor
        if abs(cost - prev) < cost_threshold:
            break
        prev = cost
        R = svd_rot(A, B, w)
    return R, w, it, r, trace


def vote(x, beta):
    """Adaptive voting on one axis (sorted sweep): (estimate, cost at it, index of the winning endpoint in sorted order)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    ends = [(x[i] - beta, 0, i) for i in range(n)] + [(x[i] + beta, 1, i) for i in range(n)]
    ends.sort()
    inset = np.zeros(n, bool)
    best = (np.inf, None, None)
    for pos, (_, t, i) in enumerate(ends):
        inset[i] = t == 0
        cnt = int(inset.sum())
        if cnt == 0:
            continue
        xs = x[inset]
        xh = xs.sum() / cnt
        cost = float(np.sum((xs - xh) ** 2) + beta * (n - cnt))
        if cost < best[0]:
            best = (cost, xh, pos)
    return best[1], best[0], best[2]


def vote_brute(x, beta):
    """The same minimum over every candidate centre, without a sweep: for every endpoint key e the set { j: entry_j <= e < exit_j }."""
    x = np.asarray(x, np.float64)
    n = len(x)
    keys = sorted([(x[i] - beta, 0, i) for i in range(n)] + [(x[i] + beta, 1, i) for i in range(n)])
    best = (np.inf, None)
    for e in keys:
        s = [j for j in range(n) if (x[j] - beta, 0, j) <= e < (x[j] + beta, 1, j)]
        if not s:
            continue
        xs = x[s]
        xh = xs.sum() / len(s)
        cost = float(np.sum((xs - xh) ** 2) + beta * (n - len(s)))
        if cost < best[0]:
            best = (cost, xh)
    return best[1], best[0]


def solve_from_clique(a, b, clique, **kw):
    """Rotation + translation from a given clique: dict(T, status, n_rot, n_trans, R, w, iters, trace)."""
    p = {**PARAMS, **kw}
    beta = p["noise_bound"]
    c = np.asarray(clique)
    out = dict(T=np.eye(4), status=1, n_rot=0, n_trans=0, K=len(c))
    if len(c) < 3:
        return out
    R, w, iters, r, trace = rotation(a, b, c, beta, p["cbar2"], p["gnc_factor"], p["max_iterations"], p["cost_threshold"])
    inl = w >= 0.5
    out.update(R=R, w=w, iters=iters, trace=trace, n_rot=int(inl.sum()))
    if inl.sum() < 3:
        return out
    pts = c[inl]
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    X = b64[pts] - a64[pts] @ R.T
    t = np.array([vote(X[:, k], beta)[0] for k in range(3)])
    out["n_trans"] = int(np.all(np.abs(X - t) <= beta, 1).sum())
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    out.update(T=T, status=0, X=X, t=t)
    return out


def teaser(a, b, **kw):
    p = {**PARAMS, **kw}
    A = graph(a, b, p["noise_bound"], p["cbar2"])
    clique, shortcut, maxcore = max_clique(A, p["kcore_threshold"])
    out = solve_from_clique(a, b, clique, **kw)
    out.update(clique=clique, shortcut=shortcut, max_core=maxcore)
    return out


def planted(m, n_in, seed, noise=0.02, outlier_scale=10.0, beta=0.3):
    """m correspondences, the first n_in of them inliers of a random motion (noise per axis uniform in +-noise), the rest random.
    Returns (a, b, T_gt, permutation applied)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w_, x_, y_, z_ = q
    R = np.array([[1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - z_ * w_), 2 * (x_ * z_ + y_ * w_)],
                  [2 * (x_ * y_ + z_ * w_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - x_ * w_)],
                  [2 * (x_ * z_ - y_ * w_), 2 * (y_ * z_ + x_ * w_), 1 - 2 * (x_ * x_ + y_ * y_)]])
    t = rng.uniform(-5, 5, 3)
    a = rng.uniform(-outlier_scale, outlier_scale, (m, 3))
    b = rng.uniform(-outlier_scale, outlier_scale, (m, 3)) + t
    b[:n_in] = a[:n_in] @ R.T + t + rng.uniform(-noise, noise, (n_in, 3))
    perm = rng.permutation(m)
    T = np.eye(4); T[:3, :3], T[:3, 3] = R, t
    return a[perm].astype(np.float32), b[perm].astype(np.float32), T, perm


GREEDY_WAVES = 16


def greedy_clique(A, seed, first):
    """The greedy clique of DESIGN §10 from `seed`: candidates of the boolean mask `first` (the max-core vertices) in ascending order,
    then any vertex in ascending order; a vertex joins when it is adjacent to every member so far.  Ascending list."""
    P = A[seed].copy()
    C = [int(seed)]
    for mask in (first, np.ones(len(P), bool)):
        last = -1
        while True:
            cand = np.nonzero(P & mask)[0]
            cand = cand[cand > last]
            if len(cand) == 0:
                break
            last = int(cand[0])
            C.append(last)
            P &= A[last]
    return sorted(C)


def reduction_model(A, kcore_threshold=0.5):
    """Plain model of the clique stage's reduction as DESIGN §10 states it.  A: boolean adjacency (tc.graph).  Returns
    (max_core, LB, nU, nR, exit):
      core numbers from networkx; 'shortcut' when max_core > kcore_threshold * M (LB, nU, nR = 0);
      otherwise LB = the largest of 16 greedy cliques (clique j seeded at the (j mod nmax)-th max-core vertex, first maximum kept),
      S = vertices of core number >= LB, U = those of S adjacent to every other vertex of S (nU), R = S \\ U (nR);
      nR = 0: 'empty_universal' when nU > LB else 'empty_incumbent';
      nR > 0: the search runs with target LB - nU: 'search_target_nonpositive' when that is <= 0, else 'search'.
    'empty_universal' cannot happen: with nR = 0, S is a clique of nU vertices; a vertex outside S has core number < LB <= nU - 1, so
    no k-core with k >= nU - 1 holds one, every vertex of S has core number exactly nU - 1 = max_core, the max-core set is S, and the
    first greedy pass collects all of it: LB >= nU.  'search_target_nonpositive' cannot happen either: a vertex of U is adjacent to all
    of the max-core subgraph, so it belongs to it (U lies in the max-core set) and is adjacent to every seed; the first pass of every
    greedy clique therefore collects all of U, and the clique ends with at least one more vertex (the seed when it is not in U, else a
    vertex adjacent to all of U, of which R holds at least one): LB >= nU + 1.  Both labels are kept so that a model run would show
    them if an argument were wrong."""
    m = A.shape[0]
    if m == 0:
        return 0, 0, 0, 0, "empty_graph"
    core = nx.core_number(to_nx(A))
    core = np.array([core[v] for v in range(m)])
    maxcore = int(core.max())
    if float(maxcore) > kcore_threshold * float(m):
        return maxcore, 0, 0, 0, "shortcut"
    first = core == maxcore
    top = np.nonzero(first)[0]
    LB = 0
    for j in range(GREEDY_WAVES):
        LB = max(LB, len(greedy_clique(A, top[j % len(top)], first)))
    S = core >= LB
    nr = int(S.sum())
    deg = A[np.ix_(S, S)].sum(1) if nr else np.zeros(0, int)
    nU = int((deg == nr - 1).sum())
    nR = nr - nU
    if nR == 0:
        return maxcore, LB, nU, 0, "empty_universal" if nU > LB else "empty_incumbent"
    return maxcore, LB, nU, nR, "search_target_nonpositive" if LB - nU <= 0 else "search"
