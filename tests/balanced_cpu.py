"""Contract S (include/lidarreg.h) in numpy: one attempt of the balanced-set selection at a time, in this project's own words.
What lr_balanced_select is compared with exactly, and what itself equals the reference's recorded run (tests/golden/g21_balanced.npz) in
order, counters and file bytes.  float64 throughout; numpy fuses nothing."""
import numpy as np

OK, DRAWS, DEGENERATE, BAD_SESSION, ROUNDS = 0, 1, 2, 3, 4


def extremes(fields, alive):
    """(m [6], M [6]) over the alive candidates, or None where S's deviation holds: a column whose M - m is not a positive finite number."""
    f = fields[alive]
    if len(f) == 0:
        return None
    with np.errstate(invalid="ignore"):
        m, M = f.min(axis=0), f.max(axis=0)
        w = M - m
    return (m, M) if (np.isfinite(w) & (w > 0.0)).all() else None


def cube_points(fields, m, M):
    """S1: both operations correctly rounded."""
    return (fields - m) / (M - m)


def distances(r, points):
    """S2: the six squares summed from the left."""
    e = r[None, :] - points
    q = e * e
    return np.sqrt(((((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]) + q[:, 4]) + q[:, 5])


def new_state(n, n_sessions):
    return dict(alive=np.ones(n, bool), n_sel=np.zeros(n_sessions, np.int64), order=[], attempts=0, misses=0, rescales=0, rescale_attempts=[],
                status=None, consumed=0)


def select(fields, session, n_cands, n_request, draws, state=None, thresh=0.1):
    """Runs attempts over `draws` [k,6] until a stop rule fires; returns the state (a dict; pass it back in to go on with the next draws).
    status: 0 = n_request selected, 1 = draws used up, 2 = S's deviation, 3 = a session id out of range or without candidates."""
    fields = np.ascontiguousarray(fields, np.float64).reshape(-1, 6)
    session = np.asarray(session, np.int64).reshape(-1)
    n_cands = np.asarray(n_cands, np.int64).reshape(-1)
    draws = np.ascontiguousarray(draws, np.float64).reshape(-1, 6)
    n = len(fields)
    st = new_state(n, len(n_cands)) if state is None else state
    st["consumed"] = 0
    if n and (session.min() < 0 or session.max() >= len(n_cands) or (n_cands[session] < 1).any()):
        st["status"] = BAD_SESSION
        return st
    if n_request == 0 or len(st["order"]) == n_request:
        st["status"] = OK
        return st
    ext = extremes(fields, st["alive"])
    if ext is None:
        st["status"] = DEGENERATE
        return st
    # the alive candidates, compacted: original index, point, session -- rebuilt only when the extremes move, cut at every commit
    idx = np.flatnonzero(st["alive"])
    pts = cube_points(fields[idx], *ext)
    k = 0
    while True:
        if k == len(draws):
            st["status"] = DRAWS
            return st
        d = distances(draws[k], pts)
        k += 1
        st["consumed"] = k
        st["attempts"] += 1
        group = np.flatnonzero(d < thresh)
        if len(group) == 0:
            st["misses"] += 1
            continue
        s = session[idx[group]]
        fullness = st["n_sel"][s].astype(np.float64) / n_cands[s].astype(np.float64)
        # the lexicographic minimum of (fullness, d, original index): idx ascends, so position order is index order
        best = group[np.lexsort((idx[group], d[group], fullness))[0]]
        chosen = int(idx[best])
        st["n_sel"][session[chosen]] += 1
        st["alive"][chosen] = False
        st["order"].append(chosen)
        held = (fields[chosen] == ext[0]).any() or (fields[chosen] == ext[1]).any()
        idx = np.delete(idx, best)
        pts = np.delete(pts, best, axis=0)
        if held:
            new = extremes(fields, st["alive"])
            if new is None:
                st["status"] = DEGENERATE
                return st
            if not (np.array_equal(new[0], ext[0]) and np.array_equal(new[1], ext[1])):
                st["rescales"] += 1
                st["rescale_attempts"].append(st["attempts"])
                ext = new
                pts = cube_points(fields[idx], *ext)
        if len(st["order"]) == n_request:
            st["status"] = OK
            return st


def save_set_bytes(rows):
    """The pair-list file of a registration set [k,27] as the reference writes it: sorted by source index, then stably by session; three
    integers, then %.16f."""
    names = "session_ind src_ind tgt_ind " + " ".join(f"mot{k}" for k in range(16)) + " trans_x trans_y trans_z roll pitch yaw overlap overlap_symmetric"
    rows = rows[np.argsort(rows[:, 1])]
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    lines = [names]
    for row in rows:
        lines.append("%d %d %d " % (row[0], row[1], row[2]) + " ".join("%.16f" % v for v in row[3:]))
    return ("\n".join(lines) + "\n").encode()


def split_subsets(rows, sizes):
    """The subset split: np.random.choice on the global generator, without replacement, each subset cut out of what is left."""
    out = []
    for size in sizes:
        pick = np.zeros(len(rows), bool)
        pick[np.random.choice(len(rows), size, replace=False)] = True
        out.append(rows[pick])
        rows = rows[~pick]
    return out
