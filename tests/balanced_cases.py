"""Inputs of the balanced-selection tests (test_balanced_cpu.py, test_gpu_balanced.py): the recorded reference runs and small crafted cases,
each named after the branch of contract S it exercises.  A case: fields [n,6], session [n], n_cands [S], n_request, draws [k,6], optionally
thresh, and `expect`: what the case must show (checked on the restatement by the CPU suite, on the device by the GPU suite)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g21_balanced.npz"))
T = 1024                     # attempts per round of lr_balanced_select (SEL_T in csrc/lr_select.hip)
MISS = [0.6] * 6             # a draw no candidate of the diagonal cases is near


def list_candidates():
    """The Apollo list fixture as 27-column candidate rows, as tests/golden/make_golden_balanced.py builds them; the six fields are the stored ones."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "lists", "ApolloSouthbay_test.npz"))
    ov = z["overlap"].astype(np.float64)
    return np.concatenate([z["session"][:, None].astype(np.float64), z["src"][:, None], z["tgt"][:, None], z["T_gt"].astype(np.float64), GOLD["fields"],
                           ov[:, None], ov[:, None]], axis=1)


def dense(cands):
    """(cands, dense session id per row, candidates per session) for rows grouped by ascending session."""
    ids, session, n_cands = np.unique(cands[:, 0], return_inverse=True, return_counts=True)
    assert (np.diff(cands[:, 0]) >= 0).all()
    return cands, session.astype(np.int32), n_cands.astype(np.int32)


def g21a():
    return dense(list_candidates()[GOLD["a/rows"]])


def g21b():
    return dense(list_candidates())


def diag(t):
    return [float(t)] * 6


def case(fields, session, n_cands, n_request, draws, expect, **kw):
    return dict(fields=np.array(fields, np.float64).reshape(-1, 6), session=np.array(session, np.int32), n_cands=np.array(n_cands, np.int32),
                n_request=int(n_request), draws=np.array(draws, np.float64).reshape(-1, 6), expect=expect, **kw)


def corners():
    """Two candidates that pin every column's range to [0, 1]: the points are then the fields themselves."""
    return [diag(0.0), diag(1.0)]


def _ulp_neighbours():
    """Three candidates whose distances to one draw are consecutive doubles: found by stepping the first coordinate ulp by ulp."""
    from tests import balanced_cpu
    r = np.array([0.3, 0.31, 0.29, 0.33, 0.3, 0.32])
    x0 = np.array([0.301, 0.33, 0.27, 0.35, 0.32, 0.30])
    d0 = balanced_cpu.distances(r, x0[None])[0]
    want = {-1: np.nextafter(d0, 0.0), 0: d0, 1: np.nextafter(d0, 1.0)}
    found = {0: x0}
    x = x0.copy()
    for step, toward in ((-1, 0.0), (1, 1.0)):          # d grows with the first coordinate (x0[0] > r[0])
        x = x0.copy()
        for _ in range(4000):
            x[0] = np.nextafter(x[0], toward)
            d = balanced_cpu.distances(r, x[None])[0]
            if d == want[step]:
                found[step] = x.copy()
                break
        assert step in found
    return r, found, d0


def crafted_cases():
    c = {}
    lone = corners() + [diag(0.3)]
    hit = [0.301] * 6
    for name, h in (("first_hit_at_T-1", T - 1), ("first_hit_at_T", T), ("first_hit_at_T+1", T + 1)):
        c[name] = case(lone, [0, 0, 0], [3], 1, [MISS] * h + [hit] + [MISS] * 7, dict(status=0, order=[2], attempts=h + 1, misses=h, consumed=h + 1))
    h = T + 37
    c["hit_at_last_draw"] = case(lone, [0, 0, 0], [3], 2, [MISS] * h + [hit], dict(status=1, order=[2], attempts=h + 1, misses=h, consumed=h + 1))
    c["no_hit_at_all"] = case(lone, [0, 0, 0], [3], 1, [MISS] * (3 * T + 5), dict(status=1, order=[], attempts=3 * T + 5, misses=3 * T + 5, consumed=3 * T + 5))
    c["request_0"] = case(lone, [0, 0, 0], [3], 0, [hit] * 3, dict(status=0, order=[], attempts=0, consumed=0))
    c["request_1"] = case(lone, [0, 0, 0], [3], 1, [hit] * 3, dict(status=0, order=[2], attempts=1, consumed=1))
    # N - 1 of N = 3: the second commit leaves one candidate alive -- status 2 with the commit kept
    c["request_N-1"] = case(lone, [0, 0, 0], [3], 2, [hit, MISS, [0.01] * 6, hit], dict(status=2, order=[2, 0], attempts=3, misses=1, consumed=3))
    # sessions of different fullness: the second draw is nearest to candidate 3 (session 0, fullness 1/4) but candidate 4 (session 1, 0/1) is taken
    c["fullness_beats_distance"] = case(corners() + [diag(0.30), diag(0.31), diag(0.33)], [0, 0, 0, 0, 1], [4, 1], 2, [diag(0.30), diag(0.31)],
                                        dict(status=0, order=[2, 4]))
    # 1/2 and 2/4 are the same fullness: the nearer candidate wins although it has the higher index and the other session
    pts = corners() + [diag(0.10), diag(0.50), diag(0.20), diag(0.30), diag(0.52), diag(0.80)]
    c["equal_fullness_from_different_quotients"] = case(pts, [2, 2, 0, 0, 1, 1, 1, 1], [2, 4, 2], 4, [diag(0.10), diag(0.20), diag(0.30), diag(0.515)],
                                                        dict(status=0, order=[2, 4, 5, 6]))
    c["duplicates_lowest_index_first"] = case(corners() + [diag(0.4), diag(0.4), diag(0.4)], [0] * 5, [5], 3, [diag(0.41)] * 3, dict(status=0, order=[2, 3, 4]))
    # one ulp below thresh is in the group, at thresh and one ulp above are not -- though their session is the emptier one
    r, found, d0 = _ulp_neighbours()
    c["one_ulp_around_thresh"] = case(corners() + [diag(0.8), found[-1], found[0], found[1]], [0, 0, 0, 0, 1, 1], [4, 2], 2, [diag(0.8), r],
                                      dict(status=0, order=[2, 3]), thresh=float(d0))
    c["at_thresh_is_a_miss"] = case(corners() + [found[0], found[1]], [0, 0, 0, 0], [4], 1, [r], dict(status=1, order=[], misses=1), thresh=float(d0))
    # the holder of a column's minimum goes: column 0 spans [0.2, 1] afterwards and the second draw hits candidate 3 only because of it
    c["minimum_holder_removed"] = case([[0.2, 0, 0, 0, 0, 0], diag(1.0), [0.0, .5, .5, .5, .5, .5], [0.4, .8, .8, .8, .8, .8]], [0] * 4, [4], 2,
                                       [[0.0, .5, .5, .5, .5, .5], [0.25, .8, .8, .8, .8, .8]], dict(status=0, order=[2, 3], rescales=1, attempts=2))
    c["minimum_holder_kept"] = case([[0.2, 0, 0, 0, 0, 0], diag(1.0), [0.0, .5, .5, .5, .5, .5], [0.4, .8, .8, .8, .8, .8]], [0] * 4, [4], 1,
                                    [[0.25, .8, .8, .8, .8, .8], MISS], dict(status=1, order=[], rescales=0))
    c["maximum_holder_removed"] = case([diag(0.0), [0.8, 1, 1, 1, 1, 1], [1.0, .5, .5, .5, .5, .5], [0.4, .2, .2, .2, .2, .2]], [0] * 4, [4], 2,
                                       [[1.0, .5, .5, .5, .5, .5], [0.5, .2, .2, .2, .2, .2]], dict(status=0, order=[2, 3], rescales=1, attempts=2))
    # two hits inside one round: attempt 9 is near candidate 2 as well, which attempt 5 took
    two = corners() + [diag(0.3), diag(0.7)]
    draws = [MISS] * 30
    draws[5], draws[9], draws[20] = diag(0.301), diag(0.299), diag(0.701)
    c["second_hit_only_before_first_commit"] = case(two, [0] * 4, [4], 2, draws, dict(status=0, order=[2, 3], attempts=21, misses=19))
    return c


def status_cases():
    """S's deviation and the device-side refusals."""
    c = {}
    hit = [0.301] * 6
    const = np.array(corners() + [diag(0.3)]); const[:, 4] = 0.5
    c["constant_column"] = dict(fields=const, status=2, order=[], consumed=0)
    nanf = np.array(corners() + [diag(0.3)]); nanf[2, 1] = np.nan
    c["nan_field"] = dict(fields=nanf, status=2, order=[], consumed=0)
    inff = np.array(corners() + [diag(0.3)]); inff[1, 3] = np.inf
    c["inf_field"] = dict(fields=inff, status=2, order=[], consumed=0)
    c["one_candidate"] = dict(fields=np.array([diag(0.3)]), session=[0], n_cands=[1], status=2, order=[], consumed=0)
    c["last_candidate"] = dict(fields=np.array(corners()), session=[0, 0], n_cands=[2], draws=[MISS, [0.99] * 6, hit], n_request=2, status=2, order=[1], consumed=2)
    c["session_too_large"] = dict(fields=np.array(corners() + [diag(0.3)]), session=[0, 1, 0], n_cands=[3], status=3, order=[], consumed=0)
    c["session_negative"] = dict(fields=np.array(corners() + [diag(0.3)]), session=[0, -1, 0], n_cands=[3], status=3, order=[], consumed=0)
    c["session_without_candidates"] = dict(fields=np.array(corners() + [diag(0.3)]), session=[0, 1, 0], n_cands=[3, 0], status=3, order=[], consumed=0)
    for p in c.values():
        p.setdefault("session", [0] * len(p["fields"])); p.setdefault("n_cands", [len(p["fields"])]); p.setdefault("n_request", 1)
        p.setdefault("draws", [hit] * 4)
        p["draws"] = np.array(p["draws"], np.float64)
    return c


def random_case(n, seed, n_sessions=3, n_draws=600, sparse=False):
    """n random candidates; half of the draws fall near a candidate's starting point, so that small sets get hits."""
    rng = np.random.default_rng(seed)
    fields = rng.uniform(-5, 5, (n, 6)) * np.array([10, 10, 1, 2, 2, 90])
    if sparse:
        session = rng.choice(np.array([0, 1, 255, 256, 4095, 32768, 65534, 65535]), n).astype(np.int32)
        n_cands = rng.integers(1, 5, n_sessions).astype(np.int32)
    else:
        session = np.sort(rng.integers(0, n_sessions, n)).astype(np.int32)
        n_cands = np.maximum(np.bincount(session, minlength=n_sessions), 1).astype(np.int32)
    lo, hi = fields.min(axis=0), fields.max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pts = np.nan_to_num((fields - lo) / (hi - lo), nan=0.5)
    draws = rng.uniform(0, 1, (n_draws, 6))
    near = rng.uniform(size=n_draws) < 0.5
    draws[near] = np.clip(pts[rng.integers(0, n, near.sum())] + rng.normal(0, 0.03, (near.sum(), 6)), 0, 1)
    return dict(fields=fields, session=session, n_cands=n_cands, draws=draws)
