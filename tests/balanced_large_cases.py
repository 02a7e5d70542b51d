"""Inputs of the large balanced-selection tests (test_balanced_large_cpu.py, test_gpu_balanced_large.py): every size follows from the constants
of csrc/lr_select.hip, read from its text, so that a changed constant moves the cases or fails here.  Cases are built from seeds and cached,
with the restatement's run of each (reference()): shared by the tests, never modified.  A case is what tests/balanced_cases.py calls one, plus
`expect` (what it must show) and, for the crafted ones, `planted`: what the CPU suite checks of the case's premise.

The crafted cases share one layout.  Candidate 0 is the origin and candidate 1 the point (1,..,1): they are never near a draw, so every column
spans [0, 1] throughout and a point is its candidate's fields.  The bulk lies in [0.05, 0.6]^6.  Planted candidates sit in pockets whose columns
1..5 are 0.72 or 0.92 -- 0.2 from each other, 0.26 from the bulk and 0.17 from candidate 1 in those columns alone -- so a draw next to a pocket
has exactly the pocket's candidates in its group, whatever column 0 does (the rescale cases move column 0 only)."""
import functools
import os
import re

import numpy as np

from tests import balanced_cases, balanced_cpu

ROOT = balanced_cases.ROOT
SRC = os.path.join(ROOT, "lidarregistration_amd", "csrc", "lr_select.hip")


def constants(text=None):
    """SEL_T, SEL_TS, SEL_PART_BLOCKS, SEL_MAX_N, SEL_MAX_SESSIONS; RESOLVE: the threads of sel_resolve_kernel (its launch bounds, its launch
    and every stride of its loops must agree); BEGIN: the same for sel_begin_kernel; WORD: the bits of a word of the mark map."""
    src = open(SRC).read() if text is None else text
    k = {}
    for name in ("SEL_T", "SEL_TS", "SEL_PART_BLOCKS", "SEL_MAX_N", "SEL_MAX_SESSIONS"):
        found = re.findall(r"^#\s*define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert len(found) == 1, (name, found)
        k[name] = int(found[0])
    for key, kernel, stride in (("RESOLVE", "sel_resolve_kernel", r"\+= (\d+)\)"), ("BEGIN", "sel_begin_kernel", r"(?<!\(size_t\))(?:gridDim|blockIdx)\.x \* (\d+)\b")):
        m = re.search(r"__launch_bounds__\((\d+)\)\s*void %s\(.*?\n\}\n" % kernel, src, re.S)
        assert m, kernel
        bound = int(m.group(1))
        strides = [int(s) for s in re.findall(stride, m.group(0))]
        launch = re.findall(r"hipLaunchKernelGGL\(%s, dim3\(\w+\), dim3\((\d+)\)" % kernel, src)
        assert len(strides) >= 3 and set(strides) == {bound} and launch == [str(bound)], (kernel, bound, strides, launch)
        k[key] = bound
    word = re.findall(r"hits\[SEL_T / (\d+)\]", src)
    assert len(word) >= 2 and len(set(word)) == 1, word
    k["WORD"] = int(word[0])
    return k


K = constants()
T, TS, WORD, R, WAVE = K["SEL_T"], K["SEL_TS"], K["WORD"], K["RESOLVE"], 64
CAP = K["SEL_PART_BLOCKS"] * K["BEGIN"]        # candidates one trip of sel_begin_kernel's grid sees (65 536)
MAX_N = K["SEL_MAX_N"]
MID = CAP + 4465                                # 70 001: past the cap, no multiple of 32
SIZES = (CAP - 1, CAP, CAP + 1, MID, 2 * CAP + 1)
THRESH = 0.1
MISS = [-1.0] * 6                               # a draw no candidate is near: the points lie in [0, 1]
EPS = 0.004                                     # a draw next to a pocket: this far off in every column (d = 0.0098)


def place(i):
    """(trip, wave, lane) of candidate i in sel_resolve_kernel's walk."""
    return (i // R, (i % R) // WAVE, i % WAVE)


# ---- random cases ------------------------------------------------------------------------------------------------------------------------
def redraw(p, seed, n_draws, far=0.0):
    """Draws for the case's present fields: half uniform, half next to a candidate; a share `far` of all moved out of the cube (sure misses)."""
    rng = np.random.default_rng(seed)
    f = p["fields"]
    lo, hi = f.min(axis=0), f.max(axis=0)
    draws = rng.uniform(0, 1, (n_draws, 6))
    near = rng.uniform(size=n_draws) < 0.5
    pts = (f[rng.integers(0, len(f), near.sum())] - lo) / (hi - lo)
    draws[near] = np.clip(pts + rng.normal(0, 0.03, pts.shape), 0, 1)
    draws[rng.uniform(size=n_draws) < far] += 2.0
    p["draws"] = draws
    return p


def size_case(n):
    p = balanced_cases.random_case(n, seed=n, n_draws=1500)
    return dict(p, n_request=200 + 25 * SIZES.index(n))


def span_case():
    """MID candidates, three of five draws sure misses: the 300 selections take more than SEL_T attempts."""
    p = redraw(balanced_cases.random_case(MID, seed=77, n_draws=1), 78, 2600, far=0.6)
    return dict(p, n_request=300)


def dense_sessions_case():
    """SEL_MAX_SESSIONS sessions of two candidates (the last of three) that lie next to each other; the draws come in pairs next to one session,
    so the second of a pair meets a mate of fullness 1/2 and, often, a farther neighbour of fullness 0."""
    ns = K["SEL_MAX_SESSIONS"]
    n = 2 * ns + 1
    rng = np.random.default_rng(4)
    scale = np.array([10, 10, 1, 2, 2, 90.0])
    base = rng.uniform(-5, 5, (ns, 6)) * scale
    session = np.minimum(np.arange(n) // 2, ns - 1).astype(np.int32)
    fields = base[session]
    fields[1::2, 0] += 0.02 * 10 * scale[0]
    fields[n - 1, 0] += 0.02 * 10 * scale[0]
    lo, hi = fields.min(axis=0), fields.max(axis=0)
    ks = rng.integers(0, ns, 450)
    draws = np.repeat((fields[2 * ks] - lo) / (hi - lo), 2, axis=0) + rng.normal(0, 0.01, (900, 6))
    return dict(fields=fields, session=session, n_cands=np.bincount(session, minlength=ns).astype(np.int32), n_request=300, draws=draws)


HOLDERS = {"first": lambda n: 0, "cap-1": lambda n: CAP - 1, "cap": lambda n: CAP, "last": lambda n: n - 1, "last_selected": lambda n: n - 1}


def extreme_case(n, where):
    """One column's minimum (holders `first`, `cap`) or maximum (`cap-1`, `last`) is held by one candidate alone, 0.27 of the column's span from
    everybody else: no draw selects it, and the extremes at the end are the ones the call opened with.  `last_selected`: the first draw is on it."""
    h = HOLDERS[where](n)
    p = balanced_cases.random_case(n, seed=n + 1, n_draws=1)
    f = p["fields"]
    col = sorted(HOLDERS).index(where) + 1
    lo, hi = f[:, col].min(), f[:, col].max()
    least = where in ("first", "cap")
    f[h, col] = lo - 0.37 * (hi - lo) if least else hi + 0.37 * (hi - lo)
    redraw(p, n + 2, 60)
    selected = where == "last_selected"
    if selected:
        p["draws"][0] = (f[h] - f.min(axis=0)) / (f.max(axis=0) - f.min(axis=0))
    return dict(p, n_request=12, planted=dict(holder=h, col=col, least=least, selected=selected),
                expect=dict(order_starts=[h], rescales=1, rescale_attempts=[1]) if selected else dict(rescales=0))


# ---- crafted cases: bulk, pockets -----------------------------------------------------------------------------------------------------------
def loc(k, c0=0.8):
    """Pocket k of 32."""
    return np.array([c0] + [0.92 if k >> b & 1 else 0.72 for b in range(5)])


def near(f, hi0=1.0):
    """A draw next to the candidate with fields f while column 0 spans [0, hi0]."""
    r = np.array(f, np.float64) + EPS
    r[0] = f[0] / hi0 + EPS
    return r


def crafted(n, seed, plant, draws, n_request, expect, n_sessions=3, bulk_session=None, **kw):
    """plant: {index: (fields, session or None)}."""
    rng = np.random.default_rng(seed)
    fields = rng.uniform(0.05, 0.6, (n, 6))
    fields[0], fields[1] = 0.0, 1.0
    session = (rng.integers(0, n_sessions, n) if bulk_session is None else np.full(n, bulk_session)).astype(np.int32)
    for i, (f, s) in plant.items():
        assert 2 <= i < n
        fields[i] = f
        if s is not None:
            session[i] = s
    return dict(fields=fields, session=session, n_cands=np.bincount(session, minlength=n_sessions).astype(np.int32), n_request=n_request,
                draws=np.array(draws, np.float64).reshape(-1, 6), expect=expect, **kw)


TIES = {"a_higher_lane": (40, R + 5), "a_lane_0_has_the_higher_index": (40, R), "b_higher_wave": (10 * WAVE + 60, 2 * R + 1), "c_trips_of_one_thread": (5, R + 5, 2 * R + 5),
        "d_three_waves_two_trips": (2 * WAVE + 2, R + WAVE + 6, R + 3 * WAVE + 2)}
TIE_NAMES = sorted(TIES) + ["e_fullness_beats_index", "f_quotients_then_d", "f_quotients_then_index", "g_fullness_beats_d_in_a_wave"]
TIE_N = 4 * R + 1                                # 4 097


def tie_case(name, base):
    """base 0: TIE_N candidates; base CAP: MID candidates and every planted index above CAP.  planted["tied"]: the candidates of the tied group
    in index order, planted["at"]: the attempt (0-based) whose group they are."""
    n = TIE_N if base == 0 else MID
    assert base % R == 0 and base + 3 * R < n
    b = lambda *idx: [base + i for i in idx]
    A, B = b(10 * WAVE + 60, 2 * R + 1)                                  # 700 (wave 10) and 2 049 (wave 0, two trips later)
    if name in TIES:
        idx = b(*TIES[name])
        return crafted(n, 31, {i: (loc(3), 0) for i in idx}, [MISS] * 3 + [near(loc(3))] * len(idx) + [MISS], len(idx),
                       dict(status=0, order=idx, attempts=3 + len(idx)), planted=dict(tied=idx, at=3, equal_d=True))
    if name == "e_fullness_beats_index":
        (Z,) = b(300)
        return crafted(n, 32, {Z: (loc(5), 0), A: (loc(3), 0), B: (loc(3), 1)}, [near(loc(5)), MISS, near(loc(3)), near(loc(3))], 3,
                       dict(status=0, order=[Z, B, A], attempts=4), planted=dict(tied=[A, B], at=2, equal_d=True, fullness_differs=True))
    if name == "g_fullness_beats_d_in_a_wave":
        Z, C, D = b(300, 40, R + 5)                                      # C: lane 40, nearer, fuller session; D: lane 5 of the same wave
        far = loc(3); far[1] += 0.03
        return crafted(n, 33, {Z: (loc(5), 0), C: (loc(3), 0), D: (far, 1)}, [near(loc(5)), near(loc(3)), near(loc(3))], 3,
                       dict(status=0, order=[Z, D, C], attempts=3), planted=dict(tied=[C, D], at=1, equal_d=False, fullness_differs=True))
    # sessions 1 and 2 have two and four candidates: one and two selections make them 1/2 and 2/4
    P, Q1, Q2, W = b(100, 200, 201, 3000)
    y = loc(3)
    if name == "f_quotients_then_d":
        y = loc(3); y[1] += 0.006                                        # the higher index is the nearer one
    pl = {P: (loc(1), 1), A: (loc(3), 1), Q1: (loc(2), 2), Q2: (loc(4), 2), B: (y, 2), W: (loc(8), 2)}
    order = [P, Q1, Q2] + ([A, B] if name == "f_quotients_then_index" else [B, A])
    return crafted(n, 34, pl, [near(loc(1)), near(loc(2)), MISS, near(loc(4)), near(loc(3)), near(loc(3))], 5, dict(status=0, order=order, attempts=6),
                   bulk_session=0, planted=dict(tied=[A, B], at=4, equal_d=name == "f_quotients_then_index", quotients=((1, 2), (2, 4))))


RESCALE_AT = 37                                  # the holder goes at this attempt (0-based) of the round
HI0 = 1.25                                       # column 0 spans [0, 1.25] while the holder lives, [0, 1] afterwards


def rescale_case(kind):
    """MID candidates; the holder of column 0's maximum, near the end, is selected at attempt RESCALE_AT.  `marked_then_miss`: the next draw is
    next to X's old point and 0.146 from its new one.  `unmarked_then_hit`: the next draw is next to X's new point and 0.154 from its old one.
    planted: holder, x, and the two attempts (0-based) that follow."""
    H, X, Z = MID - 2, CAP + R + 77, CAP + 3 * R + 9
    pl = {H: (loc(6, HI0), None), X: (loc(9, 0.75), None), Z: (loc(12, 0.3), None)}
    head = [MISS] * RESCALE_AT + [near(loc(6, HI0), HI0)]
    t = RESCALE_AT
    if kind == "marked_then_miss":
        draws = head + [near(loc(9, 0.75), HI0)] + [MISS] * 3 + [near(loc(9, 0.75))] + [MISS, near(loc(12, 0.3))]
        exp = dict(status=0, order=[H, X, Z], attempts=t + 8, misses=t + 5, rescales=1, rescale_attempts=[t + 1])
    else:
        draws = head + [near(loc(9, 0.75))] + [MISS] * 2 + [near(loc(12, 0.3))]
        exp = dict(status=0, order=[H, X, Z], attempts=t + 5, misses=t + 2, rescales=1, rescale_attempts=[t + 1])
    return crafted(MID, 35, pl, draws, 3, exp, planted=dict(holder=H, x=X, next=t + 1, kind=kind))


MARK_ATTEMPTS = (WORD - 1, WORD, 2 * WORD - 1, 2 * WORD, T - 1, T)       # 31, 32, 63, 64, SEL_T - 1 and the first of the next round


def marks_case(n, variant):
    """Six lone candidates hit at the mark map's word boundaries, misses in between.  `dead_mark`: the draw at the third of them is the
    second's again -- marked by a candidate that is committed by then -- and five are selected."""
    base = 0 if n < CAP else CAP
    idx = [base + i for i in (3, WAVE, R - 1, R, 2 * R - 1, 2 * R)]
    assert idx[-1] < n
    pl = {i: (loc(16 + k), None) for k, i in enumerate(idx)}
    draws = [MISS] * (T + 4)
    for k, a in enumerate(MARK_ATTEMPTS):
        draws[a] = near(loc(16 + k))
    order = list(idx)
    if variant == "dead_mark":
        draws[MARK_ATTEMPTS[2]] = draws[MARK_ATTEMPTS[1]]
        del order[2]
    return crafted(n, 36, pl, draws, len(order), dict(status=0, order=order, attempts=T + 1, misses=T + 1 - len(order), rescales=0),
                   planted=dict(hits=[a for k, a in enumerate(MARK_ATTEMPTS) if variant != "dead_mark" or k != 2], dead=variant == "dead_mark"))


def limit_case():
    """SEL_MAX_N candidates over 7 sessions: the minimum of every column at index 0, column 0's maximum at the last index alone, duplicates at
    MAX_N - 3 R - 7 and MAX_N - 11 (another thread's last trip), one draw on the last candidate, then seven selections out of the bulk."""
    n = MAX_N
    L, D1, D2, X = n - 1, n - 3 * R - 7, n - 11, n - R - 300
    pl = {L: (loc(6, HI0), None), D1: (loc(3), 2), D2: (loc(3), 2), X: (loc(9, 0.75), None)}
    p = crafted(n, 37, pl, [MISS], 11, dict(status=0, attempts=12, rescales=1, rescale_attempts=[4], order_starts=[D1, D2, L, X]), n_sessions=7,
                planted=dict(tied=[D1, D2], at=1, last=L, x=X))
    rng = np.random.default_rng(38)
    # column 0 spans [0, 1.25] until the last candidate goes at the fourth attempt; the bulk's draws come after it
    head = [MISS, near(loc(3), HI0), near(loc(3), HI0), near(loc(6, HI0), HI0), near(loc(9, 0.75))]
    bulk = [p["fields"][i] + rng.normal(0, 0.01, 6) for i in rng.integers(2, n - 4 * R, 12)]
    p["draws"] = np.array(head + bulk, np.float64)
    return p


MIRROR_CHUNK = T + T // 4                      # draws per chunk of the mirror's second run: a round (status 4), the rest (status 1), a new chunk


def mirror_case():
    """MID candidate rows [n, 27] over 3 sessions, the six fields uniform: every third or fourth uniform draw hits."""
    rng = np.random.default_rng(39)
    n_cands = [MID // 3, MID // 3 + 1000, MID - 2 * (MID // 3) - 1000]
    rows = np.zeros((MID, 27))
    rows[:, 0] = np.repeat([4, 9, 11], n_cands)
    rows[:, 1] = np.arange(MID)
    rows[:, 2] = rows[:, 1] + 5
    rows[:, 19:25] = rng.uniform(-5, 5, (MID, 6)) * np.array([10, 10, 1, 2, 2, 90])
    rows[:, 25:] = rng.uniform(0.2, 1, (MID, 2))
    return dict(rows=rows, n_cands=np.array(n_cands, np.int32), sizes=[300, 100], seed=91)


BUILDERS = {"span": span_case, "dense_sessions": dense_sessions_case, "limit": limit_case}
BUILDERS.update({"size_%d" % n: functools.partial(size_case, n) for n in SIZES})
BUILDERS.update({"extreme_%d_%s" % (n, w): functools.partial(extreme_case, n, w) for n in (CAP + 1, MID) for w in HOLDERS})
BUILDERS.update({"tie_%s_%d" % (name, base): functools.partial(tie_case, name, base) for name in TIE_NAMES for base in (0, CAP)})
BUILDERS.update({"rescale_%s" % k: functools.partial(rescale_case, k) for k in ("marked_then_miss", "unmarked_then_hit")})
BUILDERS.update({"marks_%d_%s" % (n, v): functools.partial(marks_case, n, v) for n in (2 * R + 1, MID) for v in ("all_live", "dead_mark")})


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's run of the case, with `fields64` as tests/test_gpu_balanced.py::same wants it."""
    p = case(name)
    ref = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"], thresh=THRESH)
    ref["fields64"] = p["fields"]
    return ref


def check_expect(name, st):
    """The counters and the order the case states, on a restatement or a device state."""
    for key, want in case(name).get("expect", {}).items():
        if key == "order_starts":
            assert list(st["order"][:len(want)]) == want, (name, key)
        elif key == "rescales_at_least":
            assert st["rescales"] >= want, (name, key)
        elif key in st:
            got = st[key]
            assert (list(got) if isinstance(want, list) else got) == want, (name, key, got, want)


def distances_at(p, removed, draw):
    """(indices alive, d) of one draw after the candidates `removed` are gone, by the restatement's S1 and S2."""
    alive = np.ones(len(p["fields"]), bool)
    alive[list(removed)] = False
    ext = balanced_cpu.extremes(p["fields"], alive)
    idx = np.flatnonzero(alive)
    return idx, balanced_cpu.distances(np.asarray(draw, np.float64), balanced_cpu.cube_points(p["fields"][idx], *ext))


@functools.lru_cache(maxsize=None)
def mirror_reference():
    """select_balanced_set by the restatement: the attempts drawn from the legacy generator, the subsets split from it."""
    m = case_mirror()
    rows, n_cands = m["rows"], m["n_cands"]
    saved = np.random.get_state()
    np.random.seed(m["seed"])
    st = None
    while st is None or st["status"] == balanced_cpu.DRAWS:
        st = balanced_cpu.select(rows[:, 19:25], np.repeat(np.arange(3), n_cands), n_cands, sum(m["sizes"]), np.random.rand(512, 6), st)
    np.random.seed(m["seed"])
    np.random.rand(st["attempts"], 6)
    subsets = balanced_cpu.split_subsets(rows[np.array(st["order"])], m["sizes"])
    np.random.set_state(saved)
    return st, subsets


@functools.lru_cache(maxsize=None)
def case_mirror():
    return mirror_case()
