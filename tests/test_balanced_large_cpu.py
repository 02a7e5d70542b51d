"""The premises of the large balanced-selection cases (tests/balanced_large_cases.py), on the numpy restatement of contract S: the sizes follow
from the constants of csrc/lr_select.hip, every crafted case has the group, the tie, the (trip, wave, lane) places, the marks and the distances
either side of thresh that it claims, and every random case gets all it requests.  No GPU."""
import numpy as np
import pytest

from tests import balanced_cpu
from tests import balanced_large_cases as L

GAP = 1e-6                   # every distance a crafted case relies on stays this far from thresh


def test_constants_and_sizes():
    assert L.K == dict(L.K, SEL_T=1024, SEL_TS=64, SEL_PART_BLOCKS=256, SEL_MAX_N=1 << 22, RESOLVE=1024, BEGIN=256, WORD=32), \
        "a constant of lr_select.hip changed: the sizes below move with it -- look at them again, then update this line"
    assert L.T % L.TS == 0 and L.TS % L.WORD == 0 and L.R % L.WAVE == 0 and L.CAP % L.R == 0
    # the begin kernel's grid is capped: a second trip only past CAP, a full set of partials from CAP - BEGIN + 1 on
    assert L.SIZES == (L.CAP - 1, L.CAP, L.CAP + 1, L.MID, 2 * L.CAP + 1) and L.CAP < L.MID < 2 * L.CAP
    assert (L.CAP + 1) % 32 and L.MID % 32 and L.MAX_N % 32 == 0            # n_pad != n twice
    assert L.TIE_N > 4 * L.R and L.MID > L.CAP + 3 * L.R
    # a text with another constant is read as such, and one whose strides disagree is refused
    text = open(L.SRC).read()
    assert L.constants(text.replace("#define SEL_PART_BLOCKS  256", "#define SEL_PART_BLOCKS  128"))["SEL_PART_BLOCKS"] == 128
    with pytest.raises(AssertionError):
        L.constants(text.replace("i += 1024)", "i += 512)", 1))
    with pytest.raises(AssertionError):
        L.constants(text.replace("__launch_bounds__(1024) void sel_resolve_kernel", "__launch_bounds__(512) void sel_resolve_kernel"))


@pytest.mark.parametrize("name", ["size_%d" % n for n in L.SIZES] + ["span", "dense_sessions"])
def test_random_cases_get_all_they_request(name):
    p, ref = L.case(name), L.reference(name)
    assert ref["status"] == 0 and len(ref["order"]) == p["n_request"] >= 200 and ref["consumed"] == ref["attempts"] <= len(p["draws"])
    assert max(ref["order"]) >= L.CAP or len(p["fields"]) < L.MID           # somebody past the cap is selected where thousands lie there
    if name == "span":
        assert ref["attempts"] > L.T and ref["misses"] > L.T // 2


def test_dense_sessions_fullness_decides():
    """Two candidates per session: with every candidate in one session instead (fullness equal throughout) another order comes out, and up to
    the first difference the states are the same -- there the fullness decided."""
    p, ref = L.case("dense_sessions"), L.reference("dense_sessions")
    assert len(p["n_cands"]) == L.K["SEL_MAX_SESSIONS"] and set(p["n_cands"][:-1]) == {2} and p["n_cands"][-1] == 3
    flat = balanced_cpu.select(p["fields"], np.zeros(len(p["fields"]), np.int32), [len(p["fields"])], p["n_request"], p["draws"])
    differ = [k for k, (a, b) in enumerate(zip(ref["order"], flat["order"])) if a != b]
    assert differ and differ[0] < 100
    assert (ref["n_sel"] == 2).sum() >= 20 and ref["n_sel"].max() <= 3


@pytest.mark.parametrize("n", (L.CAP + 1, L.MID))
@pytest.mark.parametrize("where", sorted(L.HOLDERS))
def test_extreme_cases(n, where):
    name = "extreme_%d_%s" % (n, where)
    p, ref = L.case(name), L.reference(name)
    h, col, f = p["planted"]["holder"], p["planted"]["col"], p["fields"]
    assert h == {"first": 0, "cap-1": L.CAP - 1, "cap": L.CAP}.get(where, n - 1)
    others = np.delete(f[:, col], h)
    assert f[h, col] < others.min() if p["planted"]["least"] else f[h, col] > others.max()
    assert all((np.delete(f[:, c], h).min() < f[h, c] < np.delete(f[:, c], h).max()) for c in range(6) if c != col)      # held solely, and nothing else
    assert ref["status"] == 0 and ref["attempts"] >= 1
    L.check_expect(name, ref)
    if p["planted"]["selected"]:
        assert ref["order"][0] == h and ref["rescale_attempts"] == [1] and len(ref["order"]) == 12
    else:
        assert ref["alive"][h] and ref["rescales"] == 0


def removed_before(ref_order, p, attempt):
    """The candidates a crafted case has selected before the 0-based attempt: its draws before that one that hit, in the stated order."""
    hits = [k for k in range(attempt) if p["draws"][k][0] > 0]
    return list(ref_order[:len(hits)])


@pytest.mark.parametrize("base", (0, L.CAP))
@pytest.mark.parametrize("name", L.TIE_NAMES)
def test_tie_cases(name, base):
    full = "tie_%s_%d" % (name, base)
    p, ref = L.case(full), L.reference(full)
    L.check_expect(full, ref)
    pl = p["planted"]
    tied, at = pl["tied"], pl["at"]
    assert len(p["fields"]) == (L.TIE_N if base == 0 else L.MID) and min(tied) > base and tied == sorted(tied)
    gone = removed_before(ref["order"], p, at)
    idx, d = L.distances_at(p, gone, p["draws"][at])
    assert list(idx[d < L.THRESH]) == tied                                   # S3: the group is the planted candidates and nobody else
    assert np.abs(d - L.THRESH).min() >= GAP
    dt = d[np.searchsorted(idx, tied)]
    assert (len(set(dt.view(np.uint64).tolist())) == 1) == pl["equal_d"]
    if pl["equal_d"]:
        assert all(np.array_equal(p["fields"][tied[0]], p["fields"][i]) for i in tied)
    n_sel = np.bincount(p["session"][gone], minlength=3) if gone else np.zeros(3, int)
    fullness = n_sel[p["session"][tied]] / p["n_cands"][p["session"][tied]]
    assert (len(set(fullness.tolist())) > 1) == bool(pl.get("fullness_differs"))
    places = [L.place(i) for i in tied]
    lo, hi = places[0], places[-1]                                           # of the lowest and of the highest index
    if name.startswith("a_"):
        assert lo[1] == hi[1] and lo[2] > hi[2] and lo[0] != hi[0]           # one wave, the lower index in the higher lane
        assert (hi[2] == 0) == (name == "a_lane_0_has_the_higher_index")     # lane 0 is where the wave's reduction is read
    elif name == "b_higher_wave":
        assert lo[1] > hi[1]
    elif name == "c_trips_of_one_thread":
        assert [q[0] - lo[0] for q in places] == [0, 1, 2] and len({q[1:] for q in places}) == 1
    elif name == "d_three_waves_two_trips":
        assert len({q[1] for q in places}) == 3 and len({q[0] for q in places}) == 2 and places[0][1] > places[1][1]
    elif name == "e_fullness_beats_index":
        assert lo[1] > hi[1] and fullness[1] < fullness[0] and ref["order"][1:] == [tied[1], tied[0]]
    elif name == "g_fullness_beats_d_in_a_wave":
        assert lo[1] == hi[1] and lo[2] > hi[2] and fullness[1] < fullness[0] and dt[1] - dt[0] >= GAP and ref["order"][1] == tied[1]
    else:
        assert pl["quotients"] == ((1, 2), (2, 4)) and [(int(n_sel[s]), int(p["n_cands"][s])) for s in (1, 2)] == [(1, 2), (2, 4)]
        assert fullness[0] == fullness[1] == 0.5 and lo[1] != hi[1]
        if name == "f_quotients_then_d":
            assert dt[0] - dt[1] >= GAP and ref["order"][3] == tied[1]       # the nearer one has the higher index
        else:
            assert ref["order"][3] == tied[0]


@pytest.mark.parametrize("kind", ("marked_then_miss", "unmarked_then_hit"))
def test_rescale_cases(kind):
    name = "rescale_" + kind
    p, ref = L.case(name), L.reference(name)
    L.check_expect(name, ref)
    H, X, t1 = p["planted"]["holder"], p["planted"]["x"], p["planted"]["next"]
    assert H > L.CAP + 4 * L.R and X > L.CAP and L.place(X)[0] > L.CAP // L.R and 0 < t1 < L.T - 1       # inside a round, the points rewritten over many trips
    assert ref["order"][0] == H and ref["rescale_attempts"] == [t1] and ref["attempts"] > t1
    assert p["fields"][H, 0] == np.delete(p["fields"][:, 0], H).max() * L.HI0
    idx, d = L.distances_at(p, [], p["draws"][t1 - 1])
    assert list(idx[d < L.THRESH]) == [H] and np.abs(d - L.THRESH).min() >= GAP
    old = L.distances_at(p, [], p["draws"][t1])                              # the holder still there: the points the round was evaluated with
    new = L.distances_at(p, [H], p["draws"][t1])
    group = lambda r: list(r[0][r[1] < L.THRESH])
    assert min(np.abs(old[1] - L.THRESH).min(), np.abs(new[1] - L.THRESH).min()) >= GAP
    if kind == "marked_then_miss":
        assert group(old) == [X] and group(new) == [] and ref["order"][1] == X
    else:
        assert group(old) == [] and group(new) == [X] and ref["order"][1] == X and ref["attempts"] - t1 >= 2
        # selected at exactly that attempt: a run over the draws up to it has X, one draw fewer has not
        cut = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], 3, p["draws"][:t1 + 1])
        assert cut["order"] == [H, X] and balanced_cpu.select(p["fields"], p["session"], p["n_cands"], 3, p["draws"][:t1])["order"] == [H]


@pytest.mark.parametrize("variant", ("all_live", "dead_mark"))
@pytest.mark.parametrize("n", (2 * L.R + 1, L.MID))
def test_marks_cases(n, variant):
    name = "marks_%d_%s" % (n, variant)
    p, ref = L.case(name), L.reference(name)
    L.check_expect(name, ref)
    assert L.MARK_ATTEMPTS == (31, 32, 63, 64, L.T - 1, L.T)
    marked = [k for k in range(len(p["draws"])) if p["draws"][k][0] > 0]
    assert marked == list(L.MARK_ATTEMPTS)                                   # under the points of the round's start each of them is a mark
    assert [(a // L.T, (a % L.T) // L.WORD, a % L.WORD) for a in marked] == [(0, 0, 31), (0, 1, 0), (0, 1, 31), (0, 2, 0), (0, L.T // L.WORD - 1, 31), (1, 0, 0)]
    assert p["planted"]["hits"] == [a for a in marked if not (p["planted"]["dead"] and a == 63)]
    gone = []
    for a in marked:
        before = L.distances_at(p, [], p["draws"][a])
        now = L.distances_at(p, gone, p["draws"][a])
        assert len(before[0][before[1] < L.THRESH]) == 1 and np.abs(before[1] - L.THRESH).min() >= GAP
        hit = list(now[0][now[1] < L.THRESH])
        assert len(hit) == (1 if a in p["planted"]["hits"] else 0)
        gone += hit
    assert gone == ref["order"] and (n < L.CAP or min(gone) > L.CAP)


def test_limit_case():
    p, ref = L.case("limit"), L.reference("limit")
    L.check_expect("limit", ref)
    n, pl = len(p["fields"]), p["planted"]
    assert n == L.MAX_N and len(p["n_cands"]) == 7 and len(p["draws"]) <= 24 and p["n_request"] <= 16
    assert ref["status"] == 0 and len(ref["order"]) == p["n_request"]
    f = p["fields"]
    assert (f[0] == f.min(axis=0)).all() and (f[1:].min(axis=0) > f[0]).all()                            # index 0 holds every minimum alone
    assert pl["last"] == n - 1 and f[n - 1, 0] > f[:n - 1, 0].max() and (f[n - 1, 1:] < f[:, 1:].max(axis=0)).all()
    D1, D2 = pl["tied"]
    assert D1 < D2 and D2 > L.MAX_N - L.R and np.array_equal(f[D1], f[D2]) and L.place(D1)[1:] != L.place(D2)[1:]
    idx, d = L.distances_at(p, [], p["draws"][pl["at"]])
    assert list(idx[d < L.THRESH]) == [D1, D2] and np.abs(d - L.THRESH).min() >= GAP
    assert ref["order"][:4] == [D1, D2, n - 1, pl["x"]] and ref["rescale_attempts"] == [4]
    assert len(set(p["session"][ref["order"][4:]].tolist())) >= 3 and ref["n_sel"].sum() == p["n_request"]


def test_mirror_case():
    m = L.case_mirror()
    st, subsets = L.mirror_reference()
    assert st["status"] == 0 and len(st["order"]) == sum(m["sizes"]) == 400 and [len(s) for s in subsets] == m["sizes"]
    assert len(m["rows"]) == L.MID and len(m["n_cands"]) == 3
    # hits are frequent; more than one round, and more than one chunk of the mirror's second run (test_gpu_balanced_large.py)
    assert L.T < L.MIRROR_CHUNK < st["attempts"] < 5 * len(st["order"]) and L.MIRROR_CHUNK % L.T
