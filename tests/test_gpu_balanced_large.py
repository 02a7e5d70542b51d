"""lr_balanced_select past 1 025 candidates, up to its limit of 4 194 304 (csrc/lr_select.hip), against the numpy restatement of contract S
(tests/balanced_cpu.py) on the cases of tests/balanced_large_cases.py, whose premises tests/test_balanced_large_cpu.py holds: the selection
order, status, every counter, the alive flags, n_sel and the extremes bit for bit, each call under poisoned scratch.  Needs an MI355X."""
import numpy as np
import pytest

from tests import balanced_cpu
from tests import balanced_large_cases as L
from tests.test_gpu_balanced import bits, lr, same  # noqa: F401  (lr: the module fixture)

pytestmark = pytest.mark.gpu


def device(lr, p, poison, state=None, draws=None, **kw):
    return lr.bal.select_balanced_dev(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"] if draws is None else draws, state,
                                      thresh=L.THRESH, poison=poison, **kw)


def check(lr, name, poisons=(0x00, 0xFF)):
    """The case in one call under each poison: the whole state equals the restatement's, and what the case states holds on the device."""
    p, ref = L.case(name), L.reference(name)
    for poison in poisons:
        dev = device(lr, p, poison)
        same(lr, dev, ref, len(p["fields"]), (name, poison))
        L.check_expect(name, dev)
    return dev, ref


def same_states(lr, a, b):
    """Two device states of one run."""
    for key in ("status", "n_selected", "attempts", "misses", "rescales"):
        assert a[key] == b[key], key
    assert list(a["order"]) == list(b["order"]) and bits(a["lo"]) == bits(b["lo"]) and bits(a["hi"]) == bits(b["hi"])
    assert lr.torch.equal(a["alive"], b["alive"]) and lr.torch.equal(a["n_sel"], b["n_sel"])


# ---- 1. past the begin kernel's cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L.SIZES)
def test_sizes_past_the_cap(lr, n):
    dev, ref = check(lr, "size_%d" % n)
    assert dev["n_selected"] == 200 + 25 * L.SIZES.index(n)


def test_65536_dense_sessions(lr):
    check(lr, "dense_sessions")


# ---- 2. extremes held beyond the first trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", sorted(L.HOLDERS))
@pytest.mark.parametrize("n", (L.CAP + 1, L.MID))
def test_extreme_held_by_one_candidate(lr, n, where):
    name = "extreme_%d_%s" % (n, where)
    dev, ref = check(lr, name, poisons=(0xFF, 0x00) if where == "cap" else (0xFF,))
    p = L.case(name)["planted"]
    f = L.case(name)["fields"]
    if p["selected"]:
        assert dev["rescales"] == 1 and dev["order"][0] == p["holder"]
    else:                                                    # the holder lives: its value is the column's extreme in the result block
        assert bits((dev["lo"] if p["least"] else dev["hi"])[p["col"]]) == bits(f[p["holder"], p["col"]])


# ---- 3. refusals that only a late index triggers -----------------------------------------------------------------------------------------------
def refusal_case():
    return dict(L.case("size_%d" % (L.CAP + 1)), n_request=5)


@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_non_finite_field_at_the_first_index_of_the_second_trip(lr, value):
    p = refusal_case()
    p["fields"] = p["fields"].copy()
    p["fields"][L.CAP, 4] = value
    ref = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"])
    dev = device(lr, p, 0xFF if value is np.nan else 0x00)
    assert ref["status"] == 2 and (dev["status"], dev["n_selected"], dev["consumed"], dev["attempts"]) == (2, 0, 0, 0)
    assert dev["alive"][:L.CAP + 1].cpu().numpy().all()


@pytest.mark.parametrize("what", ("too_large", "negative", "without_candidates"))
def test_bad_session_at_the_first_index_of_the_second_trip(lr, what):
    p = refusal_case()
    p["session"] = p["session"].copy()
    p["n_cands"] = np.append(p["n_cands"], 0).astype(np.int32)                # session 3 exists and has no candidates
    p["session"][L.CAP] = dict(too_large=4, negative=-1, without_candidates=3)[what]
    ref = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"])
    dev = device(lr, p, 0xFF if what == "negative" else 0x00)
    assert ref["status"] == 3 and (dev["status"], dev["n_selected"], dev["consumed"]) == (3, 0, 0)
    good = device(lr, dict(refusal_case(), n_cands=p["n_cands"]), 0xFF)       # the empty session alone, named by nobody, is fine
    assert good["status"] == 0 and good["n_selected"] == 5


@pytest.mark.parametrize("index", (3, L.CAP))
def test_resumed_state_that_does_not_add_up(lr, index):
    """A candidate's alive flag cleared by hand between two calls: n_selected plus the alive candidates is no longer n -- status 3, nothing
    consumed, the selection so far untouched.  (Index 3: the rule had no test at any size before.)"""
    p = refusal_case()
    cut = 6
    ref = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"][:cut])
    st = device(lr, p, 0x00, draws=p["draws"][:cut])
    assert ref["status"] == 1 and ref["alive"][index] and 1 <= len(ref["order"]) < 5
    assert st["status"] == 1 and list(st["order"]) == ref["order"] and st["consumed"] == cut
    st["alive"][index] = 0
    st = device(lr, p, 0xFF, state=st, draws=p["draws"][cut:])
    assert (st["status"], st["consumed"], st["attempts"], list(st["order"])) == (3, 0, cut, ref["order"])
    st["alive"][index] = 1                                   # put back, the run goes on to where the one-call run ends
    st = device(lr, p, 0xFF, state=st, draws=p["draws"][cut:])
    whole = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"])
    assert st["status"] == 0 and list(st["order"]) == whole["order"] and st["attempts"] == whole["attempts"]


# ---- 4. ties across lanes, waves and trips -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", (0, L.CAP))
@pytest.mark.parametrize("name", L.TIE_NAMES)
def test_ties(lr, name, base):
    full = "tie_%s_%d" % (name, base)
    dev, ref = check(lr, full)
    assert list(dev["order"]) == L.case(full)["expect"]["order"]


# ---- 5. a rescale inside a round ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("marked_then_miss", "unmarked_then_hit"))
def test_rescale_inside_a_round(lr, kind):
    name = "rescale_" + kind
    dev, ref = check(lr, name)
    p = L.case(name)
    assert (dev["attempts"], dev["misses"], dev["rescales"]) == (ref["attempts"], ref["misses"], 1) and ref["rescale_attempts"] == [p["planted"]["next"]]
    assert dev["rounds"] == 2                                # the round ended at the holder's attempt, the next one did the rest
    # the round of the rescale alone: it consumed exactly the attempts up to the holder's
    first = device(lr, p, 0x5A, max_rounds=1)
    assert (first["status"], first["consumed"], first["rescales"], list(first["order"])) == (4, ref["rescale_attempts"][0], 1, [p["planted"]["holder"]])
    rest = device(lr, p, 0xFF, state=first, draws=p["draws"][first["consumed"]:])
    same_states(lr, rest, dev)


# ---- 6. marks on the map's word boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("all_live", "dead_mark"))
@pytest.mark.parametrize("n", (2 * L.R + 1, L.MID))
def test_marks_on_word_boundaries(lr, n, variant):
    dev, ref = check(lr, "marks_%d_%s" % (n, variant))
    assert dev["rounds"] == 2 and dev["n_selected"] == (6 if variant == "all_live" else 5)


# ---- 7. resume and round budget past the cap -------------------------------------------------------------------------------------------------------
def test_span_resumed_over_three_calls(lr):
    p, ref = L.case("span"), L.reference("span")
    one, _ = check(lr, "span")
    assert ref["attempts"] > L.T
    # one cut inside a block of attempts, one at the attempt of the 100th selection: straight after a hit
    cut2 = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], 100, p["draws"])["attempts"]
    cut1 = cut2 // 2 + 1
    assert 1 < cut1 < cut2 < ref["attempts"] - 1
    st = None
    for k, (a, b) in enumerate(((0, cut1), (cut1, cut2), (cut2, len(p["draws"])))):
        st = device(lr, p, (0x00, 0xFF, 0x5A)[k], state=st, draws=p["draws"][a:b])
        assert st["status"] == (1 if k < 2 else 0) and (k == 2 or st["consumed"] == b - a)
        if k == 1:
            assert st["n_selected"] == 100 and st["attempts"] == cut2     # the cut is straight after a hit
    same_states(lr, st, one)
    assert st["attempts"] == ref["attempts"]


def test_span_under_a_round_budget_of_one(lr):
    p, ref = L.case("span"), L.reference("span")
    st, at, calls = None, 0, 0
    while st is None or st["status"] == 4:
        st = device(lr, p, 0xFF if calls & 1 else 0x00, state=st, draws=p["draws"][at:], max_rounds=1)
        at += st["consumed"]; calls += 1
        assert calls < 50 and st["consumed"] <= L.T
    assert calls >= 2 and at == ref["attempts"]
    same(lr, dict(st, consumed=at), ref, len(p["fields"]), "span, one round per call")


# ---- 8. the limit ------------------------------------------------------------------------------------------------------------------------------------
def test_the_limit(lr):
    dev, ref = check(lr, "limit", poisons=(0xFF,))
    p = L.case("limit")
    assert len(p["fields"]) == L.MAX_N and list(dev["order"][:4]) == p["expect"]["order_starts"] and dev["rescales"] == 1
    few = device(lr, dict(p, n_request=2), 0x00)              # the other poison, up to the duplicates
    assert (few["status"], list(few["order"]), few["attempts"]) == (0, p["planted"]["tied"], 3)
    lib = lr.ext.lib()
    assert lib.lr_balanced_select_scratch_bytes(L.MAX_N) > 48 * L.MAX_N and lib.lr_balanced_select_scratch_bytes(L.MAX_N + 1) == 0


# ---- 9. the Python mirror where hits are frequent ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk, rounds", ((None, None), (L.MIRROR_CHUNK, 1)))
def test_mirror_where_hits_are_frequent(lr, monkeypatch, chunk, rounds):
    """select_balanced_set on MID candidates: the order, the subsets and the generator's end state are the restatement's, driven by the same
    legacy-generator draws.  At this density every third or fourth draw hits and the 400 selections take some 1 500 attempts: with the
    module's own chunk (65 536 draws, 96 rounds) one device call does it, since a round ends early only at a rescale and two rounds suffice.
    So that the continuation after status 4 and after status 1 does work at this size, the second run draws SEL_T + SEL_T / 4 attempts per
    chunk and allows one round per call: a call that ends with its round (4), one that ends with its draws (1), then a new chunk -- at
    least three calls, the same result."""
    m = L.case_mirror()
    ref, subsets = L.mirror_reference()
    if chunk is not None:
        monkeypatch.setattr(lr.bal, "DRAW_CHUNK", chunk)
        monkeypatch.setattr(lr.bal, "ROUNDS_PER_CALL", rounds)
    one_call, poisons = lr.bal.select_balanced_dev, []

    def poisoned(*a, **kw):                                  # the mirror's own device calls, each under a scratch poisoned in turn
        poisons.append((0x00, 0xFF)[len(poisons) & 1])
        return one_call(*a, **dict(kw, poison=poisons[-1]))
    monkeypatch.setattr(lr.bal, "select_balanced_dev", poisoned)
    starts = np.concatenate([[0], np.cumsum(m["n_cands"])])
    blocks = {int(m["rows"][a, 0]): m["rows"][a:b] for a, b in zip(starts[:-1], starts[1:])}
    np.random.seed(m["seed"])
    sets, info = lr.bal.select_balanced_set(blocks, m["sizes"], ["first", "second"], return_info=True)
    end = np.random.get_state()
    assert len(poisons) == info["calls"]
    assert list(info["order"]) == ref["order"] and (info["attempts"], info["misses"], info["rescales"]) == (ref["attempts"], ref["misses"], ref["rescales"])
    assert np.array_equal(sets["first"], subsets[0]) and np.array_equal(sets["second"], subsets[1])
    np.random.seed(m["seed"])
    np.random.rand(ref["attempts"], 6)
    balanced_cpu.split_subsets(m["rows"][np.array(ref["order"])], m["sizes"])
    want = np.random.get_state()
    assert np.array_equal(end[1], want[1]) and end[2] == want[2]
    if chunk is None:
        assert info["calls"] == 1 + ref["rescales"] // 95 and info["rounds"] >= 2
    else:
        assert info["calls"] >= 3 and ref["attempts"] > chunk
