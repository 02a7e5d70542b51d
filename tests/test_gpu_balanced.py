"""lr_balanced_select and its Python mirror (lidarregistration_amd/balanced.py) against the numpy restatement of contract S
(tests/balanced_cpu.py) and against the reference's recorded runs (tests/golden/g21_balanced.npz): the selection order, every counter, the
state left in the caller's buffers and the columns' extremes bit for bit, under poisoned scratch.  Needs an MI355X."""
import ctypes
import hashlib

import numpy as np
import pytest

from tests import balanced_cases, balanced_cpu

pytestmark = pytest.mark.gpu

GOLD = balanced_cases.GOLD
CRAFTED = balanced_cases.crafted_cases()
STATUS = balanced_cases.status_cases()
T = balanced_cases.T


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, balanced, synth
    _ext.lib()
    class NS: pass
    ns = NS(); ns.torch = torch; ns.ext = _ext; ns.bal = balanced; ns.synth = synth
    return ns


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64).tolist()


def same(lr, dev, ref, n, what=""):
    """The device state against the restatement's."""
    assert dev["status"] == ref["status"], (what, dev["status"], ref["status"])
    assert list(dev["order"]) == list(ref["order"]), what
    assert (dev["n_selected"], dev["attempts"], dev["misses"], dev["consumed"], dev["rescales"]) == \
        (len(ref["order"]), ref["attempts"], ref["misses"], ref["consumed"], ref["rescales"]), what
    if ref["status"] != balanced_cpu.BAD_SESSION:
        assert np.array_equal(dev["alive"][:n].cpu().numpy().astype(bool), ref["alive"]), what
        assert np.array_equal(dev["n_sel"][:len(ref["n_sel"])].cpu().numpy(), ref["n_sel"]), what
        ext = balanced_cpu.extremes(ref["fields64"], ref["alive"]) if "fields64" in ref else None
        if ext is not None:
            assert bits(dev["lo"]) == bits(ext[0]) and bits(dev["hi"]) == bits(ext[1]), what


def run_both(lr, p, n_request=None, poison=0xFF, draws=None, thresh=None):
    nr = p["n_request"] if n_request is None else n_request
    dr = p["draws"] if draws is None else draws
    th = p.get("thresh", 0.1) if thresh is None else thresh
    ref = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], nr, dr, thresh=th)
    ref["fields64"] = np.asarray(p["fields"], np.float64).reshape(-1, 6)
    dev = lr.bal.select_balanced_dev(p["fields"], p["session"], p["n_cands"], nr, dr, thresh=th, poison=poison)
    return dev, ref


@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 257, 1025))
def test_sizes_equal_the_restatement(lr, n):
    p = balanced_cases.random_case(n, seed=n)
    for poison, nr in ((0x00, min(n, 40)), (0xFF, n // 2)):
        dev, ref = run_both(lr, dict(p, n_request=nr), poison=poison)
        same(lr, dev, ref, n, (n, nr))
    if n >= 63:
        assert len(ref["order"]) >= 10                       # the draws do hit


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_cases(lr, name):
    p = CRAFTED[name]
    for poison in (0x00, 0xFF):
        dev, ref = run_both(lr, p, poison=poison)
        same(lr, dev, ref, len(p["fields"]), name)
    for key, want in p["expect"].items():
        got = dev[key]
        assert (list(got) if isinstance(want, list) else got) == want, (name, key, got, want)


@pytest.mark.parametrize("name", sorted(STATUS))
def test_status_2_and_the_device_side_refusals(lr, name):
    p = STATUS[name]
    dev = lr.bal.select_balanced_dev(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"], poison=0xFF)
    assert (dev["status"], list(dev["order"]), dev["consumed"]) == (p["status"], p["order"], p["consumed"]), name


def test_run_resumed_over_three_calls(lr):
    """The same run in one call and cut at two places (one cut inside a round's block, one straight after a hit); the scratch poisoned anew
    for every call."""
    p = balanced_cases.random_case(257, seed=7, n_draws=900)
    one, ref = run_both(lr, dict(p, n_request=60))
    same(lr, one, ref, 257)
    hits = [k for k in range(1, len(ref["order"]))]
    assert ref["status"] == 0 and len(hits) > 20
    cut1, cut2 = 100, ref["consumed"] * 2 // 3
    st = None
    consumed = 0
    for k, (a, b) in enumerate(((0, cut1), (cut1, cut2), (cut2, len(p["draws"])))):
        st = lr.bal.select_balanced_dev(p["fields"], p["session"], p["n_cands"], 60, p["draws"][a:b], st, poison=(0x00, 0xFF, 0x5A)[k])
        consumed += st["consumed"]
        assert st["status"] == (1 if k < 2 else 0)
    assert consumed == ref["consumed"] == st["attempts"]
    for key in ("n_selected", "attempts", "misses", "rescales"):
        assert st[key] == one[key]
    assert list(st["order"]) == list(one["order"]) and bits(st["lo"]) == bits(one["lo"]) and bits(st["hi"]) == bits(one["hi"])
    assert lr.torch.equal(st["alive"], one["alive"]) and lr.torch.equal(st["n_sel"], one["n_sel"])


def test_round_budget_and_resume(lr):
    """max_rounds: status 4 leaves the state, and the calls that follow from `consumed` on end where the unbounded call ends."""
    p = balanced_cases.random_case(1025, seed=9, n_draws=8000)
    one, ref = run_both(lr, dict(p, n_request=800))
    same(lr, one, ref, 1025)
    assert ref["attempts"] > 2 * T                           # more than two rounds' worth
    st, at, calls = None, 0, 0
    while st is None or st["status"] == 4:
        st = lr.bal.select_balanced_dev(p["fields"], p["session"], p["n_cands"], 800, p["draws"][at:], st, max_rounds=1, poison=0xFF)
        at += st["consumed"]; calls += 1
        assert calls < 200 and st["consumed"] <= T
    assert calls >= 3 and st["status"] == one["status"] and list(st["order"]) == list(one["order"]) and st["attempts"] == one["attempts"] == at


def test_65536_sessions_sparse(lr):
    p = balanced_cases.random_case(257, seed=11, n_sessions=65536, sparse=True)
    assert p["session"].max() == 65535 and p["session"].min() == 0
    dev, ref = run_both(lr, dict(p, n_request=80))
    same(lr, dev, ref, 257)
    assert len(ref["order"]) >= 30


def test_rescale_at_more_than_one_block(lr):
    """The holder of an extreme removed among 1 025 candidates: every point is computed again."""
    p = balanced_cases.random_case(1025, seed=13)
    lo = p["fields"].min(axis=0); hi = p["fields"].max(axis=0)
    holder = int(p["fields"][:, 2].argmax())
    p["draws"][0] = (p["fields"][holder] - lo) / (hi - lo)
    dev, ref = run_both(lr, dict(p, n_request=200))
    same(lr, dev, ref, 1025)
    assert ref["order"][0] == holder and ref["rescales"] >= 1 and ref["rescale_attempts"][0] == 1


def test_call_can_be_captured_into_a_graph(lr):
    """No host synchronisation, no allocation: the call recorded once on a side stream and replayed on other contents of the same buffers
    gives what the eager calls give."""
    torch, L = lr.torch, lr.ext.lib()
    cases = [balanced_cases.random_case(257, seed=s, n_draws=300) for s in (21, 22, 23)]
    n, nd, ns = 257, 300, 3
    f = torch.empty((n, 6), dtype=torch.float64, device="cuda"); se = torch.empty(n, dtype=torch.int32, device="cuda")
    nc = torch.empty(ns, dtype=torch.int32, device="cuda"); d = torch.empty((nd, 6), dtype=torch.float64, device="cuda")
    alive = torch.empty(n, dtype=torch.uint8, device="cuda"); n_sel = torch.empty(ns, dtype=torch.int32, device="cuda")
    out = torch.empty(20, dtype=torch.int32, device="cuda"); res = torch.zeros(ctypes.sizeof(lr.ext.SelectResult), dtype=torch.uint8, device="cuda")
    sc = torch.empty(L.lr_balanced_select_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    pb = lr.ext.SelectParams(n_request=20)
    s = torch.cuda.Stream()

    def call():
        lr.ext.check(L.lr_balanced_select(f.data_ptr(), se.data_ptr(), nc.data_ptr(), n, ns, d.data_ptr(), nd, ctypes.byref(pb), alive.data_ptr(),
                                          n_sel.data_ptr(), out.data_ptr(), res.data_ptr(), sc.data_ptr(), sc.numel(), s.cuda_stream))

    def load(p):
        for dst, src in ((f, p["fields"]), (se, p["session"]), (nc, p["n_cands"]), (d, p["draws"])):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        out.fill_(-1); torch.cuda.synchronize()

    def outputs():
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (res, out, alive, n_sel)]
    eager = []
    for p in cases:
        load(p); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k, (p, want) in list(enumerate(zip(cases, eager)))[::-1]:
        load(p); sc.fill_(0xFF if k & 1 else 0x00); alive.fill_(7); g.replay()
        assert outputs() == want
    assert len(set(e[1] for e in eager)) == 3
    ref = balanced_cpu.select(cases[1]["fields"], cases[1]["session"], cases[1]["n_cands"], 20, cases[1]["draws"])
    r = lr.ext.SelectResult.from_buffer_copy(eager[1][0])
    assert (r.status, r.n_selected, r.attempts) == (ref["status"], len(ref["order"]), ref["attempts"])
    assert np.frombuffer(eager[1][1], np.int32)[:r.n_selected].tolist() == ref["order"]


def test_refusals_that_need_a_device(lr):
    """Foreign scratch and a scratch of another device; nothing is launched, a good call still works afterwards."""
    torch, L = lr.torch, lr.ext.lib()
    p = CRAFTED["request_1"]
    t = lambda X: torch.from_numpy(np.ascontiguousarray(X)).cuda()
    f, se, nc, d = t(p["fields"]), t(p["session"]), t(p["n_cands"]), t(p["draws"])
    alive = torch.empty(3, dtype=torch.uint8, device="cuda"); n_sel = torch.empty(1, dtype=torch.int32, device="cuda")
    out = torch.empty(1, dtype=torch.int32, device="cuda"); res = torch.zeros(ctypes.sizeof(lr.ext.SelectResult), dtype=torch.uint8, device="cuda")
    need = L.lr_balanced_select_scratch_bytes(3)
    scratch = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    pb = lr.ext.SelectParams(n_request=1)
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.lr_last_error().decode()

    def call(ptr=scratch.data_ptr(), nbytes=need):
        return L.lr_balanced_select(f.data_ptr(), se.data_ptr(), nc.data_ptr(), 3, 1, d.data_ptr(), len(p["draws"]), ctypes.byref(pb), alive.data_ptr(),
                                    n_sel.data_ptr(), out.data_ptr(), res.data_ptr(), ptr, nbytes, st)
    host = np.zeros(need + 256, np.uint8)
    hp = (host.ctypes.data + 255) & ~255
    assert call() == 0
    assert call(nbytes=need - 1) == -1 and "scratch too small" in err()
    assert call(ptr=scratch.data_ptr() + 8) == -1 and "aligned" in err()
    assert call(ptr=hp) == -1 and "not device memory" in err()
    L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)
    try:
        assert call() == -1 and "device" in err()
    finally:
        L.lr_debug_fake_current_device(-1)
    assert call() == 0
    torch.cuda.synchronize()
    r = lr.ext.SelectResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert (r.status, r.n_selected, out.cpu().tolist()) == (0, 1, [2])


def rng_checksum():
    st = np.random.get_state()
    return hashlib.sha256(st[1].tobytes() + np.int64(st[2]).tobytes()).hexdigest()


def test_g21a_through_the_mirror(lr, tmp_path):
    """select_balanced_set whole on the device loop: the reference's order, counters, generator state and file bytes."""
    cands, session, n_cands = balanced_cases.g21a()
    blocks = {int(s): cands[cands[:, 0] == s] for s in np.unique(cands[:, 0])}
    np.random.seed(51)
    sets, info = lr.bal.select_balanced_set(blocks, [96, 32], ["first", "second"], str(tmp_path), name="Golden", return_info=True)
    assert np.array_equal(info["order"], GOLD["a/order"]) and [info["attempts"], info["misses"]] == list(GOLD["a/counters"])
    assert rng_checksum() == str(GOLD["a/rng"])
    for name in ("first", "second"):
        assert (tmp_path / "balanced_sets" / "Golden" / (name + ".txt")).read_bytes() == GOLD["a/file_" + name].tobytes()


def test_g21b_through_the_device(lr):
    """All 7 008 rows, 876 requested, in one call: the recorded order is the yardstick (the restatement does not run here)."""
    cands, session, n_cands = balanced_cases.g21b()
    attempts = int(GOLD["b/counters"][0])
    np.random.seed(51)
    draws = np.random.rand(attempts + 500, 6)
    dev = lr.bal.select_balanced_dev(cands[:, 19:25], session, n_cands, 876, draws, poison=0xFF)
    assert dev["status"] == 0 and np.array_equal(dev["order"], GOLD["b/order"])
    assert [dev["attempts"], dev["misses"]] == list(GOLD["b/counters"]) and dev["consumed"] == attempts
    assert dev["rescales"] == len(GOLD["b/rescale_attempts"]) >= 1


def test_end_to_end_on_a_synthetic_session(lr, tmp_path):
    """create_set on two make_session drives: candidates by the GPU overlap measure, the selection by the device loop, the lists readable."""
    from lidarregistration_amd import io_lists
    ds = lr.synth.SyntheticSessions({3: lr.synth.make_session(40, seed=1, step=3.0), 5: lr.synth.make_session(40, seed=2, step=3.0)}, name="Drive")
    gen = lr.bal.BalancedSetGenerator(ds, [6, 4], ["train", "val"], dict(output_dir=str(tmp_path), candidates_per_sample=8))
    np.random.seed(51)
    sets = gen.create_set()
    cands = gen.load_candidates()
    assert set(cands) == {3, 5} and all(c.shape[1] == 27 and len(c) >= 12 for c in cands.values())
    allc = np.vstack(list(cands.values()))
    assert (allc[:, 26] >= 0.2).all() and (allc[:, 2] > allc[:, 1]).all()
    assert sets["train"].shape == (6, 27) and sets["val"].shape == (4, 27)
    both = np.vstack([sets["train"], sets["val"]])
    assert len(np.unique(both[:, :3], axis=0)) == 10 and all((allc[:, :3] == r[:3]).all(axis=1).any() for r in both)
    back = io_lists.read_pair_list(str(tmp_path / "balanced_sets" / "Drive" / "train.txt"))
    assert len(back["src"]) == 6 and set(back["session"]) <= {3, 5}
    # the selection again from the pickles, and the same by the restatement
    np.random.seed(77)
    again = gen.select_balanced_set()
    np.random.seed(77)
    blocks = list(cands.values())
    n_cands = [len(b) for b in blocks]
    st = None
    while st is None or st["status"] == balanced_cpu.DRAWS:
        st = balanced_cpu.select(allc[:, 19:25], np.repeat([0, 1], n_cands), n_cands, 10, np.random.rand(4096, 6), st)
    np.random.seed(77); np.random.rand(st["attempts"], 6)
    first, second = balanced_cpu.split_subsets(allc[np.array(st["order"])], [6, 4])
    assert np.array_equal(first, again["train"]) and np.array_equal(second, again["val"])
