"""The numpy restatement of contract S (tests/balanced_cpu.py) and the Python mirror of the balanced-set generator (balanced.py) against the
reference's own recorded runs (tests/golden/g21_balanced.npz); the refusals, struct mirrors and scratch sizes of lr_balanced_select that
need no device.  No GPU: the mirror's device call is served by the restatement here."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from lidarregistration_amd import _ext, balanced, io_lists, synth
from tests import balanced_cases, balanced_cpu, overlap_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = balanced_cases.GOLD


def rng_checksum():
    st = np.random.get_state()
    return hashlib.sha256(st[1].tobytes() + np.int64(st[2]).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def g21a_run():
    """The whole of select_balanced_set by the restatement: attempts drawn one at a time from the global generator, as the reference does."""
    cands, session, n_cands = balanced_cases.g21a()
    np.random.seed(51)
    st = None
    while st is None or st["status"] == balanced_cpu.DRAWS:
        st = balanced_cpu.select(cands[:, 19:25], session, n_cands, 128, np.random.rand(4096, 6), st)
    return cands, st


def test_restatement_equals_the_reference(g21a_run):
    cands, st = g21a_run
    assert st["status"] == 0 and np.array_equal(st["order"], GOLD["a/order"])
    assert [st["attempts"], st["misses"]] == list(GOLD["a/counters"]) and st["attempts"] - st["misses"] == 128
    # the generator after exactly the consumed attempts, then the subset split and the files
    np.random.seed(51)
    np.random.rand(st["attempts"], 6)
    first, second = balanced_cpu.split_subsets(cands[np.array(st["order"])], [96, 32])
    assert rng_checksum() == str(GOLD["a/rng"])
    assert balanced_cpu.save_set_bytes(first) == GOLD["a/file_first"].tobytes() and balanced_cpu.save_set_bytes(second) == GOLD["a/file_second"].tobytes()


def restatement_dev(fields, session, n_cands, n_request, draws, state=None, thresh=0.1, max_rounds=0, poison=None):
    """select_balanced_dev's interface on the restatement."""
    tonp = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    st = balanced_cpu.select(tonp(fields), tonp(session), tonp(n_cands), n_request, tonp(draws), state, thresh)
    st.update(n_selected=len(st["order"]), rounds=0)
    st["order"] = list(st["order"])
    out = dict(st)
    out["order"] = np.array(st["order"], np.int32)
    out["_inner"] = st
    return out


@pytest.fixture
def mirror_on_cpu(monkeypatch):
    def dev(fields, session, n_cands, n_request, draws, state=None, thresh=0.1, max_rounds=0, poison=None):
        return restatement_dev(fields, session, n_cands, n_request, draws, None if state is None else state["_inner"], thresh)
    monkeypatch.setattr(balanced, "select_balanced_dev", dev)
    monkeypatch.setattr(balanced, "_device", lambda: "cpu")


def test_mirror_files_and_redraw_protocol(mirror_on_cpu, tmp_path):
    """select_balanced_set whole: the written files equal the reference's bytes, the generator ends in the recorded state (chunked draws,
    restored and redrawn), and io_lists reads the files back to the same values."""
    cands, session, n_cands = balanced_cases.g21a()
    blocks = {int(s): cands[cands[:, 0] == s] for s in np.unique(cands[:, 0])}
    np.random.seed(51)
    sets, info = balanced.select_balanced_set(blocks, [96, 32], ["first", "second"], str(tmp_path), name="Golden", return_info=True)
    assert rng_checksum() == str(GOLD["a/rng"])
    assert np.array_equal(info["order"], GOLD["a/order"]) and [info["attempts"], info["misses"]] == list(GOLD["a/counters"])
    for name in ("first", "second"):
        path = tmp_path / "balanced_sets" / "Golden" / (name + ".txt")
        assert path.read_bytes() == GOLD["a/file_" + name].tobytes()
        back = io_lists.read_pair_list(str(path))
        rows = sets[name][np.lexsort((sets[name][:, 1], sets[name][:, 0]))]
        assert np.array_equal(back["session"], rows[:, 0].astype(np.int64)) and np.array_equal(back["src"], rows[:, 1].astype(np.int64))
        assert np.abs(back["T_gt"].reshape(-1, 16) - rows[:, 3:19]).max() <= 1e-15 * np.abs(rows[:, 3:19]).max() + 5e-17
    assert balanced.round_sizes([96, 30], 8) == [96, 32] and balanced.round_sizes(5, None) == [5] and balanced.round_sizes(5, 4) == [8]


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_motion_to_fields():
    """Against the reference's stored values, within 4 ulp of the angle in degrees (atan2 may differ in the last place between machines);
    the translations exactly.  The singular branch: a pitch of 90 degrees."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "lists", "ApolloSouthbay_test.npz"))
    T = z["T_gt"].astype(np.float64).reshape(-1, 4, 4)
    got = np.stack([balanced.motion_to_fields(t) for t in T[::7]])
    want = GOLD["fields"][::7]
    assert np.array_equal(got[:, :3], want[:, :3])
    assert ulps(got[:, 3:], want[:, 3:]).max() <= 4
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])          # Ry(90 degrees): R[0,0] = R[1,0] = 0
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = [1.0, 2.0, 3.0]
    assert np.array_equal(balanced.motion_to_fields(M), [1.0, 2.0, 3.0, 0.0, 90.0, 0.0])
    a = np.radians(30.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    M[:3, :3] = R @ Rx                                                         # still singular: the roll comes from the second row
    f = balanced.motion_to_fields(M)
    assert abs(f[3] - 30.0) < 1e-12 and f[4] == 90.0 and f[5] == 0.0
    assert balanced.get_record_field_names().split()[19:25] == ["trans_x", "trans_y", "trans_z", "roll", "pitch", "yaw"] and len(balanced.get_record_field_names().split()) == 27
    c = np.zeros((3, 27)); c[:, 19:25] = [[0, 1, 2, 3, 4, 5], [2, 2, 4, 4, 6, 6], [1, 3, 3, 5, 5, 7]]
    assert np.array_equal(balanced.to_points_in_hyper_cube(c), [[0, 0, 0, 0, 0, 0], [1, 0.5, 1, 0.5, 1, 0.5], [0.5, 1, 0.5, 1, 0.5, 1]])


def test_status_2_and_3_of_the_restatement():
    for name, p in balanced_cases.status_cases().items():
        st = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"])
        assert (st["status"], list(st["order"]), st["consumed"]) == (p["status"], p["order"], p["consumed"]), name


def test_cases_do_what_their_names_say():
    """The crafted cases of the GPU suite, through the restatement: each exercises the branch it is named after."""
    for name, p in balanced_cases.crafted_cases().items():
        st = balanced_cpu.select(p["fields"], p["session"], p["n_cands"], p["n_request"], p["draws"], thresh=p.get("thresh", 0.1))
        for key, want in p["expect"].items():
            got = st[key]
            assert (list(got) if isinstance(want, list) else got) == want, (name, key, got, want)


def test_struct_mirrors_match_the_header():
    P, R = _ext.SelectParams, _ext.SelectResult
    assert ctypes.sizeof(P) == 24 and (P.struct_size.offset, P.n_request.offset, P.thresh.offset, P.resume.offset, P.max_rounds.offset) == (0, 4, 8, 16, 20)
    assert ctypes.sizeof(R) == 136 and (R.status.offset, R.n_selected.offset, R.attempts.offset, R.misses.offset, R.consumed.offset, R.rounds.offset,
                                        R.rescales.offset, R.lo.offset, R.hi.offset) == (0, 4, 8, 16, 24, 32, 36, 40, 88)
    p = P()
    assert (p.struct_size, p.n_request, p.thresh, p.resume, p.max_rounds) == (24, 0, 0.1, 0, 0)
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    for struct, mirror in (("lr_select_params", P), ("lr_select_result", R)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f[0] for f in mirror._fields_]
    L = _ext.lib()
    assert hasattr(L, "lr_balanced_select") and hasattr(L, "lr_balanced_select_scratch_bytes") and L.lr_version() == 103
    for name in ("motion_to_fields", "to_points_in_hyper_cube", "get_record_field_names", "select_balanced_dev", "select_balanced_set", "save_set",
                 "find_farthest_overlapping_partner", "prep_candidate_record", "create_candidate_set", "BalancedSetGenerator"):
        assert callable(getattr(balanced, name))
    assert callable(synth.make_session)


def test_scratch_sizes():
    L = _ext.lib()
    ns = (0, 1, 31, 32, 33, 257, 4097, 30000, 4194304)
    sizes = [L.lr_balanced_select_scratch_bytes(n) for n in ns]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    for n, s in zip(ns, sizes):                # the control block, the partial extremes, six padded columns of points
        assert s >= 1024 + 256 * 16 * 8 + 48 * n and s <= 1024 + 256 * 16 * 8 + 48 * (n + 31) + 255
    assert L.lr_balanced_select_scratch_bytes(-1) == 0 and L.lr_balanced_select_scratch_bytes((1 << 22) + 1) == 0


def test_refusals_come_before_any_device_call():
    """struct_size, the ranges, null pointers, short and misaligned scratch -- all before the first HIP call: safe without a device.  Every
    message names the argument."""
    L = _ext.lib()
    one, big = ctypes.c_void_p(256), 1 << 40
    err = lambda: L.lr_last_error().decode()
    nan, inf = float("nan"), float("inf")

    def sel(p, n=10, n_sessions=2, fields=one, session=one, n_cands=one, draws=one, n_draws=100, alive=one, n_sel=one, out=one, res=one, scratch=one, nbytes=big):
        return L.lr_balanced_select(fields, session, n_cands, n, n_sessions, draws, n_draws, ctypes.byref(p) if p is not None else None, alive, n_sel, out,
                                    res, scratch, nbytes, None)
    p = _ext.SelectParams(n_request=1); p.struct_size = 16
    assert sel(p) == -1 and "lr_select_params.struct_size is 16" in err()
    assert sel(None) == -1 and "params" in err()
    for kw, word in ((dict(thresh=0.0), "thresh"), (dict(thresh=-0.1), "thresh"), (dict(thresh=inf), "thresh"), (dict(thresh=nan), "thresh"),
                     (dict(n_request=-1), "n_request"), (dict(n_request=11), "n_request"), (dict(max_rounds=-1), "max_rounds"),
                     (dict(max_rounds=65537), "max_rounds"), (dict(resume=2), "resume")):
        assert sel(_ext.SelectParams(**{**dict(n_request=1), **kw})) == -1 and word in err(), kw
    for kw, word in ((dict(n=-1), "n must"), (dict(n=(1 << 22) + 1), "n must"), (dict(n_sessions=0), "n_sessions"), (dict(n_sessions=65537), "n_sessions"),
                     (dict(n_draws=-1), "n_draws"), (dict(fields=None), "fields"), (dict(session=None), "session"), (dict(n_cands=None), "n_cands"),
                     (dict(draws=None), "draws"), (dict(alive=None), "alive"), (dict(n_sel=None), "n_sel"), (dict(out=None), "out"), (dict(res=None), "result"),
                     (dict(scratch=None), "scratch"), (dict(nbytes=1024), "scratch too small"), (dict(scratch=ctypes.c_void_p(264)), "aligned"),
                     (dict(n_draws=1 << 30), "rounds")):
        assert sel(_ext.SelectParams(n_request=1), **kw) == -1 and word in err(), kw


# ---- g21c: the candidate search through the mirror, the overlap served by the restatement ------------------------------------------------
def test_candidate_search_equals_the_reference():
    from tests.golden.make_golden_balanced import G21C, G21C_SIZES, MARGIN
    ds = synth.SyntheticSessions({0: synth.make_session(**G21C)}, name="Golden", phase="test")
    gen = balanced.BalancedSetGenerator(ds, G21C_SIZES, ["test"], dict(output_dir=None))
    probes, frames = [], []

    def calc_GT_overlap(A, B, GT_mot, return_both=False):
        r = overlap_cpu.overlap(A, B, GT_mot)
        if return_both:
            return r["frac"], r["frac_sym"]
        probes.append(r["frac_sym"])
        return r["frac_sym"]
    gen.calc_GT_overlap = calc_GT_overlap
    find, prep = gen.find_farthest_overlapping_partner, gen.prep_candidate_record

    def find_tap(s, i, A, N, previous_spacing=None):
        frames.append(dict(i=i, first=len(probes), prev=previous_spacing, j=-1, record=None))
        res = find(s, i, A, N, previous_spacing)
        frames[-1]["max_j"] = -1 if res is None else int(res)
        return res

    def prep_tap(s, i, j, A):
        res = prep(s, i, j, A)
        frames[-1].update(j=int(j), record=res)
        return res
    gen.find_farthest_overlapping_partner, gen.prep_candidate_record = find_tap, prep_tap
    np.random.seed(51)
    gen.create_candidate_set(0)
    assert rng_checksum() == str(GOLD["c/rng"])                           # a single session consumes the global generator as the reference does
    assert [f["i"] for f in frames] == list(GOLD["c/i"]) and [f["max_j"] for f in frames] == list(GOLD["c/max_j"]) and [f["j"] for f in frames] == list(GOLD["c/j"])
    assert np.array_equal(np.array(probes), GOLD["c/probe_overlap"]) and [f["first"] for f in frames] == list(GOLD["c/probe_start"][:-1])
    mo = gen.config.minimum_overlap
    starts = GOLD["c/probe_start"]
    for k, f in enumerate(frames):
        for q, ov in enumerate(GOLD["c/probe_overlap"][starts[k]:starts[k + 1]]):
            assert abs(ov - mo) >= MARGIN and (f["prev"] is None or q > 0 or abs(abs(ov / mo - 1) - 0.1) >= MARGIN)
    want = GOLD["c/records"]
    for f, w in zip(frames, want):
        if f["record"] is None:
            assert np.isnan(w).all()
            continue
        assert np.array_equal(f["record"][:19], w[:19]) and np.array_equal(f["record"][19:22], w[19:22]) and np.array_equal(f["record"][25:], w[25:])
        assert ulps(f["record"][22:25], w[22:25]).max() <= 4
    got = gen.candidates[0]
    assert got.shape == GOLD["c/cands"].shape and np.array_equal(got[:, :22], GOLD["c/cands"][:, :22])
    assert len(got) >= 16 and len(set(GOLD["c/max_j"] - GOLD["c/i"])) >= 3 and (np.diff(GOLD["c/probe_start"]) == 1).any() and (np.diff(GOLD["c/probe_start"]) > 1).any()
