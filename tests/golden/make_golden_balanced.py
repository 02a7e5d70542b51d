"""What the reference's balanced-set generator does on this repository's fixtures, recorded -- not restated.

Runs only where the reference tree exists.  BalancedDatasetGenerator/GenerateBalancedSet.py is imported as it is, through the stand-in
modules make_golden_overlap.reference_generator() sets up; its own select_balanced_set / select_sample / to_points_in_hyper_cube /
save_set / PerSessionCounter (g21a, g21b) and create_candidate_set / find_farthest_overlapping_partner / prep_candidate_record (g21c) are
called unbound on a namespace object, with its own motion_to_fields (utils/tools_3d.py).

  g21a  1 024 rows of tests/golden/lists/ApolloSouthbay_test.npz (every row 7008 k / 1024, k = 0..1023: all seven sessions) as
        candidates; select_balanced_set whole with subset_sizes [96, 32], seed 51.  Recorded: the selection order (original row of every
        select_sample hit), attempts, misses, the bytes of both .txt files, a checksum of the generator's state at the end.
  g21b  all 7 008 rows, 876 requested, seed 51: the order, the counters, the attempts at which a removal moved a column's extreme.
  g21c  the candidate search on one synth.make_session drive; `downsample` is the restatement tests/overlap_cpu.py (as in g17: the
        control flow and the record are pinned, not the down-sampling).  Per source frame: the probes (j, overlap), max_j, the chosen j,
        the 27-column record.  Every overlap comparison stays 1e-6 away from its threshold (asserted).

The candidates' six fields are stored as data (math.atan2 may differ in the last place between machines).  Only inputs, recorded outputs
and checksums are stored, in g21_balanced.npz.

    python tests/golden/make_golden_balanced.py
"""
import functools
import hashlib
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SEED = 51
G21C = dict(n_frames=48, n_points=6000, seed=51, step=3.0, yaw_step_deg=1.5)      # seeds tried for the 1e-6 margins: 1 (51)
G21C_SIZES = [6]
MARGIN = 1e-6
METHODS = ("downsample", "NN", "make_open3d_point_cloud", "overlap_fraction", "calc_GT_overlap", "get_relative_motion",
           "find_farthest_overlapping_partner", "prep_candidate_record", "get_record_field_names", "get_cands_list_file_name",
           "create_candidate_set", "to_points_in_hyper_cube", "select_sample", "save_set", "select_balanced_set")


def rng_checksum():
    st = np.random.get_state()
    return hashlib.sha256(st[1].tobytes() + np.int64(st[2]).tobytes()).hexdigest()


def namespace(module, ds, sizes, names, output_dir):
    cfg = dict(vars(module.default_config))
    cfg.update(output_dir=output_dir, max_spacing=int(cfg["max_spacing_in_sec"] / ds.time_step))
    ns = types.SimpleNamespace(config=types.SimpleNamespace(**cfg), DS_full=ds, subset_sizes=list(sizes), subset_names=list(names))
    for f in METHODS:
        setattr(ns, f, functools.partial(getattr(module.BalancedSetGenerator, f), ns))
    return ns


def list_candidates(module):
    """The Apollo list fixture as 27-column candidate rows: the fields by the reference's motion_to_fields, both overlap columns the
    fixture's overlap."""
    z = np.load(os.path.join(HERE, "lists", "ApolloSouthbay_test.npz"))
    T = z["T_gt"].astype(np.float64)
    fields = np.stack([module.motion_to_fields(t.reshape(4, 4)) for t in T])
    ov = z["overlap"].astype(np.float64)
    return np.concatenate([z["session"][:, None].astype(np.float64), z["src"][:, None], z["tgt"][:, None], T, fields, ov[:, None], ov[:, None]], axis=1)


def run_selection(module, cands, sizes, names):
    """select_balanced_set whole on `cands`; the taps record what the loop does."""
    assert len(np.unique(cands, axis=0)) == len(cands)
    sessions = [int(s) for s in np.unique(cands[:, 0])]
    ds = types.SimpleNamespace(name="Golden", phase="test", sessions_list=sessions, time_step=0.1)
    with tempfile.TemporaryDirectory() as tmp:
        ns = namespace(module, ds, sizes, names, tmp)
        for s in sessions:
            with open(ns.get_cands_list_file_name(s, ds.phase), "wb") as fid:
                pickle.dump(cands[cands[:, 0] == s], fid)
        remaining = list(range(len(cands)))
        log = dict(order=[], attempts=0, misses=0, rescale_attempts=[])
        inner = ns.select_sample

        def tap(c, points, P):
            res = inner(c, points, P)
            log["attempts"] += 1
            if res is None:
                log["misses"] += 1
                return res
            new = res[1]
            differ = np.flatnonzero((c[:-1] != new).any(axis=1))
            pos = int(differ[0]) if len(differ) else len(c) - 1
            assert np.array_equal(res[0][0], c[pos])
            log["order"].append(remaining.pop(pos))
            f0, f1 = c[:, 19:25], new[:, 19:25]
            if len(f1) and not (np.array_equal(f0.min(axis=0), f1.min(axis=0)) and np.array_equal(f0.max(axis=0), f1.max(axis=0))):
                log["rescale_attempts"].append(log["attempts"])
            return res
        ns.select_sample = tap
        np.random.seed(SEED)
        t0 = time.time()
        ns.select_balanced_set()
        log["seconds"] = time.time() - t0
        log["rng"] = rng_checksum()
        log["files"] = [open(os.path.join(tmp, "balanced_sets", ds.name, n + ".txt"), "rb").read() for n in names]
    return log


def run_candidate_search(module):
    from lidarregistration_amd import synth
    ds = synth.SyntheticSessions({0: synth.make_session(**G21C)}, name="Golden", phase="test")
    with tempfile.TemporaryDirectory() as tmp:
        ns = namespace(module, ds, G21C_SIZES, ["test"], tmp)
        frames, state = [], dict(j=None)
        load, overlap, find, prep = ds.load_PC, ns.calc_GT_overlap, ns.find_farthest_overlapping_partner, ns.prep_candidate_record

        def load_tap(s, j):
            state["j"] = j
            return load(s, j)

        def overlap_tap(A, B, mot, return_both=False):
            res = overlap(A, B, mot, return_both=return_both)
            if not return_both:
                frames[-1]["probes"].append((state["j"], float(res)))
            return res

        def find_tap(s, i, A, N, previous_spacing=None):
            frames.append(dict(i=i, probes=[], prev=previous_spacing, max_j=-1, j=-1, record=None))
            res = find(s, i, A, N, previous_spacing)
            frames[-1]["max_j"] = -1 if res is None else int(res)
            return res

        def prep_tap(s, i, j, A):
            res = prep(s, i, j, A)
            frames[-1]["j"] = int(j)
            frames[-1]["record"] = res
            return res
        ds.load_PC = load_tap
        ns.calc_GT_overlap, ns.find_farthest_overlapping_partner, ns.prep_candidate_record = overlap_tap, find_tap, prep_tap
        np.random.seed(SEED)
        ns.create_candidate_set(0)
        rng = rng_checksum()
        with open(ns.get_cands_list_file_name(0, ds.phase), "rb") as fid:
            cands = pickle.load(fid)
    mo = ns.config.minimum_overlap
    gap = np.inf
    for f in frames:
        for k, (j, ov) in enumerate(f["probes"]):
            gap = min(gap, abs(ov - mo))
            if k == 0 and f["prev"] is not None:
                gap = min(gap, abs(abs(ov / mo - 1) - 0.1))
        if f["record"] is not None:
            gap = min(gap, abs(f["record"][26] - mo))
    assert gap >= MARGIN, gap
    return frames, cands, rng, gap


def main():
    from tests.golden import make_golden_overlap
    make_golden_overlap.reference_generator()
    module = sys.modules["GenerateBalancedSet"]
    out = {}
    cands = list_candidates(module)
    out["fields"] = cands[:, 19:25].copy()
    rows_a = (np.arange(1024) * len(cands)) // 1024
    out["a/rows"] = rows_a.astype(np.int32)
    a = run_selection(module, cands[rows_a], [96, 32], ["first", "second"])
    out["a/order"] = np.array(a["order"], np.int32)
    out["a/counters"] = np.array([a["attempts"], a["misses"]], np.int64)
    out["a/rng"] = np.array(a["rng"])
    out["a/file_first"] = np.frombuffer(a["files"][0], np.uint8)
    out["a/file_second"] = np.frombuffer(a["files"][1], np.uint8)
    print(f"g21a: {len(a['order'])} selected in {a['attempts']} attempts ({a['misses']} misses), {a['seconds']:.1f} s")
    b = run_selection(module, cands, [876], ["all"])
    assert len(b["rescale_attempts"]) >= 1
    out["b/order"] = np.array(b["order"], np.int32)
    out["b/counters"] = np.array([b["attempts"], b["misses"]], np.int64)
    out["b/rescale_attempts"] = np.array(b["rescale_attempts"], np.int64)
    print(f"g21b: {len(b['order'])} selected in {b['attempts']} attempts, extremes moved at {b['rescale_attempts']}, {b['seconds']:.1f} s")
    frames, cands_c, rng, gap = run_candidate_search(module)
    out["c/i"] = np.array([f["i"] for f in frames], np.int32)
    out["c/max_j"] = np.array([f["max_j"] for f in frames], np.int32)
    out["c/j"] = np.array([f["j"] for f in frames], np.int32)
    out["c/probe_start"] = np.cumsum([0] + [len(f["probes"]) for f in frames]).astype(np.int32)
    out["c/probe_j"] = np.array([p[0] for f in frames for p in f["probes"]], np.int32)
    out["c/probe_overlap"] = np.array([p[1] for f in frames for p in f["probes"]], np.float64)
    out["c/records"] = np.stack([f["record"] if f["record"] is not None else np.full(27, np.nan) for f in frames])
    out["c/cands"] = cands_c
    out["c/rng"] = np.array(rng)
    print(f"g21c: {len(frames)} source frames, {len(out['c/probe_j'])} probes, {len(cands_c)} candidates, least margin {gap:.2e}")
    path = os.path.join(HERE, "g21_balanced.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
