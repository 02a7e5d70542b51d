"""Device time of the balanced-set selection (lr_balanced_select) on two inputs:

  g21b   the 7 008 rows of tests/golden/lists/ApolloSouthbay_test.npz as candidates (7 sessions), 876 requested -- the reference's recorded run
         of tests/golden/g21_balanced.npz, whose order the device must reproduce;
  x4     28 032 candidates, 7 008 requested: the same rows four times, copy 0 as it is, copies 1..3 with every field moved by a normal
         deviate of 2 % of its column's standard deviation (numpy default_rng(51)); the sessions stay the seven (four times the candidates each).

Both draw their attempts from numpy's legacy generator seeded with 51, as select_balanced_set does.  A first run in chunks finds how many
attempts the selection takes; the timed call is then ONE lr_balanced_select over exactly those draws, already on the device: the time between
two events around it, median and minimum of --reps calls after a warm-up, with the launches it enqueued (3 + 2 per round), the rounds that
did something and the attempts -- once with the rounds that always suffice (max_rounds 0) and once with exactly the rounds it needs.  For context the same selection runs through the numpy restatement (tests/balanced_cpu.py) on this box's
CPU, one thread: whole for g21b; for x4 until --restate-seconds have passed, the rest extrapolated from the attempts done (said in the
output).  The orders are compared.  There is no parent figure and no target.  Prints one JSON line and writes it to --out (default
profiles/balanced_bench.json).

    python tools/balanced_bench.py [--reps 5] [--cases g21b,x4] [--restate-seconds 60] [--no-restate]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import _ext, balanced, devmem  # noqa: E402
from tests import balanced_cases, balanced_cpu  # noqa: E402

SEED = 51
CHUNK = 65536


def inputs(name):
    cands, session, n_cands = balanced_cases.g21b()
    fields = cands[:, 19:25].copy()
    if name == "g21b":
        return fields, session, n_cands, 876
    rng = np.random.default_rng(SEED)
    sd = fields.std(axis=0)
    copies = [fields] + [fields + rng.normal(size=fields.shape) * 0.02 * sd for _ in range(3)]
    return np.vstack(copies), np.tile(session, 4), (n_cands * 4).astype(np.int32), 7008


def find_attempts(fields, session, n_cands, n_request):
    """The selection in chunks of draws, as select_balanced_set runs it: (attempts, order, device calls)."""
    np.random.seed(SEED)
    st, calls, left = None, 0, np.zeros((0, 6))
    while st is None or st["status"] in (1, 4):
        if len(left) == 0:
            left = np.random.rand(CHUNK, 6)
        st = balanced.select_balanced_dev(fields, session, n_cands, n_request, left, st, max_rounds=balanced.ROUNDS_PER_CALL)
        left = left[st["consumed"]:]
        calls += 1
    assert st["status"] == 0, st["status"]
    return int(st["attempts"]), st["order"], calls, int(st["rounds"])


def timed_call(fields, session, n_cands, n_request, attempts, reps, dev, per_round, max_rounds=0):
    np.random.seed(SEED)
    draws = torch.from_numpy(np.random.rand(attempts, 6)).to(dev)
    f = torch.from_numpy(fields).to(dev); s = torch.from_numpy(session).to(dev); nc = torch.from_numpy(n_cands).to(dev)
    times, st = [], None
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        st = balanced.select_balanced_launch(f, s, nc, n_request, draws, max_rounds=max_rounds)
        e1.record(); e1.synchronize()
        if k:
            times.append(e0.elapsed_time(e1))
    st.update(devmem.as_dict(devmem.read_struct(st["res"], _ext.SelectResult)))
    rounds_enqueued = max_rounds or min(attempts, n_request + (attempts + per_round - 1) // per_round)
    return float(np.median(times)), float(min(times)), st, 3 + 2 * rounds_enqueued


def restate(fields, session, n_cands, n_request, limit_s):
    np.random.seed(SEED)
    st, t0 = None, time.perf_counter()
    while st is None or st["status"] == balanced_cpu.DRAWS:
        if limit_s and time.perf_counter() - t0 > limit_s:
            break
        st = balanced_cpu.select(fields, session, n_cands, n_request, np.random.rand(4096, 6), st)
    return st, time.perf_counter() - t0


def run(name, a, dev):
    fields, session, n_cands, n_request = inputs(name)
    attempts, order, calls, rounds = find_attempts(fields, session, n_cands, n_request)
    med, mn, st, launches = timed_call(fields, session, n_cands, n_request, attempts, a.reps, dev, a.attempts_per_round)
    one_order = st["out"][:st["n_selected"]].cpu().numpy()
    assert st["status"] == 0 and st["attempts"] == attempts and np.array_equal(one_order, order)
    row = dict(case=name, candidates=len(fields), requested=n_request, attempts=attempts, rounds=int(st["rounds"]), launches=launches, device_ms=med,
               device_ms_min=mn, us_per_round=1e3 * med / max(int(st["rounds"]), 1), rescales=int(st["rescales"]), chunked_calls=calls)
    # the same call with just the rounds it needs enqueued (max_rounds): what the rounds that return at their first instruction cost
    med2, mn2, st2, launches2 = timed_call(fields, session, n_cands, n_request, attempts, a.reps, dev, a.attempts_per_round, max_rounds=int(st["rounds"]))
    assert st2["status"] == 0 and st2["attempts"] == attempts and np.array_equal(st2["out"][:st2["n_selected"]].cpu().numpy(), order)
    row.update(exact_rounds_launches=launches2, exact_rounds_device_ms=med2, exact_rounds_device_ms_min=mn2)
    if name == "g21b":
        row["equals_recorded_order"] = bool(np.array_equal(order, balanced_cases.GOLD["b/order"]))
    if not a.no_restate:
        ref, secs = restate(fields, session, n_cands, n_request, 0 if name == "g21b" else a.restate_seconds)
        k = len(ref["order"])
        row.update(restatement_s=secs, restatement_attempts=int(ref["attempts"]), restatement_selected=k, restatement_whole=ref["status"] == 0,
                   restatement_order_equal=bool(np.array_equal(ref["order"], order[:k])))
        if ref["status"] != 0:
            row["restatement_s_extrapolated"] = secs * attempts / max(int(ref["attempts"]), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=str, default="g21b,x4")
    ap.add_argument("--restate-seconds", type=float, default=60.0)
    ap.add_argument("--no-restate", action="store_true")
    ap.add_argument("--attempts-per-round", type=int, default=balanced.SELECT_T, help="SEL_T of the library under LIDARREG_LIB, if it is another build")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "balanced_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [run(name, a, dev) for name in a.cases.split(",")]
    line = json.dumps({"bench": "balanced_select", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "library": os.path.basename(_ext.LIB_PATH), "attempts_per_round": a.attempts_per_round, "rounds_per_call_of_the_mirror": balanced.ROUNDS_PER_CALL,
                       "seed": SEED, "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
