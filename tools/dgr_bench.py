"""Time of the DGR refinement (lr_dgr_refine / lr_dgr_refine_batch) at m = 2000, 12000 and 32768 correspondences of which 30 % are live
(the rest carry weights below the clip), one pair and a batch of 64 pairs.

Problems: tests/dgr_cases.planted (planted motion, 5 cm noise; every live row an inlier or an outlier with its weight, the dead rows
weight 0.01 under clip 0.05).  Two settings per shape, each warmed up once, then timed `reps` times between two device events (median,
minimum, maximum):
  * `loop`: ratio 0 and max_iter 200, so that exactly 200 iterations run -- ms / 200 is the time of one iteration (the two setup launches,
    a few microseconds, are in it);
  * `call`: what DGR passes (ratio 1e-4, 1000 iterations at most): the time of a call and the iterations it took (pair 0's in a batch).

--reference PATH (or LIDARREG_REFERENCE) times, on the CPU and with no GPU involved, the reference's own GlobalRegistration on the 3000-row
golden case in float32 as shipped: seconds per call and per iteration, median of `reps`.  It runs only where the reference tree exists and
prints a JSON line of its own.

    python tools/dgr_bench.py [--sizes 2000,12000,32768] [--batches 1,64] [--reps 5]
    python tools/dgr_bench.py --reference /path/to/reference
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CLIP = 0.05
LOOP_ITERS = 200


def stats(times):
    return dict(ms=float(np.median(times)), ms_min=float(min(times)), ms_max=float(max(times)))


def problem(m, seed):
    from tests import dgr_cases as cases
    c = cases.planted(seed, m, 0.4, 0.05, 0.3)
    rng = np.random.default_rng([seed, m])
    w = np.maximum(c["weights"], np.float32(CLIP))
    w[rng.random(m) >= 0.3] = 0.01                   # 70 % of the rows are clipped
    return c["src"], c["tgt"], w


def run(m, batch, reps):
    import torch
    from lidarregistration_amd import corrset, dgr
    from tests import dgr_cases as cases
    ps = [problem(m, 1000 + k) for k in range(batch)]
    t = [[torch.from_numpy(a).cuda() for a in p] for p in ps]
    srcs, tgts, ws = ([p[k] for p in t] for k in range(3))
    row = dict(m=m, batch=batch)
    for tag, kw in (("loop", dict(cases.PARAMS, ratio=0.0, max_iter=LOOP_ITERS)), ("call", dict(cases.PARAMS))):
        call = corrset.BatchCall(dgr.SOLVER, srcs, tgts, weights=ws, single=batch == 1, clip=CLIP, **kw)
        call.timed()                                 # warm-up of this shape
        times = [call.timed() for _ in range(reps)]
        T, info = call.results()[0]
        assert info["status"] == 0 and abs(info["L"] - 0.3 * m) < 0.05 * m
        row[tag] = dict(stats(times), iterations=info["iterations"] + 1, L=info["L"])
        if tag == "loop":
            assert info["iterations"] == LOOP_ITERS - 1
            row[tag]["us_per_iteration"] = 1e3 * row[tag]["ms"] / LOOP_ITERS
        else:
            row[tag]["us_per_iteration"] = 1e3 * row[tag]["ms"] / (info["iterations"] + 1)
    return row


def reference(path, reps):
    import torch
    sys.path.insert(0, os.path.join(path, "DGR"))
    import core.registration as cr
    from tests import dgr_cases as cases
    c = cases.golden_case("m3000")
    X, Y, w = torch.from_numpy(c["src"]), torch.from_numpy(c["tgt"]), torch.from_numpy(c["weights"]).reshape(-1, 1)
    times, its = [], 0
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        _, _, info = cr.GlobalRegistration(X, Y, weights=w, break_threshold_ratio=cases.PARAMS["ratio"], quantization_size=cases.PARAMS["quantization_size"])
        times.append(time.perf_counter() - t0)
        its = info["iterations"] + 1
    times = times[1:]
    return dict(bench="dgr_reference_cpu", case="m3000", threads=torch.get_num_threads(), iterations=its, s=float(np.median(times)), s_min=float(min(times)),
                s_max=float(max(times)), us_per_iteration=1e6 * float(np.median(times)) / its)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="2000,12000,32768")
    ap.add_argument("--batches", type=str, default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", type=str, default=None)
    a = ap.parse_args()
    if a.reference:
        print(json.dumps(reference(a.reference, a.reps)))
        return
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [run(m, b, a.reps) for m in (int(v) for v in a.sizes.split(",")) for b in (int(v) for v in a.batches.split(","))]
    print(json.dumps({"bench": "dgr_refine", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                      "results": rows}))


if __name__ == "__main__":
    main()
