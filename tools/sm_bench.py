"""Throughput of the spectral-matching solve (lr_sm_batch) at M = 2048, 8192, 16384 correspondences, batch 1 and 32.

Problems: planted correspondence sets shaped like the 30k-point surrogate's mutual-NN lists (40 % inliers with +-0.1 m noise per axis,
outliers uniform in a 100 m box).  Prints one JSON line: per (M, batch) the median device time of the call, pairs/s, and the
compatibility evaluations per second (iterations * M^2 per pair), which DESIGN.md §11 compares with the vector-issue floor.

    python tools/sm_bench.py [--batches 1,32] [--reps 5] [--sizes 2048,8192,16384]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lidarregistration_amd import corrset, sm  # noqa: E402
from teaser_bench import problem  # noqa: E402


def run(m, batch, reps, device):
    probs = [problem(m, 1000 * m + k, device) for k in range(batch)]
    bc = corrset.BatchCall(sm.SOLVER, [a for a, _ in probs], [b for _, b in probs], outputs=False)
    p = bc.params
    st = torch.cuda.current_stream()

    def call():
        bc.launch(st.cuda_stream)

    call(); torch.cuda.synchronize()                          # warm-up
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    infos = [info for _, info in bc.results()]
    ms_call = float(np.median(times))
    return dict(M=m, batch=batch, call_ms=ms_call, call_ms_min=float(min(times)), pairs_per_s=batch / (ms_call * 1e-3),
                evals_per_s=batch * p.iterations * float(m) * m / (ms_call * 1e-3), ok=int(sum(i["status"] == 0 for i in infos)), K=infos[0]["K"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=str, default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=str, default="2048,8192,16384")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [run(int(m), int(b), a.reps, dev) for m in a.sizes.split(",") for b in a.batches.split(",")]
    print(json.dumps({"bench": "sm_batch", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                      "results": rows}))


if __name__ == "__main__":
    main()
