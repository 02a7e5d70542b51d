"""Device time of lr_nn_wide (exact top-2 feature NN for descriptors of 33..128 numbers) at n x n rows and D = 33, 64, 128, next to
lr_nn_top2 at D = 32 on the same box (the same contract: the only existing yardstick) and to the f32-MFMA bound: 2 n^2 D' flop at
155 TFLOP/s, D' = D padded to the kernel's step count (what the matrix cores really multiply).

Every figure is the time between two events around the call (all of its kernels: norms, the tile kernel, the strip merge), median and
minimum of --reps calls after a warm-up.  Kernel times come from a run of their own under `rocprofv3 --kernel-trace --stats`.  Prints
one JSON line and writes it to --out (default profiles/nnw_bench.json).

    python tools/nnw_bench.py [--n 30000] [--dims 33,64,128] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import _ext, matching, synth  # noqa: E402

PEAK_F32_MFMA = 155e12


def timed(fn, reps):
    fn(); fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def steps(d):
    return 18 if d <= 36 else 24 if d <= 48 else 32 if d <= 64 else 48 if d <= 96 else 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--dims", type=str, default="33,64,128")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nnw_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = a.n
    rows = []
    for d in [32] + [int(x) for x in a.dims.split(",")]:
        F0, F1 = synth.make_features(n, n, d, 0.5, 0.5, 51)
        t0, t1 = torch.from_numpy(F0).to(dev), torch.from_numpy(F1).to(dev)
        idx1 = torch.empty(n, dtype=torch.int32, device=dev); idx2 = torch.empty_like(idx1)
        s1 = torch.empty(n, dtype=torch.float32, device=dev); s2 = torch.empty_like(s1)
        if d == 32:
            fn = lambda: matching.nn_top2_dev(t0, t1, want_2nd=True, want_dist=True)
            name, padded = "lr_nn_top2", 32
        else:
            fn = lambda: matching.nn_wide_into(t0, t1, idx1, idx2, s1, s2)
            name, padded = "lr_nn_wide", 2 * steps(d)
        med, mn = timed(fn, a.reps)
        flop = 2.0 * n * n * padded
        rows.append(dict(entry=name, n0=n, n1=n, dim=d, dim_padded=padded, ms=med, ms_min=mn, bound_ms=flop / PEAK_F32_MFMA * 1e3,
                         tflops=flop / (med * 1e-3) / 1e12, share_of_f32_mfma_peak=flop / PEAK_F32_MFMA / (med * 1e-3)))
    line = json.dumps({"bench": "nn_wide", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "note": "lr_nn_top2 runs an f16 filter pass plus exact verification, not n^2 f32 products: its tflops column is nominal",
                       "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
