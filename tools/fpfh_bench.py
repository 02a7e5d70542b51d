"""Device time of lr_fpfh (FPFH at radius 5 voxel, 100 neighbours) and of the whole fpfh.extract recipe on the points of a 0.3 m
down-sampled synthetic scan frame nearest to the sensor: 4 000, 30 000 and 75 000 of them (the density of real use: a share of the lists
hits the cap of 100).

Every figure is the time between two events around the call, median and minimum of --reps calls after a warm-up.  The times per stage
(grid, lists, SPFH, FPFH: one kernel each, fp_list_kernel / fp_spfh_kernel / fp_fpfh_kernel and the nn_* grid kernels) come from a run of
their own under `rocprofv3 --kernel-trace --stats`:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fpfh_bench.py --sizes 30000 --reps 5 --out ""

Prints one JSON line and writes it to --out (default profiles/fpfh_bench.json).

    python tools/fpfh_bench.py [--sizes 4000,30000,75000] [--raw 600000] [--voxel 0.3] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import bbrf, fpfh, overlap, synth  # noqa: E402


def timed(fn, reps):
    fn(); fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4000,30000,75000")
    ap.add_argument("--raw", type=int, default=600000)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fpfh_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    v = a.voxel
    raw = synth.make_scan_pair(a.raw, seed=51)[0]
    ds = overlap.voxel_down_sample(raw, v)
    ds = ds[torch.argsort((ds * ds).sum(dim=1))]              # nearest to the sensor first
    rows = []
    for want in [int(s) for s in a.sizes.split(",")]:
        pts = ds[:want].contiguous()
        n = int(pts.shape[0])
        nrm, _ = bbrf.normals_dev(pts, radius=2.0 * v, max_nn=30)
        _, _, info = fpfh.fpfh_dev(pts, nrm, 5.0 * v, 100, want_f64=False)
        med, mn = timed(lambda: fpfh.fpfh_dev(pts, nrm, 5.0 * v, 100, want_f64=False), a.reps)
        nmed, nmin = timed(lambda: bbrf.normals_dev(pts, radius=2.0 * v, max_nn=30), a.reps)
        rows.append(dict(n=n, radius=5.0 * v, max_nn=100, fpfh_ms=med, fpfh_ms_min=mn, normals_ms=nmed, normals_ms_min=nmin,
                         capped_share=info["capped"] / max(n, 1), zero_rows=info["zero_rows"]))
    sub = raw[:min(len(raw), 120000)]
    emed, emin = timed(lambda: fpfh.extract(sub, v), a.reps)
    line = json.dumps({"bench": "fpfh", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "note": "fpfh_ms and normals_ms include one device-to-host read of the info block (a synchronisation) per call",
                       "downsampled_rows": int(ds.shape[0]), "results": rows,
                       "extract": dict(raw=len(sub), rows=int(fpfh.extract(sub, v)[0].shape[0]), ms=emed, ms_min=emin)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
