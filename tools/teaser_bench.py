"""Throughput of the batched TEASER++ solve (lr_teaser_batch) and its four stages at M = 4k, 8k, 16k correspondences, batch 32.

Problems: planted correspondence sets shaped like the 30k-point surrogate's mutual-NN lists (40 % inliers with +-0.1 m noise
per axis, outliers uniform in a 100 m box).  Prints one JSON line: pairs/s of the whole call and per-stage device times (library
events, lr_teaser_timing) with the work and bytes per stage computed from the shapes.

    python tools/teaser_bench.py [--batch 32] [--reps 3] [--sizes 4096,8192,16384]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lidarregistration_amd import _ext, corrset, teaser  # noqa: E402


def problem(m, seed, device):
    g = torch.Generator(device=device); g.manual_seed(seed)
    n_in = int(0.4 * m)
    q = torch.randn(4, generator=g, device=device, dtype=torch.float64); q = q / q.norm()
    w, x, y, z = q.tolist()
    R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], device=device, dtype=torch.float64)
    a = (torch.rand(m, 3, generator=g, device=device, dtype=torch.float64) - 0.5) * 100
    b = (torch.rand(m, 3, generator=g, device=device, dtype=torch.float64) - 0.5) * 100
    b[:n_in] = a[:n_in] @ R.T + 2.0 + (torch.rand(n_in, 3, generator=g, device=device, dtype=torch.float64) - 0.5) * 0.2
    perm = torch.randperm(m, generator=g, device=device)
    return a[perm].float().contiguous(), b[perm].float().contiguous()


def run(m, batch, reps, device):
    L = _ext.lib()
    probs = [problem(m, 1000 * m + k, device) for k in range(batch)]
    bc = corrset.BatchCall(teaser.SOLVER, [a for a, _ in probs], [b for _, b in probs], outputs=False)
    st = torch.cuda.current_stream()

    def call():
        bc.launch(st.cuda_stream)

    call(); torch.cuda.synchronize()                          # warm-up
    whole, stages = [], []
    check(L.lr_teaser_timing(1))
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        whole.append(e0.elapsed_time(e1))
        out = (ctypes.c_float * 4)()
        check(L.lr_teaser_stage_times(out))
        stages.append(list(out))
    check(L.lr_teaser_timing(0))
    infos = [info for _, info in bc.results()]
    K = float(np.mean([i["K"] for i in infos])); n_rot = float(np.mean([i["n_rot_inliers"] for i in infos]))
    gnc = float(np.mean([i["gnc_iters"] for i in infos]))
    st_ms = np.median(np.array(stages), 0)
    W = (m + 63) // 64
    work = {   # per batch, from shapes
        "graph": {"pair_tests": batch * m * m, "bytes_written": batch * m * W * 8},
        "clique": {"adjacency_bytes_read_peel": batch * m * W * 8 * 2, "greedy_row_ands": batch * 16 * K * W},
        "rotation": {"fp64_tim_residuals": batch * K * (gnc + 1)},
        "translation": {"fp64_endpoint_point_tests": batch * 3 * 2 * n_rot * n_rot},
    }
    return dict(M=m, batch=batch, pairs_per_s=batch / (np.median(whole) * 1e-3), call_ms=float(np.median(whole)),
                stage_ms=dict(zip(["graph", "clique", "rotation", "translation"], [float(v) for v in st_ms])),
                mean_K=K, mean_rot_inliers=n_rot, mean_gnc_iters=gnc, exact=int(sum(i["exact"] for i in infos)),
                ok=int(sum(i["status"] == 0 for i in infos)), work=work)


def check(rc):
    _ext.check(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=str, default="4096,8192,16384")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [run(int(m), a.batch, a.reps, dev) for m in a.sizes.split(",")]
    print(json.dumps({"bench": "teaser_batch", "device": torch.cuda.get_device_name(dev), "results": rows}))


if __name__ == "__main__":
    main()
