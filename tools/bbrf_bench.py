"""Device time of the Best-Buddies refinement (lr_bbrf, 100 iterations) on synthetic scan pairs of 3k, 30k and 120k raw points
(synth.make_scan_pair), both frames down-sampled at voxel 0.3, cloud 0 moved by the true motion off by a small rigid motion, all normals
(0, 0, 1) -- what the reference's refinement tester hands to BBR_F.

Every figure is the time between two events around the call, median and minimum of --reps calls after a warm-up.  The split into grid +
search, pair and step kernels comes from a kernel trace of one call, taken in a child process of its own (rocprofv3 --kernel-trace
--stats): the difference between the event time and the kernels' sum is what the gaps between the dependent launches cost.  For context
only, the same clouds go through a host form of one iteration (scipy's cKDTree on at most 16 threads for the two searches, the numpy
restatement tests/bbrf_cpu.py for the loss and the gradient) in the same run.  There is no parent figure and no target.  Prints one JSON
line and writes it to --out (default profiles/bbrf_bench.json).

    python tools/bbrf_bench.py [--sizes 3000,30000,120000] [--reps 5] [--no-trace]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import _ext, devmem, overlap, synth  # noqa: E402

VOXEL, OFF_DEG, OFF_M = 0.3, 0.8, 0.05
GROUPS = (("search", ("nn_",)), ("transform", ("bb_xform", "bb_init")), ("pair", ("bb_pair",)), ("step", ("bb_step",)))


def small_motion(seed, deg, shift):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(np.radians(deg)) * K + (1.0 - np.cos(np.radians(deg))) * (K @ K)
    t = rng.normal(size=3); T[:3, 3] = shift * t / np.linalg.norm(t)
    return T


def clouds(n, dev):
    A, B, T = synth.make_scan_pair(n, n)
    M = small_motion(71, OFF_DEG, OFF_M) @ T
    a, b = overlap.voxel_down_sample(A, VOXEL), overlap.voxel_down_sample(B, VOXEL)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    a = torch.stack([((float(M[r, 0]) * x + float(M[r, 1]) * y) + float(M[r, 2]) * z) + float(M[r, 3]) for r in range(3)], dim=1).contiguous()
    nz = lambda k: torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev).repeat(k, 1).contiguous()
    return a, nz(int(a.shape[0])), b.contiguous(), nz(int(b.shape[0]))


def make_call(a, na, b, nb, dev):
    L = _ext.lib()
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    p = _ext.BbrfParams()
    res = torch.zeros(ctypes.sizeof(_ext.BbrfResult), dtype=torch.uint8, device=dev)
    log = torch.zeros((p.n_iter, 8), dtype=torch.float64, device=dev)
    sc = devmem.scratch(L.lr_bbrf_scratch_bytes(n0, n1, p.n_iter), dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _ext.check(L.lr_bbrf(a.data_ptr(), na.data_ptr(), n0, b.data_ptr(), nb.data_ptr(), n1, ctypes.byref(p), res.data_ptr(), log.data_ptr(),
                             sc.data_ptr(), sc.numel(), st))
    return call, res, log


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def host_iteration(a, na, b, nb, threads, reps=3):
    """One iteration at the starting pose on the host: median seconds."""
    from scipy.spatial import cKDTree
    from tests import bbrf_cpu
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        Bp, nBp, _, dW = bbrf_cpu.move(b, nb, [0.0] * 6)
        f = cKDTree(Bp).query(a, k=1, workers=threads)[1]
        r = cKDTree(a).query(Bp, k=1, workers=threads)[1]
        keep = r[f] == np.arange(len(a))
        terms, _ = bbrf_cpu.pair_terms(a, na, b, nb, Bp, nBp, dW, f, keep)
        [terms[:, c].sum() for c in range(7)]
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def trace_split(n):
    """Kernel time of one traced call by group, in ms, from a child process under the profiler; None (and why) where that is not possible."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="bbrf_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bb", "--", sys.executable, os.path.abspath(__file__), "--one", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, f"trace run failed (exit {r.returncode})"
        ms, calls = {g: 0.0 for g, _ in GROUPS}, {g: 0 for g, _ in GROUPS}
        ms["other"], calls["other"] = 0.0, 0
        kernels = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            short = name.split("(")[0].split(" ")[-1]
            if short.startswith(("nn_", "bb_")):
                kernels[short] = round(float(row.get("TotalDurationNs", 0.0)) / 1e6, 3)
            g = next((g for g, pre in GROUPS if any(q in name for q in pre)), "other")
            ms[g] += float(row.get("TotalDurationNs", 0.0)) / 1e6; calls[g] += int(float(row.get("Calls", 0)))
        return dict(kernel_ms=ms, launches=calls, calls_traced=2, by_kernel_ms=kernels), None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(n, reps, dev, threads, trace):
    a, na, b, nb = clouds(n, dev)
    call, res, log = make_call(a, na, b, nb, dev)
    med, mn = timed(call, reps)
    r = devmem.read_struct(res, _ext.BbrfResult)
    host_s = host_iteration(a.cpu().numpy(), na.cpu().numpy(), b.cpu().numpy(), nb.cpu().numpy(), threads)
    row = dict(n=n, n0=int(a.shape[0]), n1=int(b.shape[0]), bbrf_ms=med, bbrf_ms_min=mn, iters_run=r.iters_run, status=r.status, best_iter=r.best_iter,
               best_loss=r.best_loss, n_pairs_best=r.n_pairs_best, launches=7 + 15 * r.iters_run, host_iteration_ms=host_s * 1e3)
    if trace:
        split, why = trace_split(n)
        row["trace"] = split if split is not None else dict(unavailable=why)
        if split is not None:                      # the traced child makes a warm-up call and one more: per call = half
            row["kernel_ms_per_call"] = sum(split["kernel_ms"].values()) / split["calls_traced"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="3000,30000,120000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", type=int, default=0, help="run lr_bbrf twice at this size and exit (what the trace's child process does)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "bbrf_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.one:
        call, _, _ = make_call(*clouds(a.one, dev), dev)
        call(); call(); torch.cuda.synchronize()
        return
    threads = min(16, os.cpu_count() or 1)
    rows = [run(int(n), a.reps, dev, threads, not a.no_trace) for n in a.sizes.split(",")]
    line = json.dumps({"bench": "bbrf", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "host_threads": threads, "voxel": VOXEL, "off_deg": OFF_DEG, "off_m": OFF_M, "n_iter": 100, "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
