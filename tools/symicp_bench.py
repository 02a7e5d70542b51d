"""Device time of the symmetric ICP (lr_symicp at its defaults, and lr_normals2 in front of it) on synthetic scan pairs of 3k, 30k and 120k
raw points (synth.make_scan_pair), both frames down-sampled at voxel 0.3, cloud 0 moved by the true motion off by a small rigid motion,
normals at radius 1.0 / 32 neighbours, points with fewer than 5 neighbours dropped -- what symicp.symmetric_icp runs.

Every figure is the time between two events around the call, median and minimum of --reps calls after a warm-up.  The split into grid +
search, transform, pair and step kernels comes from a kernel trace of one call, taken in a child process of its own (rocprofv3
--kernel-trace --stats).  For context only, lr_icp (point-to-point, full clouds, float32) and lr_bbrf (100 iterations, all normals
(0, 0, 1), tools/bbrf_bench.py's call) on the same pair in the same run, and the pose errors of the symmetric ICP and of lr_icp against
the planted motion.  There is no parent figure and no target.  Prints one JSON line and writes it to --out (default
profiles/symicp_bench.json).

    python tools/symicp_bench.py [--sizes 3000,30000,120000] [--reps 5] [--no-trace]
"""
import argparse
import csv
import ctypes
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bbrf_bench  # noqa: E402
from lidarregistration_amd import _ext, devmem, symicp  # noqa: E402
from lidarregistration_amd.ransac import icp_dev  # noqa: E402

VOXEL, OFF_DEG, OFF_M = bbrf_bench.VOXEL, bbrf_bench.OFF_DEG, bbrf_bench.OFF_M
GROUPS = (("search", ("nn_",)), ("transform", ("sy_xform", "sy_init")), ("pair", ("sy_pair",)), ("step", ("sy_step",)))
timed = bbrf_bench.timed


def clouds(n, dev):
    """(a, b: the down-sampled pair as lr_bbrf's bench builds it; A, nA, B, nB: what lr_symicp gets)."""
    a, _, b, _ = bbrf_bench.clouds(n, dev)
    out = []
    for x in (a, b):
        nrm, cnt, _ = symicp.normals_counted(x)
        keep = cnt >= symicp.MIN_NB
        out += [x[keep].contiguous(), nrm[keep].contiguous()]
    return (a, b, *out)


def make_call(A, nA, B, nB, dev):
    L = _ext.lib()
    n0, n1 = int(A.shape[0]), int(B.shape[0])
    p = _ext.SymicpParams()
    res = torch.zeros(ctypes.sizeof(_ext.SymicpResult), dtype=torch.uint8, device=dev)
    log = torch.zeros((p.n_iter, 8), dtype=torch.float64, device=dev)
    sc = devmem.scratch(L.lr_symicp_scratch_bytes(n0, n1), dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _ext.check(L.lr_symicp(A.data_ptr(), nA.data_ptr(), n0, B.data_ptr(), nB.data_ptr(), n1, ctypes.byref(p), res.data_ptr(), log.data_ptr(),
                               sc.data_ptr(), sc.numel(), st))
    return call, res, log


def make_normals_call(x, dev):
    L = _ext.lib()
    n = int(x.shape[0])
    out = torch.empty((n, 3), dtype=torch.float64, device=dev); cnt = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    sc = devmem.scratch(L.lr_normals_scratch_bytes(n), dev)
    st = torch.cuda.current_stream().cuda_stream
    return lambda: _ext.check(L.lr_normals2(x.data_ptr(), n, symicp.NORMAL_RADIUS, symicp.NORMAL_MAX_NN, out.data_ptr(), cnt.data_ptr(), info.data_ptr(),
                                            sc.data_ptr(), sc.numel(), st))


def errors(M, truth):
    c = (np.trace(M[:3, :3].T @ truth[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(M[:3, 3] - truth[:3, 3])), math.degrees(math.acos(min(1.0, max(-1.0, c))))


def trace_split(n):
    """Kernel time of the traced calls by group, in ms, from a child process under the profiler; None (and why) where that is not possible."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="symicp_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sy", "--", sys.executable, os.path.abspath(__file__), "--one", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, f"trace run failed (exit {r.returncode})"
        ms, calls = {g: 0.0 for g, _ in GROUPS}, {g: 0 for g, _ in GROUPS}
        kernels = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            short = name.split("(")[0].split(" ")[-1]
            if short.startswith("nm_"):          # the normals in front of the traced calls: reported, not part of lr_symicp
                kernels[short] = round(float(row.get("TotalDurationNs", 0.0)) / 1e6, 3)
                continue
            g = next((g for g, pre in GROUPS if any(q in name for q in pre)), None)
            if g is None:
                continue
            kernels[short] = round(float(row.get("TotalDurationNs", 0.0)) / 1e6, 3)
            ms[g] += float(row.get("TotalDurationNs", 0.0)) / 1e6; calls[g] += int(float(row.get("Calls", 0)))
        return dict(kernel_ms=ms, launches=calls, calls_traced=2, by_kernel_ms=kernels,
                    note="the search group includes the grid launches of the two lr_normals2 calls in front of the traced calls"), None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(n, reps, dev, trace):
    a, b, A, nA, B, nB = clouds(n, dev)
    truth_B_to_A = bbrf_bench.small_motion(71, OFF_DEG, OFF_M)
    call, res, log = make_call(A, nA, B, nB, dev)
    med, mn = timed(call, reps)
    r = devmem.read_struct(res, _ext.SymicpResult)
    ste, sre = errors(np.array(r.B_to_A).reshape(4, 4), truth_B_to_A)
    nm_med, nm_min = timed(make_normals_call(a, dev), reps)
    a32, b32 = a.float().contiguous(), b.float().contiguous()
    icp_out = []
    icp_med, icp_min = timed(lambda: icp_out.append(icp_dev(a32, b32, np.eye(4), max_dist=2.0 * VOXEL)), reps)
    ite, ire = errors(np.asarray(icp_out[-1][0], np.float64), np.linalg.inv(truth_B_to_A))
    bb_call, _, _ = bbrf_bench.make_call(*bbrf_bench.clouds(n, dev), dev)
    bb_med, bb_min = timed(bb_call, reps)
    row = dict(n=n, n0_full=int(a.shape[0]), n1_full=int(b.shape[0]), n0=int(A.shape[0]), n1=int(B.shape[0]), symicp_ms=med, symicp_ms_min=mn,
               iters_run=r.iters_run, converged=r.converged, status=r.status, n_pairs=r.n_pairs, mean_sq=r.mean_sq, launches=7 + 15 * r.iters_run,
               te_m=ste, re_deg=sre, normals2_ms=nm_med, normals2_ms_min=nm_min, icp_ms=icp_med, icp_ms_min=icp_min, icp_te_m=ite, icp_re_deg=ire,
               bbrf_ms=bb_med, bbrf_ms_min=bb_min)
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
    ap.add_argument("--one", type=int, default=0, help="run lr_symicp twice at this size and exit (what the trace's child process does)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "symicp_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.one:
        call, _, _ = make_call(*clouds(a.one, dev)[2:], dev)
        call(); call(); torch.cuda.synchronize()
        return
    rows = [run(int(n), a.reps, dev, not a.no_trace) for n in a.sizes.split(",")]
    p = _ext.SymicpParams()
    line = json.dumps({"bench": "symicp", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "voxel": VOXEL, "off_deg": OFF_DEG, "off_m": OFF_M,
                       "params": dict(n_iter=p.n_iter, max_dist=p.max_dist, min_cos=p.min_cos, eps_rot=p.eps_rot, eps_trans=p.eps_trans, piv_eps=p.piv_eps,
                                      normal_radius=symicp.NORMAL_RADIUS, max_nn=symicp.NORMAL_MAX_NN, min_nb=symicp.MIN_NB),
                       "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
