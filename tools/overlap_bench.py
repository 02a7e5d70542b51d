"""Device time of the pair overlap measure (lr_overlap_batch) and of the Open3D-style down-sampling (lr_voxel_mean) on synthetic raw
frames of 30k and 120k points, voxel 1.0 and 0.3, batch 1 and 32 (one source frame against `batch` target frames: the candidate loop of
GenerateBalancedSet.py:321-371).

Every figure is the time between two events around the call, median and minimum of --reps calls after a warm-up.  For context only, the
same clouds go through the host's numpy + scipy form of the same measure (np.unique cells, np.add.at centroids, cKDTree.query on at most
16 threads) in the same run.  Prints one JSON line and writes it to --out (default profiles/overlap_bench.json).

    python tools/overlap_bench.py [--sizes 30000,120000] [--voxels 1.0,0.3] [--batches 1,32] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import _ext, devmem, synth  # noqa: E402


def host_downsample(X, voxel):
    vmb = X.min(axis=0) - voxel * 0.5
    c = np.floor((X - vmb) / voxel).astype(np.int64)
    _, inv = np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], return_inverse=True)
    s = np.zeros((inv.max() + 1, 3))
    np.add.at(s, inv, X)
    return s / np.bincount(inv)[:, None]


def host_overlap(A, B, T, voxel):
    from scipy.spatial import cKDTree
    a, b = host_downsample(A @ T[:3, :3].T + T[:3, 3], voxel), host_downsample(B, voxel)
    d, _ = cKDTree(b).query(a, k=1, workers=min(16, os.cpu_count() or 1))
    n = int((d < np.sqrt(2) * voxel).sum())
    return n / len(a), min(n / len(a), n / len(b))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def run(n, voxel, batch, reps, dev):
    L = _ext.lib()
    frames = [synth.make_scan_pair(n, n, seed=7000 + k, forward=4.0 + (3.0 * k) % 40, yaw_deg=2.0 + k % 9) for k in range(batch)]
    A = frames[0][0]
    Ad = torch.from_numpy(A).to(dev)
    Bd = [torch.from_numpy(f[1]).to(dev) for f in frames]
    Td = [torch.from_numpy(f[2].reshape(16).copy()).to(dev) for f in frames]
    vp = ctypes.c_void_p
    xyz0 = (vp * batch)(*[Ad.data_ptr()] * batch); xyz1 = (vp * batch)(*[b.data_ptr() for b in Bd]); Ts = (vp * batch)(*[t.data_ptr() for t in Td])
    ns = (ctypes.c_int32 * batch)(*[n] * batch)
    p = _ext.OverlapParams(voxel_size=voxel)
    res = torch.zeros((batch, ctypes.sizeof(_ext.OverlapResult)), dtype=torch.uint8, device=dev)
    scratch = devmem.scratch(L.lr_overlap_scratch_bytes(n, n) * batch, dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _ext.check(L.lr_overlap_batch(batch, xyz0, ns, xyz1, ns, Ts, ctypes.byref(p), res.data_ptr(), scratch.data_ptr(), scratch.numel(), st))
    med, mn = timed(call, reps)
    out = [devmem.read_struct(res, _ext.OverlapResult, k) for k in range(batch)]
    cent = torch.empty((n, 3), dtype=torch.float64, device=dev); info = torch.zeros(4, dtype=torch.int32, device=dev)
    vs = devmem.scratch(L.lr_voxel_mean_scratch_bytes(n), dev)

    def down():
        _ext.check(L.lr_voxel_mean(Ad.data_ptr(), n, None, voxel, cent.data_ptr(), None, None, None, info.data_ptr(), vs.data_ptr(), vs.numel(), st))
    dmed, dmin = timed(down, reps)
    t0 = time.perf_counter()
    host = [host_overlap(A, f[1], f[2], voxel) for f in frames[:min(batch, 4)]]
    host_ms = (time.perf_counter() - t0) * 1e3 / len(host)
    return dict(n=n, voxel=voxel, batch=batch, call_ms=med, call_ms_min=mn, pair_ms=med / batch, voxel_mean_ms=dmed, voxel_mean_ms_min=dmin,
                host_pair_ms=host_ms, rows0=out[0].n0_ds, rows1=out[0].n1_ds, frac=[round(o.frac, 4) for o in out[:4]],
                frac_host=[round(h[0], 4) for h in host], ok=int(sum(o.status == 0 for o in out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="30000,120000")
    ap.add_argument("--voxels", type=str, default="1.0,0.3")
    ap.add_argument("--batches", type=str, default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "overlap_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [run(int(n), float(v), int(b), a.reps, dev) for n in a.sizes.split(",") for v in a.voxels.split(",") for b in a.batches.split(",")]
    line = json.dumps({"bench": "overlap_batch", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "host_threads": min(16, os.cpu_count() or 1), "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
