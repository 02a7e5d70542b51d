"""Device time of the exact nearest neighbour (lr_nn3) and of the Z-only refinement (lr_refine_z) on synthetic scan pairs of 30k and
120k raw points (synth.make_scan_pair), both frames down-sampled at voxel 0.3, the raw motion off by 0.37 m in z -- the input of the
generator's refine_motion on a NuScenes-like pair.

Every figure is the time between two events around the call, median and minimum of --reps calls after a warm-up.  The share of queries
that the first phase of the search left to the second is reported with it.  For context only, the same clouds go through the host's
numpy + scipy form of the same loop (cKDTree.query on at most 16 threads) in the same run.  Prints one JSON line and writes it to --out
(default profiles/refine_z_bench.json).

    python tools/refine_z_bench.py [--sizes 30000,120000] [--reps 5]
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
from lidarregistration_amd import _ext, devmem, overlap, synth  # noqa: E402

VOXEL, Z_OFF = 0.3, 0.37


def host_refine(A, B, raw, voxel, threads):
    """GenerateBalancedSet.py:257-291 as the host runs it: (dz, seconds per NN query)."""
    from scipy.spatial import cKDTree
    A_ = A @ raw[:3, :3].T + raw[:3, 3]
    tree = cKDTree(B)
    dz, nn_s = 0.0, []
    for _ in range(10):
        t0 = time.perf_counter()
        _, ind = tree.query(A_, k=1, workers=threads)
        nn_s.append(time.perf_counter() - t0)
        Bs = B[ind]
        valid = np.sqrt(np.sum((A_[:, :2] - Bs[:, :2]) ** 2, axis=1)) <= voxel
        z = A_[valid, 2] - Bs[valid, 2]
        w = 1 / np.abs(z)
        w = np.minimum(w, np.median(w))
        mean = np.sum(w * z) / np.sum(w)
        A_[:, 2] -= mean
        dz -= mean
        if abs(mean) < 1e-6:
            break
    return dz, float(np.median(nn_s))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def run(n, reps, dev, threads):
    L = _ext.lib()
    A, B, T = synth.make_scan_pair(n, n)
    raw = T.copy(); raw[2, 3] += Z_OFF
    a, b = overlap.voxel_down_sample(A, VOXEL), overlap.voxel_down_sample(B, VOXEL)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    Td = torch.from_numpy(raw.reshape(16).copy()).to(dev)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    a_moved = torch.stack([((float(raw[r, 0]) * x + float(raw[r, 1]) * y) + float(raw[r, 2]) * z) + float(raw[r, 3]) for r in range(3)], dim=1).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    idx = torch.empty(n0, dtype=torch.int32, device=dev); dist = torch.empty(n0, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    ns = devmem.scratch(L.lr_nn3_scratch_bytes(n0, n1), dev)
    pn = _ext.Nn3Params()

    def nn():
        _ext.check(L.lr_nn3(a_moved.data_ptr(), n0, b.data_ptr(), n1, ctypes.byref(pn), idx.data_ptr(), dist.data_ptr(), info.data_ptr(), ns.data_ptr(), ns.numel(), st))
    nn_med, nn_min = timed(nn, reps)
    far = int(info.cpu()[3])
    res = torch.zeros(ctypes.sizeof(_ext.RefineZResult), dtype=torch.uint8, device=dev)
    zs = devmem.scratch(L.lr_refine_z_scratch_bytes(n0, n1), dev)
    pz = _ext.RefineZParams(xy_gate=VOXEL)

    def rz():
        _ext.check(L.lr_refine_z(a.data_ptr(), n0, b.data_ptr(), n1, Td.data_ptr(), ctypes.byref(pz), res.data_ptr(), zs.data_ptr(), zs.numel(), st))
    rz_med, rz_min = timed(rz, reps)
    r = devmem.read_struct(res, _ext.RefineZResult)
    t0 = time.perf_counter()
    host_dz, host_nn = host_refine(a.cpu().numpy(), b.cpu().numpy(), raw, VOXEL, threads)
    host_ms = (time.perf_counter() - t0) * 1e3
    return dict(n=n, n0=n0, n1=n1, nn3_ms=nn_med, nn3_ms_min=nn_min, far_share=far / max(n0, 1), refine_z_ms=rz_med, refine_z_ms_min=rz_min,
                repeats=r.repeats, n_valid=r.n_valid, status=r.status, dz=r.dz, host_refine_ms=host_ms, host_nn_ms=host_nn * 1e3, host_dz=host_dz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="30000,120000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "refine_z_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    threads = min(16, os.cpu_count() or 1)
    rows = [run(int(n), a.reps, dev, threads) for n in a.sizes.split(",")]
    line = json.dumps({"bench": "refine_z", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "host_threads": threads, "voxel": VOXEL, "z_off": Z_OFF, "results": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
