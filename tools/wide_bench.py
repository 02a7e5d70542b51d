"""The wide workspace (descriptors of 33..128 numbers) on one MI355X, next to the routes it replaces.

(a) one pair, n x n rows at D = 33, 64, 128: forward top-2 + reverse + mutual through the workspace (lr_nn_top2 + lr_nn_to_mutual) against
    the stand-alone route (matching.nn_wide_dev + matching.mutual_wide_dev: two lr_nn_wide calls plus torch index plumbing); the two
    routes' lists are compared, and the share of cloud-1 rows the reverse pass visits (the unique forward targets) is reported.
(b) lr_register_batch, 32 pairs of 5 000 and of 30 000 points at D = 33, MNN and GPF (GC defaults, --iters hypotheses), against 32
    lr_register_pair calls back to back on a wide workspace; pairs/s for both, and the forward NN kernel's f32-MFMA rate from the
    library's own events around its launches (2 n0 n1 D' flop per pair, D' = D padded to the kernel's steps; merge kernel included).

Every time is between two device events after a warm-up, median and minimum of --reps repeats.  No clock is set; the shader clock the box
runs at under load is recorded before (a) and after (b) with the library's own probe (LR_OPT_CLOCK_PROBE: shader cycles over 100 MHz ticks
of the narrow filter-pass blocks, on a 30 000 x 30 000 x 32 lr_nn_top2), next to the device name and the CU count.  Prints one JSON line
and writes it to --out.

    python tools/wide_bench.py [--n 30000] [--dims 33,64,128] [--sizes 5000,30000] [--pairs 32] [--iters 50000] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lidarregistration_amd import FR, _ext, matching, synth  # noqa: E402

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


def shader_clock_mhz(dev, n=30000, calls=20):
    """The shader clock under NN load, from the library's probe on the narrow path (the wide kernels carry no probe)."""
    F0, F1 = synth.make_features(n, n, 32, 0.5, 1.0, 7)
    t0, t1 = torch.from_numpy(F0).to(dev), torch.from_numpy(F1).to(dev)
    ws = _ext.Workspace(n, n, 32, 1)
    idx1 = torch.empty(n, dtype=torch.int32, device=dev)
    call = lambda: _ext.check(_ext.lib().lr_nn_top2(ws.handle, t0.data_ptr(), n, t1.data_ptr(), n, 32, idx1.data_ptr(), None, None, None,
                                                    torch.cuda.current_stream().cuda_stream))
    call(); torch.cuda.synchronize()
    ws.set_option("clock_probe", 1)
    ws.clock(reset=True)
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    mhz, _, _ = ws.clock(reset=True)
    ws.close()
    return mhz


class Args:
    def __init__(self, **kw):
        self.mode = "MNN"; self.codebase = "GC"; self.iters = 50000; self.prosac = True
        self.GPF_grid_wid = 10; self.GPF_factor = 2.0
        self.__dict__.update(kw)


def one_pair(n, d, reps, dev):
    F0, F1 = synth.make_features(n, n, d, 0.5, 0.5, 51)
    t0, t1 = torch.from_numpy(F0).to(dev), torch.from_numpy(F1).to(dev)
    L = _ext.lib()
    ws = _ext.Workspace.wide(n, n, d, 1)
    st = torch.cuda.current_stream().cuda_stream
    idx1 = torch.empty(n, dtype=torch.int32, device=dev); idx2 = torch.empty_like(idx1)
    is_bb = torch.empty(n, dtype=torch.uint8, device=dev)
    o = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)

    def through_workspace():
        _ext.check(L.lr_nn_top2(ws.handle, t0.data_ptr(), n, t1.data_ptr(), n, d, idx1.data_ptr(), idx2.data_ptr(), None, None, st))
        _ext.check(L.lr_nn_to_mutual(ws.handle, t0.data_ptr(), n, t1.data_ptr(), n, d, idx1.data_ptr(), idx2.data_ptr(), is_bb.data_ptr(),
                                     o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), cnt.data_ptr(), st))

    got = {}

    def stand_alone():
        i1, i2, _, _ = matching.nn_wide_dev(t0, t1, want_2nd=True)
        got["r"] = (i1,) + tuple(matching.mutual_wide_dev(t0, t1, i1, i2))

    ws_ms = timed(through_workspace, reps)
    sa_ms = timed(stand_alone, reps)
    m = int(cnt.item())
    i1, bb, a0, a1, a2 = got["r"]
    same = (bool(torch.equal(i1, idx1)) and bool(torch.equal(bb, is_bb)) and m == a0.shape[0] and bool(torch.equal(o[0][:m], a0))
            and bool(torch.equal(o[1][:m], a1)) and bool(torch.equal(o[2][:m], a2)))
    visited = int(torch.unique(idx1).numel())
    ws.close()
    return dict(n0=n, n1=n, dim=d, workspace_ms=ws_ms[0], workspace_ms_min=ws_ms[1], stand_alone_ms=sa_ms[0], stand_alone_ms_min=sa_ms[1],
                speedup=sa_ms[0] / ws_ms[0], same_lists=same, mutual_pairs=m, reverse_rows_visited=visited, reverse_rows_share=visited / n)


def batch(n, d, npairs, mode, iters, reps, dev):
    pairs = []
    for k in range(npairs):
        p = synth.make_pair_dev(N=n, D=d, seed=100 + k, device=dev)
        pairs.append((p["xyz0"], p["xyz1"], p["feats0"], p["feats1"]))
    params = FR.pair_params(Args(mode=mode, iters=iters))
    params.icp = 0
    wsb = _ext.Workspace.wide(n, n, d, iters, max_pairs=npairs)
    ws1 = _ext.Workspace.wide(n, n, d, iters)
    size = ctypes.sizeof(_ext.PairResult)
    outb = torch.zeros((npairs, size), dtype=torch.uint8, device=dev); outs = torch.zeros_like(outb)

    def batched():
        FR.register_batch_dev(pairs, params, out=outb, ws=wsb)

    def sequential():
        for k, p in enumerate(pairs):
            FR.register_pair_dev(*p, params, out=outs[k], ws=ws1)

    b_ms = timed(batched, reps)
    s_ms = timed(sequential, reps)
    same = bool(torch.equal(outb, outs))
    ok = sum(_ext.PairResult.from_buffer_copy(outb[k].cpu().numpy().tobytes()).status == 0 for k in range(npairs))
    # the forward NN kernel's own launches, from the library's events (one timed sample per call)
    wsb.timing(True); torch.cuda.synchronize()
    for _ in range(reps):          # (one sample is in flight at a time: each is folded into the sums before the next call)
        batched(); torch.cuda.synchronize()
        ms, samples = wsb.stage_times()
    wsb.timing(False)
    fwd_ms = ms[2] / max(samples, 1)
    flop = 2.0 * n * n * 2 * steps(d) * npairs
    wsb.close(); ws1.close()
    return dict(n=n, dim=d, pairs=npairs, mode=mode, iters=iters, batch_ms=b_ms[0], batch_ms_min=b_ms[1], sequential_ms=s_ms[0], sequential_ms_min=s_ms[1],
                batch_pairs_per_s=npairs / (b_ms[0] * 1e-3), sequential_pairs_per_s=npairs / (s_ms[0] * 1e-3), same_bytes=same, pairs_registered=int(ok),
                forward_nn_ms=fwd_ms, forward_nn_samples=samples, forward_nn_tflops=flop / (fwd_ms * 1e-3) / 1e12 if fwd_ms > 0 else None,
                forward_nn_share_of_f32_mfma_peak=flop / PEAK_F32_MFMA / (fwd_ms * 1e-3) if fwd_ms > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--dims", type=str, default="33,64,128")
    ap.add_argument("--sizes", type=str, default="5000,30000")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "wide_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    clock = [shader_clock_mhz(dev)]
    a_rows = [one_pair(a.n, int(d), a.reps, dev) for d in a.dims.split(",")]
    b_rows = [batch(int(n), 33, a.pairs, mode, a.iters, a.reps, dev) for n in a.sizes.split(",") for mode in ("MNN", "GPF")]
    clock.append(shader_clock_mhz(dev))
    line = json.dumps({"bench": "wide_workspace", "device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                       "shader_clock_mhz_before_after": clock,
                       "one_pair": a_rows, "batch": b_rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
