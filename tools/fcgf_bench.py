"""Device time of the FCGF feature extractor (lr_fcgf_extract, conv1_kernel_size 5, random weights) on one synthetic LiDAR-like frame
(synth.make_scan_pair) of about 4 000, 30 000 and 100 000 voxels at 0.3 m, the cells in the order fcgf.FCGF.extract hands them over.

Every figure is the time between two events around the call: one warm-up per shape, then the median of --reps calls with minimum and
maximum.  The split needs no profiler: a call with tap = 1 stops behind conv1, so its time is the map building (tables, level sets,
gather tables) plus the one vector kernel; the rest of a whole call is the 22 launches of the gather-convolution kernel and the
normalisation.  FLOP rates of that rest, three ways, counted on the host from the same maps (tests/fcgf_cpu.kernel_map):
  dense-equivalent  2 n_out K^3 Cin Cout per stage -- what a dense evaluation of the same active rows would cost;
  issued            what the kernel issues: per (row tile, offset) that has a neighbour, the whole tile x Cin x Cout;
  pairs             2 Cin Cout per (output row, present neighbour) -- the useful work.
Prints one JSON line and writes it to --out (default profiles/fcgf_bench.json).

    python tools/fcgf_bench.py [--points 4400,40000,180000] [--reps 5]

--batch 1,2,8,32 times the batched entry (lr_fcgf_extract_batch) instead: per batch size B, B frames of about 30 000 voxels through one
call, per cloud, beside lr_fcgf_extract on each of the same frames in the same run (the yardstick: that code is the single entry's), the
batch cut behind conv1 for the maps' share, and the effect of the level-0 row order on the single call and on the host-counted
issued / pair flop.  Writes profiles/fcgf_batch_bench.json.

    python tools/fcgf_bench.py --batch 1,2,8,32 [--reps 5]
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
from lidarregistration_amd import _ext, devmem, fcgf, synth, voxel  # noqa: E402
from tests import fcgf_cases, fcgf_cpu  # noqa: E402

TILE = {32: 128, 64: 64, 128: 64, 256: 64}        # output rows per block of sp_conv_kernel (csrc/lr_sparse.h) by Cout (every column tile of a row tile issues the same offsets)


def work(cells, k1=5):
    """(dense-equivalent, issued, pair) flop of stages 2..23 on these cells."""
    L = fcgf_cpu.levels(cells)
    nb = [fcgf_cpu.kernel_map(L[l], L[l], 3, 1 << l) for l in range(4)]
    dn = [fcgf_cpu.kernel_map(L[l + 1], L[l], 3, 1 << l) for l in range(3)]
    up = [fcgf_cpu.kernel_map(L[l], L[l + 1], 3, -(1 << l)) for l in range(3)]
    ident = [(0, np.arange(len(L[0])), None)]
    lvl_map = {2: (0, nb[0]), 3: (0, nb[0]), 4: (1, dn[0]), 5: (1, nb[1]), 6: (1, nb[1]), 7: (2, dn[1]), 8: (2, nb[2]), 9: (2, nb[2]), 10: (3, dn[2]),
               11: (3, nb[3]), 12: (3, nb[3]), 13: (2, up[2]), 14: (2, nb[2]), 15: (2, nb[2]), 16: (1, up[1]), 17: (1, nb[1]), 18: (1, nb[1]),
               19: (0, up[0]), 20: (0, nb[0]), 21: (0, nb[0]), 22: (0, ident), 23: (0, ident)}
    dense = issued = pairs = 0
    for s, (_, _, k3, cin, cout) in enumerate(fcgf.stage_plan(k1), 1):
        if s == 1:
            continue
        lvl, maps = lvl_map[s]
        mac = 2 * cin * cout
        dense += len(L[lvl]) * k3 * mac
        for _, ro, _ in maps:
            pairs += len(ro) * mac
            issued += len(np.unique(ro // TILE[cout])) * TILE[cout] * mac
    return dense, issued, pairs, [len(x) for x in L]


def make_call(m, cells, tap):
    """The library call alone, on buffers made once."""
    L = _ext.lib()
    n = int(cells.shape[0])
    sc = devmem.scratch(L.lr_fcgf_scratch_bytes(n), cells.device)
    res = torch.zeros(16, dtype=torch.uint8, device=cells.device)
    out = torch.zeros((n, 256 if tap else 32), dtype=torch.float32, device=cells.device)
    p = _ext.FcgfParams(conv1_kernel_size=m.conv1_kernel_size, tap=tap)
    st = torch.cuda.current_stream().cuda_stream
    return lambda: _ext.check(L.lr_fcgf_extract(cells.data_ptr(), None, n, m.weights.data_ptr(), m.weights.numel() * 4, ctypes.byref(p), res.data_ptr(),
                                                out.data_ptr(), None, sc.data_ptr(), sc.numel(), st))


def timed(fn, reps, per=1):
    """Median, minimum and maximum over `reps` calls of the time between two events around fn(), divided by `per`; one warm-up."""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def make_batch_call(m, frames):
    """lr_fcgf_extract_batch alone on these frames, on buffers made once."""
    L = _ext.lib()
    B, ns = len(frames), [int(c.shape[0]) for c in frames]
    dev = frames[0].device
    sc = devmem.scratch(L.lr_fcgf_batch_scratch_bytes(B, sum(ns)), dev)
    res = torch.zeros(16 * B, dtype=torch.uint8, device=dev)
    outs = [torch.zeros((n, 32), dtype=torch.float32, device=dev) for n in ns]
    p = _ext.FcgfParams(conv1_kernel_size=m.conv1_kernel_size, tap=0)
    st = torch.cuda.current_stream().cuda_stream
    vp = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    cp, op, np_ = vp(frames), vp(outs), (ctypes.c_int32 * B)(*ns)

    def call(keep=(frames, outs)):          # (the pointer arrays hold addresses only: the closure keeps the tensors alive)
        _ext.check(L.lr_fcgf_extract_batch(B, cp, None, np_, m.weights.data_ptr(), m.weights.numel() * 4, ctypes.byref(p), res.data_ptr(), op, sc.data_ptr(),
                                           sc.numel(), st))
    call()                                   # a refused cloud (status 2 / 3) would be timed as if it had been computed: look once
    blocks = res.cpu().numpy().view(np.int32).reshape(B, 4)
    assert (blocks[:, 0] == 0).all() and blocks[:, 1].tolist() == ns, blocks.tolist()
    return call


def frame_cells(n0, seed):
    """The cells of one frame as fcgf.FCGF.extract_batch builds them: voxel de-duplication, floor(xyz / 0.3) in fp64."""
    raw = synth.make_scan_pair(n0=n0, seed=seed)[0]
    _, sel = voxel.voxel_downsample(raw, 0.3)
    return torch.floor(torch.as_tensor(raw).to(device="cuda", dtype=torch.float64)[sel] / 0.3).to(torch.int32).contiguous()


def batch_rows(m, sizes, reps, n0=40000):
    """One row per batch size B: B frames of about 30 000 voxels (different seeds) through ONE lr_fcgf_extract_batch, per cloud, next to
    lr_fcgf_extract on each of the same frames in the same run; the batch cut behind conv1 (the library's bench hook) gives the maps'
    share.  Then the row order alone, on frame 0 and through the single call, whose code is the parent's: the order extract() hands
    over, a random order and key order (what the batch entry puts level 0 in), with the host-counted issued / pair flop of each."""
    L = _ext.lib()
    frames = [frame_cells(n0, 100 + b) for b in range(max(sizes))]
    single = [timed(make_call(m, c, 0), reps) for c in frames]
    rows = []
    for B in sizes:
        call = make_batch_call(m, frames[:B])
        whole = timed(call, reps, per=B)
        L.lr_debug_fcgf_batch_stop_after(1)
        try:
            maps = timed(call, reps, per=B)
        finally:
            L.lr_debug_fcgf_batch_stop_after(0)
        del call
        s = single[:B]
        rows.append(dict(clouds=B, voxels=[int(c.shape[0]) for c in frames[:B]], batch_per_cloud=whole, batch_maps_and_conv1_per_cloud=maps,
                         maps_share=maps["median_ms"] / whole["median_ms"],
                         single_call=dict(median_ms=float(np.median([x["median_ms"] for x in s])), min_ms=min(x["min_ms"] for x in s), max_ms=max(x["max_ms"] for x in s)),
                         batch_max_below_single_min=whole["max_ms"] < min(x["min_ms"] for x in s)))
    c0 = frames[0].cpu().numpy()
    orders = dict(as_extracted=c0, shuffled=c0[np.random.default_rng(1).permutation(len(c0))], key_order=c0[np.lexsort((c0[:, 2], c0[:, 1], c0[:, 0]))])
    order_rows = {}
    for name, cells in orders.items():
        dense, issued, pairs, _ = work(cells)
        t = torch.from_numpy(np.ascontiguousarray(cells)).cuda()
        order_rows[name] = dict(issued_flop=issued, pair_flop=pairs, issued_over_pair=issued / pairs, single_call=timed(make_call(m, t, 0), reps),
                                single_call_maps_and_conv1=timed(make_call(m, t, 1), reps))
    return rows, order_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4400,40000,180000", help="raw returns per frame (about 4 000, 30 000 and 100 000 voxels)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", default="", help="batch sizes, e.g. 1,2,8,32: time lr_fcgf_extract_batch on that many 30 000-voxel frames instead of the single-frame rows")
    ap.add_argument("--out", default=None, help="default: profiles/fcgf_bench.json, with --batch profiles/fcgf_batch_bench.json")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "fcgf_batch_bench.json" if a.batch else "fcgf_bench.json")
    m = fcgf.FCGF.from_state_dict(fcgf_cases.make_state_dict(0, 5), 5)
    if a.batch:
        rows, orders = batch_rows(m, [int(v) for v in a.batch.split(",")], a.reps)
        line = json.dumps(dict(tool="fcgf_bench --batch", device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows, row_order_on_frame_0=orders))
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    rows = []
    for n0 in (int(v) for v in a.points.split(",")):
        raw = synth.make_scan_pair(n0=n0, seed=3)[0]
        _, sel = voxel.voxel_downsample(raw, 0.3)
        cells = torch.floor(torch.as_tensor(raw).cuda()[sel] / 0.3).to(torch.int32).contiguous()
        dense, issued, pairs, levels = work(cells.cpu().numpy())
        whole = timed(make_call(m, cells, 0), a.reps)
        maps = timed(make_call(m, cells, 1), a.reps)
        conv_ms = whole["median_ms"] - maps["median_ms"]
        rows.append(dict(voxels=levels[0], levels=levels, whole=whole, maps_and_conv1=maps, maps_share=maps["median_ms"] / whole["median_ms"],
                         conv_share=conv_ms / whole["median_ms"], dense_equivalent_flop=dense, issued_flop=issued, pair_flop=pairs,
                         dense_equivalent_tflops=dense / conv_ms * 1e-9, issued_tflops=issued / conv_ms * 1e-9, pair_tflops=pairs / conv_ms * 1e-9))
    out = dict(tool="fcgf_bench", device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows)
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
