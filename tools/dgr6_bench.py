"""Device time of DGR's 6-D inlier network (lr_dgr_inlier, random weights of ResUNetBN2C's shape) on the correspondences of one synthetic
LiDAR-like frame pair (synth.make_scan_pair) at 0.3 m: every voxel of frame 0 with its feature nearest neighbour in frame 1, the features
from the FCGF extractor (random weights), as dgr.DGR.register builds them.

Every figure is the time between two events around the call: one warm-up per shape, then the median of --reps calls with minimum and
maximum.  The split needs no profiler: a call with tap = 1 stops behind conv1, so its time is the map building (tables, level sets, the
ten dense gather tables) plus the one vector kernel; the rest of a whole call is the 21 launches of the gather-convolution kernel and the
final vector kernel.  FLOP rates of that rest, three ways, counted on the host from the same maps (tests/dgr6_cpu.kernel_map):
  dense-equivalent  2 n_out 729 Cin Cout per stage -- what a dense evaluation of the same active rows would cost;
  issued            what the kernel issues: per (row tile, offset) that has a neighbour, the whole tile x Cin x Cout;
  pairs             2 Cin Cout per (output row, present neighbour) -- the useful work.
Prints one JSON line and writes it to --out (default profiles/dgr6_bench.json).

    python tools/dgr6_bench.py [--points 4400,40000] [--reps 5]
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
from lidarregistration_amd import _ext, devmem, dgr, fcgf, synth  # noqa: E402
from lidarregistration_amd.matching import nn_top2_dev  # noqa: E402
from tests import dgr6_cpu, fcgf_cases  # noqa: E402


def tile(cout):
    return 128 if cout % 64 else 64          # output rows per block of sp_conv_kernel (csrc/lr_sparse.h)


def work(rows, widths):
    """(dense-equivalent, issued, pair) flop of stages 2..23 on these rows, and the level counts."""
    L = dgr6_cpu.levels(rows)
    org = dgr6_cpu.origin(rows)
    nb = [dgr6_cpu.kernel_map(L[l], L[l], 1 << l, org) for l in range(4)]
    dn = [dgr6_cpu.kernel_map(L[l + 1], L[l], 1 << l, org) for l in range(3)]
    up = [dgr6_cpu.kernel_map(L[l], L[l + 1], -(1 << l), org) for l in range(3)]
    ident = [(0, np.arange(len(L[0])), None)]
    lvl_map = {2: (0, nb[0]), 3: (0, nb[0]), 4: (1, dn[0]), 5: (1, nb[1]), 6: (1, nb[1]), 7: (2, dn[1]), 8: (2, nb[2]), 9: (2, nb[2]), 10: (3, dn[2]),
               11: (3, nb[3]), 12: (3, nb[3]), 13: (2, up[2]), 14: (2, nb[2]), 15: (2, nb[2]), 16: (1, up[1]), 17: (1, nb[1]), 18: (1, nb[1]),
               19: (0, up[0]), 20: (0, nb[0]), 21: (0, nb[0]), 22: (0, ident), 23: (0, ident)}
    dense = issued = pairs = 0
    for s, (k, cin, cout) in enumerate(dgr6_cpu.stage_shapes(widths), 1):
        if s == 1:
            continue
        lvl, maps = lvl_map[s]
        mac = 2 * cin * cout
        dense += len(L[lvl]) * k * mac
        for _, ro, _ in maps:
            pairs += len(ro) * mac
            issued += (len(np.unique(ro // tile(cout))) * tile(cout) if s < 23 else len(ro)) * mac
    return dense, issued, pairs, [len(x) for x in L]


def make_call(net, rows, tap):
    """The library call alone, on buffers made once."""
    L = _ext.lib()
    n = int(rows.shape[0])
    w8 = (ctypes.c_int32 * 8)(*net.widths)
    sc = devmem.scratch(L.lr_dgr_inlier_scratch_bytes(n, ctypes.byref(w8)), rows.device)
    res = torch.zeros(16, dtype=torch.uint8, device=rows.device)
    out = torch.zeros(n * (max(net.widths) if tap else 1), dtype=torch.float32, device=rows.device)
    p = _ext.DgrInlierParams(tap=tap, widths=net.widths)
    st = torch.cuda.current_stream().cuda_stream
    blob = net.weights_blob

    def call():
        _ext.check(L.lr_dgr_inlier(rows.data_ptr(), n, blob.data_ptr(), blob.numel() * 4, ctypes.byref(p), res.data_ptr(), out.data_ptr(), None, sc.data_ptr(),
                                   sc.numel(), st))
    call()                                   # a refused input (status 2 / 3) would be timed as if it had been computed: look once
    block = res.cpu().numpy().view(np.int32)
    assert block[0] == 0 and block[1] == n, block.tolist()
    return call


def timed(fn, reps):
    """Median, minimum and maximum over `reps` calls of the time between two events around fn(); one warm-up."""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def make_batch_call(net, rows_list):
    """One lr_dgr_inlier_batch over the pairs, on buffers made once."""
    L = _ext.lib()
    P = len(rows_list)
    ns = [int(r.shape[0]) for r in rows_list]
    dev = rows_list[0].device
    w8 = (ctypes.c_int32 * 8)(*net.widths)
    sc = devmem.scratch(L.lr_dgr_inlier_batch_scratch_bytes(P, sum(ns), ctypes.byref(w8)), dev)
    res = torch.zeros(16 * P, dtype=torch.uint8, device=dev)
    outs = [torch.zeros(n, dtype=torch.float32, device=dev) for n in ns]
    p = _ext.DgrInlierParams(tap=0, widths=net.widths)
    st = torch.cuda.current_stream().cuda_stream
    blob = net.weights_blob
    vp = lambda ts: (ctypes.c_void_p * P)(*[t.data_ptr() for t in ts])
    coords, logit, n_arr = vp(rows_list), vp(outs), (ctypes.c_int32 * P)(*ns)

    def call():
        _ext.check(L.lr_dgr_inlier_batch(P, coords, n_arr, blob.data_ptr(), blob.numel() * 4, ctypes.byref(p), res.data_ptr(), logit, sc.data_ptr(), sc.numel(), st))
    call()
    block = res.cpu().numpy().view(np.int32).reshape(P, 4)
    assert not block[:, 0].any() and block[:, 1].tolist() == ns, block.tolist()
    return call


def correspondences(reg, feat, net, n0, seed):
    raw0, raw1, _ = synth.make_scan_pair(n0=n0, seed=seed)
    k0, _, c0 = reg.preprocess(raw0)
    k1, _, c1 = reg.preprocess(raw1)
    idx1 = nn_top2_dev(feat.features(c0), feat.features(c1), want_2nd=False)[0].long()
    return net.coords6(k0, k1, torch.arange(idx1.shape[0], device=idx1.device), idx1, 0.3)


def bench_batch(reg, feat, net, reps):
    """The rows of the one-pair table as batches: 8 distinct pairs of about 4 000 correspondences and 4 of about 30 000 (different
    synth.make_scan_pair seeds).  (a) lr_dgr_inlier once per pair back to back on one stream, (b) ONE lr_dgr_inlier_batch; the same
    process, the same method (`timed`)."""
    out = []
    for pairs, n0 in ((8, 4400), (4, 40000)):
        rows = [correspondences(reg, feat, net, n0, 3 + s) for s in range(pairs)]
        singles = [make_call(net, r, 0) for r in rows]
        one = timed(lambda: [c() for c in singles], reps)
        batch = timed(make_batch_call(net, rows), reps)
        spread = one["max_ms"] - one["min_ms"]
        out.append(dict(pairs=pairs, correspondences=[int(r.shape[0]) for r in rows], one_pair_calls=one, batch_call=batch,
                        one_pair_ms_per_pair=one["median_ms"] / pairs, batch_ms_per_pair=batch["median_ms"] / pairs,
                        ratio_one_pair_over_batch=one["median_ms"] / batch["median_ms"], one_pair_spread_ms=spread,
                        batch_not_above_one_pair_by_more_than_its_spread=bool(batch["median_ms"] <= one["median_ms"] + spread)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4400,40000", help="raw returns per frame (about 4 000 and 30 000 correspondences)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgr6_bench.json"))
    ap.add_argument("--batch", action="store_true", help="time lr_dgr_inlier_batch against the one-pair entry called per pair, and put the "
                    "result under the key 'batch' of the line already in --out (the one-pair table there is kept)")
    a = ap.parse_args()
    feat = fcgf.FCGF.from_state_dict(fcgf_cases.make_state_dict(0, 5), 5)
    net = dgr.InlierNet.from_stages(dgr6_cpu.random_stages(dgr6_cpu.WIDTHS, seed=0))
    reg = dgr.DGR(feat, net, voxel_size=0.3)
    if a.batch:
        doc = json.loads(open(a.out).read()) if os.path.exists(a.out) else dict(tool="dgr6_bench")
        doc["batch"] = dict(device=torch.cuda.get_device_name(0), widths=list(net.widths), reps=a.reps, shapes=bench_batch(reg, feat, net, a.reps))
        line = json.dumps(doc)
        print(json.dumps(doc["batch"]))
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    out_rows = []
    for n0 in (int(v) for v in a.points.split(",")):
        raw0, raw1, _ = synth.make_scan_pair(n0=n0, seed=3)
        k0, _, c0 = reg.preprocess(raw0)
        k1, _, c1 = reg.preprocess(raw1)
        idx1 = nn_top2_dev(feat.features(c0), feat.features(c1), want_2nd=False)[0].long()
        rows = net.coords6(k0, k1, torch.arange(idx1.shape[0], device=idx1.device), idx1, 0.3)
        dense, issued, pairs, levels = work(rows.cpu().numpy(), net.widths)
        whole = timed(make_call(net, rows, 0), a.reps)
        maps = timed(make_call(net, rows, 1), a.reps)
        conv_ms = whole["median_ms"] - maps["median_ms"]
        out_rows.append(dict(correspondences=levels[0], levels=levels, whole=whole, maps_and_conv1=maps, maps_share=maps["median_ms"] / whole["median_ms"],
                             conv_share=conv_ms / whole["median_ms"], dense_equivalent_flop=dense, issued_flop=issued, pair_flop=pairs,
                             dense_equivalent_tflops=dense / conv_ms * 1e-9, issued_tflops=issued / conv_ms * 1e-9, pair_tflops=pairs / conv_ms * 1e-9))
    line = json.dumps(dict(tool="dgr6_bench", device=torch.cuda.get_device_name(0), widths=list(net.widths), reps=a.reps, rows=out_rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
