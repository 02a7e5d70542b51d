"""What the correspondence-set back ends (teaser.py, sm.py) share: the ctypes plumbing of a lr_*_batch / lr_* call (BatchCall) and the
batched engine of ``python -m test --algo TEASER | SM`` (eval_pairs).  A back end describes its solver to them (Solver) and keeps its
own correspondences_dev, params and result decoding.  The C side's counterpart is csrc/lr_corrset.h.
"""
import ctypes
import time
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from . import FR as fr
from . import _ext, devmem, harness, ransac
from .devmem import ptr, read_struct
from .matching import _f32, _stream


@dataclass(frozen=True)
class Solver:
    """A back end as BatchCall needs it: the library's entry points by name, the ctypes mirrors of its params / result structs, its
    per-pair output arrays in the ABI's order as (dtype, fill value), and what turns a result struct into the info dict."""
    single: str
    batch: str
    scratch_bytes: str
    params: type
    result: type
    outputs: tuple
    info: Callable


class BatchCall:
    """One call of a solver over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0), built once and launched as often as wanted.
    Owns the scratch (npairs arenas of scratch_bytes(max m)), the result buffer, the per-pair output tensors `outs[i][k]` (outputs=False:
    none are asked for) and the ctypes pointer arrays.  ms: the counts passed as m (default: the rows); m_devs: optional device int32
    tensors with a smaller live count; poison: fill the scratch with this byte first (test hook); single: go through the single-pair
    entry point (one pair); kw: the solver's params."""

    def __init__(self, solver, srcs, tgts, ms=None, m_devs=None, poison=None, single=False, outputs=True, **kw):
        L = _ext.lib()
        self.solver, self.n = solver, len(srcs)
        self.srcs = [_f32(s).reshape(-1, 3) for s in srcs]
        self.tgts = [_f32(t).reshape(-1, 3) for t in tgts]
        dev = self.srcs[0].device
        self.ms = [int(s.shape[0]) for s in self.srcs] if ms is None else [int(v) for v in ms]
        self.scratch = devmem.scratch(getattr(L, solver.scratch_bytes)(max(self.ms)) * self.n, dev, poison)
        self.res = torch.zeros(ctypes.sizeof(solver.result) * self.n, dtype=torch.uint8, device=dev)
        self.outs = [[torch.full((max(m, 1),), fill, dtype=dt, device=dev) for m in self.ms] if outputs else None for dt, fill in solver.outputs]
        self.m_devs = m_devs
        self.params = solver.params(**kw)
        if single:
            assert self.n == 1
            self._fn = getattr(L, solver.single)
            pairs = (ptr(self.srcs[0]), ptr(self.tgts[0]), self.ms[0], ptr(m_devs and m_devs[0]))
            outs = [ptr(o and o[0]) for o in self.outs]
        else:
            arr = lambda ts: None if ts is None else (ctypes.c_void_p * self.n)(*[ptr(t) for t in ts])
            self._fn = getattr(L, solver.batch)
            pairs = (self.n, arr(self.srcs), arr(self.tgts), (ctypes.c_int32 * self.n)(*self.ms), arr(m_devs))
            outs = [arr(o) for o in self.outs]
        self._args = (*pairs, ctypes.byref(self.params), self.res.data_ptr(), *outs, self.scratch.data_ptr(), self.scratch.numel())

    def launch(self, stream):
        _ext.check(self._fn(*self._args, stream))

    def timed(self):
        """launch() on the current stream between two events, synchronised: the device time of the call in ms."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        self.launch(_stream())
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1)

    def results(self):
        """[(T 4x4 float64, info dict)] per pair (the copy synchronises with the current stream)."""
        host = self.res.cpu()
        rs = [read_struct(host, self.solver.result, k) for k in range(self.n)]
        return [(np.array(r.T[:], np.float64).reshape(4, 4), self.solver.info(r)) for r in rs]


def timed_icp(ws, p, T, dev):
    """lr_icp of pair p from T (the harness' settings, test.py:183-189) on the current stream, timed by its own events: (T_icp 4x4, seconds)."""
    Tin = torch.from_numpy(np.ascontiguousarray(T.reshape(16))).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    T_icp, _ = ransac.icp_launch(ws, p["xyz0"], p["xyz1"], Tin.data_ptr(), _stream(), max_dist=2 * fr.VOXEL_SIZE)
    e1.record(); e1.synchronize()
    return T_icp.cpu().numpy().reshape(4, 4), e0.elapsed_time(e1) * 1e-3


def eval_pairs(source, indices, args, correspondences_dev, solve, row_hook=None, exact=None, device=None, batch=32, nstreams=3, verbose=False):
    """The engine behind teaser.eval_pairs / sm.eval_pairs over `indices` of `source`: per window of `batch` pairs, the back end's
    correspondences_dev runs pair by pair on the single-pair entry points (spread over `nstreams` streams), the correspondences' xyz are
    gathered, ONE solve(srcs, tgts) -> ([(T, info, ...)], device ms) solves the window, and ICP follows through lr_icp.  row_hook(row, T,
    info) -> T may replace a pair's transform (and record what it likes); `exact` is handed on to the EvalRun.  Column 9 = the pair's
    share of its window's solve (the call's device time split evenly); the NN / filter time is not billed (TEASER_plus_plus.py:109-123)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    n = len(indices)
    stats = np.full((n, 22), np.nan)
    Ts = np.tile(np.eye(4), (n, 1, 1))
    whole = np.zeros(n)
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(1, nstreams))]
    wss = [None] * batch
    tot = dict(data_s=0.0, registration_s=0.0, icp_s=0.0, stats_s=0.0, pairs=n)
    use_icp = getattr(args, "icp", True)
    # whatever ends the loop, every workspace is released on the way out (harness.eval_pairs)
    try:
        for w0 in range(0, n, batch):
            rows = list(range(w0, min(n, w0 + batch)))
            t0 = time.time()
            pairs = [source.get_dev(indices[r], dev) for r in rows]
            torch.cuda.synchronize(dev)
            t1 = time.time()
            corr = []
            for j, p in enumerate(pairs):
                s = streams[j % len(streams)]
                harness.slot_workspace(wss, j, p["feats0"].shape[0], p["feats1"].shape[0], p["feats0"].shape[1], 1, headroom=1.25, sync=dev)
                with torch.cuda.stream(s):
                    corr.append(correspondences_dev(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], args, wss[j], s.cuda_stream))
            torch.cuda.synchronize(dev)
            counts = [int(v) for v in torch.stack([c[2][0] for c in corr]).cpu()]
            srcs = [p["xyz0"][c[0][:m].long()] for p, c, m in zip(pairs, corr, counts)]
            tgts = [p["xyz1"][c[1][:m].long()] for p, c, m in zip(pairs, corr, counts)]
            out, ms = solve(srcs, tgts)
            t2 = time.time()
            for j, r in enumerate(rows):
                T, info = out[j][:2]
                Ts[r] = T if row_hook is None else row_hook(r, T, info)
                whole[r] = ms * 1e-3 / len(rows)
                p = pairs[j]
                harness.write_row(stats, r, Ts[r], p["T_gt"], whole[r], (t1 - t0) / len(rows), p["feats0"].shape[0], counts[j], source.ids(indices[r]),
                                  icp=timed_icp(wss[j], p, Ts[r], dev) if use_icp else None)
            tot["data_s"] += t1 - t0; tot["registration_s"] += t2 - t1; tot["icp_s"] += time.time() - t2
            if verbose:
                print(f"{time.strftime('%m/%d %H:%M:%S')} Finished pair:{rows[-1]}/{n}", flush=True)
        torch.cuda.synchronize(dev)
    finally:
        for ws in wss:
            if ws is not None:
                ws.close()
    return harness.EvalRun(stats, Ts, whole, tot, exact)
