"""What the correspondence-set back ends (teaser.py, sm.py, pointdsc.py, dgr.py) share: the ctypes plumbing of a lr_*_batch / lr_* call
(BatchCall: lr_teaser, lr_sm, lr_pdsc_encode, lr_pdsc_solve, lr_pdsc_register, lr_dgr_refine and their _batch forms) and the batched
engine of ``python -m test --algo TEASER | SM | PointDSC | DGR`` (eval_pairs).  A back end describes each entry-point pair to them (Solver,
In, Out) and keeps its own correspondences_dev, params and result decoding.  The C side's counterpart is csrc/lr_corrset.h.
"""
import ctypes
import time
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from . import FR as fr
from . import _ext, devmem, harness, ransac
from .devmem import ptr
from .matching import _device, _stream


def _m(m, params):
    return m


@dataclass(frozen=True)
class In:
    """An extra per-pair input: BatchCall's keyword for it (a list with one entry per pair; the list or an entry may be None: NULL), its
    dtype and the shape one pair's array is brought to."""
    name: str
    dtype: torch.dtype
    shape: tuple


@dataclass(frozen=True)
class Out:
    """An output array: its name (the `want_<name>` selector of a per-pair output), dtype, the fill an entry the library does not write
    keeps (tests read it), its columns (None: one-dimensional; an int; or the name of the params field that holds the number) and its
    rows as a function of (m, params).  The tensor has max(rows, 1) rows."""
    name: str
    dtype: torch.dtype
    fill: float
    width: object = None
    rows: Callable = _m

    def alloc(self, m, params, dev):
        w = getattr(params, self.width) if isinstance(self.width, str) else self.width
        return torch.full((max(self.rows(m, params), 1),) + (() if w is None else (w,)), self.fill, dtype=self.dtype, device=dev)


@dataclass(frozen=True)
class Solver:
    """A back end as BatchCall needs it, in the order every entry point of the family takes its arguments: the pairs; `inputs`, the extra
    per-pair inputs; `call_args`, the keywords of call-level arguments passed as they are; `params`, the ctypes mirrors of the params
    struct(s); the `result` struct; `outputs`, the per-pair outputs; `extras`, outputs of the single-pair entry point only, asked for
    with the keyword `extras_flag` (on the batched one: an AssertionError with `extras_msg`); the scratch.  single / batch /
    scratch_bytes: the library's entry points by name; info: what turns a result struct into the info dict."""
    single: str
    batch: str
    scratch_bytes: str
    params: tuple
    result: type
    outputs: tuple
    info: Callable = None
    inputs: tuple = ()
    call_args: tuple = ()
    extras: tuple = ()
    extras_flag: str = ""
    extras_msg: str = ""


def _arr(ts, n):
    """The ctypes array of n device pointers of a batched call: None for a missing list, NULL for a missing entry."""
    return None if ts is None else (ctypes.c_void_p * n)(*[ptr(t) for t in ts])


def _asked(ts, want):
    """The output tensors as a call sees them: all, none (False: NULL for the whole array) or NULL per entry (a list of bools)."""
    return ts if want is None or ts is None else None if want is False else [t if ok else None for t, ok in zip(ts, want)]


class BatchCall:
    """One call of a solver over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0), built once and launched as often as wanted.
    Owns the scratch (npairs arenas of scratch_bytes(max m)), the result buffer, the extra inputs `inputs[i][k]`, the full-length per-pair
    output tensors `outs[i][k]` (outputs=False: none exist), the single-only `extras` and the ctypes pointer arrays.  ms: the counts
    passed as m (default: the rows); m_devs: optional device int32 tensors with a smaller live count (an entry may be None); poison: fill
    the scratch with this byte first (test hook); single: go through the single-pair entry point (one pair); params: the params structs
    ready made (a solver with several); device: where the buffers live (default: the current HIP device).  kw: the solver's inputs and
    call-level arguments by name, want_<output> (None: all; False: NULL for the whole array; a list of bools: NULL per entry -- the tensor
    of an output that was not asked for keeps its fill), the solver's extras_flag, and the fields of its params struct."""

    def __init__(self, solver, srcs, tgts, ms=None, m_devs=None, poison=None, single=False, outputs=True, params=None, device=None, **kw):
        L = _ext.lib()
        self.solver, self.n = solver, len(srcs)
        dev = _device() if device is None else torch.device(device)
        to = lambda t, dtype, shape: torch.as_tensor(t).to(device=dev, dtype=dtype).contiguous().reshape(shape)
        self.srcs = [to(s, torch.float32, (-1, 3)) for s in srcs]
        self.tgts = [to(t, torch.float32, (-1, 3)) for t in tgts]
        self.ms = [int(s.shape[0]) for s in self.srcs] if ms is None else [int(v) for v in ms]
        self.m_devs = m_devs
        given = [kw.pop(i.name, None) for i in solver.inputs]
        self.inputs = [g and [None if t is None else to(t, i.dtype, i.shape) for t in g] for g, i in zip(given, solver.inputs)]
        head = [kw.pop(a) for a in solver.call_args]
        wants = [kw.pop("want_" + o.name, None) for o in solver.outputs]
        extras = bool(solver.extras) and kw.pop(solver.extras_flag, False)
        assert params is None or not kw, kw
        self.all_params = tuple(P(**kw) for P in solver.params) if params is None else tuple(params)
        self.params = p = self.all_params[-1]          # (the struct the output shapes depend on)
        self.scratch = devmem.scratch(getattr(L, solver.scratch_bytes)(max(self.ms)) * self.n, dev, poison)
        self.res = torch.zeros(ctypes.sizeof(solver.result) * self.n, dtype=torch.uint8, device=dev)
        self.outs = [[o.alloc(m, p, dev) for m in self.ms] if outputs else None for o in solver.outputs]
        self.extras = [o.alloc(self.ms[0], p, dev) for o in solver.extras] if extras else None
        if single:
            assert self.n == 1
            self._fn = getattr(L, solver.single)
            at = lambda ts: ptr(ts and ts[0])
            pairs = (at(self.srcs), at(self.tgts), self.ms[0], at(m_devs))
            tail = [ptr(t) for t in self.extras] if extras else [None] * len(solver.extras)
        else:
            assert not extras, solver.extras_msg
            self._fn = getattr(L, solver.batch)
            at = lambda ts: _arr(ts, self.n)
            pairs = (self.n, at(self.srcs), at(self.tgts), (ctypes.c_int32 * self.n)(*self.ms), at(m_devs))
            tail = []
        self._args = (*pairs, *map(at, self.inputs), *head, *map(ctypes.byref, self.all_params), self.res.data_ptr(),
                      *[at(_asked(o, w)) for o, w in zip(self.outs, wants)], *tail, self.scratch.data_ptr(), self.scratch.numel())

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

    def raw(self):
        """The result blocks as bytes, one per pair (the copy synchronises with the current stream)."""
        host, size = self.res.cpu().numpy().tobytes(), ctypes.sizeof(self.solver.result)
        return [host[k * size:(k + 1) * size] for k in range(self.n)]

    def structs(self):
        """The result structs, one per pair (one copy, as raw())."""
        return [self.solver.result.from_buffer_copy(b) for b in self.raw()]

    def results(self):
        """[(T 4x4 float64, info dict)] per pair (the copy synchronises with the current stream)."""
        return [(np.array(r.T[:], np.float64).reshape(4, 4), self.solver.info(r)) for r in self.structs()]


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
