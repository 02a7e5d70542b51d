"""The batched inlier-network entry (contract n4 of include/lidarreg.h) without a GPU: its scratch size function, every refusal that is
decided before the device is touched, how dgr.InlierNet.logits_batch splits a list over several library calls, and the host side of the
weight-sum decision of dgr.DGRTail.register_batch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, dgr
from tests import dgr6_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 131072
THIN, WIDTHS = dgr6_cpu.THIN, dgr6_cpu.WIDTHS


def _w8(w):
    return ctypes.byref((ctypes.c_int32 * 8)(*w))


def test_batch_scratch_bytes_is_closed_outside_the_ranges_and_monotone():
    L = _ext.lib()
    f = lambda p, t, w=THIN: L.lr_dgr_inlier_batch_scratch_bytes(p, t, _w8(w))
    for npairs in (-1, 0, 9, 1000):
        assert f(npairs, 100) == 0, npairs
    for total in (-1, MAX_N + 1, 1 << 30):
        assert f(1, total) == 0 and f(8, total) == 0, total
    for bad in ((32, 64, 128, 256, 128, 64, 64, 0), (16,) * 8, (48,) * 8, (288,) * 8):
        assert f(2, 100, bad) == 0, bad
    assert L.lr_dgr_inlier_batch_scratch_bytes(2, 100, None) == 0
    assert f(1, 0) > 0 and f(8, 0) > 0 and f(1, MAX_N) > 0 and f(8, MAX_N) > 0
    totals = [0, 1, 63, 64, 65, 100, 2047, 2048, 2049, 4097, 30000, 1 << 16, MAX_N - 1, MAX_N]
    for w in (THIN, WIDTHS):
        for npairs in (1, 2, 7, 8):
            sizes = [f(npairs, t, w) for t in totals]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (npairs, sizes)                  # monotone in the rows ...
            assert all(s % 256 == 0 for s in sizes)
        for t in totals:
            sizes = [f(b, t, w) for b in range(1, 9)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (t, sizes)                      # ... and in the pairs
            assert f(1, t, w) >= L.lr_dgr_inlier_scratch_bytes(t, _w8(w)) > 0, t                   # one pair: at least the single entry's


def _arr(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_batch_refusals_before_any_launch_name_the_argument_and_the_pair():
    """P4 without a device: every pointer below is a made-up address that a refused call never reads."""
    L = _ext.lib()
    need_w = L.lr_dgr_inlier_weights_bytes(_w8(THIN))
    ns = [100, 0, 50]
    need_s = L.lr_dgr_inlier_batch_scratch_bytes(3, sum(ns), _w8(THIN))
    P = lambda **kw: _ext.DgrInlierParams(**{"widths": THIN, **kw})
    ok = dict(B=3, coords=_arr([0x10000, None, 0x11000]), n=_ints(ns), w=0x20000, wb=need_w, p=P(), res=0x30000, out=_arr([0x40000, None, 0x41000]),
              s=None, sb=need_s)

    def call(**kw):
        a = {**ok, **kw}
        rc = L.lr_dgr_inlier_batch(a["B"], a["coords"], a["n"], a["w"], a["wb"], ctypes.byref(a["p"]) if a["p"] is not None else None, a["res"], a["out"],
                                   a["s"], a["sb"], None)
        return rc, L.lr_last_error().decode()
    p = P(); p.struct_size = 8
    many = 9
    cases = [(dict(p=p), "struct_size"), (dict(p=None), "null params"), (dict(p=P(widths=(32, 32, 32, 32, 32, 32, 32, 48))), "width"),
             (dict(p=P(tap=1)), "tap must be 0"), (dict(p=P(tap=23)), "tap must be 0"), (dict(p=P(tap=-1)), "tap must be 0"),
             (dict(B=0), "npairs"), (dict(B=-3), "npairs"),
             (dict(B=many, coords=_arr([0x10000] * many), n=_ints([1] * many), out=_arr([0x40000] * many)), "npairs"),
             (dict(coords=None), "null coords"), (dict(n=None), "null n"), (dict(out=None), "null logit_out"),
             (dict(n=_ints([100, -1, 50])), "n[1]"), (dict(n=_ints([100, 0, MAX_N + 1])), "n[2]"),
             (dict(n=_ints([MAX_N, 0, 1])), "sum of n"), (dict(n=_ints([MAX_N // 2, 0, MAX_N // 2 + 1])), "sum of n"),
             (dict(coords=_arr([0x10000, None, None])), "null coords[2]"), (dict(coords=_arr([None, None, 0x11000])), "null coords[0]"),
             (dict(out=_arr([0x40000, None, None])), "null logit_out[2]"), (dict(n=_ints([100, 7, 50])), "null coords[1]"),
             (dict(res=None), "null results"),
             (dict(w=None), "null weights"), (dict(w=0x20008), "16-byte aligned"), (dict(wb=need_w - 4), "weights_bytes"),
             (dict(p=P(widths=WIDTHS)), "weights_bytes"),
             (dict(), "null scratch"), (dict(s=0x50000, sb=need_s - 1), "scratch too small"), (dict(s=0x50010), "256-byte aligned")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("lr_dgr_inlier_batch"), (kw, rc, msg)
    assert sum([MAX_N // 2, 0, MAX_N // 2 + 1]) == 131073
    # an empty pair needs neither pointer; the sum at its limit passes the size checks (and is then stopped at the scratch)
    rc, msg = call(n=_ints([MAX_N - 50, 0, 50]))
    assert rc == -1 and "null scratch" in msg
    assert L.lr_version() == 103                                                                           # new entry points only
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    assert all(re.search(r"LR_API\s+\w+\s+" + s + r"\(", hdr) for s in ("lr_dgr_inlier_batch_scratch_bytes", "lr_dgr_inlier_batch"))
    assert {"lr_dgr_inlier_batch_scratch_bytes", "lr_dgr_inlier_batch"} <= set(_ext.SYMBOLS)


class _Recorder(dgr.InlierNet):
    """logits_batch with the library call replaced: records what every call is given."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.widths = THIN
        self.last_info = None
        self.calls = []

    def _call_batch(self, coords, poison=None):
        ns = [int(c.shape[0]) for c in coords]
        self.calls.append(ns)
        res = np.zeros((len(ns), 4), np.int32)
        res[:, 1] = ns; res[:, 2] = ns
        # pair k of a call carries (which call, k inside the call): the outputs must come back in the caller's order
        outs = [torch.full((n,), float(len(self.calls) * 1000 + k)) for k, n in enumerate(ns)]
        return outs, torch.from_numpy(res.view(np.uint8).reshape(-1))


def _cells(n):
    return torch.zeros((n, 6), dtype=torch.int32)


H = MAX_N // 2


@pytest.mark.parametrize("sizes,want", [
    ([1] * 8, [8]),
    ([1] * 9, [8, 1]),
    ([H, H], [2]),                                                       # exactly 131 072 rows: one call
    ([H, H, 1], [2, 1]),
    ([H, H + 1, 5], [1, 2]),                                             # one row too many: the second pair opens a call
    ([MAX_N, 0, 1, MAX_N], [2, 1, 1]),                                   # an empty pair costs no rows
    ([3, 0, 0], [3]),
    ([], []),
], ids=lambda v: "-".join(str(x) for x in v)[:40] or "none")
def test_logits_batch_splits_at_8_pairs_and_at_131072_rows(sizes, want):
    m = _Recorder()
    outs = m.logits_batch([_cells(n) for n in sizes])
    assert [len(ns) for ns in m.calls] == want
    assert [n for ns in m.calls for n in ns] == sizes                     # every pair once, in order
    assert all(len(ns) <= 8 and sum(ns) <= MAX_N for ns in m.calls)
    assert [tuple(o.shape) for o in outs] == [(n,) for n in sizes]
    tags = [float((c + 1) * 1000 + k) for c, cnt in enumerate(want) for k in range(cnt)]
    assert [float(o[0]) for o in outs if o.shape[0]] == [t for t, n in zip(tags, sizes) if n]
    assert m.last_info == [dict(status=0, n=n, n_tap=n) for n in sizes]


def test_logits_batch_refuses_a_pair_above_the_row_limit_by_its_index():
    m = _Recorder()
    with pytest.raises(ValueError, match=r"coords6_list\[0\]"):
        m.logits_batch([_cells(MAX_N + 1)])
    with pytest.raises(ValueError, match=r"coords6_list\[2\]"):
        m.logits_batch([_cells(3), _cells(0), _cells(MAX_N + 1)])
    assert m.calls == []


@pytest.mark.parametrize("M", [3999, 4000, 4001, 30000])
def test_the_host_threshold_rule_on_recorded_result_blocks(M):
    """G9 on the host: w1 < max(4000, M) clip is the safeguard (status 2), w1 at the threshold refines -- the comparison of two doubles
    the device makes when the threshold is handed to it."""
    clip = 0.05
    tail = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=clip)
    thr = max(4000, M) * clip
    assert tail.wsum_threshold(M) == thr and (thr == 200.0) == (M <= 4000)
    block = lambda w1, L=100, status=0: dict(status=status, iterations=37, break_count=20, loss=0.25, L=L, w1=w1)
    assert tail.status_of(block(np.nextafter(thr, 0.0)), M) == 2            # one ulp below
    assert tail.status_of(block(thr), M) == 0                               # at the threshold
    assert tail.status_of(block(np.nextafter(thr, np.inf)), M) == 0
    assert tail.status_of(block(thr, status=3), M) == 3                     # a refinement's own status is kept
    assert tail.status_of(block(0.0, L=0), M) == 1                          # no live row wins
    assert tail.status_of(block(thr, L=0), M) == 1
