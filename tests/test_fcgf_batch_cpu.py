"""The batched FCGF entry (contract n2 of include/lidarreg.h) without a GPU: its scratch size function, every refusal that is decided before
the device is touched, and how fcgf.FCGF.features_batch splits a list over several library calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, fcgf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 1 << 20


def test_batch_scratch_bytes_is_closed_outside_the_ranges_and_monotone():
    L = _ext.lib()
    f = L.lr_fcgf_batch_scratch_bytes
    for nclouds in (-1, 0, 65, 1000):
        assert f(nclouds, 100) == 0, nclouds
    for total in (-1, MAX_N + 1, 1 << 30):
        assert f(1, total) == 0 and f(64, total) == 0, total
    assert f(1, 0) > 0 and f(64, 0) > 0 and f(1, MAX_N) > 0 and f(64, MAX_N) > 0
    totals = [0, 1, 63, 64, 65, 100, 2047, 2048, 2049, 4097, 30000, 1 << 16, MAX_N - 1, MAX_N]
    for nclouds in (1, 2, 63, 64):
        sizes = [f(nclouds, t) for t in totals]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (nclouds, sizes)                    # monotone in the rows ...
        assert all(s % 256 == 0 for s in sizes)
    for t in totals:
        sizes = [f(b, t) for b in range(1, 65)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (t, sizes[:4])                      # ... and in the clouds
        assert f(1, t) >= L.lr_fcgf_scratch_bytes(t) > 0, t                                        # one cloud: at least the single entry's


def _arr(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_batch_refusals_before_any_launch_name_the_argument_and_the_cloud():
    """B4 without a device: every pointer below is a made-up address that a refused call never reads."""
    L = _ext.lib()
    need_w = L.lr_fcgf_weights_bytes(5)
    ns = [100, 0, 50]
    need_s = L.lr_fcgf_batch_scratch_bytes(3, sum(ns))
    ok = dict(B=3, coords=_arr([0x10000, None, 0x11000]), feat_in=None, n=_ints(ns), w=0x20000, wb=need_w, p=_ext.FcgfParams(), res=0x30000,
              out=_arr([0x40000, None, 0x41000]), s=None, sb=need_s)

    def call(**kw):
        a = {**ok, **kw}
        rc = L.lr_fcgf_extract_batch(a["B"], a["coords"], a["feat_in"], a["n"], a["w"], a["wb"], ctypes.byref(a["p"]) if a["p"] is not None else None,
                                     a["res"], a["out"], a["s"], a["sb"], None)
        return rc, L.lr_last_error().decode()
    p = _ext.FcgfParams(); p.struct_size = 8
    many = 65
    cases = [(dict(p=p), "struct_size"), (dict(p=None), "null params"), (dict(p=_ext.FcgfParams(conv1_kernel_size=4)), "conv1_kernel_size"),
             (dict(p=_ext.FcgfParams(tap=1)), "tap must be 0"), (dict(p=_ext.FcgfParams(tap=23)), "tap must be 0"), (dict(p=_ext.FcgfParams(tap=-1)), "tap must be 0"),
             (dict(B=0), "nclouds"), (dict(B=-3), "nclouds"),
             (dict(B=many, coords=_arr([0x10000] * many), n=_ints([1] * many), out=_arr([0x40000] * many)), "nclouds"),
             (dict(coords=None), "null coords"), (dict(n=None), "null n"), (dict(out=None), "null feat_out"),
             (dict(n=_ints([100, -1, 50])), "n[1]"), (dict(n=_ints([100, 0, MAX_N + 1])), "n[2]"),
             (dict(n=_ints([MAX_N, 0, 1])), "sum of n"), (dict(n=_ints([MAX_N // 2, 0, MAX_N // 2 + 1])), "sum of n"),
             (dict(coords=_arr([0x10000, None, None])), "null coords[2]"), (dict(coords=_arr([None, None, 0x11000])), "null coords[0]"),
             (dict(out=_arr([0x40000, None, None])), "null feat_out[2]"), (dict(n=_ints([100, 7, 50])), "null coords[1]"),
             (dict(res=None), "null results"),
             (dict(w=None), "null weights"), (dict(w=0x20008), "16-byte aligned"), (dict(wb=need_w - 4), "weights_bytes"),
             (dict(p=_ext.FcgfParams(conv1_kernel_size=5), wb=L.lr_fcgf_weights_bytes(3)), "weights_bytes"),
             (dict(), "null scratch"), (dict(s=0x50000, sb=need_s - 1), "scratch too small"), (dict(s=0x50010), "256-byte aligned")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("lr_fcgf_extract_batch"), (kw, rc, msg)
    # an empty cloud needs neither pointer; the sum at its limit passes the size checks (and is then stopped at the scratch)
    rc, msg = call(n=_ints([MAX_N - 50, 0, 50]))
    assert rc == -1 and "null scratch" in msg
    assert L.lr_version() == 103                                                                           # new entry points only
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    assert all(re.search(r"LR_API\s+\w+\s+" + s + r"\(", hdr) for s in ("lr_fcgf_batch_scratch_bytes", "lr_fcgf_extract_batch"))


class _Recorder(fcgf.FCGF):
    """features_batch with the library call replaced: records what every call is given."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.conv1_kernel_size = 5
        self.last_info = None
        self.calls = []

    def _call_batch(self, coords, feat_in, poison=None):
        ns = [int(c.shape[0]) for c in coords]
        self.calls.append((ns, [None if f is None else int(f.shape[0]) for f in feat_in]))
        res = np.zeros((len(ns), 4), np.int32)
        res[:, 1] = ns; res[:, 2] = ns
        # row k of cloud b carries (which call, b inside the call, k): the outputs must come back in the caller's order
        outs = [torch.full((n, 32), float(len(self.calls) * 1000 + b)) for b, n in enumerate(ns)]
        return outs, torch.from_numpy(res.view(np.uint8).reshape(-1))


def _cells(n):
    return torch.zeros((n, 3), dtype=torch.int32)


@pytest.mark.parametrize("sizes,want", [
    ([1] * 64, [64]),
    ([1] * 65, [64, 1]),
    ([1] * 129, [64, 64, 1]),
    ([MAX_N // 2, MAX_N // 2], [2]),                                     # exactly 2^20 rows: one call
    ([MAX_N // 2, MAX_N // 2, 1], [2, 1]),
    ([MAX_N // 2, MAX_N // 2 + 1, 5], [1, 2]),                           # one row too many: the second cloud opens a call
    ([MAX_N, 0, 1, MAX_N], [2, 1, 1]),                                   # an empty cloud costs no rows
    ([3, 0, 0], [3]),
    ([], []),
], ids=lambda v: "-".join(str(x) for x in v)[:40] or "none")
def test_features_batch_splits_at_64_clouds_and_at_2_20_rows(sizes, want):
    m = _Recorder()
    outs = m.features_batch([_cells(n) for n in sizes])
    assert [len(ns) for ns, _ in m.calls] == want
    assert [n for ns, _ in m.calls for n in ns] == sizes                  # every cloud once, in order
    assert all(len(ns) <= 64 and sum(ns) <= MAX_N for ns, _ in m.calls)
    assert [tuple(o.shape) for o in outs] == [(n, 32) for n in sizes]
    tags = [float((c + 1) * 1000 + b) for c, k in enumerate(want) for b in range(k)]
    assert [float(o[0, 0]) for o in outs if o.shape[0]] == [t for t, n in zip(tags, sizes) if n]
    assert m.last_info == [dict(status=0, n=n, n_tap=n) for n in sizes]


def test_features_batch_carries_feat_in_per_cloud_and_checks_its_length():
    m = _Recorder()
    m.features_batch([_cells(4), _cells(2), _cells(3)], [None, np.ones(2, np.float32), [1.0, 2.0, 3.0]])
    assert m.calls == [([4, 2, 3], [None, 2, 3])]
    with pytest.raises(ValueError, match=r"feat_in_list\[1\]"):
        m.features_batch([_cells(4), _cells(2)], [None, np.ones(3, np.float32)])
    with pytest.raises(ValueError, match="entries"):
        m.features_batch([_cells(4), _cells(2)], [None])
