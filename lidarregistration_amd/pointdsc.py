"""PointDSC's SC-NonLocal correspondence encoder and confidence head on top of liblidarreg.so: lr_pdsc_encode / lr_pdsc_encode_batch
(csrc/lr_pdsc.hip).  Given the correspondences of a pair it returns a 128-d feature and an inlier logit per correspondence -- the
reference's classifier output (Experiments/models/PointDSC.py:171, :190-191), usable as a learned pre-filter in front of the RANSAC,
SM and TEASER back ends.  Seed picking, the neural spectral matching, the per-seed fits and post_refinement are not built (DESIGN.md
§16).  The contract is stated in include/lidarreg.h and restated in numpy in tests/pdsc_cpu.py.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _ext, devmem
from .devmem import ptr
from .matching import _f32, _stream

C = 128                    # channels (fixed)
IN_DIM, IN_PAD = 6, 8      # input features; rows of the packed first layer (two zero rows)
BN_EPS = 1e-5              # torch.nn.BatchNorm1d's default, which the reference keeps
IGNORED = ("sigma", "sigma_spat")


def layer_plan(num_layers):
    """The blob's blocks in order: (conv key prefix | tuple of prefixes stacked along the outputs, BatchNorm key prefix | None, rows of
    Wt in the blob, outputs)."""
    plan = [("encoder.layer0", None, IN_PAD, C)]
    for i in range(num_layers):
        pcn, nl = f"encoder.blocks.PointCN_layer_{i}", f"encoder.blocks.NonLocal_layer_{i}"
        plan += [(pcn + ".0", pcn + ".1", C, C),
                 (tuple(f"{nl}.projection_{x}" for x in "qkv"), None, C, 3 * C),
                 (nl + ".fc_message.0", nl + ".fc_message.1", C, C // 2),
                 (nl + ".fc_message.3", nl + ".fc_message.4", C // 2, C // 2),
                 (nl + ".fc_message.6", None, C // 2, C)]
    plan += [("classification.0", None, C, 32), ("classification.2", None, 32, 32), ("classification.4", None, 32, 1)]
    return plan


def expected_keys(num_layers):
    keys = []
    for conv, bn, _, _ in layer_plan(num_layers):
        for c in (conv if isinstance(conv, tuple) else (conv,)):
            keys += [c + ".weight", c + ".bias"]
        if bn:
            keys += [bn + s for s in (".weight", ".bias", ".running_mean", ".running_var")]
    return keys


def _np64(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.asarray(v, np.float64)


def check_keys(sd, num_layers):
    """Refuses a missing or an extra key by name; sigma, sigma_spat and the BatchNorms' num_batches_tracked are ignored."""
    want = set(expected_keys(num_layers))
    have = {k for k in sd if k not in IGNORED and not k.endswith("num_batches_tracked")}
    missing, extra = sorted(want - have), sorted(have - want)
    if missing:
        raise KeyError(f"PointDSC state dict for {num_layers} layers: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    if extra:
        raise KeyError(f"PointDSC state dict for {num_layers} layers: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))


def fold(sd, num_layers, dtype=np.float32):
    """[(Wt [rows,out], scale [out], offset [out])] per block of the blob, as `dtype`: the conv's weight transposed (float32 holds it as
    the reference does), BatchNorm folded in fp64 and rounded once (float64: not at all -- what tests/pdsc_cpu.py evaluates)."""
    check_keys(sd, num_layers)
    blocks = []
    for conv, bn, rows, n_out in layer_plan(num_layers):
        convs = conv if isinstance(conv, tuple) else (conv,)
        W = np.concatenate([_np64(sd[c + ".weight"]).reshape(_np64(sd[c + ".weight"]).shape[0], -1) for c in convs], axis=0)      # [out, in]
        b = np.concatenate([_np64(sd[c + ".bias"]).reshape(-1) for c in convs])
        if W.shape[0] != n_out or W.shape[1] > rows or (W.shape[1] != rows and rows != IN_PAD) or b.shape != (n_out,):
            raise ValueError(f"PointDSC state dict: {convs[0]}.weight has shape {W.shape}, expected ({n_out}, {IN_DIM if rows == IN_PAD else rows})")
        Wt = np.zeros((rows, n_out), np.float64)
        Wt[:W.shape[1]] = W.T
        if bn:
            scale = _np64(sd[bn + ".weight"]) / np.sqrt(_np64(sd[bn + ".running_var"]) + BN_EPS)
            offset = (b - _np64(sd[bn + ".running_mean"])) * scale + _np64(sd[bn + ".bias"])
        else:
            scale, offset = np.ones(n_out), b
        blocks.append((Wt.astype(dtype), scale.astype(dtype), offset.astype(dtype)))
    return blocks


def pack(sd, num_layers):
    """The flat float32 blob of lr_pdsc_weights_bytes(num_layers) bytes (the order include/lidarreg.h documents)."""
    return np.concatenate([np.concatenate([Wt.reshape(-1), s, o]) for Wt, s, o in fold(sd, num_layers)]).astype(np.float32)


def unpack(blob, num_layers):
    """pack() undone: the blocks of a blob."""
    blocks, at = [], 0
    for _, _, rows, n_out in layer_plan(num_layers):
        Wt = blob[at:at + rows * n_out].reshape(rows, n_out); at += rows * n_out
        blocks.append((Wt, blob[at:at + n_out], blob[at + n_out:at + 2 * n_out])); at += 2 * n_out
    assert at == len(blob), (at, len(blob))
    return blocks


def packed_floats(num_layers):
    return sum(rows * n_out + 2 * n_out for _, _, rows, n_out in layer_plan(num_layers))


class PointDSCEncoder:
    """The encoder with one set of weights on one device."""

    def __init__(self, blob, num_layers=12, sigma_d=1.2, device=None):
        L = _ext.lib()
        self.num_layers, self.sigma_d = int(num_layers), float(sigma_d)
        self.params = _ext.PdscParams(num_layers=self.num_layers, sigma_d=self.sigma_d)
        blob = np.ascontiguousarray(blob, np.float32).reshape(-1)
        if blob.nbytes != L.lr_pdsc_weights_bytes(self.num_layers):
            raise ValueError(f"weight blob of {blob.nbytes} bytes, lr_pdsc_weights_bytes({self.num_layers}) = {L.lr_pdsc_weights_bytes(self.num_layers)}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.weights = torch.from_numpy(blob).to(self.device)

    @classmethod
    def from_state_dict(cls, sd, num_layers=12, sigma_d=1.2, device=None):
        """sd: the reference's state dict (models.PointDSC.PointDSC().state_dict(), tensors or arrays): encoder.layer0.*,
        encoder.blocks.PointCN_layer_i.{0,1}.*, encoder.blocks.NonLocal_layer_i.{projection_q,projection_k,projection_v,fc_message.*}.*,
        classification.{0,2,4}.*.  sigma, sigma_spat and num_batches_tracked are ignored; any other missing or extra key is refused."""
        return cls(pack(sd, num_layers), num_layers, sigma_d, device)

    def encode_batch(self, srcs, tgts, ms=None, m_devs=None, poison=None, single=False, timed=False, want_feat=None, want_conf=None):
        """lr_pdsc_encode_batch over len(srcs) ragged pairs ([M_k,3] float32 each, any M_k incl. 0).  ms: the counts passed as m (default:
        the rows); m_devs: optional device int32 tensors with a smaller live count (an entry may be None); poison: fill the scratch with
        this byte first (test hook); single: go through lr_pdsc_encode (one pair).  want_feat / want_conf: which outputs the library is
        asked for -- None: all; False: none, the call gets NULL for the whole feat_out / conf_out array; a list of bools: NULL for the
        entries that are False.  The tensor of an output that was not asked for comes back with its -1 fill.  Returns [(features
        [m,128], confidence [m], info dict)] with device tensors -- and, with timed, the device time of the call in ms."""
        L = _ext.lib()
        n = len(srcs)
        srcs = [_f32(s).reshape(-1, 3) for s in srcs]; tgts = [_f32(t).reshape(-1, 3) for t in tgts]
        dev = srcs[0].device
        ms = [int(s.shape[0]) for s in srcs] if ms is None else [int(v) for v in ms]
        scratch = devmem.scratch(L.lr_pdsc_scratch_bytes(max(ms)) * n, dev, poison)
        res = torch.zeros(ctypes.sizeof(_ext.PdscResult) * n, dtype=torch.uint8, device=dev)
        # (the fills are what an entry the library must not write keeps: tests read them)
        feats = [torch.full((max(m, 1), C), -1.0, dtype=torch.float32, device=dev) for m in ms]
        confs = [torch.full((max(m, 1),), -1.0, dtype=torch.float32, device=dev) for m in ms]
        w = (self.weights.data_ptr(), self.weights.numel() * 4, ctypes.byref(self.params), res.data_ptr())
        # the output tensors as the call sees them: None for the whole array, or None per entry
        asked = lambda ts, want: ts if want is None else None if want is False else [t if ok else None for t, ok in zip(ts, want)]
        fo, co = asked(feats, want_feat), asked(confs, want_conf)
        if single:
            assert n == 1
            fn = L.lr_pdsc_encode
            args = (ptr(srcs[0]), ptr(tgts[0]), ms[0], ptr(m_devs and m_devs[0]), *w, ptr(fo and fo[0]), ptr(co and co[0]))
        else:
            arr = lambda ts: None if ts is None else (ctypes.c_void_p * n)(*[ptr(t) for t in ts])
            fn = L.lr_pdsc_encode_batch
            args = (n, arr(srcs), arr(tgts), (ctypes.c_int32 * n)(*ms), arr(m_devs), *w, arr(fo), arr(co))
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        _ext.check(fn(*args, scratch.data_ptr(), scratch.numel(), _stream()))
        ev1.record()
        torch.cuda.current_stream().synchronize()
        host = res.cpu()
        infos = [devmem.read_struct(host, _ext.PdscResult, k) for k in range(n)]
        out = [(feats[k][:m], confs[k][:m], dict(status=r.status, m=r.m, dead=r.dead)) for k, (m, r) in enumerate(zip(ms, infos))]
        self.last_raw = (feats, confs)
        return (out, ev0.elapsed_time(ev1)) if timed else out

    def encode(self, src, tgt, m_dev=None, poison=None, want_feat=None, want_conf=None):
        """lr_pdsc_encode on one correspondence set: (features [m,128], confidence [m]) as device tensors; want_feat / want_conf = False
        passes NULL for that output (its tensor keeps the -1 fill)."""
        f, c, self.last_info = self.encode_batch([src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True,
                                                 want_feat=want_feat, want_conf=want_conf)[0]
        return f, c
