"""PointDSC on top of liblidarreg.so.  The encoder: lr_pdsc_encode / lr_pdsc_encode_batch (csrc/lr_pdsc.hip) return a 128-d feature and
an inlier logit per correspondence -- the reference's classifier output (Experiments/models/PointDSC.py:171, :190-191), usable as a
learned pre-filter in front of the RANSAC, SM and TEASER back ends.  The tail: lr_pdsc_solve / lr_pdsc_register
(csrc/lr_pdsc_solve.hip) pick the seeds, run the per-seed neural spectral matching and fits, select the best hypothesis and refine it
(DESIGN.md §17): ``solve``, ``PointDSCModel`` and ``eval_pairs``, the engine of ``python -m test --algo PointDSC``.  The contracts are
stated in include/lidarreg.h and restated in numpy in tests/pdsc_cpu.py and tests/pdsc_solve_cpu.py.  There is no CPU fallback.
"""
import json
import os

import numpy as np
import torch

from . import _ext, corrset, devmem

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
        call = corrset.BatchCall(ENCODE, srcs, tgts, ms, m_devs, poison, single, params=(self.params,), **self._blob(), want_feat=want_feat, want_conf=want_conf)
        t = call.timed()
        feats, confs = self.last_raw = tuple(call.outs)
        out = [(feats[k][:m], confs[k][:m], dict(status=r.status, m=r.m, dead=r.dead)) for k, (m, r) in enumerate(zip(call.ms, call.structs()))]
        return (out, t) if timed else out

    def _blob(self):
        return dict(blob=self.weights.data_ptr(), blob_bytes=self.weights.numel() * 4)

    def encode(self, src, tgt, m_dev=None, poison=None, want_feat=None, want_conf=None):
        """lr_pdsc_encode on one correspondence set: (features [m,128], confidence [m]) as device tensors; want_feat / want_conf = False
        passes NULL for that output (its tensor keeps the -1 fill)."""
        f, c, self.last_info = self.encode_batch([src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True,
                                                 want_feat=want_feat, want_conf=want_conf)[0]
        return f, c


# ---- the tail: seeds, neural spectral matching, fits, selection, refinement (lr_pdsc_solve, lr_pdsc_register) ----------------------
def solve_params(**kw):
    """lr_pdsc_solve_params: the reference's Lidar settings unless overridden."""
    return _ext.PdscSolveParams(**kw)


def _solve_info(r):
    d = devmem.as_dict(r)
    d.pop("reserved"); d.pop("T")
    return d


_cap = lambda m, p: int(m * p.ratio)        # rows of seeds_out and of the trace arrays
_FEAT, _CONF = corrset.Out("feat", torch.float32, -1.0, C), corrset.Out("conf", torch.float32, -1.0)
_LABELS, _SEEDS = corrset.Out("labels", torch.uint8, 255), corrset.Out("seeds", torch.int32, -7, rows=_cap)
_BLOB = ("blob", "blob_bytes")              # the weight blob's device address and its byte count
# the three entry-point families as corrset.BatchCall sees them, inputs and outputs in the ABI's order
ENCODE = corrset.Solver("lr_pdsc_encode", "lr_pdsc_encode_batch", "lr_pdsc_scratch_bytes", (_ext.PdscParams,), _ext.PdscResult, (_FEAT, _CONF),
                        call_args=_BLOB)
SOLVE = corrset.Solver("lr_pdsc_solve", "lr_pdsc_solve_batch", "lr_pdsc_solve_scratch_bytes", (solve_params,), _ext.PdscSolveResult, (_LABELS, _SEEDS),
                       inputs=(corrset.In("feat", torch.float32, (-1, C)), corrset.In("conf", torch.float32, (-1,))),
                       extras=(corrset.Out("knn", torch.int32, -7, "k", _cap), corrset.Out("weights", torch.float32, -7.0, "k", _cap),
                               corrset.Out("seed_T", torch.float64, -7.0, 16, _cap), corrset.Out("counts", torch.int32, -7, None, _cap)),
                       extras_flag="trace", extras_msg="the trace outputs belong to the single call")
REGISTER = corrset.Solver("lr_pdsc_register", "lr_pdsc_register_batch", "lr_pdsc_register_scratch_bytes", (_ext.PdscParams, solve_params),
                          _ext.PdscSolveResult, (_FEAT, _CONF, _LABELS, _SEEDS), call_args=_BLOB)


def _decode(call, labels, seeds):
    """[(T, labels [m], info)] of a solve / register call; info["seeds"] are the seeds that were written."""
    out = []
    for k, (m, r) in enumerate(zip(call.ms, call.structs())):
        info = _solve_info(r)
        info["seeds"] = seeds[k][:max(info["n_seeds"], 0)]
        out.append((np.array(r.T, np.float64).reshape(4, 4), labels[k][:m], info))
    return out


def solve_batch(srcs, tgts, feats, confs, ms=None, m_devs=None, poison=None, single=False, timed=False, trace=False, want_labels=None,
                want_seeds=None, **params):
    """lr_pdsc_solve_batch over len(srcs) ragged pairs: src / tgt [M_k,3], feat [M_k,128], conf [M_k] float32 (what the encoder returned).
    ms, m_devs, poison, single as PointDSCEncoder.encode_batch; want_labels / want_seeds as its want_feat.  trace (single only): info
    also carries 'knn' int32 [n_seeds,k], 'weights' float32 [n_seeds,k], 'seed_T' float64 [n_seeds,4,4] and 'counts' int32 [n_seeds].
    Returns [(T 4x4 float64 array, labels uint8 device tensor [m], info dict)] -- and, with timed, the device time of the call in ms."""
    call = corrset.BatchCall(SOLVE, srcs, tgts, ms, m_devs, poison, single, feat=feats, conf=confs, trace=trace, want_labels=want_labels,
                             want_seeds=want_seeds, **params)
    t = call.timed()
    solve_batch.last_raw = tuple(call.outs)
    out = _decode(call, *call.outs)
    if trace:
        ns, tr = out[0][2]["n_seeds"], tuple(call.extras)
        out[0][2].update(knn=tr[0][:ns], weights=tr[1][:ns], seed_T=tr[2][:ns].reshape(-1, 4, 4), counts=tr[3][:ns], raw_trace=tr)
    return (out, t) if timed else out


def solve(src, tgt, feat, conf, m_dev=None, poison=None, trace=False, want_labels=None, want_seeds=None, **params):
    """lr_pdsc_solve on one pair: (T 4x4 float64 array, labels uint8 device tensor [m], info dict)."""
    return solve_batch([src], [tgt], [feat], [conf], None, None if m_dev is None else [m_dev], poison, single=True, trace=trace,
                       want_labels=want_labels, want_seeds=want_seeds, **params)[0]


class PointDSCModel:
    """The whole network in inference mode: an encoder with its weights and the tail's parameters; sigma comes from the state dict."""

    def __init__(self, encoder, **solve_kw):
        self.encoder = encoder
        self.solve_kw = dict(sigma_d=encoder.sigma_d, **solve_kw)
        solve_params(**self.solve_kw)        # (an unknown keyword fails here)

    @classmethod
    def from_state_dict(cls, sd, num_layers=12, sigma_d=1.2, device=None, **solve_kw):
        """sd: the reference's state dict (PointDSCEncoder.from_state_dict); its learned `sigma` (PointDSC.py:97) is S5's sigma unless
        solve_kw names one."""
        if "sigma" in sd and "sigma" not in solve_kw:
            solve_kw["sigma"] = float(_np64(sd["sigma"]).reshape(-1)[0])
        return cls(PointDSCEncoder.from_state_dict(sd, num_layers, sigma_d, device), **solve_kw)

    def register_batch(self, srcs, tgts, ms=None, m_devs=None, poison=None, single=False, timed=False, want_feat=None, want_conf=None):
        """lr_pdsc_register_batch (single: lr_pdsc_register): [(T 4x4 float64 array, labels uint8 device tensor [m], info dict)]; info
        carries 'feat' and 'conf' (device tensors; the -1 fill where want_feat / want_conf did not ask for them)."""
        call = corrset.BatchCall(REGISTER, srcs, tgts, ms, m_devs, poison, single, params=(self.encoder.params, solve_params(**self.solve_kw)),
                                 **self.encoder._blob(), want_feat=want_feat, want_conf=want_conf)
        t = call.timed()
        feats, confs, labels, seeds = call.outs
        out = _decode(call, labels, seeds)
        for k, m in enumerate(call.ms):
            out[k][2].update(feat=feats[k][:m], conf=confs[k][:m])
        return (out, t) if timed else out

    def register(self, src, tgt, m_dev=None, poison=None):
        return self.register_batch([src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True)[0]

    def forward(self, data):
        """The reference's call shape in testing mode (PointDSC.py:121-197): data['src_keypts'], data['tgt_keypts'] [1,M,3] ->
        {'final_trans' [1,4,4], 'final_labels' [1,M]} float32 tensors on the inputs' device (data['corr_pos'] is their centred
        concatenation, which the encoder forms itself)."""
        src, tgt = torch.as_tensor(data["src_keypts"]), torch.as_tensor(data["tgt_keypts"])
        assert src.shape[0] == 1, "bs = 1, as the reference's pick_seeds and post_refinement"
        T, labels, _ = self.register(src.reshape(-1, 3), tgt.reshape(-1, 3))
        return {"final_trans": torch.from_numpy(T).to(dtype=torch.float32, device=labels.device)[None], "final_labels": labels.to(torch.float32)[None]}

    __call__ = forward


# ---- the CLI's engine: python -m test --algo PointDSC --chosen_snapshot DIR ------------------------------------------------------------
NUM_NODE = 12000          # Experiments/test.py:247
LIDAR_THRESHOLD, LIDAR_SIGMA_D = 0.6, 1.2      # what test.py:338-339 overrides the snapshot's config with


def load_snapshot(dirpath, device=None):
    """The reference's snapshot layout (test.py:333, :392): DIR/config.json and DIR/models/model_best.pkl (a torch.save of the state dict).
    inlier_threshold and sigma_d are overridden as test.py:338-339 does; nms_radius is the inlier threshold (:389); sigma_d is rounded to
    float32, as the reference's sigma_spat parameter holds it."""
    with open(os.path.join(dirpath, "config.json")) as fid:
        cfg = json.load(fid)
    if int(cfg.get("in_dim", 6)) != IN_DIM or int(cfg.get("num_channels", C)) != C:
        raise ValueError(f"PointDSC snapshot {dirpath}: in_dim {cfg.get('in_dim')} / num_channels {cfg.get('num_channels')}; this build is {IN_DIM} / {C}")
    sd = torch.load(os.path.join(dirpath, "models", "model_best.pkl"), map_location="cpu")
    return PointDSCModel.from_state_dict(sd, num_layers=int(cfg["num_layers"]), sigma_d=float(np.float32(LIDAR_SIGMA_D)), device=device,
                                         num_iterations=int(cfg.get("num_iterations", 10)), ratio=float(cfg.get("ratio", 0.1)), k=int(cfg.get("k", 40)),
                                         nms_radius=LIDAR_THRESHOLD, inlier_threshold=LIDAR_THRESHOLD)


def select_source(n0, num_node, seed):
    """The at most num_node source points of a pair (LidarFeatureExtractor.py:99-100): every point, or the first num_node of a
    permutation seeded by (seed, n0) -- None when every point is taken."""
    return None if n0 <= num_node else np.sort(np.random.default_rng([int(seed), int(n0)]).permutation(n0)[:num_node])


def correspondences_dev(xyz0, xyz1, F0, F1, args, ws, stream):
    """The reference's extractor with use_mutual False (LidarFeatureExtractor.py:94-117): every selected source point with its nearest
    target descriptor, through lr_nn_top2; no filter.  The target is not subsampled (deviation: the reference also draws num_node of its
    points).  Returns (idx0, idx1 device int32, count device int32 [1]); nothing is synchronised."""
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    sel = select_source(n0, int(getattr(args, "num_node", NUM_NODE)), int(getattr(args, "seed", 51)))
    if sel is None:
        idx0 = torch.arange(n0, dtype=torch.int32, device=dev)
    else:
        idx0 = torch.from_numpy(sel.astype(np.int32)).to(dev)
        F0 = F0[idx0.long()].contiguous()
    m = idx0.shape[0]
    idx1 = torch.empty(m, dtype=torch.int32, device=dev)
    _ext.check(_ext.lib().lr_nn_top2(ws.handle, F0.data_ptr(), m, F1.data_ptr(), n1, d, idx1.data_ptr(), None, None, None, stream))
    return idx0, idx1, torch.full((1,), m, dtype=torch.int32, device=dev)


def eval_pairs(source, indices, args, device=None, batch=32, nstreams=3, verbose=False):
    """--algo PointDSC over `indices` of `source` (corrset.eval_pairs): ONE lr_pdsc_register_batch per window.  Returns a harness.EvalRun.
    Column 9 = the pair's share of its window's register call (its device time split evenly), as for --algo SM."""
    if str(getattr(args, "solver", "SVD")).upper() == "RANSAC":
        raise ValueError("--solver RANSAC is not built: --algo PointDSC fits by SVD (--solver SVD)")
    snap = getattr(args, "chosen_snapshot", None)
    if not snap:
        raise ValueError("--algo PointDSC needs --chosen_snapshot DIR (DIR/config.json, DIR/models/model_best.pkl)")
    model = load_snapshot(snap, device)
    batch = min(int(batch), 64)                      # (LR_MAX_BATCH)

    def solve(srcs, tgts):
        out, ms = model.register_batch(srcs, tgts, timed=True, want_feat=False, want_conf=False)
        return [(T, info, labels) for T, labels, info in out], ms
    return corrset.eval_pairs(source, indices, args, correspondences_dev, solve, device=device, batch=batch, nstreams=nstreams, verbose=verbose)
