"""Deep Global Registration's robust pose refinement on top of liblidarreg.so: lr_dgr_refine / lr_dgr_refine_batch (csrc/lr_dgr.hip).

``GlobalRegistration`` keeps the reference's call shape (DGR/core/registration.py:135-194); ``refine`` / ``refine_batch`` are the device
calls; ``DGRTail`` is what DeepGlobalRegistration.register does once it has the inlier weights (DGR/core/deep_global_registration.py:
403-459): the weight-sum decision, the refinement or the safeguard RANSAC, then ICP.  The contract the refinement implements is stated in
include/lidarreg.h (d1) and DESIGN.md §19.

``InlierNet`` is the 6-D inlier network that gives the weights (lr_dgr_inlier, csrc/lr_dgr6.hip; contract n3, DESIGN.md §20, restated in
numpy in tests/dgr6_cpu.py) and ``DGR`` the whole DeepGlobalRegistration.register (:352-459): voxel de-duplication, FCGF features, the
feature nearest neighbour, the inlier network, the tail.  Their batched forms -- ``InlierNet.logits_batch`` / ``weights_batch``
(lr_dgr_inlier_batch, csrc/lr_dgr6_batch.h; contract n4, DESIGN.md §20.7: up to 8 pairs and 131 072 rows per call), ``DGRTail.register_batch``
and ``DGR.register_batch`` -- give every pair the bytes of its one-pair call, and ``eval_pairs`` is the engine of ``python -m test --algo
DGR --dgr_weights FILE``.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _ext, corrset, devmem, resunet
from .devmem import ptr
from .matching import _f32, _stream

RESULT_BYTES = ctypes.sizeof(_ext.DgrResult)
MAX_REFINE_BATCH = 64                                 # LR_MAX_BATCH: pairs per lr_dgr_refine_batch
STATUS = {0: "refined", 1: "no live correspondence", 2: "weight sum below the threshold", 3: "non-finite loss or parameter"}


def params(**kw):
    """lr_dgr_params: GlobalRegistration's defaults unless overridden (max_iter, max_break, quantization_size, lr, gamma, ratio, clip,
    wsum_threshold)."""
    return _ext.DgrParams(**kw)


def _info(r):
    return dict(status=r.status, iterations=r.iterations, break_count=r.break_count, loss=r.loss, L=r.L, w1=r.w1)


# the refinement as corrset.BatchCall sees it: after the pairs come the weights and the initial transforms (keywords weights, T_inits:
# per pair None or float32 [M_k] / a 4x4); the single-pair entry point alone keeps the per-iteration log (keyword log)
SOLVER = corrset.Solver("lr_dgr_refine", "lr_dgr_refine_batch", "lr_dgr_scratch_bytes", (params,), _ext.DgrResult, (), _info,
                        inputs=(corrset.In("weights", torch.float32, (-1,)), corrset.In("T_inits", torch.float64, (16,))),
                        extras=(corrset.Out("log", torch.float64, np.nan, 10, lambda m, p: p.max_iter),), extras_flag="log",
                        extras_msg="the log belongs to the single-pair entry point")


def refine_batch(srcs, tgts, weights=None, T_inits=None, ms=None, m_devs=None, poison=None, **kw):
    """lr_dgr_refine_batch: [(T 4x4, info dict)] per pair and the device time of the call in ms."""
    call = corrset.BatchCall(SOLVER, srcs, tgts, ms, m_devs, poison, weights=weights, T_inits=T_inits, **kw)
    ms_ = call.timed()
    return call.results(), ms_


def refine(src, tgt, weights=None, T_init=None, m_dev=None, log=False, poison=None, **kw):
    """lr_dgr_refine on one weighted correspondence set: (T 4x4 float64, info dict); with log, info["log"] is the [max_iter,10] float64 log
    (row i: the nine parameters iteration i was evaluated at, its loss)."""
    call = corrset.BatchCall(SOLVER, [src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True, log=log,
                             weights=None if weights is None else [weights], T_inits=None if T_init is None else [T_init], **kw)
    call.launch(_stream())
    T, info = call.results()[0]
    if log:
        info["log"] = call.extras[0].cpu().numpy()
    return T, info


def GlobalRegistration(points, trans_points, weights=None, max_iter=1000, verbose=False, stat_freq=20, max_break_count=20,
                       break_threshold_ratio=1e-5, loss_fn=None, quantization_size=1):
    """DGR/core/registration.py:135-194: (R [3,3], t [1,3] float64 CPU tensors, {'iterations', 'loss', 'break_count'}).  weights None: every
    weight is 1 (the reference's unweighted mean).  A custom loss_fn is not supported: the loss is HighDimSmoothL1Loss."""
    if loss_fn is not None:
        raise NotImplementedError("GlobalRegistration on the HIP path runs HighDimSmoothL1Loss only")
    T, info = refine(points, trans_points, weights, max_iter=int(max_iter), max_break=int(max_break_count), ratio=float(break_threshold_ratio),
                     quantization_size=float(quantization_size))
    if info["status"] != 0:
        raise _ext.LidarRegError(f"GlobalRegistration: {STATUS[info['status']]}")
    if verbose:
        print(info["iterations"], info["loss"])
    return (torch.from_numpy(T[:3, :3].copy()), torch.from_numpy(T[:3, 3].copy()).reshape(1, 3),
            {"iterations": info["iterations"], "loss": info["loss"], "break_count": info["break_count"]})


class DGRTail:
    """DeepGlobalRegistration.register from its weights on (deep_global_registration.py:394-459).  weights_fn(xyz0, xyz1, idx0, idx1) ->
    weights [M] is the hook the inlier network plugs into (functools.partial(InlierNet.weights, voxel_size=v)); it is asked only when
    register() is given no weights."""

    def __init__(self, voxel_size=0.3, clip_weight_thresh=0.05, use_icp=True, weights_fn=None, seed=51):
        self.voxel_size, self.clip_weight_thresh, self.use_icp, self.weights_fn, self.seed = float(voxel_size), float(clip_weight_thresh), bool(use_icp), weights_fn, seed
        self.last = None             # info of the last register(): the refinement's result block and which path ran

    def register(self, xyz0, xyz1, idx0, idx1, weights=None, m_threshold=None):
        """-> {'base': T, 'w_icp': T_icp}.  m_threshold: the correspondence count M the weight-sum threshold is taken from when it is not
        the number of rows given (DGR.register, which drops clipped rows of a set above the refinement's limit); None = the rows given.  'base': the refinement (ratio 1e-4, quantization 2 * voxel, :415-421) when the clipped weights
        sum to at least max(4000, M) * clip_weight_thresh (:407), else the safeguard: 4-point RANSAC with the edge-length checker over
        the given correspondences, 80 000 iterations, threshold 2 * voxel, confidence 0.9999 (:60-76, :437-444)."""
        from .ransac import icp_dev, ransac_dev
        if weights is None:
            if self.weights_fn is None:
                raise ValueError("DGRTail.register needs weights or a weights_fn")
            weights = self.weights_fn(xyz0, xyz1, idx0, idx1)
        x0, x1 = _f32(xyz0).reshape(-1, 3), _f32(xyz1).reshape(-1, 3)
        i0 = torch.as_tensor(np.asarray(idx0) if not torch.is_tensor(idx0) else idx0).to(x0.device).long().reshape(-1)
        i1 = torch.as_tensor(np.asarray(idx1) if not torch.is_tensor(idx1) else idx1).to(x0.device).long().reshape(-1)
        src, tgt = x0[i0].contiguous(), x1[i1].contiguous()
        m = int(src.shape[0])
        thr = 2 * self.voxel_size
        T, info = refine(src, tgt, weights, ratio=1e-4, quantization_size=thr, clip=self.clip_weight_thresh,
                         wsum_threshold=max(4000, m if m_threshold is None else int(m_threshold)) * self.clip_weight_thresh)
        info["path"] = "refinement"
        if info["status"] in (1, 2):
            T, r = ransac_dev(src, tgt, 80000, sample_size=4, use_elc=True, thr=thr, seed=self.seed, confidence=0.9999)
            if r["best_h"] < 0:
                T = np.eye(4)
            info["path"], info["ransac"] = "safeguard", r
        self.last = info
        res = {"base": T, "w_icp": T}
        if self.use_icp:
            res["w_icp"], _ = icp_dev(x0, x1, T, max_dist=thr)
        return res

    def wsum_threshold(self, m):
        """max(4000, M) * clip_weight_thresh (:407) as the double `register` hands to the library."""
        return max(4000, int(m)) * self.clip_weight_thresh

    def status_of(self, info, m):
        """G9 on the host, from the result block of a refinement run with wsum_threshold = 0 (lr_dgr_refine_batch takes ONE threshold per
        call, DGR's is per pair): 1 no live row, 2 when w1 < max(4000, M) clip -- the comparison of two doubles the device makes -- else
        the block's own status."""
        if info["L"] == 0:
            return 1
        return 2 if info["w1"] < self.wsum_threshold(m) else info["status"]

    def register_batch(self, xyz0s, xyz1s, idx0s, idx1s, weights, m_thresholds=None, inlier_statuses=None):
        """`register` for many pairs: -> [{'base', 'w_icp'}], self.last a list of infos.  Every pair is refined in lr_dgr_refine_batch calls
        of up to 64 pairs with wsum_threshold = 0; the weight-sum decision is status_of's, and the refinement of a pair that takes the
        safeguard is discarded (its info is G9's: the identity was never returned, iterations = break_count = 0, loss = 0).  A safeguarded
        pair runs the same RANSAC as in `register`.  inlier_statuses (InlierNet.weights_batch): a pair the network refused (2 / 3) takes
        the safeguard too, with info['inlier_status'] set, so that one bad pair never ends a shard."""
        from .ransac import icp_dev, ransac_dev
        P = len(xyz0s)
        lists = dict(xyz1s=xyz1s, idx0s=idx0s, idx1s=idx1s, weights=weights, m_thresholds=m_thresholds, inlier_statuses=inlier_statuses)
        for name, v in lists.items():
            if v is not None and len(v) != P:
                raise ValueError(f"{name} has {len(v)} entries, xyz0s {P}")
        thr = 2 * self.voxel_size
        x0s, x1s, srcs, tgts, ws = [], [], [], [], []
        for k in range(P):
            x0, x1 = _f32(xyz0s[k]).reshape(-1, 3), _f32(xyz1s[k]).reshape(-1, 3)
            i0, i1 = (torch.as_tensor(np.asarray(i) if not torch.is_tensor(i) else i).to(x0.device).long().reshape(-1) for i in (idx0s[k], idx1s[k]))
            src, tgt = x0[i0].contiguous(), x1[i1].contiguous()
            if int(src.shape[0]) > MAX_TAIL:
                raise ValueError(f"pair {k}: {int(src.shape[0])} correspondences, lr_dgr_refine takes at most {MAX_TAIL}")
            x0s.append(x0); x1s.append(x1); srcs.append(src); tgts.append(tgt)
            ws.append(torch.as_tensor(weights[k]).to(device=x0.device, dtype=torch.float32).reshape(-1))
        out = []
        for at in range(0, P, MAX_REFINE_BATCH):
            end = min(P, at + MAX_REFINE_BATCH)
            out += refine_batch(srcs[at:end], tgts[at:end], weights=ws[at:end], ratio=1e-4, quantization_size=thr, clip=self.clip_weight_thresh,
                                wsum_threshold=0.0)[0]
        res, self.last = [], []
        for k, (T, info) in enumerate(out):
            m = int(srcs[k].shape[0]) if m_thresholds is None or m_thresholds[k] is None else int(m_thresholds[k])
            refused = 0 if inlier_statuses is None else int(inlier_statuses[k])
            info["path"] = "refinement"
            status = self.status_of(info, m)
            if refused:
                info["inlier_status"] = refused
            if refused or status in (1, 2):
                if status in (1, 2):
                    info.update(status=status, iterations=0, break_count=0, loss=0.0)
                T, r = ransac_dev(srcs[k], tgts[k], 80000, sample_size=4, use_elc=True, thr=thr, seed=self.seed, confidence=0.9999)
                if r["best_h"] < 0:
                    T = np.eye(4)
                info["path"], info["ransac"] = "safeguard", r
            self.last.append(info)
            one = {"base": T, "w_icp": T}
            if self.use_icp:
                one["w_icp"], _ = icp_dev(x0s[k], x1s[k], T, max_dist=thr)
            res.append(one)
        return res


# ---- the 6-D inlier network -----------------------------------------------------------------------------------------------------------
N_STAGES = resunet.N_STAGES
NK = 729                                              # 3^6 offsets
MAX_N = 131072                                        # rows per lr_dgr_inlier
MAX_PAIRS = 8                                         # pairs per lr_dgr_inlier_batch (three tag bits), MAX_N rows together
MAX_TAIL = 32768                                      # rows per lr_dgr_refine
WIDTHS = (32, 64, 128, 256, 128, 64, 64, 64)          # ResUNetBN2C: C1 C2 C3 C4 (down), T4 T3 T2 T1 (up)
_WIDTH_KEYS = ("conv1", "conv2", "conv3", "conv4", "conv4_tr", "conv3_tr", "conv2_tr", "conv1_tr")
_SD = "DGR inlier state dict"


def offset_index(o):
    """I1: idx(o) = sum_a (o_a + 1) 3^a for o in {-1,0,1}^6, axis 0 fastest [upstream-recalled].  The one place the offset order lives on
    the Python side: a checkpoint in another order is a permutation of the 729 slices at packing time (inlier_fold)."""
    o = np.asarray(o, np.int64)
    return ((o + 1) * 3 ** np.arange(6)).sum(-1)


def check_widths(widths, key=None):
    widths = tuple(int(w) for w in widths)
    if len(widths) != 8:
        raise ValueError(f"widths must be eight numbers (C1 C2 C3 C4 T4 T3 T2 T1), not {widths!r}")
    for i, w in enumerate(widths):
        if w < 32 or w > 256 or w % 32:
            raise ValueError(f"{_SD}: {key[i] if key else _WIDTH_KEYS[i]}.kernel: width {w} is not a multiple of 32 in 32..256")
    return widths


def inlier_stage_plan(widths=WIDTHS):
    """The 23 stages in order: (conv module, norm module | None, offsets, Cin, Cout) -- the module names of DGR/model/resunet.py:442-596."""
    return resunet.stage_plan(check_widths(widths), NK, NK, 1)


def inlier_packed_floats(widths=WIDTHS):
    return resunet.packed_floats(inlier_stage_plan(widths))


def widths_of(sd):
    """I5: the eight widths from the kernels' shapes.  conv1.kernel must be [729, 1, C] (K = 3 and the feature `ones`)."""
    out = []
    for key in _WIDTH_KEYS:
        shape = resunet.np64(sd, key + ".kernel", None, _SD).shape
        if key == "conv1" and (len(shape) != 3 or shape[0] != NK or shape[1] != 1):
            raise ValueError(f"{_SD}: conv1.kernel has shape {shape}, expected [729, 1, C]: conv1_kernel_size 3 and inlier_feature_type 'ones'")
        out.append(int(shape[-1]))
    return check_widths(out)


def inlier_fold(sd, dtype=np.float32):
    """[(W [offsets,Cin,Cout], scale [Cout], offset [Cout])] per stage as `dtype`, the widths read from the kernels (I5): BatchNorm folded
    in fp64 and rounded once, as fcgf.fold.  A missing or extra key, a wrong shape or a non-finite value is a ValueError naming the key."""
    return resunet.fold(sd, inlier_stage_plan(widths_of(sd)), _SD, True, dtype)


def inlier_pack(stages):
    """The flat float32 blob of lr_dgr_inlier_weights_bytes(widths) bytes from inlier_fold's stages: per stage W, scale, offset."""
    return resunet.pack(stages)


def widths_of_stages(stages):
    c = [stages[i][0].shape[-1] for i in (0, 3, 6, 9, 12, 15, 18, 21)]
    return check_widths(c)


class InlierNet:
    """The inlier network with one set of weights on one device."""

    def __init__(self, blob, widths=WIDTHS, device=None):
        L = _ext.lib()
        self.widths = check_widths(widths)
        self._w8 = (ctypes.c_int32 * 8)(*self.widths)
        blob = np.ascontiguousarray(blob, np.float32).reshape(-1)
        want = L.lr_dgr_inlier_weights_bytes(ctypes.byref(self._w8))
        if want == 0 or blob.nbytes != want:
            raise ValueError(f"weight blob of {blob.nbytes} bytes, lr_dgr_inlier_weights_bytes({self.widths}) = {want}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.weights_blob = torch.from_numpy(blob).to(self.device)
        self.couts = [p[4] for p in inlier_stage_plan(self.widths)]
        self.last_info = None

    @classmethod
    def from_stages(cls, stages, device=None):
        return cls(inlier_pack(stages), widths_of_stages(stages), device)

    @classmethod
    def from_state_dict(cls, sd, device=None):
        """sd: the reference's state_dict_inlier (tensors or arrays): <conv>.kernel, final.bias and <norm>.bn.{weight, bias, running_mean,
        running_var[, num_batches_tracked]}; any other key is refused."""
        return cls.from_stages(inlier_fold(sd), device)

    @classmethod
    def from_checkpoint(cls, path, device=None):
        """The reference's DGR checkpoint (deep_global_registration.py:105-152): torch.load(path)['state_dict_inlier']; where the file
        carries its config, inlier_model and inlier_feature_type are checked.  The config is a pickled Python object, so the file is read with
        weights_only=False, as the reference reads it: load checkpoints you trust."""
        state = torch.load(path, map_location="cpu", weights_only=False)
        cfg = state.get("config") if isinstance(state, dict) else None
        if cfg is not None:
            get = cfg.get if isinstance(cfg, dict) else lambda k, d=None: getattr(cfg, k, d)
            model, feat = get("inlier_model", "ResUNetBN2C"), get("inlier_feature_type", "ones")
            if feat != "ones":
                raise ValueError(f"DGR checkpoint: inlier_feature_type {feat!r} is not supported (only 'ones')")
            if model != "ResUNetBN2C":
                raise ValueError(f"DGR checkpoint: inlier_model {model!r} is not supported (only 'ResUNetBN2C')")
        if not isinstance(state, dict) or "state_dict_inlier" not in state:
            raise ValueError("DGR checkpoint: missing key 'state_dict_inlier'")
        return cls.from_state_dict(state["state_dict_inlier"], device)

    def _call(self, coords6, tap, poison=None):
        L = _ext.lib()
        dev = self.device
        coords = torch.as_tensor(coords6).to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 6)
        n = int(coords.shape[0])
        need = L.lr_dgr_inlier_scratch_bytes(n, ctypes.byref(self._w8))
        if need == 0:
            raise ValueError(f"lr_dgr_inlier takes at most {MAX_N} rows, not {n}")
        scratch = devmem.scratch(need, dev, poison)
        res = torch.zeros(ctypes.sizeof(_ext.DgrInlierResult), dtype=torch.uint8, device=dev)
        out = torch.zeros(max(n, 1) * (max(self.widths) if tap else 1), dtype=torch.float32, device=dev)
        tc = torch.zeros((max(n, 1), 6), dtype=torch.int32, device=dev) if tap else None
        params = _ext.DgrInlierParams(tap=int(tap), widths=self.widths)
        with torch.cuda.device(dev):
            _ext.check(L.lr_dgr_inlier(ptr(coords, n), n, self.weights_blob.data_ptr(), self.weights_blob.numel() * 4, ctypes.byref(params), res.data_ptr(),
                                       ptr(out, n), ptr(tc, n), scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream))
        return n, out, tc, res

    def logits(self, coords6, poison=None):
        """coords6 [n,6] integer cells (distinct) -> [n] float32 device tensor, entry i for row i.  self.last_info: the result block
        (status 2: a duplicate row, 3: an axis wider than the extent limit; the logits are 0 then).  poison: test hook, as FCGF.features."""
        n, out, _, res = self._call(coords6, 0, poison)
        r = devmem.read_struct(res, _ext.DgrInlierResult)
        self.last_info = dict(status=r.status, n=r.n, n_tap=r.n_tap)
        return out[:n]

    def tap(self, coords6, s):
        """Stage s (1..23) alone: (activations [n_level, Cout], the level's cells [n_level, 6]) as device tensors."""
        if not 1 <= int(s) <= N_STAGES:
            raise ValueError(f"tap stage must lie in 1..{N_STAGES}")
        n, out, tc, res = self._call(coords6, int(s))
        r = devmem.read_struct(res, _ext.DgrInlierResult)
        self.last_info = dict(status=r.status, n=r.n, n_tap=r.n_tap)
        cout = self.couts[int(s) - 1]
        return out[:r.n_tap * cout].reshape(r.n_tap, cout), tc[:r.n_tap]

    def coords6(self, xyz0, xyz1, idx0, idx1, voxel_size):
        """cat(floor(xyz0[idx0] / voxel), floor(xyz1[idx1] / voxel)) in fp64 (deep_global_registration.py:193, :382) -> [M,6] int32."""
        dev = self.device
        c = []
        for xyz, idx in ((xyz0, idx0), (xyz1, idx1)):
            x = torch.as_tensor(xyz).to(device=dev, dtype=torch.float64).reshape(-1, 3)
            i = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx).to(dev).long().reshape(-1)
            c.append(torch.floor(x / float(voxel_size)).to(torch.int32)[i])
        return torch.cat(c, 1).contiguous()

    def weights(self, xyz0, xyz1, idx0, idx1, voxel_size=0.3):
        """DGRTail's weights_fn bound to a voxel size (functools.partial(net.weights, voxel_size=v)): sigmoid of the logits (:389-390),
        [M] float32 device tensor.  A refused input (last_info['status'] != 0) raises."""
        w = torch.sigmoid(self.logits(self.coords6(xyz0, xyz1, idx0, idx1, voxel_size)))
        if self.last_info["status"] != 0:
            raise _ext.LidarRegError(f"lr_dgr_inlier: status {self.last_info['status']} (2: duplicate correspondence cell, 3: an axis wider than the extent limit)")
        return w

    def _call_batch(self, coords, poison=None):
        """One lr_dgr_inlier_batch over device tensors coords[k] [n_k,6] int32 (at most MAX_PAIRS pairs and MAX_N rows together) ->
        (outs [n_k], the result blocks as one uint8 tensor)."""
        L = _ext.lib()
        dev = self.device
        P = len(coords)
        ns = [int(c.shape[0]) for c in coords]
        outs = [torch.zeros(max(n, 1), dtype=torch.float32, device=dev) for n in ns]
        res = torch.zeros(P * ctypes.sizeof(_ext.DgrInlierResult), dtype=torch.uint8, device=dev)
        scratch = devmem.scratch(L.lr_dgr_inlier_batch_scratch_bytes(P, sum(ns), ctypes.byref(self._w8)), dev, poison)
        arr = lambda ts: (ctypes.c_void_p * P)(*[ptr(t, n) for t, n in zip(ts, ns)])
        params = _ext.DgrInlierParams(tap=0, widths=self.widths)
        with torch.cuda.device(dev):
            _ext.check(L.lr_dgr_inlier_batch(P, arr(coords), (ctypes.c_int32 * P)(*ns), self.weights_blob.data_ptr(), self.weights_blob.numel() * 4,
                                             ctypes.byref(params), res.data_ptr(), arr(outs), scratch.data_ptr(), scratch.numel(),
                                             torch.cuda.current_stream().cuda_stream))
        return [o[:n] for o, n in zip(outs, ns)], res

    def logits_batch(self, coords6_list, poison=None):
        """`logits` for many pairs through lr_dgr_inlier_batch (contract n4): coords6_list[k] [n_k,6] -> a list of [n_k] device tensors in
        the caller's order, each holding the bytes `logits` gives for that pair alone.  self.last_info: one dict per pair; the status is
        per pair.  A longer list is split, in order, into calls of at most MAX_PAIRS pairs and MAX_N rows; a pair that alone exceeds MAX_N
        rows is a ValueError naming its index."""
        dev = self.device
        coords = [torch.as_tensor(c).to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 6) for c in coords6_list]
        for k, c in enumerate(coords):
            if int(c.shape[0]) > MAX_N:
                raise ValueError(f"coords6_list[{k}] has {int(c.shape[0])} rows: lr_dgr_inlier_batch takes at most {MAX_N}")
        outs, blocks = [], []
        at = 0
        while at < len(coords):
            end, rows = at + 1, int(coords[at].shape[0])
            while end < len(coords) and end - at < MAX_PAIRS and rows + int(coords[end].shape[0]) <= MAX_N:
                rows += int(coords[end].shape[0]); end += 1
            o, res = self._call_batch(coords[at:end], poison)
            outs += o; blocks.append(res)
            at = end
        self.last_info = []
        for res in blocks:
            host = res.cpu()
            for k in range(host.numel() // ctypes.sizeof(_ext.DgrInlierResult)):
                r = devmem.read_struct(host, _ext.DgrInlierResult, k)
                self.last_info.append(dict(status=r.status, n=r.n, n_tap=r.n_tap))
        return outs

    def weights_batch(self, xyz0s, xyz1s, idx0s, idx1s, voxel_size=0.3):
        """`weights` for many pairs: ([sigmoid of the logits, [M_k] float32 device tensor], [the network's status per pair]).  It does not
        raise on a refused pair (status 2 / 3: its logits are 0): DGRTail.register_batch sends such a pair to the safeguard."""
        logits = self.logits_batch([self.coords6(*a, voxel_size) for a in zip(xyz0s, xyz1s, idx0s, idx1s)])
        return [torch.sigmoid(l) for l in logits], [i["status"] for i in self.last_info]


def correspondences_dev(xyz0, xyz1, F0, F1, args, ws, stream):
    """fcgf_feature_matching (deep_global_registration.py:206-218): every source point with its nearest target descriptor, through
    lr_nn_top2; no filter, no subsampling.  Returns (idx0, idx1 device int32, count device int32 [1]); nothing is synchronised."""
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    idx0 = torch.arange(n0, dtype=torch.int32, device=dev)
    idx1 = torch.empty(n0, dtype=torch.int32, device=dev)
    _ext.check(_ext.lib().lr_nn_top2(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, idx1.data_ptr(), None, None, None, stream))
    return idx0, idx1, torch.full((1,), n0, dtype=torch.int32, device=dev)


def eval_pairs(source, indices, args, device=None, batch=32, nstreams=3, verbose=False):
    """--algo DGR over `indices` of `source` (corrset.eval_pairs).  Per window one solve(srcs, tgts): the 6-D cells (floor in fp64 of the
    gathered points / voxel), InlierNet.weights_batch, DGRTail.register_batch without ICP -- the engine's own ICP follows.  Returns a
    harness.EvalRun.  Column 9 = the pair's share of its window's solve (device time between two events, split evenly), as for --algo SM.
    A pair above the refinement's MAX_TAIL rows keeps the rows the clip leaves, as DGR.register does."""
    from . import FR as fr
    path = getattr(args, "dgr_weights", None)
    if not path:
        raise ValueError("--algo DGR needs --dgr_weights FILE (the reference's DGR checkpoint: state_dict_inlier)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    net = InlierNet.from_checkpoint(path, dev)
    tail = DGRTail(fr.VOXEL_SIZE, float(getattr(args, "dgr_clip_weight_thresh", 0.05)), use_icp=False, seed=int(getattr(args, "seed", 51)))
    return corrset.eval_pairs(source, indices, args, correspondences_dev, lambda srcs, tgts: solve_window(net, tail, srcs, tgts), device=device,
                              batch=min(int(batch), MAX_REFINE_BATCH), nstreams=nstreams, verbose=verbose)


def drop_clipped(w, clip, *rows):
    """DGR.register's path for a set above MAX_TAIL rows: the rows the clip kills never reach the tail (the same live rows in the same
    order, so the same bits) -> (w, *rows) of the kept ones."""
    keep = (w > 0) & (w >= clip)
    return (w[keep],) + tuple(r[keep] for r in rows)


def solve_window(net, tail, srcs, tgts):
    """One window of --algo DGR on gathered correspondences src[i] <-> tgt[i]: ([(T 4x4, info)], device ms)."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    ar = [torch.arange(int(s.shape[0]), device=net.device) for s in srcs]
    ws, statuses = net.weights_batch(srcs, tgts, ar, ar, tail.voxel_size)
    ms = [int(s.shape[0]) for s in srcs]
    srcs, tgts = list(srcs), list(tgts)
    for k, m in enumerate(ms):
        if m > MAX_TAIL:
            ws[k], srcs[k], tgts[k] = drop_clipped(ws[k], tail.clip_weight_thresh, srcs[k], tgts[k])
            if int(srcs[k].shape[0]) > MAX_TAIL:
                raise ValueError(f"{int(srcs[k].shape[0])} of {m} correspondences survive the clip: lr_dgr_refine takes at most {MAX_TAIL}")
    ar = [torch.arange(int(s.shape[0]), device=net.device) for s in srcs]
    res = tail.register_batch(srcs, tgts, ar, ar, ws, m_thresholds=ms, inlier_statuses=statuses)
    ev1.record(); ev1.synchronize()
    return [(r["base"], info) for r, info in zip(res, tail.last)], ev0.elapsed_time(ev1)


class DGR:
    """DeepGlobalRegistration (deep_global_registration.py:352-459) with safeguard_method 'correspondence': fcgf an fcgf.FCGF, inlier an
    InlierNet."""

    def __init__(self, fcgf, inlier, voxel_size=0.3, clip_weight_thresh=0.05, use_icp=True, seed=51):
        self.fcgf, self.inlier, self.voxel_size, self.clip_weight_thresh = fcgf, inlier, float(voxel_size), float(clip_weight_thresh)
        self.tail = DGRTail(voxel_size, clip_weight_thresh, use_icp, None, seed)
        self.last = None             # what the last register() saw: the counts, the weights, the tail's info

    def preprocess(self, xyz):
        """:169-196: (kept points float64, the same as float32, their cells [n,3] int32), device tensors."""
        from . import voxel
        x64 = torch.as_tensor(xyz).to(device=self.inlier.device, dtype=torch.float64).reshape(-1, 3)
        x32, sel = voxel.voxel_downsample(x64, self.voxel_size)
        kept = x64[sel]
        return kept, x32, torch.floor(kept / self.voxel_size).to(torch.int32)

    def register(self, xyz0, xyz1, only_calc_weights=False):
        """-> {'base': T, 'w_icp': T_icp}; only_calc_weights: the weights [M] (:391).  The network takes up to MAX_N correspondences, the
        refinement MAX_TAIL: above that the rows the clip kills are dropped before the tail sees them (the same live rows in the same
        order, so the same bits; the weight-sum threshold keeps the original count).  Still above: ValueError."""
        from .matching import nn_top2_dev
        with torch.cuda.device(self.inlier.device):
            k0, x0, c0 = self.preprocess(xyz0)
            k1, x1, c1 = self.preprocess(xyz1)
            f0, f1 = self.fcgf.features(c0), self.fcgf.features(c1)
            idx1 = nn_top2_dev(f0, f1, want_2nd=False)[0].long()              # fcgf_feature_matching (:206-218)
            idx0 = torch.arange(idx1.shape[0], device=idx1.device)
            m = int(idx0.shape[0])
            if m > MAX_N:
                raise ValueError(f"{m} correspondences: lr_dgr_inlier takes at most {MAX_N}")
            w = self.inlier.weights(k0, k1, idx0, idx1, self.voxel_size)
            self.last = dict(m=m, weights=w, idx0=idx0, idx1=idx1)
            if only_calc_weights:
                return w
            if m > MAX_TAIL:
                keep = (w > 0) & (w >= self.clip_weight_thresh)
                idx0, idx1, w = idx0[keep], idx1[keep], w[keep]
                if int(idx0.shape[0]) > MAX_TAIL:
                    raise ValueError(f"{int(idx0.shape[0])} of {m} correspondences survive the clip: lr_dgr_refine takes at most {MAX_TAIL}")
            self.last.update(m_tail=int(idx0.shape[0]), idx0_tail=idx0, idx1_tail=idx1, weights_tail=w, xyz0=x0, xyz1=x1)
            res = self.tail.register(x0, x1, idx0, idx1, weights=w, m_threshold=m)
            self.last["tail"] = self.tail.last
            return res

    def register_batch(self, pairs):
        """`register` for a list of (xyz0, xyz1): -> [{'base', 'w_icp'}], each the bytes `register` gives for that pair; self.last a list.
        The voxel de-duplication per cloud, FCGF.features_batch over all 2 P clouds, the feature nearest neighbour per pair,
        InlierNet.weights_batch, per pair the drop of the clipped rows of a set above MAX_TAIL, then DGRTail.register_batch.  A pair the
        inlier network refuses takes the safeguard (its info carries inlier_status) where `register` raises."""
        from .matching import nn_top2_dev
        with torch.cuda.device(self.inlier.device):
            pre = [(self.preprocess(a), self.preprocess(b)) for a, b in pairs]
            feats = self.fcgf.features_batch([c[2] for p in pre for c in p])
            for b, info in enumerate(self.fcgf.last_info):
                if info["status"] != 0:
                    raise _ext.LidarRegError(f"lr_fcgf_extract_batch: cloud {b % 2} of pair {b // 2}: status {info['status']}")
            idx0s, idx1s = [], []
            for k in range(len(pairs)):
                idx1 = nn_top2_dev(feats[2 * k], feats[2 * k + 1], want_2nd=False)[0].long()
                if int(idx1.shape[0]) > MAX_N:
                    raise ValueError(f"pair {k}: {int(idx1.shape[0])} correspondences: lr_dgr_inlier takes at most {MAX_N}")
                idx0s.append(torch.arange(idx1.shape[0], device=idx1.device)); idx1s.append(idx1)
            k0s, k1s = [p[0][0] for p in pre], [p[1][0] for p in pre]
            x0s, x1s = [p[0][1] for p in pre], [p[1][1] for p in pre]
            ws, statuses = self.inlier.weights_batch(k0s, k1s, idx0s, idx1s, self.voxel_size)
            ms = [int(i.shape[0]) for i in idx0s]
            self.last = [dict(m=m, weights=w, idx0=i0, idx1=i1, inlier_status=s) for m, w, i0, i1, s in zip(ms, ws, idx0s, idx1s, statuses)]
            t0, t1, tw = list(idx0s), list(idx1s), list(ws)
            for k, m in enumerate(ms):
                if m > MAX_TAIL:
                    tw[k], t0[k], t1[k] = drop_clipped(ws[k], self.clip_weight_thresh, idx0s[k], idx1s[k])
                    if int(t0[k].shape[0]) > MAX_TAIL:
                        raise ValueError(f"pair {k}: {int(t0[k].shape[0])} of {m} correspondences survive the clip: lr_dgr_refine takes at most {MAX_TAIL}")
                self.last[k].update(m_tail=int(t0[k].shape[0]), idx0_tail=t0[k], idx1_tail=t1[k], weights_tail=tw[k], xyz0=x0s[k], xyz1=x1s[k])
            res = self.tail.register_batch(x0s, x1s, t0, t1, tw, m_thresholds=ms, inlier_statuses=statuses)
            for k, info in enumerate(self.tail.last):
                self.last[k]["tail"] = info
            return res
