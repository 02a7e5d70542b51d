"""Deep Global Registration's robust pose refinement on top of liblidarreg.so: lr_dgr_refine / lr_dgr_refine_batch (csrc/lr_dgr.hip).

``GlobalRegistration`` keeps the reference's call shape (DGR/core/registration.py:135-194); ``refine`` / ``refine_batch`` are the device
calls; ``DGRTail`` is what DeepGlobalRegistration.register does once it has the inlier weights (DGR/core/deep_global_registration.py:
403-459): the weight-sum decision, the refinement or the safeguard RANSAC, then ICP.  The contract the refinement implements is stated in
include/lidarreg.h (d1) and DESIGN.md §19.

``InlierNet`` is the 6-D inlier network that gives the weights (lr_dgr_inlier, csrc/lr_dgr6.hip; contract n3, DESIGN.md §20, restated in
numpy in tests/dgr6_cpu.py) and ``DGR`` the whole DeepGlobalRegistration.register (:352-459): voxel de-duplication, FCGF features, the
feature nearest neighbour, the inlier network, the tail.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _ext, corrset, devmem, resunet
from .devmem import ptr
from .matching import _f32, _stream

RESULT_BYTES = ctypes.sizeof(_ext.DgrResult)
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


# ---- the 6-D inlier network -----------------------------------------------------------------------------------------------------------
N_STAGES = resunet.N_STAGES
NK = 729                                              # 3^6 offsets
MAX_N = 131072                                        # rows per lr_dgr_inlier
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
