"""Deep Global Registration's robust pose refinement on top of liblidarreg.so: lr_dgr_refine / lr_dgr_refine_batch (csrc/lr_dgr.hip).

``GlobalRegistration`` keeps the reference's call shape (DGR/core/registration.py:135-194); ``refine`` / ``refine_batch`` are the device
calls; ``DGRTail`` is what DeepGlobalRegistration.register does once it has the inlier weights (DGR/core/deep_global_registration.py:
403-459): the weight-sum decision, the refinement or the safeguard RANSAC, then ICP.  The inlier network is not built: weights are given, or
come from a ``weights_fn`` hook.  The contract the refinement implements is stated in include/lidarreg.h (d1) and DESIGN.md §19.
"""
import ctypes

import numpy as np
import torch

from . import _ext, corrset
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
    weights [M] is the hook a later inlier network plugs into; it is asked only when register() is given no weights."""

    def __init__(self, voxel_size=0.3, clip_weight_thresh=0.05, use_icp=True, weights_fn=None, seed=51):
        self.voxel_size, self.clip_weight_thresh, self.use_icp, self.weights_fn, self.seed = float(voxel_size), float(clip_weight_thresh), bool(use_icp), weights_fn, seed
        self.last = None             # info of the last register(): the refinement's result block and which path ran

    def register(self, xyz0, xyz1, idx0, idx1, weights=None):
        """-> {'base': T, 'w_icp': T_icp}.  'base': the refinement (ratio 1e-4, quantization 2 * voxel, :415-421) when the clipped weights
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
                         wsum_threshold=max(4000, m) * self.clip_weight_thresh)
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
