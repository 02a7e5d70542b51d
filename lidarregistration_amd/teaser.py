"""TEASER++ back end (``--algo TEASER``) on top of liblidarreg.so: lr_teaser / lr_teaser_batch (csrc/lr_teaser.hip).

``TEASER`` keeps the reference's call shape (Experiments/algorithms/TEASER_plus_plus.py:101-126); ``eval_pairs`` is the batched
engine of ``python -m test --algo TEASER``: per window, the NN search and the BB_first grid filter run pair by pair on the existing
single-pair entry points (spread over streams), the correspondences' xyz are gathered, and ONE lr_teaser_batch call solves the
window; ICP follows through lr_icp (the engine and the call plumbing are corrset.py's).  The contract the solver implements is stated in include/lidarreg.h and DESIGN.md §10.
"""
import ctypes

import numpy as np
import torch

from . import _ext, corrset
from .matching import _f32, _stream

RESULT_BYTES = ctypes.sizeof(_ext.TeaserResult)
VOXEL_SIZE = 0.3          # TEASER_plus_plus.py: noise_bound = VOXEL_SIZE


def params(**kw):
    """lr_teaser_params: the reference's settings unless overridden (noise_bound, cbar2, kcore_threshold, gnc_factor,
    max_iterations, cost_threshold, node_budget, time_budget_ms)."""
    return _ext.TeaserParams(**kw)


def _info(r):
    return dict(status=r.status, K=r.K, exact=r.exact, max_core=r.max_core, lb=r.lb, nodes=int(r.nodes), gnc_iters=r.gnc_iters,
                n_rot_inliers=r.n_rot_inliers, n_trans_inliers=r.n_trans_inliers)


# the solver as corrset.BatchCall sees it; the one per-pair output is the clique (int32, -1 where nothing is written)
SOLVER = corrset.Solver("lr_teaser", "lr_teaser_batch", "lr_teaser_scratch_bytes", (params,), _ext.TeaserResult,
                        (corrset.Out("clique", torch.int32, -1),), _info)


def _decode(call):
    return [(T, info, c[:info["K"]].cpu().numpy().astype(np.int64)) for (T, info), c in zip(call.results(), call.outs[0])]


def teaser_batch_dev(srcs, tgts, ms=None, m_devs=None, poison=None, **kw):
    """lr_teaser_batch over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0).  ms: live counts passed as m (default: the
    rows); m_devs: optional device int32 tensors with a smaller live count.  Returns [(T 4x4, info dict, clique int array)] and the
    device time of the call in ms.  poison: fill the scratch with this byte first (test hook)."""
    call = corrset.BatchCall(SOLVER, srcs, tgts, ms, m_devs, poison, **kw)
    ms = call.timed()
    return _decode(call), ms


def teaser_dev(src, tgt, m_dev=None, poison=None, **kw):
    """lr_teaser on one correspondence set: (T 4x4 float64, info dict, clique ascending int64 array)."""
    call = corrset.BatchCall(SOLVER, [src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True, **kw)
    call.launch(_stream())
    return _decode(call)[0]


def correspondences_dev(xyz0, xyz1, F0, F1, args, ws, stream):
    """NN (with second neighbour) + Grid_Prioritized_Filter(BB_first=True) on device, as TEASER_plus_plus.py:109-110 runs them.
    Returns (idx0, idx1 device int32 [n0], count device int32[2] = (M, has_score)); nothing is synchronised."""
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    i1 = torch.empty(n0, dtype=torch.int32, device=dev); i2 = torch.empty_like(i1)
    o0 = torch.empty_like(i1); o1 = torch.empty_like(i1); o2 = torch.empty_like(i1)
    sc = torch.empty(n0, dtype=torch.float32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    L = _ext.lib()
    _ext.check(L.lr_nn_top2(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, i1.data_ptr(), i2.data_ptr(), None, None, stream))
    _ext.check(L.lr_gpf_bb_first(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, i1.data_ptr(), i2.data_ptr(), xyz0.data_ptr(),
                                 int(getattr(args, "GPF_grid_wid", 10)), float(getattr(args, "GPF_max_matches", 10 ** 9)),
                                 o0.data_ptr(), o1.data_ptr(), o2.data_ptr(), sc.data_ptr(), cnt.data_ptr(), cnt[1:].data_ptr(), stream))
    return o0, o1, cnt


def TEASER(A_pcd, B_pcd, A_feats, B_feats, A_tensor, args):
    """TEASER_plus_plus.py:101-126: FCGF correspondences (find_2nn + BB_first GPF) -> TEASER++ -> (T 4x4, elapsed_time).
    elapsed_time = the second neighbour's surcharge (0 here: fused NN kernel, matching.find_2nn) + the solve's device time; the
    GPF call is not billed, as in the reference.  A_pcd / B_pcd: anything with .points (open3d-like) or [N,3] arrays."""
    pts = lambda p: np.asarray(getattr(p, "points", p), np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    xyz0, xyz1 = _f32(pts(A_pcd)), _f32(pts(B_pcd))
    F0, F1 = _f32(A_feats), _f32(B_feats)
    ws = _ext.Workspace.for_dim(F0.shape[0], F1.shape[0], F0.shape[1], 1)
    try:
        o0, o1, cnt = correspondences_dev(xyz0, xyz1, F0, F1, args, ws, _stream())
        m = int(cnt[0].item())
        src, tgt = xyz0[o0[:m].long()], xyz1[o1[:m].long()]
        (T, info, _), ms = teaser_batch_dev([src], [tgt], time_budget_ms=_budget_ms(args))
    finally:
        torch.cuda.synchronize(dev)
        ws.close()
    if getattr(args, "mode", None) == "FAIL_TOLERANT" and not info["exact"]:
        T = np.eye(4)
    return T, ms * 1e-3


def _budget_ms(args):
    return float(getattr(args, "teaser_max_wait", 10.0)) * 1e3          # MAX_WAIT = 10 s (TEASER_plus_plus.py:14)


def eval_pairs(source, indices, args, device=None, batch=32, nstreams=3, verbose=False):
    """--algo TEASER over `indices` of `source` (corrset.eval_pairs).  Returns a harness.EvalRun with totals and `exact`.  Column 9 = the
    pair's share of its window's solve (device time of the lr_teaser_batch call split evenly) + the second neighbour's surcharge (0); the
    NN / GPF time is not billed (TEASER_plus_plus.py:109-123)."""
    exact = np.ones(len(indices), np.int32)
    fail_tolerant = getattr(args, "mode", None) == "FAIL_TOLERANT"

    def row(r, T, info):
        exact[r] = info["exact"]
        return np.eye(4) if fail_tolerant and not info["exact"] else T

    return corrset.eval_pairs(source, indices, args, correspondences_dev, lambda srcs, tgts: teaser_batch_dev(srcs, tgts, time_budget_ms=_budget_ms(args)),
                              row, exact, device, batch, nstreams, verbose)
