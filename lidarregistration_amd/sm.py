"""Spectral-matching back end (``--algo SM``) on top of liblidarreg.so: lr_sm / lr_sm_batch (csrc/lr_sm.hip).

``SM`` keeps the reference's call shape (Experiments/baseline_scripts/baseline_3DMatch.py:19-53); ``eval_pairs`` is the batched engine of
``python -m test --algo SM``: per window, the correspondences come pair by pair from the existing single-pair entry points (mutual nearest
neighbours, or the grid filter with ``--mode GPF``; spread over streams), their xyz are gathered, and ONE lr_sm_batch call solves the
window; ICP follows through lr_icp (the engine and the call plumbing are corrset.py's).  The contract the solver implements is stated in include/lidarreg.h and DESIGN.md §11.
"""
import ctypes

import numpy as np
import torch

from . import _ext, corrset
from .matching import _stream

RESULT_BYTES = ctypes.sizeof(_ext.SmResult)
INLIER_THRESHOLD = 0.6    # baseline_KITTI.py:51 (= 2 * VOXEL_SIZE, the CLI's threshold)


def params(**kw):
    """lr_sm_params: the reference's settings unless overridden (iterations, inlier_threshold, top_ratio)."""
    return _ext.SmParams(**kw)


def _info(r):
    return dict(status=r.status, K=r.K, m=r.m, weight_sum=r.weight_sum)


# the solver as corrset.BatchCall sees it; per-pair outputs in the ABI's order: the eigenvector, the labels
SOLVER = corrset.Solver("lr_sm", "lr_sm_batch", "lr_sm_scratch_bytes", (params,), _ext.SmResult,
                        (corrset.Out("eig", torch.float32, -1.0), corrset.Out("labels", torch.uint8, 255)), _info)


def _decode(call):
    eigs, labels = call.outs
    return [(T, info, labels[k][:m].cpu().numpy(), eigs[k][:m].cpu().numpy()) for k, ((T, info), m) in enumerate(zip(call.results(), call.ms))]


def sm_batch_dev(srcs, tgts, ms=None, m_devs=None, poison=None, **kw):
    """lr_sm_batch over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0).  ms: the counts passed as m (default: the rows);
    m_devs: optional device int32 tensors with a smaller live count.  Returns [(T 4x4, info dict, labels uint8 [m], eig float32 [m])]
    and the device time of the call in ms.  poison: fill the scratch with this byte first (test hook)."""
    call = corrset.BatchCall(SOLVER, srcs, tgts, ms, m_devs, poison, **kw)
    ms = call.timed()
    return _decode(call), ms


def sm_dev(src, tgt, m_dev=None, poison=None, **kw):
    """lr_sm on one correspondence set: (T 4x4 float64, info dict, labels uint8 [m], eig float32 [m])."""
    call = corrset.BatchCall(SOLVER, [src], [tgt], None, None if m_dev is None else [m_dev], poison, single=True, **kw)
    call.launch(_stream())
    return _decode(call)[0]


def SM(corr, src_keypts, tgt_keypts, args, top_ratio=0.1):
    """baseline_3DMatch.py:19-53: (pred_trans [1,4,4], pred_labels [1,M]) float32 tensors on the inputs' device.  src_keypts / tgt_keypts
    [1,M,3] are what is read (corr is their concatenation in the reference's callers); args.inlier_threshold as there."""
    src, tgt = torch.as_tensor(src_keypts), torch.as_tensor(tgt_keypts)
    T, _, labels, _ = sm_dev(src.reshape(-1, 3), tgt.reshape(-1, 3), inlier_threshold=float(getattr(args, "inlier_threshold", INLIER_THRESHOLD)),
                             top_ratio=float(top_ratio), iterations=int(getattr(args, "SM_iters", 10)))
    return (torch.from_numpy(T).to(dtype=torch.float32, device=src.device)[None],
            torch.from_numpy(labels.astype(np.float32)).to(src.device)[None])


def correspondences_dev(xyz0, xyz1, F0, F1, args, ws, stream):
    """NN + the CLI's filter on device: mutual nearest neighbours (matching.py:222-239), or Grid_Prioritized_Filter (matching.py:100-205)
    with --mode GPF.  Returns (idx0, idx1 device int32 [n0], count device int32 [1]); nothing is synchronised."""
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    gpf = str(getattr(args, "mode", "MNN")).upper() == "GPF"
    i1 = torch.empty(n0, dtype=torch.int32, device=dev); i2 = torch.empty_like(i1)
    o0 = torch.empty_like(i1); o1 = torch.empty_like(i1); o2 = torch.empty_like(i1)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _ext.lib()
    _ext.check(L.lr_nn_top2(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, i1.data_ptr(), i2.data_ptr() if gpf else None, None, None, stream))
    if gpf:
        sc = torch.empty(n0, dtype=torch.float32, device=dev)
        _ext.check(L.lr_gpf(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, i1.data_ptr(), i2.data_ptr(), xyz0.data_ptr(),
                            int(getattr(args, "GPF_grid_wid", 10)), float(getattr(args, "GPF_factor", 2.0)),
                            o0.data_ptr(), o1.data_ptr(), o2.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stream))
    else:
        _ext.check(L.lr_nn_to_mutual(ws.handle, F0.data_ptr(), n0, F1.data_ptr(), n1, d, i1.data_ptr(), None, None,
                                     o0.data_ptr(), o1.data_ptr(), None, cnt.data_ptr(), stream))
    return o0, o1, cnt


def solver_kw(args):
    return dict(iterations=int(getattr(args, "SM_iters", 10)), top_ratio=float(getattr(args, "SM_top_ratio", 0.05)), inlier_threshold=INLIER_THRESHOLD)


def eval_pairs(source, indices, args, device=None, batch=32, nstreams=3, verbose=False):
    """--algo SM over `indices` of `source` (corrset.eval_pairs).  Returns a harness.EvalRun.  Column 9 = the pair's share of its window's
    solve (device time of the lr_sm_batch call split evenly); the NN / filter time is not billed (as for --algo TEASER)."""
    kw = solver_kw(args)
    return corrset.eval_pairs(source, indices, args, correspondences_dev, lambda srcs, tgts: sm_batch_dev(srcs, tgts, **kw),
                              device=device, batch=batch, nstreams=nstreams, verbose=verbose)
