"""Best-Buddies refinement (BBR-F) and hybrid-search point normals on the GPU: the second refinement of the reference's refinement tester
(FCGF_FAST/net/BBR_F.py, called from FCGF_FAST/net/refinement_tester.py:75-93), on top of lr_bbrf / lr_normals (csrc/lr_bbrf.hip).  The
whole 100-step loop -- two exact nearest-neighbour searches, the loss and its analytic gradient, Adam -- is one library call without a
host synchronisation.  The contract is stated in include/lidarreg.h and DESIGN.md §14.  No CPU fallback.
"""
import ctypes
import math
from time import time

import numpy as np
import torch

from . import _ext, devmem
from .devmem import as_dict, f64, ptr, read_struct
from .matching import _device, _stream
from .overlap import voxel_down_sample

NUM_SAMPLES = 30000         # BBR_F.py:269
REFINE_VOXEL = 0.3          # the refinement tester's voxel_size


def normals_dev(X, radius=0.01, max_nn=13, poison=None):
    """lr_normals of X [n,3] (float64).  Returns (normals [n,3] float64 device tensor, dict(status, n_dropped, n_default))."""
    dev = _device()
    x = f64(X, dev)
    n = int(x.shape[0])
    L = _ext.lib()
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = devmem.scratch(L.lr_normals_scratch_bytes(n), dev, poison)
    _ext.check(L.lr_normals(ptr(x, n), n, float(radius), int(max_nn), out.data_ptr(), info.data_ptr(),
                            scratch.data_ptr(), scratch.numel(), _stream()))
    status, dropped, default, _ = (int(v) for v in info.cpu())
    return out[:n], dict(status=status, n_dropped=dropped, n_default=default)


def calc_normals(X, knn_for_normals=13, radius=0.01):
    """BBR_F.py:236-241: Open3D's estimate_normals with KDTreeSearchParamHybrid(radius, max_nn) as an [n,3] float64 numpy array.  With
    the reference's radius of 1 cm on clouds down-sampled at 0.3 m every point is its own only neighbour and every normal (0, 0, 1)."""
    return normals_dev(X, radius, knn_for_normals)[0].cpu().numpy()


def bbr_f_dev(A, B, nA, nB, poison=None, want_log=True, **params):
    """lr_bbrf on tensors or arrays A, nA [n0,3], B, nB [n1,3] (evaluated in float64); params: the fields of lr_bbrf_params.  Returns
    (result dict with T and B_to_A as 4x4 numpy arrays, log [n_iter, 8] float64 device tensor or None)."""
    dev = _device()
    a, b, na, nb = f64(A, dev), f64(B, dev), f64(nA, dev), f64(nB, dev)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    assert na.shape[0] == n0 and nb.shape[0] == n1, "one normal per point"
    L = _ext.lib()
    p = _ext.BbrfParams(**params)
    res = torch.zeros(ctypes.sizeof(_ext.BbrfResult), dtype=torch.uint8, device=dev)
    log = torch.full((max(int(p.n_iter), 1), 8), math.nan, dtype=torch.float64, device=dev) if want_log else None
    scratch = devmem.scratch(L.lr_bbrf_scratch_bytes(n0, n1, max(1, min(int(p.n_iter), 1000))), dev, poison)
    _ext.check(L.lr_bbrf(ptr(a, n0), ptr(na, n0), n0, ptr(b, n1), ptr(nb, n1), n1, ctypes.byref(p), res.data_ptr(),
                         ptr(log), scratch.data_ptr(), scratch.numel(), _stream()))
    return as_dict(read_struct(res, _ext.BbrfResult)), log


def _downsample(X, X_normals, num_samples):
    inds = np.random.permutation(X.shape[0])[:num_samples]          # the global generator, as BBR_F.py:262
    return X[inds, :], X_normals[inds, :]


def BBR_F(A, B, normals=None, return_info=False):
    """BBR_F.py:267-322: (A_to_B 4x4 float64 numpy, elapsed seconds).  Normals on the full clouds (calc_normals; normals = (nA, nB)
    overrides them), each cloud cut to 30 000 points by np.random.permutation, 100 iterations, the pose of the least loss, inverted.
    elapsed covers what the reference's covers: the normals, the sub-sampling and the loop.  return_info: (A_to_B, elapsed, result
    dict, log as numpy)."""
    start_time = time()
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3); B = np.ascontiguousarray(B, np.float64).reshape(-1, 3)
    A_normals = calc_normals(A) if normals is None else np.ascontiguousarray(normals[0], np.float64).reshape(-1, 3)
    B_normals = calc_normals(B) if normals is None else np.ascontiguousarray(normals[1], np.float64).reshape(-1, 3)
    A, A_normals = _downsample(A, A_normals, NUM_SAMPLES)
    B, B_normals = _downsample(B, B_normals, NUM_SAMPLES)
    r, log = bbr_f_dev(A, B, A_normals, B_normals, want_log=return_info)
    A_to_B = r["T"]
    elapsed = time() - start_time
    return (A_to_B, elapsed, r, log.cpu().numpy()) if return_info else (A_to_B, elapsed)


def calc_errors(T_pred, T_gt, rot_thresh, trans_thresh, eps=1e-16):
    """refinement_tester.py:119-130: [recall, translation error, rotation error in degrees]."""
    if T_pred is None:
        return np.array([0, np.inf, np.inf])
    rte = np.linalg.norm(T_pred[:3, 3] - T_gt[:3, 3])
    rre = np.arccos(np.clip((np.trace(T_pred[:3, :3].T @ T_gt[:3, :3]) - 1) / 2, -1 + eps, 1 - eps)) * 180 / math.pi
    return np.array([rte < trans_thresh and rre < rot_thresh, rte, rre])


def refinement_sample(gt_motion, init_motion, PC0, PC1, rot_thresh, trans_thresh, voxel_size=REFINE_VOXEL, symmetric=False):
    """refinement_tester.py:75-90: the twelve result columns [ICP recall, te, re, time, BBR recall, te, re, time, symmetric-ICP recall,
    te, re, time] of one pair: both clouds down-sampled at voxel_size, cloud 0 moved by the coarse motion, the ground truth taken
    relative to it, then ICP (lr_icp at 2 voxel_size, exactly overlap.refine_motion's), BBR-F and, with symmetric=True, the symmetric
    ICP (symicp.symmetric_icp at 2 voxel_size: lr_symicp, upstream-recalled, parity unpinned -- the reference calls an external binary).
    symmetric=False, the default, leaves columns 8-11 NaN."""
    from .ransac import icp_dev
    init = np.ascontiguousarray(init_motion, np.float64).reshape(4, 4)
    a = voxel_down_sample(PC0, voxel_size); b = voxel_down_sample(PC1, voxel_size)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    a = torch.stack([((float(init[r, 0]) * x + float(init[r, 1]) * y) + float(init[r, 2]) * z) + float(init[r, 3]) for r in range(3)], dim=1)
    gt = np.ascontiguousarray(gt_motion, np.float64).reshape(4, 4) @ np.linalg.inv(init)
    t0 = time()
    ICP_M, _ = icp_dev(a.float().contiguous(), b.float().contiguous(), np.eye(4), max_dist=2.0 * float(voxel_size))
    ICP_time = time() - t0
    BBR_M, BBR_time = BBR_F(a.cpu().numpy(), b.cpu().numpy())
    nan = float("nan")
    sym = [nan, nan, nan, nan]
    if symmetric:
        from .symicp import symmetric_icp
        SYM_M, SYM_time = symmetric_icp(a, b, max_dist=2.0 * float(voxel_size))
        sym = [*calc_errors(SYM_M, gt, rot_thresh, trans_thresh), SYM_time]
    return np.array([*calc_errors(ICP_M, gt, rot_thresh, trans_thresh), ICP_time, *calc_errors(BBR_M, gt, rot_thresh, trans_thresh), BBR_time,
                     *sym])
