"""Symmetric ICP on the GPU: the third refinement of the reference's refinement tester (FCGF_FAST/net/symmetric_icp.py:47-82, called from
FCGF_FAST/net/refinement_tester.py:75-93), on top of lr_symicp (csrc/lr_symicp.hip) and lr_normals2.  The reference shells out to trimesh2's
mesh_align, a binary outside its tree: upstream-recalled, parity unpinned.  What runs here is the algorithm of the paper behind that binary
(Rusinkiewicz, A Symmetric Objective Function for ICP, 2019) as stated in include/lidarreg.h f9 and DESIGN.md §23: per iteration two exact
nearest-neighbour searches, one fused reduction of the 6 x 6 normal equations, a Cholesky solve and the split rotation, the whole loop one
library call without a host synchronisation.  No CPU fallback.
"""
import ctypes
import math
from time import time

import numpy as np
import torch

from . import _ext, devmem
from .devmem import as_dict, f64, ptr, read_struct
from .matching import _device, _stream

REFINE_VOXEL = 0.3          # the refinement tester's voxel_size; max_dist defaults to two of them
NORMAL_RADIUS = 1.0         # hybrid-search radius and neighbour cap of the normals, and the least count at which a normal is kept
NORMAL_MAX_NN = 32
MIN_NB = 5


def normals_counted(X, radius=NORMAL_RADIUS, max_nn=NORMAL_MAX_NN, poison=None):
    """lr_normals2 of X [n,3] (float64).  Returns (normals [n,3] float64, counts [n] int32, both device tensors, dict(status, n_dropped,
    n_default)).  counts[i] = the neighbours point i took, itself included (0 .. max_nn; 0 for a non-finite point): a normal with a
    count below 3 is the default (0, 0, 1), which a true vertical normal cannot be told from otherwise."""
    dev = _device()
    x = f64(X, dev)
    n = int(x.shape[0])
    L = _ext.lib()
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev)
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = devmem.scratch(L.lr_normals_scratch_bytes(n), dev, poison)
    _ext.check(L.lr_normals2(ptr(x, n), n, float(radius), int(max_nn), out.data_ptr(), cnt.data_ptr(), info.data_ptr(),
                             scratch.data_ptr(), scratch.numel(), _stream()))
    status, dropped, default, _ = (int(v) for v in info.cpu())
    return out[:n], cnt[:n], dict(status=status, n_dropped=dropped, n_default=default)


def symicp_dev(A, nA, B, nB, poison=None, want_log=True, T_init=None, **params):
    """lr_symicp on tensors or arrays A, nA [n0,3] (fixed), B, nB [n1,3] (moving), evaluated in float64; params: the fields of
    lr_symicp_params; T_init: a 4x4 start B -> A.  Returns (result dict with T and B_to_A as 4x4 numpy arrays, log [n_iter, 8] float64
    device tensor or None)."""
    dev = _device()
    a, b, na, nb = f64(A, dev), f64(B, dev), f64(nA, dev), f64(nB, dev)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    assert na.shape[0] == n0 and nb.shape[0] == n1, "one normal per point"
    L = _ext.lib()
    t0 = devmem.T_dev(T_init, dev)
    p = _ext.SymicpParams(T_init=ptr(t0), **params)
    res = torch.zeros(ctypes.sizeof(_ext.SymicpResult), dtype=torch.uint8, device=dev)
    log = torch.full((max(int(p.n_iter), 1), 8), math.nan, dtype=torch.float64, device=dev) if want_log else None
    scratch = devmem.scratch(L.lr_symicp_scratch_bytes(n0, n1), dev, poison)
    _ext.check(L.lr_symicp(ptr(a, n0), ptr(na, n0), n0, ptr(b, n1), ptr(nb, n1), n1, ctypes.byref(p), res.data_ptr(),
                           ptr(log), scratch.data_ptr(), scratch.numel(), _stream()))
    return as_dict(read_struct(res, _ext.SymicpResult)), log


def symmetric_icp(PC_to, PC_from, normal_radius=NORMAL_RADIUS, max_nn=NORMAL_MAX_NN, min_nb=MIN_NB, return_info=False, **params):
    """symmetric_icp.py:47 (called as symmetric_icp(A, B)): (A_to_B 4x4 float64 numpy, elapsed seconds), the matrix calc_errors compares
    with gt_motion, as BBR_F's.  Normals and neighbour counts of both clouds (lr_normals2), the points with fewer than min_nb neighbours
    dropped (their normal is the default, not a measurement), lr_symicp with PC_to fixed and PC_from moving, the inverse of its pose.
    elapsed covers all of it.  params: fields of lr_symicp_params.  return_info: (A_to_B, elapsed, result dict, log as numpy)."""
    start_time = time()
    dev = _device()
    clouds = []
    for X in (PC_to, PC_from):
        x = f64(np.ascontiguousarray(X, np.float64) if isinstance(X, np.ndarray) else X, dev)
        nrm, cnt, _ = normals_counted(x, normal_radius, max_nn)
        keep = cnt >= int(min_nb)
        clouds.append((x[keep].contiguous(), nrm[keep].contiguous()))
    (a, na), (b, nb) = clouds
    r, log = symicp_dev(a, na, b, nb, want_log=return_info, **params)
    A_to_B = r["T"]
    elapsed = time() - start_time
    return (A_to_B, elapsed, r, log.cpu().numpy()) if return_info else (A_to_B, elapsed)
