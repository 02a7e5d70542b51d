"""Voxel-grid down-sampling (one centroid per voxel), the pair overlap measure, the exact nearest neighbour and the refinement of a
ground-truth motion on the GPU: the cloud-level primitives of the reference's balanced-set generator
(BalancedDatasetGenerator/GenerateBalancedSet.py) and of its refinement tester (FCGF_FAST/net/refinement_tester.py), on top of
lr_voxel_mean / lr_overlap / lr_overlap_batch (csrc/lr_overlap.hip) and lr_nn3 / lr_refine_z (csrc/lr_nn3.hip).

Two different operations carry similar names here.  ``voxel_down_sample`` (this module) is Open3D's: every occupied voxel is replaced by
the centroid of its points.  ``voxel.voxel_downsample`` is MinkowskiEngine's de-duplication: the first point of every cell is kept.
The contract is stated in include/lidarreg.h and DESIGN.md §12; what of it is recalled from Open3D rather than pinned is marked there.
No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _ext, devmem
from .devmem import T_dev, as_dict, f64, ptr, read_struct
from .matching import _device, _stream

OVERLAP_VOXEL = 1.0         # GenerateBalancedSet.py:171
MAX_PAIRS = 64              # pairs per lr_overlap_batch call


def voxel_mean_dev(X, voxel_size, T=None, poison=None):
    """lr_voxel_mean of X [n,3] (evaluated in float64), optionally moved by T (4x4) first.  Returns a dict of device tensors trimmed to
    the rows -- cent [rows,3] float64, cent_f32 [rows,3] float32, counts, first (int32) -- and rows, dropped, status (ints).
    poison: fill the scratch with this byte first (test hook)."""
    dev = _device()
    x = f64(X, dev)
    n = int(x.shape[0])
    L = _ext.lib()
    Td = T_dev(T, dev)
    m = max(n, 1)
    cent = torch.empty((m, 3), dtype=torch.float64, device=dev); cent32 = torch.empty((m, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(m, dtype=torch.int32, device=dev); first = torch.empty(m, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = devmem.scratch(L.lr_voxel_mean_scratch_bytes(n), dev, poison)
    _ext.check(L.lr_voxel_mean(ptr(x, n), n, ptr(Td), float(voxel_size), cent.data_ptr(), cent32.data_ptr(), counts.data_ptr(), first.data_ptr(),
                               info.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    rows, dropped, status, _ = (int(v) for v in info.cpu())
    return dict(cent=cent[:rows], cent_f32=cent32[:rows], counts=counts[:rows], first=first[:rows], rows=rows, dropped=dropped, status=status)


def voxel_down_sample(X, voxel_size, T=None, return_counts=False):
    """Open3D's ``PointCloud.voxel_down_sample`` as GenerateBalancedSet.py:143-147 and refinement_tester.py:69-73 call it: the centroid of
    every occupied voxel, float64 device tensor [rows,3], rows in scan order of each voxel's first point (Open3D's own row order is
    unspecified).  T (4x4), if given, moves the cloud first.  Points with a non-finite coordinate are dropped.  Not to be confused with
    ``voxel.voxel_downsample``, which keeps the first point of every cell (MinkowskiEngine)."""
    r = voxel_mean_dev(X, voxel_size, T)
    if r["status"] == 2:
        raise _ext.LidarRegError("voxel_down_sample: the cloud spans 2^21 voxels or more on an axis")
    return (r["cent"], r["counts"]) if return_counts else r["cent"]


def overlap_dev(A, B, T=None, voxel_size=OVERLAP_VOXEL, radius=0.0, poison=None):
    """lr_overlap on one pair: A [n0,3] (moved by T, 4x4, if given) against B [n1,3].  Returns the lr_overlap_result as a dict."""
    dev = _device()
    a, b = f64(A, dev), f64(B, dev)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    L = _ext.lib()
    Td = T_dev(T, dev)
    p = _ext.OverlapParams(voxel_size=float(voxel_size), radius=float(radius))
    res = torch.zeros((1, ctypes.sizeof(_ext.OverlapResult)), dtype=torch.uint8, device=dev)
    scratch = devmem.scratch(L.lr_overlap_scratch_bytes(n0, n1), dev, poison)
    _ext.check(L.lr_overlap(ptr(a, n0), n0, ptr(b, n1), n1, ptr(Td), ctypes.byref(p), res.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    return as_dict(read_struct(res, _ext.OverlapResult))


def overlap_batch_dev(pairs, voxel_size=OVERLAP_VOXEL, radius=0.0, poison=None):
    """ONE lr_overlap_batch call over `pairs`: a list of up to 64 (A, B) or (A, B, T) -- the candidate loop of
    GenerateBalancedSet.py:321-371 (one source frame against many targets).  Returns the per-pair result dicts."""
    dev = _device()
    npairs = len(pairs)
    L = _ext.lib()
    As = [f64(pr[0], dev) for pr in pairs]; Bs = [f64(pr[1], dev) for pr in pairs]
    Ts = [T_dev(pr[2] if len(pr) > 2 else None, dev) for pr in pairs]
    n0 = [int(a.shape[0]) for a in As]; n1 = [int(b.shape[0]) for b in Bs]
    ptrs = lambda ts, ns: (ctypes.c_void_p * npairs)(*[ptr(t, n) for t, n in zip(ts, ns)])
    tp = (ctypes.c_void_p * npairs)(*[ptr(t) for t in Ts])
    p = _ext.OverlapParams(voxel_size=float(voxel_size), radius=float(radius))
    res = torch.zeros((max(npairs, 1), ctypes.sizeof(_ext.OverlapResult)), dtype=torch.uint8, device=dev)
    per = L.lr_overlap_scratch_bytes(max(n0, default=0), max(n1, default=0))
    scratch = devmem.scratch(per * npairs, dev, poison)
    _ext.check(L.lr_overlap_batch(npairs, ptrs(As, n0), (ctypes.c_int32 * npairs)(*n0), ptrs(Bs, n1), (ctypes.c_int32 * npairs)(*n1), tp,
                                  ctypes.byref(p), res.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    return [as_dict(read_struct(res, _ext.OverlapResult, k)) for k in range(npairs)]


def _fractions(r, who):
    if r["status"] == 2:
        raise _ext.LidarRegError(f"{who}: a cloud spans 2^21 voxels or more on an axis")
    return r["frac"], r["frac_sym"]          # status 1 (an empty cloud): (0.0, 0.0), where the reference divides by zero


def overlap_fraction(A, B, voxel_size=OVERLAP_VOXEL):
    """GenerateBalancedSet.py:155-179: (overlap_frac, overlap_frac_symmetric) -- the share of A's voxels (after down-sampling both clouds at
    `voxel_size`, 1 m there) with a voxel centre of B closer than sqrt(2) voxel, and the minimum of that and the same count over B's
    voxels (the reference's own "symmetric": one numerator)."""
    return _fractions(overlap_dev(A, B, None, voxel_size), "overlap_fraction")


def calc_GT_overlap(A, B, GT_mot, return_both=False, overlap_measure="symmetric"):
    """GenerateBalancedSet.py:186-205: the overlap of A moved by GT_mot with B.  return_both: both measures; otherwise the one
    `overlap_measure` names ('src_to_tgt' | 'symmetric'; config.overlap_measure there)."""
    frac, sym = _fractions(overlap_dev(A, B, GT_mot, OVERLAP_VOXEL), "calc_GT_overlap")
    if return_both:
        return frac, sym
    assert overlap_measure in ("src_to_tgt", "symmetric"), "overlap_measure should be set to either 'src_to_tgt' or 'symmetric'"
    return frac if overlap_measure == "src_to_tgt" else sym


def refine_inputs(GT_mot_orig, A, B, downsample=True, voxel_size=0.3):
    """What refine_motion hands to the ICP (GenerateBalancedSet.py:233-243): (a moved by GT_mot_orig, b) as float32 device clouds; the
    down-sampling and the transform are float64."""
    dev = _device()
    a = voxel_down_sample(A, voxel_size) if downsample else f64(A, dev)
    b = voxel_down_sample(B, voxel_size) if downsample else f64(B, dev)
    M = np.ascontiguousarray(GT_mot_orig, np.float64)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    a_corr = torch.stack([((float(M[r, 0]) * x + float(M[r, 1]) * y) + float(M[r, 2]) * z) + float(M[r, 3]) for r in range(3)], dim=1)
    return a_corr.float().contiguous(), b.float().contiguous()


def refine_motion(GT_mot_orig, A, B, downsample=True, voxel_size=0.3, refine_GT_Z_only=False):
    """GenerateBalancedSet.py:220-246, the ICP branch: both clouds down-sampled (Open3D's voxel grid), `a` moved by GT_mot_orig, point-to-point
    ICP from the identity with max distance 2 voxel_size and Open3D's default criteria (lr_icp), and icp_mot @ GT_mot_orig returned
    (4x4 float64 numpy).  The Z-only variant (:257-) is not reached through this flag: refine_GT(..., z_only=True) dispatches to
    refine_motion_Z_only."""
    if refine_GT_Z_only:
        raise NotImplementedError("refine_motion: this is the ICP branch; the Z-only refinement is refine_GT(..., z_only=True) / refine_motion_Z_only")
    from .ransac import icp_dev
    a_corr, b = refine_inputs(GT_mot_orig, A, B, downsample, voxel_size)
    icp_mot, _ = icp_dev(a_corr, b, np.eye(4), max_dist=2.0 * float(voxel_size))
    return icp_mot @ np.ascontiguousarray(GT_mot_orig, np.float64)


def nearest_neighbour_dev(A, B, cell=0.0, poison=None):
    """lr_nn3: for every point of A [n0,3] its exact nearest neighbour among B [n1,3] (float64, unbounded; the lowest index on equal
    distance).  Returns a dict: dist [n0] float64 and idx [n0] int32 device tensors (idx -1 / dist inf: a non-finite query, or no finite
    target), status (1: no finite target), n0_dropped, n1_dropped, n_far (queries resolved by the second phase).  cell: edge of the
    search grid, 0 = automatic; the result does not depend on it."""
    dev = _device()
    a, b = f64(A, dev), f64(B, dev)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    L = _ext.lib()
    idx = torch.empty(max(n0, 1), dtype=torch.int32, device=dev); dist = torch.empty(max(n0, 1), dtype=torch.float64, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    p = _ext.Nn3Params(cell=float(cell))
    scratch = devmem.scratch(L.lr_nn3_scratch_bytes(n0, n1), dev, poison)
    _ext.check(L.lr_nn3(ptr(a, n0), n0, ptr(b, n1), n1, ctypes.byref(p), idx.data_ptr(), dist.data_ptr(), info.data_ptr(), scratch.data_ptr(),
                        scratch.numel(), _stream()))
    status, d0, d1, far = (int(v) for v in info.cpu())
    return dict(dist=dist[:n0], idx=idx[:n0], status=status, n0_dropped=d0, n1_dropped=d1, n_far=far)


def nearest_neighbour(A, B):
    """GenerateBalancedSet.py:149-153 `NN`: (d float64 [n0], inds int64 [n0]) as numpy arrays -- cKDTree(B).query(A, k=1).  Where the
    reference raises on non-finite input, such a query gets (inf, -1) and such a target point is never a neighbour."""
    r = nearest_neighbour_dev(A, B)
    return r["dist"].cpu().numpy(), r["idx"].cpu().numpy().astype(np.int64)


def refine_z_dev(A, B, T=None, xy_gate=0.3, max_repeats=10, min_change=1e-6, cell=0.0, poison=None):
    """lr_refine_z: A [n0,3] (moved by T, 4x4, if given) against B [n1,3], the clouds as given.  Returns the lr_refine_z_result as a dict."""
    dev = _device()
    a, b = f64(A, dev), f64(B, dev)
    n0, n1 = int(a.shape[0]), int(b.shape[0])
    L = _ext.lib()
    Td = T_dev(T, dev)
    p = _ext.RefineZParams(xy_gate=float(xy_gate), max_repeats=int(max_repeats), min_change=float(min_change), cell=float(cell))
    res = torch.zeros((1, ctypes.sizeof(_ext.RefineZResult)), dtype=torch.uint8, device=dev)
    scratch = devmem.scratch(L.lr_refine_z_scratch_bytes(n0, n1), dev, poison)
    _ext.check(L.lr_refine_z(ptr(a, n0), n0, ptr(b, n1), n1, ptr(Td), ctypes.byref(p), res.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    return as_dict(read_struct(res, _ext.RefineZResult))


def refine_motion_Z_only(raw_mot, A, B, voxel_size, return_info=False):
    """GenerateBalancedSet.py:257-291: raw_mot with [2,3] + dz, dz from the IRLS over the z distances of the nearest-neighbour pairs
    that lie within voxel_size in xy (lr_refine_z, at most 10 repeats, stop below 1e-6).  The clouds are used as given.  Returns a NEW
    4x4 float64 numpy matrix (the reference adds dz into its caller's array); return_info: (matrix, result block as a dict).  Status 1
    (no valid pair) and 2 (half the pairs coincide in z), where the reference returns NaN, leave dz as accumulated so far."""
    M = np.array(raw_mot, dtype=np.float64, copy=True).reshape(4, 4)
    r = refine_z_dev(A, B, M, xy_gate=float(voxel_size))
    M[2, 3] += r["dz"]
    return (M, r) if return_info else M


def refine_GT(GT_mot_orig, A, B, downsample=True, voxel_size=0.3, z_only=False):
    """GenerateBalancedSet.py:233-246, both branches (z_only = config.refine_GT_Z_only, True for the reference's NuScenes and
    LyftLEVEL5): the clouds down-sampled (Open3D's voxel grid) unless downsample is False, then refine_motion_Z_only on the float64
    centroids, or the ICP branch (refine_motion: float32 clouds into lr_icp)."""
    if not z_only:
        return refine_motion(GT_mot_orig, A, B, downsample, voxel_size)
    dev = _device()
    a = voxel_down_sample(A, voxel_size) if downsample else f64(A, dev)
    b = voxel_down_sample(B, voxel_size) if downsample else f64(B, dev)
    return refine_motion_Z_only(GT_mot_orig, a, b, voxel_size)


def refine_session(clouds, raw_motions, voxel_size=0.3, z_only=False):
    """GenerateBalancedSet.py:293-319 `refine_session_GT`, the host loop: clouds[i] [n_i,3], raw_motions[i] the 4x4 motion of frame i to
    frame i + 1.  Every frame is down-sampled once; returns the list of positions (4x4 float64 numpy), positions[0] the identity."""
    assert len(raw_motions) == len(clouds) - 1, "one raw motion per consecutive pair of frames"
    B_ = voxel_down_sample(clouds[0], voxel_size)
    B_pos = np.eye(4, dtype=np.float64)
    positions = [B_pos]
    for i in range(1, len(clouds)):
        A_, A_pos = B_, B_pos
        B_ = voxel_down_sample(clouds[i], voxel_size)
        mot = refine_GT(raw_motions[i - 1], A_, B_, downsample=False, voxel_size=voxel_size, z_only=z_only)
        B_pos = mot @ A_pos
        positions.append(B_pos)
    return positions
