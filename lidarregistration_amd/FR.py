"""Drop-in for the reference's ``Experiments/algorithms/FR.py``: ``FR(A, B, A_feat, B_feat, args, T_gt)``.

Same positional signature and 8-tuple as FR.py:16,119.  The whole pair (NN -> filter -> RANSAC ->
refit) runs as ONE call into the C ABI (``lr_register_pair``) with no host synchronisation until the
496-byte result block is read back.
"""
import ctypes
from time import time

import numpy as np
import torch

from . import _ext
from .matching import _device, _f32, _stream, measure_inlier_ratio, workspace, workspace_for  # noqa: F401 (workspace: the tools' FR.workspace)
from .ransac import DEFAULT_SEED, PRECHECK

VOXEL_SIZE = 0.3            # FR.py:18
MODES = {"MNN": _ext.LR_MODE_MNN, "MMN": _ext.LR_MODE_MNN,      # README.md:55 spells it MMN
         "GPF": _ext.LR_MODE_GPF, "no_filter": _ext.LR_MODE_NO_FILTER}


class PointCloud:
    """Minimal stand-in for open3d.geometry.PointCloud where Open3D is not installed (the harness reads .points / calls .transform)."""

    def __init__(self, xyz):
        self.points = np.asarray(xyz, np.float64)

    def transform(self, T):
        T = np.asarray(T, np.float64)
        self.points = self.points @ T[:3, :3].T + T[:3, 3]
        return self


_O3D = []      # [module or None] once looked up


def make_open3d_point_cloud(xyz):
    """FR.py:20-23: an open3d.geometry.PointCloud over `xyz` (float64 [n,3]) -- what the reference's FR() returns as pcd0 / pcd1 and what its
    harness hands to o3d.pipelines.registration.registration_icp (test.py:185-187).  A real Open3D cloud wherever `open3d` imports; the
    stand-in above otherwise (this image has no Open3D), which serves this package's own harness and lr_icp."""
    if not _O3D:
        try:
            import open3d as o3d
            _O3D.append(o3d)
        except Exception:
            _O3D.append(None)
    o3d = _O3D[0]
    if o3d is None:
        return PointCloud(xyz)
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(np.ascontiguousarray(xyz, np.float64))
    return pcd


def pair_params(args):
    """Translate the reference's argparse namespace (Experiments/test.py:294-313) into lr_pair_params."""
    mode = getattr(args, "mode", "MNN")
    assert mode in MODES, "unknown mode"                               # FR.py:56
    codebase = getattr(args, "codebase", "GC")
    assert codebase in ("GC", "open3D"), "unknown codebase"            # FR.py:113-114
    iters = getattr(args, "iters", None)
    iters = 500 * 10 ** 3 if iters is None else int(iters)            # FR.py:65-67
    thr = 2 * VOXEL_SIZE
    local_opt = 0
    if codebase == "GC":
        sample_size = 3
        fast_rejection = getattr(args, "fast_rejection", "ELC")
        assert fast_rejection in PRECHECK, "unknown fast_rejection"               # GC_RANSAC.py:29-34: NONE | ELC | SPRT
        if float(getattr(args, "spatial_coherence_weight", 0.0)) != 0.0:
            # GC_RANSAC.py:22: the graph-cut term of the local optimisation; only weight 0 (the reference's default) is built
            raise NotImplementedError("--spatial_coherence_weight != 0 is not implemented on the HIP path")
        use_elc = PRECHECK[fast_rejection]
        conf = float(getattr(args, "GC_conf", 0.999))                  # GC_RANSAC.py:26, test.py:312
        sampler = 1 if getattr(args, "prosac", True) else 2            # test.py:308 (default True), GC_RANSAC.py:24; unique indices
        scoring = 2                                                    # MSAC at the truncated threshold (3/2 thr)^2, as GC-RANSAC scores models
        # GC_RANSAC.py:36-37; the final least squares always runs.  gcransac_python.cpp:518-521,553-556 switch the optimisation off
        # only inside the branches with a pre-verification: with --fast_rejection NONE the wrapper ignores --GC_LO False (:571-591)
        local_opt = 1 if (getattr(args, "GC_LO", True) or fast_rejection == "NONE") else 2
    else:
        sampler = 0
        scoring = 0                                                    # Open3D: fitness, then inlier RMSE
        sample_size = int(getattr(args, "ransac_n", 4))                # FR.py:134
        use_elc = True                                                 # FR.py:135 edge-length checker
        conf = float(getattr(args, "o3d_conf", 0.9995))                # FR.py:136
    rp = _ext.RansacParams(sample_size, int(use_elc), np.float32(thr * thr), iters, int(getattr(args, "seed", DEFAULT_SEED)),
                           conf, int(getattr(args, "ransac_batch", 0)), sampler, int(getattr(args, "prosac_growth", 0)),
                           int(getattr(args, "ransac_scoring", scoring)), int(getattr(args, "ransac_local_opt", local_opt)),
                           int(getattr(args, "lo_rounds", 0)), int(getattr(args, "lo_trials", 0)), int(getattr(args, "lo_max_calls", 0)),
                           int(getattr(args, "min_iters", 0)))           # 0: the defaults of gcransac_python.cpp:513-517 (lidarreg.h)
    p = _ext.PairParams()
    p.mode = MODES[mode]
    # open3D codebase: FR.py:99-111 refits over the original NN pairs; the GC codebase returns what pygcransac returns --
    # the locally optimised model after its own final least squares over the inliers among the pairs it was given
    # (GC_RANSAC.py:46-55), which is part of the RANSAC call itself (ransac.local_opt), so no refit stage follows
    p.refit = int(getattr(args, "refit", 0 if codebase == "GC" else 1))
    p.ransac = rp
    p.gpf_grid_wid = int(getattr(args, "GPF_grid_wid", 10))
    p.gpf_factor = float(getattr(args, "GPF_factor", 2.0))
    p.refit_thr2 = thr ** 2                                            # FR.py:105, fp64
    p.icp = int(getattr(args, "icp", False))                           # the harness' ICP stage (test.py:183-189), off inside FR()
    return p


def register_pair_dev(xyz0, xyz1, feats0, feats1, params, out=None, ws=None, stream=None):
    """Enqueue one pair; returns the device result buffer (uint8[496]).  No synchronisation."""
    n0, n1, d = feats0.shape[0], feats1.shape[0], feats0.shape[1]
    if ws is None:
        ws = workspace_for(n0, n1, params.ransac.iters, d)
    if out is None:
        out = torch.empty(ctypes.sizeof(_ext.PairResult), dtype=torch.uint8, device=feats0.device)
    _ext.check(_ext.lib().lr_register_pair(ws.handle, xyz0.data_ptr(), xyz1.data_ptr(), feats0.data_ptr(), feats1.data_ptr(),
                                            n0, n1, d, ctypes.byref(params), out.data_ptr(),
                                            _stream() if stream is None else stream))
    return out


def register_batch_dev(pairs, params, out=None, ws=None, stream=None):
    """Enqueue `pairs` = [(xyz0, xyz1, feats0, feats1), ...] (float32 device tensors, sizes may differ from pair to pair) as
    ONE batched call (lr_register_batch): every kernel of the path is launched once for all pairs.  Returns the device
    result buffer uint8[len(pairs), 496].  No synchronisation; `ws` must have been created with max_pairs >= len(pairs)."""
    P = len(pairs)
    d = pairs[0][2].shape[1]
    n0 = [int(p[2].shape[0]) for p in pairs]; n1 = [int(p[3].shape[0]) for p in pairs]
    if ws is None:
        ws = _ext.Workspace.for_dim(max(n0), max(n1), d, params.ransac.iters, max_pairs=P)
    if out is None:
        out = torch.empty((P, ctypes.sizeof(_ext.PairResult)), dtype=torch.uint8, device=pairs[0][2].device)
    VP, IP = ctypes.c_void_p * P, ctypes.c_int32 * P
    _ext.check(_ext.lib().lr_register_batch(ws.handle, P, VP(*[p[0].data_ptr() for p in pairs]), VP(*[p[1].data_ptr() for p in pairs]),
                                             VP(*[p[2].data_ptr() for p in pairs]), VP(*[p[3].data_ptr() for p in pairs]),
                                             IP(*n0), IP(*n1), d, ctypes.byref(params), out.data_ptr(),
                                             _stream() if stream is None else stream))
    return out


def read_result(out):
    """Device result block -> _ext.PairResult (synchronises on the copy)."""
    return _ext.PairResult.from_buffer_copy(out.cpu().numpy().tobytes())


def pair_lists(ws, n0, n_corr, dev):
    """(nn_idx1 [n0], corr_idx0 [n_corr], corr_idx1 [n_corr]) numpy arrays of the last pair on ws."""
    nn1 = torch.empty(n0, dtype=torch.int32, device=dev)
    c0 = torch.empty(n0, dtype=torch.int32, device=dev)
    c1 = torch.empty(n0, dtype=torch.int32, device=dev)
    _ext.check(_ext.lib().lr_workspace_lists(ws.handle, n0, nn1.data_ptr(), None, c0.data_ptr(), c1.data_ptr(), _stream()))
    return nn1.cpu().numpy(), c0[:n_corr].cpu().numpy(), c1[:n_corr].cpu().numpy()


_SHARE = {}          # (n0, n1 rounded up to 1024, device index, wide kernel or not) -> the second neighbour's share of the forward NN time


def share_key(n0, n1, device, dim=32):
    return ((int(n0) + 1023) // 1024, (int(n1) + 1023) // 1024, torch.device(device).index, int(dim) > 32)
last_timing = {}     # of the last FR() call: whole_path_s, forward_nn_s, second_nn_share, reference_style_s (= the returned elapsed_time)


def second_nn_share(f0, f1, ws, reps=3):
    """matching.py:12-18 times find_nn(return_2nd=False) and find_nn(return_2nd=True) on every call and bills their DIFFERENCE
    (FR.py:117).  Here the forward NN runs once per call; its second-neighbour share is measured once per cloud-size class with the
    same two calls (device events) and applied to the forward-NN time of each call."""
    n0, n1 = int(f0.shape[0]), int(f1.shape[0])
    key = share_key(n0, n1, f0.device, f0.shape[1])
    if key not in _SHARE:
        i1 = torch.empty(n0, dtype=torch.int32, device=f0.device); i2 = torch.empty_like(i1)
        st = torch.cuda.current_stream(f0.device)
        t = [0.0, 0.0]
        for k in range(2 * (reps + 1)):
            two = k % 2
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _ext.check(_ext.lib().lr_nn_top2(ws.handle, f0.data_ptr(), n0, f1.data_ptr(), n1, f0.shape[1], i1.data_ptr(),
                                              i2.data_ptr() if two else None, None, None, st.cuda_stream))
            e1.record(st); e1.synchronize()
            if k >= 2:
                t[two] += e0.elapsed_time(e1)
        _SHARE[key] = max(0.0, 1.0 - t[0] / t[1]) if t[1] > 0 else 0.0
    return _SHARE[key]


def FR(A, B, A_feat, B_feat, args, T_gt):
    """FR.py:16-119.  Returns (T, elapsed_time, pcd0, pcd1, num_pairs_init, inlier_ratio_init,
    num_pairs_filtered, inlier_ratio_filtered).  elapsed_time is what FR.py:117 bills: filter + RANSAC (+ refit) + the second
    neighbour's surcharge -- NOT the first nearest-neighbour search, which the reference treats as given (matching.py:7-11).  The
    whole device path of the call (forward NN included) is in FR.last_timing["whole_path_s"]."""
    xyz0_np = torch.as_tensor(A).detach().cpu().numpy().astype(np.float64)
    xyz1_np = torch.as_tensor(B).detach().cpu().numpy().astype(np.float64)
    pcd0, pcd1 = make_open3d_point_cloud(xyz0_np), make_open3d_point_cloud(xyz1_np)          # FR.py:28-29
    dev = _device()
    xyz0, xyz1 = _f32(A), _f32(B)
    f0, f1 = _f32(A_feat), _f32(B_feat)
    params = pair_params(args)
    params.icp = 0                     # FR() returns the registration only (FR.py:119); ICP is the harness' stage (test.py:183-189)
    n0, n1 = f0.shape[0], f1.shape[0]
    ws = workspace_for(n0, n1, params.ransac.iters, f0.shape[1])

    share = second_nn_share(f0, f1, ws)
    ws.timing(True)
    torch.cuda.synchronize(dev)
    start_time = time()
    out = register_pair_dev(xyz0, xyz1, f0, f1, params, ws=ws)
    r = read_result(out)                                   # the only device->host sync of the pair
    whole = time() - start_time
    ms, _ = ws.stage_times()                               # the library's own events of this call: [whole call, forward NN, ...]
    ws.timing(False)
    billed_out = ms[1] * 1e-3 * (1.0 - share)              # the first-neighbour part of the forward NN
    elapsed_time = max(whole - billed_out, 0.0)
    last_timing.clear()
    last_timing.update(whole_path_s=whole, forward_nn_s=ms[1] * 1e-3, second_nn_share=share, reference_style_s=elapsed_time)

    T = np.array(r.T[:], np.float64).reshape(4, 4)
    if r.status != 0:
        T = np.eye(4)                                      # GC_RANSAC.py:51-52: failure -> identity

    # statistics outside the timed region, as FR.py:43,61
    idx1, ci0, ci1 = pair_lists(ws, n0, int(r.n_corr), dev)
    num_pairs_init = n0
    inlier_ratio_init = measure_inlier_ratio(np.arange(n0), idx1, pcd0, pcd1, T_gt, VOXEL_SIZE)
    num_pairs_filtered = int(r.n_corr)
    inlier_ratio_filtered = measure_inlier_ratio(ci0, ci1, pcd0, pcd1, T_gt, VOXEL_SIZE)
    return T, elapsed_time, pcd0, pcd1, num_pairs_init, inlier_ratio_init, num_pairs_filtered, inlier_ratio_filtered
