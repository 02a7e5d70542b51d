"""TEASER++ back end (``--algo TEASER``) on top of liblidarreg.so: lr_teaser / lr_teaser_batch (csrc/lr_teaser.hip).

``TEASER`` keeps the reference's call shape (Experiments/algorithms/TEASER_plus_plus.py:101-126); ``eval_pairs`` is the batched
engine of ``python -m test --algo TEASER``: per window, the NN search and the BB_first grid filter run pair by pair on the existing
single-pair entry points (spread over streams), the correspondences' xyz are gathered, and ONE lr_teaser_batch call solves the
window; ICP follows through lr_icp.  The contract the solver implements is stated in include/lidarreg.h and DESIGN.md §10.
"""
import ctypes
import time

import numpy as np
import torch

from . import _ext, harness
from .matching import _f32, _stream

RESULT_BYTES = ctypes.sizeof(_ext.TeaserResult)
VOXEL_SIZE = 0.3          # TEASER_plus_plus.py: noise_bound = VOXEL_SIZE


def params(**kw):
    """lr_teaser_params: the reference's settings unless overridden (noise_bound, cbar2, kcore_threshold, gnc_factor,
    max_iterations, cost_threshold, node_budget, time_budget_ms)."""
    return _ext.TeaserParams(**kw)


def _scratch(nbytes, device):
    # 256-byte aligned device scratch (torch's allocator aligns to 512)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _result(buf, k=0):
    return _ext.TeaserResult.from_buffer_copy(buf[k * RESULT_BYTES:(k + 1) * RESULT_BYTES].cpu().numpy().tobytes())


def _info(r):
    return dict(status=r.status, K=r.K, exact=r.exact, max_core=r.max_core, lb=r.lb, nodes=int(r.nodes), gnc_iters=r.gnc_iters,
                n_rot_inliers=r.n_rot_inliers, n_trans_inliers=r.n_trans_inliers)


def teaser_batch_dev(srcs, tgts, ms=None, m_devs=None, poison=None, **kw):
    """lr_teaser_batch over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0).  ms: live counts passed as m (default: the
    rows); m_devs: optional device int32 tensors with a smaller live count.  Returns [(T 4x4, info dict, clique int array)] and the
    device time of the call in ms.  poison: fill the scratch with this byte first (test hook)."""
    n = len(srcs)
    srcs = [_f32(s).reshape(-1, 3) for s in srcs]
    tgts = [_f32(t).reshape(-1, 3) for t in tgts]
    dev = srcs[0].device
    ms = [int(s.shape[0]) for s in srcs] if ms is None else [int(v) for v in ms]
    per = _ext.lib().lr_teaser_scratch_bytes(max(ms))
    scratch = _scratch(per * n, dev)
    if poison is not None:
        scratch.fill_(int(poison))
    res = torch.zeros(RESULT_BYTES * n, dtype=torch.uint8, device=dev)
    cliques = [torch.full((max(m, 1),), -1, dtype=torch.int32, device=dev) for m in ms]
    V = ctypes.c_void_p * n
    p = params(**kw)
    md = None if m_devs is None else V(*[None if t is None else t.data_ptr() for t in m_devs])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    _ext.check(_ext.lib().lr_teaser_batch(n, V(*[s.data_ptr() for s in srcs]), V(*[t.data_ptr() for t in tgts]), (ctypes.c_int32 * n)(*ms),
                                           md, ctypes.byref(p), res.data_ptr(), V(*[c.data_ptr() for c in cliques]),
                                           scratch.data_ptr(), scratch.numel(), _stream()))
    ev1.record()
    torch.cuda.current_stream().synchronize()
    out = []
    for k in range(n):
        r = _result(res, k)
        out.append((np.array(r.T[:], np.float64).reshape(4, 4), _info(r), cliques[k][:r.K].cpu().numpy().astype(np.int64)))
    return out, ev0.elapsed_time(ev1)


def teaser_dev(src, tgt, m_dev=None, poison=None, **kw):
    """lr_teaser on one correspondence set: (T 4x4 float64, info dict, clique ascending int64 array)."""
    src, tgt = _f32(src).reshape(-1, 3), _f32(tgt).reshape(-1, 3)
    m = int(src.shape[0])
    scratch = _scratch(_ext.lib().lr_teaser_scratch_bytes(m), src.device)
    if poison is not None:
        scratch.fill_(int(poison))
    res = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device=src.device)
    clique = torch.full((max(m, 1),), -1, dtype=torch.int32, device=src.device)
    p = params(**kw)
    _ext.check(_ext.lib().lr_teaser(src.data_ptr(), tgt.data_ptr(), m, None if m_dev is None else m_dev.data_ptr(), ctypes.byref(p),
                                     res.data_ptr(), clique.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    r = _result(res)
    return np.array(r.T[:], np.float64).reshape(4, 4), _info(r), clique[:r.K].cpu().numpy().astype(np.int64)


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
    ws = _ext.Workspace(F0.shape[0], F1.shape[0], F0.shape[1], 1)
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
    """--algo TEASER over `indices` of `source`.  Returns a harness.EvalRun with totals and `exact`.  Column 9 = the pair's share of
    its window's solve (device time of the lr_teaser_batch call split evenly) + the second neighbour's surcharge (0); the NN / GPF
    time is not billed (TEASER_plus_plus.py:109-123)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    n = len(indices)
    stats = np.full((n, 22), np.nan)
    Ts = np.tile(np.eye(4), (n, 1, 1))
    exact = np.ones(n, np.int32)
    whole = np.zeros(n)
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(1, nstreams))]
    wss = [None] * batch
    tot = dict(data_s=0.0, registration_s=0.0, icp_s=0.0, stats_s=0.0, pairs=n)
    use_icp = getattr(args, "icp", True)
    # whatever ends the loop, every workspace is released on the way out (harness.eval_pairs)
    try:
        for w0 in range(0, n, batch):
            rows = list(range(w0, min(n, w0 + batch)))
            t0 = time.time()
            pairs = [source.get_dev(indices[r], dev) for r in rows]
            torch.cuda.synchronize(dev)
            t1 = time.time()
            corr = []
            for j, p in enumerate(pairs):
                s = streams[j % len(streams)]
                harness.slot_workspace(wss, j, p["feats0"].shape[0], p["feats1"].shape[0], p["feats0"].shape[1], 1, headroom=1.25, sync=dev)
                with torch.cuda.stream(s):
                    corr.append(correspondences_dev(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], args, wss[j], s.cuda_stream))
            torch.cuda.synchronize(dev)
            counts = [int(v) for v in torch.stack([c[2][0] for c in corr]).cpu()]
            srcs = [p["xyz0"][c[0][:m].long()] for p, c, m in zip(pairs, corr, counts)]
            tgts = [p["xyz1"][c[1][:m].long()] for p, c, m in zip(pairs, corr, counts)]
            out, ms = teaser_batch_dev(srcs, tgts, time_budget_ms=_budget_ms(args))
            t2 = time.time()
            for j, r in enumerate(rows):
                T, info, _ = out[j]
                exact[r] = info["exact"]
                if getattr(args, "mode", None) == "FAIL_TOLERANT" and not info["exact"]:
                    T = np.eye(4)
                Ts[r] = T
                whole[r] = ms * 1e-3 / len(rows)
                p = pairs[j]
                harness.write_row(stats, r, T, p["T_gt"], whole[r], (t1 - t0) / len(rows), p["feats0"].shape[0], counts[j], source.ids(indices[r]),
                                  icp=_icp(wss[j], p, Ts[r], dev) if use_icp else None)
            tot["data_s"] += t1 - t0; tot["registration_s"] += t2 - t1; tot["icp_s"] += time.time() - t2
            if verbose:
                print(f"{time.strftime('%m/%d %H:%M:%S')} Finished pair:{rows[-1]}/{n}", flush=True)
        torch.cuda.synchronize(dev)
    finally:
        for ws in wss:
            if ws is not None:
                ws.close()
    return harness.EvalRun(stats, Ts, whole, tot, exact)


def _icp(ws, p, T, dev):
    """lr_icp from T on the current stream, timed by its own events: (T_icp 4x4, seconds)."""
    Tin = torch.from_numpy(np.ascontiguousarray(T.reshape(16))).to(dev)
    T_icp = torch.empty(16, dtype=torch.float64, device=dev)
    res_icp = torch.empty(ctypes.sizeof(_ext.IcpResult), dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _ext.check(_ext.lib().lr_icp(ws.handle, p["xyz0"].data_ptr(), p["xyz0"].shape[0], p["xyz1"].data_ptr(), p["xyz1"].shape[0], Tin.data_ptr(),
                                 2 * VOXEL_SIZE, 30, 1e-6, 1e-6, T_icp.data_ptr(), res_icp.data_ptr(), _stream()))
    e1.record(); e1.synchronize()
    return T_icp.cpu().numpy().reshape(4, 4), e0.elapsed_time(e1) * 1e-3
