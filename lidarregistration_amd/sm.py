"""Spectral-matching back end (``--algo SM``) on top of liblidarreg.so: lr_sm / lr_sm_batch (csrc/lr_sm.hip).

``SM`` keeps the reference's call shape (Experiments/baseline_scripts/baseline_3DMatch.py:19-53); ``eval_pairs`` is the batched engine of
``python -m test --algo SM``: per window, the correspondences come pair by pair from the existing single-pair entry points (mutual nearest
neighbours, or the grid filter with ``--mode GPF``; spread over streams), their xyz are gathered, and ONE lr_sm_batch call solves the
window; ICP follows through lr_icp.  The contract the solver implements is stated in include/lidarreg.h and DESIGN.md §11.
"""
import ctypes
import time

import numpy as np
import torch

from . import _ext, harness
from .matching import _f32, _stream
from .teaser import _icp, _scratch

RESULT_BYTES = ctypes.sizeof(_ext.SmResult)
INLIER_THRESHOLD = 0.6    # baseline_KITTI.py:51 (= 2 * VOXEL_SIZE, the CLI's threshold)


def params(**kw):
    """lr_sm_params: the reference's settings unless overridden (iterations, inlier_threshold, top_ratio)."""
    return _ext.SmParams(**kw)


def _result(buf, k=0):
    return _ext.SmResult.from_buffer_copy(buf[k * RESULT_BYTES:(k + 1) * RESULT_BYTES].cpu().numpy().tobytes())


def _info(r):
    return dict(status=r.status, K=r.K, m=r.m, weight_sum=r.weight_sum)


def sm_batch_dev(srcs, tgts, ms=None, m_devs=None, poison=None, **kw):
    """lr_sm_batch over len(srcs) pairs ([M_k,3] float32 each, any M_k incl. 0).  ms: the counts passed as m (default: the rows);
    m_devs: optional device int32 tensors with a smaller live count.  Returns [(T 4x4, info dict, labels uint8 [m], eig float32 [m])]
    and the device time of the call in ms.  poison: fill the scratch with this byte first (test hook)."""
    n = len(srcs)
    srcs = [_f32(s).reshape(-1, 3) for s in srcs]
    tgts = [_f32(t).reshape(-1, 3) for t in tgts]
    dev = srcs[0].device
    ms = [int(s.shape[0]) for s in srcs] if ms is None else [int(v) for v in ms]
    scratch = _scratch(_ext.lib().lr_sm_scratch_bytes(max(ms)) * n, dev)
    if poison is not None:
        scratch.fill_(int(poison))
    res = torch.zeros(RESULT_BYTES * n, dtype=torch.uint8, device=dev)
    eigs = [torch.full((max(m, 1),), -1.0, dtype=torch.float32, device=dev) for m in ms]
    labels = [torch.full((max(m, 1),), 255, dtype=torch.uint8, device=dev) for m in ms]
    V = ctypes.c_void_p * n
    p = params(**kw)
    md = None if m_devs is None else V(*[None if t is None else t.data_ptr() for t in m_devs])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    _ext.check(_ext.lib().lr_sm_batch(n, V(*[s.data_ptr() for s in srcs]), V(*[t.data_ptr() for t in tgts]), (ctypes.c_int32 * n)(*ms), md,
                                       ctypes.byref(p), res.data_ptr(), V(*[e.data_ptr() for e in eigs]), V(*[l.data_ptr() for l in labels]),
                                       scratch.data_ptr(), scratch.numel(), _stream()))
    ev1.record()
    torch.cuda.current_stream().synchronize()
    out = []
    for k in range(n):
        r = _result(res, k)
        out.append((np.array(r.T[:], np.float64).reshape(4, 4), _info(r), labels[k][:ms[k]].cpu().numpy(), eigs[k][:ms[k]].cpu().numpy()))
    return out, ev0.elapsed_time(ev1)


def sm_dev(src, tgt, m_dev=None, poison=None, **kw):
    """lr_sm on one correspondence set: (T 4x4 float64, info dict, labels uint8 [m], eig float32 [m])."""
    src, tgt = _f32(src).reshape(-1, 3), _f32(tgt).reshape(-1, 3)
    m = int(src.shape[0])
    scratch = _scratch(_ext.lib().lr_sm_scratch_bytes(m), src.device)
    if poison is not None:
        scratch.fill_(int(poison))
    res = torch.zeros(RESULT_BYTES, dtype=torch.uint8, device=src.device)
    eig = torch.full((max(m, 1),), -1.0, dtype=torch.float32, device=src.device)
    labels = torch.full((max(m, 1),), 255, dtype=torch.uint8, device=src.device)
    p = params(**kw)
    _ext.check(_ext.lib().lr_sm(src.data_ptr(), tgt.data_ptr(), m, None if m_dev is None else m_dev.data_ptr(), ctypes.byref(p), res.data_ptr(),
                                 eig.data_ptr(), labels.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()))
    r = _result(res)
    return np.array(r.T[:], np.float64).reshape(4, 4), _info(r), labels[:m].cpu().numpy(), eig[:m].cpu().numpy()


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
    """--algo SM over `indices` of `source`.  Returns a harness.EvalRun.  Column 9 = the pair's share of its window's solve (device time
    of the lr_sm_batch call split evenly); the NN / filter time is not billed (as for --algo TEASER)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    n = len(indices)
    stats = np.full((n, 22), np.nan)
    Ts = np.tile(np.eye(4), (n, 1, 1))
    whole = np.zeros(n)
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(1, nstreams))]
    wss = [None] * batch
    tot = dict(data_s=0.0, registration_s=0.0, icp_s=0.0, stats_s=0.0, pairs=n)
    use_icp = getattr(args, "icp", True)
    kw = solver_kw(args)
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
            out, ms = sm_batch_dev(srcs, tgts, **kw)
            t2 = time.time()
            for j, r in enumerate(rows):
                Ts[r] = out[j][0]
                whole[r] = ms * 1e-3 / len(rows)
                p = pairs[j]
                harness.write_row(stats, r, Ts[r], p["T_gt"], whole[r], (t1 - t0) / len(rows), p["feats0"].shape[0], counts[j], source.ids(indices[r]),
                                  icp=_icp(wss[j], p, Ts[r], dev) if use_icp else None)
            tot["data_s"] += t1 - t0; tot["registration_s"] += t2 - t1; tot["icp_s"] += time.time() - t2
            if verbose:
                print(f"{time.strftime('%m/%d %H:%M:%S')} Finished pair:{rows[-1]}/{n}", flush=True)
        torch.cuda.synchronize(dev)
    finally:
        for ws in wss:
            if ws is not None:
                ws.close()
    return harness.EvalRun(stats, Ts, whole, tot, None)
