"""The batched Python layer of Deep Global Registration on the GPU: InlierNet.weights_batch, DGRTail.register_batch and DGR.register_batch
against their one-pair forms, bit for bit.  Thin inlier widths and random FCGF weights: the transforms mean nothing, what is pinned is that
a pair gets in a batch what it gets alone, on the refinement path, on the safeguard (the weight sum below the pair's OWN threshold, no live
row, a pair the network refused) and on the drop path of a set above the refinement's limit."""
import functools

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, dgr, fcgf, synth
from tests import dgr6_cpu, dgr_cases, fcgf_cases

pytestmark = pytest.mark.gpu
THIN = dgr6_cpu.THIN


@functools.lru_cache(maxsize=None)
def stages():
    return dgr6_cpu.random_stages(THIN, seed=0)


@functools.lru_cache(maxsize=None)
def model():
    return dgr.InlierNet.from_stages(stages())


@functools.lru_cache(maxsize=None)
def fcgf_model():
    return fcgf.FCGF.from_state_dict(fcgf_cases.make_state_dict(0, 5), 5)


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_weights_batch_equals_weights_per_pair_and_reports_a_refused_pair():
    rng = np.random.default_rng(4)
    sets = []
    for n0, n1 in ((300, 280), (1, 5), (150, 400)):
        xyz0, xyz1 = rng.uniform(-3, 3, (n0, 3)), rng.uniform(-3, 3, (n1, 3))
        _, k0 = np.unique(np.floor(xyz0 / 0.3).astype(np.int64), axis=0, return_index=True)
        xyz0 = xyz0[np.sort(k0)]
        sets.append((xyz0, xyz1, np.arange(len(xyz0)), rng.integers(0, n1, len(xyz0))))
    m = model()
    ws, statuses = m.weights_batch(*zip(*sets), voxel_size=0.3)
    assert statuses == [0, 0, 0] and [i["status"] for i in m.last_info] == [0, 0, 0]
    for k, s in enumerate(sets):
        want = m.weights(*s, voxel_size=0.3)
        assert ws[k].dtype == torch.float32 and ws[k].device == want.device and same_bytes(host(ws[k]), host(want)), k
    # a duplicate correspondence cell in the middle pair: `weights` raises, the batch reports it and goes on
    x0, x1, i0, i1 = sets[2]
    dup = (np.concatenate([x0, x0[:1]]), x1, np.arange(len(x0) + 1), np.concatenate([i1, i1[:1]]))
    with pytest.raises(_ext.LidarRegError, match="status 2"):
        m.weights(*dup, voxel_size=0.3)
    ws2, statuses = m.weights_batch(*zip(sets[0], dup, sets[1]), voxel_size=0.3)
    assert statuses == [0, 2, 0] and (host(ws2[1]) == np.float32(0.5)).all()
    assert same_bytes(host(ws2[0]), host(ws[0])) and same_bytes(host(ws2[2]), host(ws[1]))


def test_register_batch_of_the_tail_equals_register_on_every_path():
    """Five ragged planted sets.  0, 1: the weights carry the refinement.  2: M = 5 000 > 4 000, so its threshold is 250, not the others' 200:
    499 live rows of weight 0.5 sum to 249.5, just below ITS threshold and above theirs.  3: no live row.  4: refused by the network."""
    cases = [dgr_cases.planted(11, 600, 0.6, 0.02, 0.3), dgr_cases.planted(12, 900, 0.7, 0.05, -0.2), dgr_cases.planted(13, 5000, 0.5, 0.02, 0.1),
             dgr_cases.planted(14, 300, 0.5, 0.02, 0.4), dgr_cases.planted(15, 400, 0.6, 0.02, -0.3)]
    weights = [c["weights"].copy() for c in cases]
    weights[2] = np.zeros(5000, np.float32); weights[2][np.nonzero(cases[2]["inlier"])[0][:499]] = 0.5
    weights[3] = np.zeros(300, np.float32)
    weights[4] = np.full(400, 0.5, np.float32)                               # sigmoid(0): what a refused pair's zero logits give
    srcs, tgts = [c["src"] for c in cases], [c["tgt"] for c in cases]
    ar = [np.arange(len(s)) for s in srcs]
    tail = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=0.05)
    got = tail.register_batch(srcs, tgts, ar, ar, weights, inlier_statuses=[0, 0, 0, 0, 2])
    infos = tail.last
    assert isinstance(infos, list) and [i["path"] for i in infos] == ["refinement", "refinement", "safeguard", "safeguard", "safeguard"]
    assert infos[2]["w1"] == 249.5 and infos[2]["status"] == 2 and 200.0 <= infos[2]["w1"] < tail.wsum_threshold(5000) == 250.0
    assert infos[3]["status"] == 1 and infos[3]["L"] == 0
    assert infos[4]["inlier_status"] == 2 and all("inlier_status" not in i for i in infos[:4])
    one = dgr.DGRTail(voxel_size=0.3, clip_weight_thresh=0.05)
    for k in range(5):
        w = weights[k] if k != 4 else np.zeros(400, np.float32)                # the refused pair alone: the safeguard on its correspondences
        want = one.register(srcs[k], tgts[k], ar[k], ar[k], weights=w)
        assert one.last["path"] == infos[k]["path"], k
        assert same_bytes(got[k]["base"], want["base"]) and same_bytes(got[k]["w_icp"], want["w_icp"]), k
        if k < 4:
            for f in ("status", "iterations", "break_count", "loss", "L", "w1"):
                assert infos[k][f] == one.last[f], (k, f)
    assert np.abs(got[0]["base"] - cases[0]["T_gt"]).max() < 0.5                # (the refinement did refine)
    # with the first pair's count as every pair's M the third refines: the threshold is the pair's own
    got2 = tail.register_batch(srcs[2:3], tgts[2:3], ar[2:3], ar[2:3], weights[2:3], m_thresholds=[600])
    assert tail.last[0]["path"] == "refinement" and not same_bytes(got2[0]["base"], got[2]["base"])


def test_register_batch_of_the_whole_pipeline_equals_register_per_pair():
    """Two small pairs and one whose correspondences exceed the refinement's limit: it takes the drop path in both.  The final bias is set
    from that pair's own logits so that a few thousand of its rows survive the clip (as tests/test_gpu_dgr6.py does)."""
    raws = [synth.make_scan_pair(n0=3000, seed=21)[:2], synth.make_scan_pair(n0=60000, seed=7)[:2], synth.make_scan_pair(n0=3500, seed=22)[:2]]
    base = dgr.DGR(fcgf_model(), model(), voxel_size=0.3, clip_weight_thresh=0.05)
    w0 = np.clip(host(base.register(*raws[1], only_calc_weights=True)).astype(np.float64), 1e-7, 1 - 1e-7)
    m_big = len(w0)
    assert dgr.MAX_TAIL < m_big <= dgr.MAX_N
    st = [tuple(s) for s in stages()]
    shift = np.log(0.05 / 0.95) - np.quantile(np.log(w0 / (1 - w0)), 1 - 3000.0 / m_big)
    st[22] = (st[22][0], st[22][1], (st[22][2] + np.float32(shift)).astype(np.float32))
    net = dgr.InlierNet.from_stages(st)
    reg = dgr.DGR(fcgf_model(), net, voxel_size=0.3, clip_weight_thresh=0.05)
    got = reg.register_batch(raws)
    last = reg.last
    assert isinstance(last, list) and len(got) == 3 and last[1]["m"] == m_big and 1000 < last[1]["m_tail"] < 10000
    assert last[0]["m_tail"] == last[0]["m"] and last[2]["m_tail"] == last[2]["m"] and [l["inlier_status"] for l in last] == [0, 0, 0]
    one = dgr.DGR(fcgf_model(), net, voxel_size=0.3, clip_weight_thresh=0.05)
    for k, raw in enumerate(raws):
        want = one.register(*raw)
        for f in ("weights", "idx1", "idx0_tail", "idx1_tail", "weights_tail", "xyz0", "xyz1"):
            assert same_bytes(host(last[k][f]), host(one.last[f])), (k, f)
        assert last[k]["m"] == one.last["m"] and last[k]["m_tail"] == one.last["m_tail"] and last[k]["tail"]["path"] == one.last["tail"]["path"], k
        assert same_bytes(got[k]["base"], want["base"]) and same_bytes(got[k]["w_icp"], want["w_icp"]), k
        assert np.isfinite(got[k]["base"]).all()
