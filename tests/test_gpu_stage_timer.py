"""The stage timer of a workspace (lr_workspace_timing / _timing_read / _stage_times): which calls make a sample and which of its
intervals are recorded.  Structure only, never a duration.  Slots of lr_workspace_stage_times: out[0] whole call, out[1] forward NN,
out[2] / out[3] forward / reverse filter pass, out[4] RANSAC generation + scoring of the first batch, out[5] reverse NN.
And: a batched call that is refused part-way leaves nothing behind that a later single-pair call on the workspace could see.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest

from lidarregistration_amd import synth
from tests.conftest import Args

pytestmark = pytest.mark.gpu

N0, N1, DIM, ITERS = 3000, 2500, 32, 2048
RAGGED = [(N0, N1), (2000, 2500), (2500, 1800)]


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.torch = torch; ns.ext = _ext
    dev = torch.device("cuda", 0)
    ns.pairs = []
    for k, (n0, n1) in enumerate(RAGGED):
        p = synth.make_pair(N=n0, N1=n1, rho=0.5, s=0.9, seed=610 + k)
        ns.pairs.append(tuple(torch.from_numpy(p[key]).to(dev) for key in ("xyz0", "xyz1", "feats0", "feats1")))
    ns.mnn = FR.pair_params(Args(mode="MNN", codebase="open3D", iters=ITERS, ransac_n=3, o3d_conf=1.0))
    ns.no_filter = FR.pair_params(Args(mode="no_filter", codebase="open3D", iters=ITERS, ransac_n=3, o3d_conf=1.0))
    return ns


def _ws(lr, timing=True, max_pairs=1):
    ws = lr.ext.Workspace(N0, N1, DIM, ITERS, max_pairs=max_pairs)
    if timing:
        ws.timing(True)
    return ws


def _stage_times(lr, ws):
    lr.torch.cuda.synchronize()
    return ws.stage_times()


def _timing_read(lr, ws):
    lr.torch.cuda.synchronize()
    nn, ransac, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    lr.ext.check(lr.ext.lib().lr_workspace_timing_read(ws.handle, ctypes.byref(nn), ctypes.byref(ransac), ctypes.byref(n)))
    return nn.value, ransac.value, n.value


def _whole_call_shape(out):
    """One timed call with both NN directions: every interval recorded, nested as the events are."""
    assert out[0] >= out[1] + out[5]
    assert out[1] >= out[2] > 0
    assert out[5] >= out[3] > 0
    assert 0 < out[4] <= out[0]


def test_one_mnn_call_is_one_sample_with_every_interval(lr):
    ws = _ws(lr)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)
    out, n = _stage_times(lr, ws)
    assert n == 1
    _whole_call_shape(out)
    # the two sums of lr_workspace_timing_read for that single sample (float32 on both sides)
    nn, ransac, n2 = _timing_read(lr, ws)
    assert n2 == 1
    assert np.float32(nn) == np.float32(out[2]) + np.float32(out[3])
    assert ransac == out[4]


def test_calls_before_a_read_add_one_sample(lr):
    ws = _ws(lr)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)
    out, n = _stage_times(lr, ws)
    assert n == 1
    _whole_call_shape(out)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)      # (the read collected the sample: the next call is timed again)
    assert _stage_times(lr, ws)[1] == 2


def test_no_filter_call_has_no_reverse_intervals(lr):
    ws = _ws(lr)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.no_filter, ws=ws)
    out, n = _stage_times(lr, ws)
    assert n == 1
    assert out[3] == 0 and out[5] == 0
    assert out[0] >= out[1] >= out[2] > 0 and 0 < out[4] <= out[0]


def test_ragged_batch_is_one_sample_of_the_same_shape(lr):
    ws = _ws(lr, max_pairs=len(RAGGED))
    lr.FR.register_batch_dev(lr.pairs, lr.mnn, ws=ws)
    out, n = _stage_times(lr, ws)
    assert n == 1
    _whole_call_shape(out)
    nn, ransac, _ = _timing_read(lr, ws)
    assert np.float32(nn) == np.float32(out[2]) + np.float32(out[3]) and ransac == out[4]


def test_lone_nn_top2_records_the_forward_filter_pass_only(lr):
    ws = _ws(lr)
    f0, f1 = lr.pairs[0][2], lr.pairs[0][3]
    i1 = lr.torch.empty(N0, dtype=lr.torch.int32, device=f0.device); i2 = lr.torch.empty_like(i1)
    lr.ext.check(lr.ext.lib().lr_nn_top2(ws.handle, f0.data_ptr(), N0, f1.data_ptr(), N1, DIM, i1.data_ptr(), i2.data_ptr(), None, None,
                                          lr.torch.cuda.current_stream().cuda_stream))
    out, n = _stage_times(lr, ws)
    assert n == 1
    assert out[2] > 0
    assert [out[k] for k in (0, 1, 3, 4, 5)] == [0, 0, 0, 0, 0]
    assert _timing_read(lr, ws) == (out[2], 0, 1)


def test_timing_off_records_nothing(lr):
    ws = _ws(lr, timing=False)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)
    out, n = _stage_times(lr, ws)
    assert n == 0 and out == [0] * 6
    assert _timing_read(lr, ws) == (0, 0, 0)


def test_timing_on_again_zeroes_the_sums(lr):
    ws = _ws(lr)
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)
    assert _stage_times(lr, ws)[1] == 1
    lr.FR.register_pair_dev(*lr.pairs[0], lr.mnn, ws=ws)      # (a sample that is still pending goes too)
    lr.torch.cuda.synchronize()
    ws.timing(True)
    out, n = _stage_times(lr, ws)
    assert n == 0 and out == [0] * 6
    assert _timing_read(lr, ws) == (0, 0, 0)


def test_single_pair_call_after_a_batch_refused_part_way(lr):
    """lr_register_batch with iters above the workspace's max_iters comes back with LR_ESIZE from the RANSAC stage, after the NN and
    filter stages of all three pairs were enqueued; the single-pair call that follows must not see any of it."""
    P = len(RAGGED)
    too_many = lr.FR.pair_params(Args(mode="MNN", codebase="open3D", iters=2 * ITERS, ransac_n=3, o3d_conf=1.0))
    used = _ws(lr, timing=False, max_pairs=P)
    with pytest.raises(lr.ext.LidarRegError, match="iters exceeds the workspace"):
        lr.FR.register_batch_dev(lr.pairs, too_many, ws=used)
    after = lr.FR.register_pair_dev(*lr.pairs[1], lr.mnn, ws=used).cpu().numpy()
    unused = _ws(lr, timing=False, max_pairs=P)
    fresh = lr.FR.register_pair_dev(*lr.pairs[1], lr.mnn, ws=unused).cpu().numpy()
    assert after.tobytes() == fresh.tobytes() and len(after.tobytes()) == ctypes.sizeof(lr.ext.PairResult)
    assert lr.ext.PairResult.from_buffer_copy(after.tobytes()).status == 0
