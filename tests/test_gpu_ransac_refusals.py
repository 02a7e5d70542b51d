"""What lr_ransac refuses, in which order, and with which words: every refusal of lr_ransac_run (csrc/lr_ransac.hip, ransac_resolve) through
lr_ransac and through lr_register_pair, one fault at a time and two at a time.  The expected strings are the literals of the source; a
struct with two faults gets the message of the check that comes first.  A refused call leaves nothing behind: the valid call that follows on the
same workspace returns what it returns on a fresh one.  Needs an MI355X."""
import ctypes

import pytest

from tests.conftest import Args

pytestmark = pytest.mark.gpu

MAX_N, DIM, MAX_ITERS, M = 64, 32, 16, 8
EINVAL, ESIZE = -1, -4

# the ten refusal groups in the order the checks come in: (name, field -> faulty value, code, message)
GROUPS = [
    ("scoring", dict(scoring=3), EINVAL, "lr_ransac: scoring must be 0 (count, then error), 1 (MSAC) or 2 (MSAC at GC-RANSAC's truncated threshold)"),
    ("lo", dict(lo_trials=21), EINVAL, "lr_ransac: lo_rounds, lo_trials (<= 20), lo_max_calls and min_iters must be >= 0 (0 = default)"),
    ("sample_size", dict(sample_size=5), EINVAL, "lr_ransac: sample_size must be 3 or 4"),
    ("iters", dict(iters=MAX_ITERS + 1), ESIZE, "lr_ransac: iters exceeds the workspace"),
    ("m", dict(m=MAX_N + 1), ESIZE, "lr_ransac: m exceeds the workspace"),
    ("thr2", dict(thr2=0.0), EINVAL, "lr_ransac: thr2 must be in (0, 2048)"),
    ("use_elc", dict(use_elc=3), EINVAL, "lr_ransac: use_elc must be 0 (no pre-verification), 1 (edge-length check) or 2 (SPRT)"),
    ("sampler", dict(sampler=3), EINVAL, "lr_ransac: sampler must be 0 (uniform), 1 (PROSAC) or 2 (uniform, unique indices)"),
    ("local_opt", dict(local_opt=3), EINVAL, "lr_ransac: local_opt must be 0, 1 or 2"),
    ("prosac_growth", dict(prosac_growth=-1), EINVAL, "lr_ransac: prosac_growth must be >= 0"),
]
# the other members of the second group (one message for all four)
LO_GROUP = [dict(lo_rounds=-1), dict(lo_trials=-1), dict(lo_max_calls=-1), dict(min_iters=-1)]
# two faults: every adjacent pair of groups, and the first with the last.  The earlier check answers -- except that lr_ransac itself
# checks m (same words) before it hands the struct on, so through that entry point a too large m answers before everything else
PAIRS = [(k, k + 1) for k in range(len(GROUPS) - 1)] + [(0, len(GROUPS) - 1)]
M_GROUP = 4


def _first(a, b):
    return M_GROUP if M_GROUP in (a, b) else min(a, b)


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.torch = torch; ns.ext = _ext; ns.ransac = ransac
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    # clouds of the workspace's size (+ 1 row, so that the pointers of the too-large call are good for what it claims) related by a rigid motion
    c, s = 0.8, 0.6
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    xyz0 = (torch.rand(MAX_N + 1, 3, generator=g) * 20.0 - 10.0).float()
    xyz1 = (xyz0 @ R.T + torch.tensor([1.0, -2.0, 0.5])).float()
    feats = torch.nn.functional.normalize(torch.randn(MAX_N + 1, DIM, generator=g), dim=1).float()
    ns.xyz0, ns.xyz1, ns.feats = xyz0.to(dev).contiguous(), xyz1.to(dev).contiguous(), feats.to(dev).contiguous()
    ns.ws = _ext.Workspace(MAX_N, MAX_N, DIM, MAX_ITERS)
    ns.fresh = _valid(ns, _ext.Workspace(MAX_N, MAX_N, DIM, MAX_ITERS))
    r = _ext.RansacResult.from_buffer_copy(ns.fresh[1])
    assert r.best_h >= 0 and r.best_count == M and r.n_ids == MAX_ITERS      # (an exact rigid motion: every correspondence is an inlier)
    return ns


def _stream(lr):
    return lr.torch.cuda.current_stream().cuda_stream


def _ransac(lr, ws, fields):
    """lr_ransac over the first m correspondences with the valid parameters, `fields` on top -> (code, message, T bytes, result bytes)"""
    fields = dict(fields)
    m = fields.pop("m", M)
    p = lr.ransac.ransac_params(MAX_ITERS, sample_size=3, use_elc=True, thr=0.6)
    for k, v in fields.items():
        setattr(p, k, v)
    T = lr.torch.zeros(16, dtype=lr.torch.float64, device=lr.xyz0.device)
    res = lr.torch.zeros(ctypes.sizeof(lr.ext.RansacResult), dtype=lr.torch.uint8, device=lr.xyz0.device)
    rc = lr.ext.lib().lr_ransac(ws.handle, lr.xyz0.data_ptr(), lr.xyz1.data_ptr(), m, None, ctypes.byref(p), T.data_ptr(), res.data_ptr(), _stream(lr))
    msg = lr.ext.lib().lr_last_error().decode() if rc != 0 else ""
    return rc, msg, T.cpu().numpy().tobytes(), res.cpu().numpy().tobytes()


def _valid(lr, ws):
    rc, msg, T, res = _ransac(lr, ws, {})
    assert rc == 0, msg
    return T, res


def _register_pair(lr, ws, fields):
    """lr_register_pair (no filter: the RANSAC stage sees the n0 nearest-neighbour pairs) with `fields` on top of valid parameters -> (code, message)"""
    fields = dict(fields)
    n0 = fields.pop("m", MAX_N)
    p = lr.FR.pair_params(Args(mode="no_filter", codebase="open3D", iters=MAX_ITERS, ransac_n=3, o3d_conf=1.0))
    for k, v in fields.items():
        setattr(p.ransac, k, v)
    out = lr.torch.zeros(ctypes.sizeof(lr.ext.PairResult), dtype=lr.torch.uint8, device=lr.xyz0.device)
    rc = lr.ext.lib().lr_register_pair(ws.handle, lr.xyz0.data_ptr(), lr.xyz1.data_ptr(), lr.feats.data_ptr(), lr.feats.data_ptr(), n0, MAX_N, DIM,
                                        ctypes.byref(p), out.data_ptr(), _stream(lr))
    return rc, (lr.ext.lib().lr_last_error().decode() if rc != 0 else "")


def _nothing_left_behind(lr):
    assert _valid(lr, lr.ws) == lr.fresh


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_single_fault_ransac(lr, group):
    _, fields, code, message = group
    rc, msg, _, _ = _ransac(lr, lr.ws, fields)
    assert (rc, msg) == (code, message)
    _nothing_left_behind(lr)


@pytest.mark.parametrize("fields", LO_GROUP, ids=[next(iter(f)) for f in LO_GROUP])
def test_single_fault_ransac_lo_group(lr, fields):
    rc, msg, _, _ = _ransac(lr, lr.ws, fields)
    assert (rc, msg) == (GROUPS[1][2], GROUPS[1][3])
    _nothing_left_behind(lr)


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{GROUPS[a][0]}+{GROUPS[b][0]}" for a, b in PAIRS])
def test_double_fault_ransac(lr, a, b):
    rc, msg, _, _ = _ransac(lr, lr.ws, {**GROUPS[a][1], **GROUPS[b][1]})
    assert (rc, msg) == GROUPS[_first(a, b)][2:]
    _nothing_left_behind(lr)


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_single_fault_register_pair(lr, group):
    name, fields, code, message = group
    if name == "m":      # a cloud above the workspace is turned away by the entry point's own check of its clouds, before any stage
        code, message = ESIZE, f"lr_register_pair: ({MAX_N + 1},{MAX_N}) exceeds workspace ({MAX_N},{MAX_N})"
    rc, msg = _register_pair(lr, lr.ws, fields)
    assert (rc, msg) == (code, message)
    _nothing_left_behind(lr)


def test_valid_register_pair_goes_through(lr):
    """(the parameters the refused calls start from are good ones)"""
    rc, msg = _register_pair(lr, lr.ws, {})
    assert rc == 0, msg
    lr.torch.cuda.synchronize()
    _nothing_left_behind(lr)
