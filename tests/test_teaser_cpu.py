"""CPU-side checks of the TEASER++ back end: the numpy restatement of the contract (tests/teaser_cpu.py) and the C ABI of
lr_teaser / lr_teaser_batch (layouts, argument checks before any HIP call).  No device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from lidarregistration_amd import _ext
from tests import teaser_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_recovers_planted_motion():
    for seed in range(3):
        a, b, T_gt, _ = tc.planted(80, 30, seed)
        out = tc.teaser(a, b)
        assert out["status"] == 0 and not out["shortcut"]
        assert len(out["clique"]) >= 30
        dR = np.linalg.norm(out["T"][:3, :3] - T_gt[:3, :3])
        assert dR < 1e-2 and np.linalg.norm(out["T"][:3, 3] - T_gt[:3, 3]) < 0.1
        assert out["n_rot"] >= 30 and out["n_trans"] >= 30


def test_voting_equals_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 25))
        x = np.concatenate([rng.normal(0, 0.1, n), rng.uniform(-3, 3, int(rng.integers(0, 10)))])
        if trial % 5 == 0:
            x = np.round(x, 1)                     # ties between endpoints
        est, cost, _ = tc.vote(x, 0.3)
        est_b, cost_b = tc.vote_brute(x, 0.3)
        assert cost == pytest.approx(cost_b, rel=0, abs=1e-12) and est == pytest.approx(est_b, rel=0, abs=1e-12)


def test_graph_equals_naive_double_loop():
    a, b, _, _ = tc.planted(70, 25, 3)
    # pairs placed on the threshold: |a_i - a_j| = 1, |b_i - b_j| = 1.6 exactly representable differences
    a[0], a[1], b[0], b[1] = (0, 0, 0), (1, 0, 0), (0, 0, 0), (1.6, 0, 0)
    a[2], a[3], b[2], b[3] = (0, 0, 0), (0, 0.5, 0), (0, 0, 0), (0, 1.1, 0)
    G = tc.graph(a, b)
    assert np.array_equal(G, tc.graph_naive(a, b))
    assert np.array_equal(G, G.T) and not G.diagonal().any()


def test_kcore_shortcut_both_branches():
    # a clique of 12 plus 4 pendant vertices: max core 11 > 0.5 * 16 -> the shortcut returns the max-core set
    A = np.zeros((16, 16), bool)
    A[:12, :12] = True
    for k in range(4):
        A[12 + k, k] = A[k, 12 + k] = True
    np.fill_diagonal(A, False)
    c, fired, mc = tc.max_clique(A, 0.5)
    assert fired and mc == 11 and list(c) == list(range(12))
    c, fired, _ = tc.max_clique(A, 1.0)                      # disabled: the exact clique
    assert not fired and list(c) == list(range(12))
    # sparse graph: max core 2 of 30 -> no shortcut
    B = np.zeros((30, 30), bool)
    for i in range(30):
        B[i, (i + 1) % 30] = B[(i + 1) % 30, i] = True
    c, fired, mc = tc.max_clique(B, 0.5)
    assert not fired and mc == 2 and len(c) == 2


@pytest.fixture(scope="module")
def L():
    _ext.build()
    return _ext.lib()


def test_header_declares_and_library_exports_teaser_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    declared = set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", hdr))
    for s in ("lr_teaser_scratch_bytes", "lr_teaser", "lr_teaser_batch", "lr_teaser_timing", "lr_teaser_stage_times"):
        assert s in declared and s in _ext.SYMBOLS and hasattr(L, s)


def test_teaser_struct_layouts_match_header():
    P, R = _ext.TeaserParams, _ext.TeaserResult
    assert ctypes.sizeof(P) == 72 and P.struct_size.offset == 0 and P.max_iterations.offset == 4 and P.noise_bound.offset == 8
    assert P.cbar2.offset == 16 and P.kcore_threshold.offset == 24 and P.gnc_factor.offset == 32 and P.cost_threshold.offset == 40
    assert P.node_budget.offset == 48 and P.time_budget_ms.offset == 56 and P.rotation_tim_graph.offset == 64 and P.estimate_scaling.offset == 68
    assert ctypes.sizeof(R) == 176 and R.status.offset == 128 and R.K.offset == 132 and R.exact.offset == 136 and R.max_core.offset == 140
    assert R.lb.offset == 144 and R.nodes.offset == 152 and R.gnc_iters.offset == 160 and R.n_rot_inliers.offset == 164
    assert R.n_trans_inliers.offset == 168
    p = P()
    assert p.struct_size == 72 and p.noise_bound == 0.3 and p.max_iterations == 10000 and p.gnc_factor == 1.4 and p.kcore_threshold == 0.5


def test_teaser_arguments_refused_before_any_hip_call(L):
    assert L.lr_version() == 103
    one = ctypes.c_void_p(256)
    big = ctypes.c_size_t(1 << 40)

    def call(p, m=10, scratch=one):
        return L.lr_teaser(one, one, m, None, ctypes.byref(p), one, None, scratch, big, None)

    p = _ext.TeaserParams(); p.struct_size = 64
    assert call(p) == -1 and b"struct_size" in L.lr_last_error()
    for kw in (dict(noise_bound=0.0), dict(noise_bound=float("nan")), dict(cbar2=-1.0), dict(kcore_threshold=0.0), dict(kcore_threshold=1.5),
               dict(gnc_factor=1.0), dict(max_iterations=-1), dict(node_budget=0), dict(time_budget_ms=0.0),
               dict(rotation_tim_graph=1), dict(estimate_scaling=1)):
        assert call(_ext.TeaserParams(**kw)) == -1, kw
    assert call(_ext.TeaserParams(), m=-1) == -1
    assert call(_ext.TeaserParams(), m=40000) == -4
    assert call(_ext.TeaserParams(), scratch=None) == -1
    assert L.lr_teaser(one, one, 10, None, ctypes.byref(_ext.TeaserParams()), one, None, one, ctypes.c_size_t(16), None) == -4
    V = ctypes.c_void_p * 65
    assert L.lr_teaser_batch(65, V(), V(), (ctypes.c_int32 * 65)(), None, ctypes.byref(_ext.TeaserParams()), one, None, one, big, None) == -1
    assert L.lr_teaser_batch(0, V(), V(), (ctypes.c_int32 * 65)(), None, ctypes.byref(_ext.TeaserParams()), one, None, one, big, None) == -1
    assert L.lr_teaser_scratch_bytes(-1) == 0 and L.lr_teaser_scratch_bytes(40000) == 0
    assert L.lr_teaser_scratch_bytes(16384) > L.lr_teaser_scratch_bytes(4096) > 0
