"""lr_nn_wide without a device: fixture G28 (the reference's matching.py on descriptors of 33, 64 and 128 numbers) against the oracle,
the entry point's refusals (they come before the device check), the scratch sizes, the stand-alone host check program, and what
matching.py refuses at these widths."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from lidarregistration_amd import _ext, synth
from tests.conftest import ROOT, golden

TAGS = ("d33", "d64", "d128")
U = 2.0 ** -24


def pick_bound(D, a, b):
    """How far the exact squared distance of a row b picked by a float32 evaluation of the contract (or of the reference's formula:
    the bound holds for any summation order) can lie above the smallest one, per candidate: the D-term dot product and the two D-term
    norms carry gamma_D = D u / (1 - D u) of |a|.|b| <= |a||b| each (2 |a||b| + |a|^2 + |b|^2 = (|a| + |b|)^2 in all), the sum of the
    norms, the final fma and the square root (2 u on the square) one rounding each, of at most (|a| + |b|)^2."""
    gamma = D * U / (1.0 - D * U)
    s = np.sqrt((a * a).sum(-1)) + np.sqrt((b * b).sum(-1))
    return (gamma + 4.0 * U) * s * s


def d2_exact(F0, F1, i, j):
    d = F0[i].astype(np.float64) - F1[j].astype(np.float64)
    return (d * d).sum(-1)


def assert_picks_agree(F0, F1, ours, ref):
    """Rows may differ only where the two picks' float64 distances lie within both picks' bounds; at most 1 % of the rows."""
    bad = np.nonzero(ours != ref)[0]
    assert len(bad) <= len(ours) // 100
    A = F0[bad].astype(np.float64)
    e = pick_bound(F0.shape[1], A, F1[ours[bad]].astype(np.float64)) + pick_bound(F0.shape[1], A, F1[ref[bad]].astype(np.float64))
    assert np.all(np.abs(d2_exact(F0, F1, bad, ours[bad]) - d2_exact(F0, F1, bad, ref[bad])) <= e)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_equals_reference_golden(oracle, tag):
    g = golden("g28_nn_wide.npz")
    n0, n1, d, seed = [int(v) for v in g[f"{tag}_shape"]]
    F0, F1 = synth.make_features(n0, n1, d, 0.5, 0.5, seed)
    i1, i2, s1, s2 = oracle.nn_top2(F0, F1)
    assert_picks_agree(F0, F1, i1, g[f"{tag}_idx1"])
    assert_picks_agree(F0, F1, i2, g[f"{tag}_idx2"])
    # this fixture's seed was chosen so that the reference needs no tolerance against float64; the oracle then needs none either
    assert np.array_equal(i1, g[f"{tag}_idx1"]) and np.array_equal(i2, g[f"{tag}_idx2"])
    m = oracle.nn_to_mutual(F0, F1, np.arange(n0), i1.astype(np.int64), i2.astype(np.int64))
    for ours, key in zip(m, ("m0", "m1", "m2")):
        assert np.array_equal(ours, g[f"{tag}_{key}"])
    assert 0 < len(m[0]) < n0


def test_pick_bound_covers_the_float32_contract(oracle):
    """The tolerance rule itself, where it is needed: near-duplicate columns, so that float32 and float64 pick differently on many rows."""
    rng = np.random.default_rng(5)
    for d in (33, 128):
        F0 = rng.standard_normal((300, d)).astype(np.float32)
        base = rng.standard_normal((40, d)).astype(np.float32)
        F1 = (np.repeat(base, 5, axis=0) * (1.0 + 3e-8 * rng.standard_normal((200, 1)))).astype(np.float32)
        i1, _, _, _ = oracle.nn_top2(F0, F1)
        A, B = F0.astype(np.float64), F1.astype(np.float64)
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
        ref = d2.argmin(1)
        bad = np.nonzero(i1 != ref)[0]
        e = pick_bound(d, A[bad], B[i1[bad]]) + pick_bound(d, A[bad], B[ref[bad]])
        assert np.all(np.abs(d2_exact(F0, F1, bad, i1[bad]) - d2_exact(F0, F1, bad, ref[bad])) <= e)


def _call(L, **kw):
    a = dict(F0=256, n0=100, F1=256, n1=90, dim=33, idx1=256, idx2=None, s1=None, s2=None, scratch=256, bytes=1 << 40)
    a.update(kw)
    rc = L.lr_nn_wide(a["F0"], a["n0"], a["F1"], a["n1"], a["dim"], a["idx1"], a["idx2"], a["s1"], a["s2"], a["scratch"], a["bytes"], None)
    return rc, L.lr_last_error().decode()


def test_refusals_and_scratch_sizes():
    L = _ext.lib()
    assert L.lr_version() == 103                                         # new entry points only
    for dim in (1, 16, 32):
        rc, msg = _call(L, dim=dim)
        assert rc == -1 and msg.startswith("lr_nn_wide:") and "use lr_nn_top2" in msg
    for dim in (0, -3, 129, 4096):
        rc, msg = _call(L, dim=dim)
        assert rc == -1 and "33..128" in msg and "lr_nn_top2" not in msg
    for kw, word in ((dict(n0=-1), "n0 / n1"), (dict(n1=(1 << 22) + 1), "n0 / n1"), (dict(F0=None), "null F0"), (dict(F1=None), "null F1"),
                     (dict(idx1=None), "null idx1"), (dict(scratch=None), "null scratch"), (dict(scratch=264), "aligned"),
                     (dict(bytes=L.lr_nn_wide_scratch_bytes(100, 90, 33) - 1), "scratch too small")):
        rc, msg = _call(L, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    sb = L.lr_nn_wide_scratch_bytes
    assert sb(100, 90, 32) == 0 and sb(100, 90, 129) == 0 and sb(-1, 90, 33) == 0 and sb(100, (1 << 22) + 1, 33) == 0
    for n0, n1 in ((0, 0), (1, 1), (33, 31), (2049, 4097), (30000, 30000), (1 << 22, 1 << 22)):
        for dim in (33, 128):
            assert sb(n0, n1, dim) >= 256 and sb(n0, n1, dim) % 256 == 0
    assert sb(1 << 22, 1 << 22, 128) < 64 << 20                          # the norms only: no partials, no n0 x n1 matrix
    # the workspace keeps refusing 33
    h = ctypes.c_void_p()
    assert L.lr_workspace_create(ctypes.byref(h), 100, 100, 33, 10) == -1


def test_host_check_program_builds_and_runs_clean():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lidarregistration_amd", "csrc"), "nnw_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nnw_host_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
