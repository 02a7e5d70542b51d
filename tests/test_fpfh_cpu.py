"""The FPFH contract without a device: the numpy restatement's invariants, a literal restatement of the recalled Open3D algorithm (acos,
atan2, repeated +=) against the contract form, fpfh.match's normalisation and mutual rule, the entry point's refusals and scratch sizes."""
import math

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, fpfh
from tests import bbrf_cpu, fpfh_cpu

RADIUS, MAX_NN = 1.5, 100


@pytest.fixture(scope="module")
def cloud():
    X, N = fpfh_cpu.scan_cloud()
    F, info = fpfh_cpu.fpfh(X, N, RADIUS, MAX_NN)
    return X, N, F, info


def test_blocks_sum_to_200_or_the_row_is_zero(cloud):
    X, N, F, info = cloud
    assert len(X) > 2000 and info["status"] == 0 and info["dropped"] == 0 and 0 < info["capped"] < len(X)
    zero = ~F.any(axis=1)
    assert zero.sum() == info["zero_rows"]
    sums = F.reshape(len(X), 3, 11).sum(axis=2)
    assert np.all(np.abs(sums[~zero] - 200.0) <= 1e-9) and np.all(F >= 0.0)


def test_short_lists_give_zero_rows_and_the_counts():
    X = np.array([[0.0, 0, 0], [0.1, 0, 0], [50.0, 0, 0], [np.nan, 0, 0], [0.0, 0.1, 0]])
    N = np.tile([0.0, 0.0, 1.0], (5, 1))
    F, info = fpfh_cpu.fpfh(X, N, 1.0, 2)
    assert not F[2].any() and not F[3].any() and F[0].any() and F[1].any() and F[4].any()
    assert info == dict(status=0, dropped=1, zero_rows=2, capped=3)
    F0, info0 = fpfh_cpu.fpfh(np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 2)
    assert F0.shape == (0, 33) and info0["status"] == 1
    # an exact duplicate pair on its own: the other copy has d2 == 0 and is skipped, the row is the point's own SPFH (bins 5, 5, 5)
    D = np.array([[1.0, 2, 3], [1.0, 2, 3]])
    Fd, _ = fpfh_cpu.fpfh(D, N[:2], 1.0, 10)
    want = np.zeros(33); want[[5, 16, 27]] = 100.0
    assert np.array_equal(Fd[0], want) and np.array_equal(Fd[1], want)


def test_permutation_of_the_input_permutes_the_output(cloud):
    X, N, F, _ = cloud
    sel = np.flatnonzero((np.abs(X[:, 0]) < 4.0) & (np.abs(X[:, 1]) < 4.0))
    Xs, Ns = X[sel], N[sel]
    Fs, _ = fpfh_cpu.fpfh(Xs, Ns, RADIUS, MAX_NN)
    perm = np.random.default_rng(3).permutation(len(sel))
    Fp, _ = fpfh_cpu.fpfh(Xs[perm], Ns[perm], RADIUS, MAX_NN)
    # the lists are ordered by (d2, index): equal distances may swap under the permutation and with them the order of a chain's terms,
    # so the rows agree to rounding, not to the bit; the histogram counts themselves (F4) are order-free
    np.testing.assert_allclose(Fp, Fs[perm], rtol=0, atol=1e-9)


def test_angle_bin_form_equals_the_atan2_form():
    rng = np.random.default_rng(11)
    y, x = rng.standard_normal(200000), rng.standard_normal(200000)
    want = np.clip(np.floor(11.0 * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int64)
    assert np.array_equal(fpfh_cpu.angle_bin(y, x), want)
    assert [int(fpfh_cpu.angle_bin(*p)) for p in ((0.0, -1.0), (-0.0, -1.0), (0.0, 0.0), (0.0, 1.0), (-0.0, 0.0))] == [10, 0, 5, 5, 5]
    f = np.concatenate([rng.uniform(-1.2, 1.2, 100000), [-1.0, 1.0, 0.0, -1.0 + 2.0 / 11.0]])
    assert np.array_equal(fpfh_cpu.unit_bin(f), np.clip(np.floor(11.0 * (f + 1.0) * 0.5), 0, 10).astype(np.int64))


def literal_pair(p1, n1, p2, n2):
    """Open3D's ComputePairFeatures as recalled, with the libm calls it makes."""
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    d = (p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2])
    L = math.sqrt(dot(d, d))
    if L == 0.0:
        return 0.0, 0.0, 0.0
    a1 = dot(n1, d) / L; a2 = dot(n2, d) / L
    acos = lambda t: math.acos(t) if t <= 1.0 else math.nan          # C's acos: NaN past 1, and a comparison with NaN is false
    if acos(abs(a1)) > acos(abs(a2)):
        n1, n2 = n2, n1; d = (-d[0], -d[1], -d[2]); f3 = -a2
    else:
        f3 = a1
    v = cross(d, n1)
    vn = math.sqrt(dot(v, v))
    if vn == 0.0:
        return 0.0, 0.0, 0.0
    v = (v[0] / vn, v[1] / vn, v[2] / vn)
    w = cross(n1, v)
    return math.atan2(dot(w, n2), dot(n1, n2)), dot(v, n2), f3


def literal_fpfh(X, N, nbrs, d2):
    n = len(X)
    S = np.zeros((n, 33))
    clamp = lambda h: max(0, min(10, int(h)))
    P, Q = X.tolist(), N.tolist()
    for i in range(n):
        nb = nbrs[i]
        if len(nb) > 1:
            incr = 100.0 / (len(nb) - 1)
            for k in nb[1:]:
                f1, f2, f3 = literal_pair(P[i], Q[i], P[k], Q[k])
                S[i, clamp(math.floor(11 * (f1 + math.pi) / (2.0 * math.pi)))] += incr
                S[i, 11 + clamp(math.floor(11 * (f2 + 1.0) * 0.5))] += incr
                S[i, 22 + clamp(math.floor(11 * (f3 + 1.0) * 0.5))] += incr
    F = np.zeros((n, 33))
    for i in range(n):
        nb = nbrs[i]
        if len(nb) > 1:
            s = [0.0, 0.0, 0.0]
            for e in range(1, len(nb)):
                dist = d2[i][e]
                if dist == 0.0:
                    continue
                vals = S[nb[e]] / dist
                for b in range(3):          # sum[j / 11] += val for j in order: a left-to-right running sum (cumsum is one)
                    s[b] = float(np.cumsum(np.concatenate(([s[b]], vals[11 * b:11 * b + 11])))[-1])
                F[i] += vals
            for b in range(3):
                if s[b] != 0.0:
                    s[b] = 100.0 / s[b]
            F[i] = F[i] * np.repeat(s, 11) + S[i]
    return F


def test_literal_restatement_agrees_with_the_contract(cloud):
    X, N, F, _ = cloud
    idx, d2, ln = fpfh_cpu.lists(X, RADIUS, MAX_NN)
    nbrs = [idx[i, :ln[i]] for i in range(len(X))]
    G = literal_fpfh(X, N, nbrs, d2)
    row_err = np.abs(G - F).max(axis=1)
    differ = row_err > 1e-9
    print("rows that differ in a bin:", int(differ.sum()), "of", len(X), "-- largest error among the others:", row_err[~differ].max())
    # a pair feature on a bin edge (acos rounding two tiny arguments to pi / 2, an angle on an edge) moves a count; it reaches the
    # rows of every point that has the pair's owner in its list, so rows, not pairs, are counted: at most 1 % of the points
    assert differ.sum() <= len(X) // 100
    assert np.all(row_err[~differ] <= 1e-9)


def test_match_normalisation_and_mutual_rule():
    rng = np.random.default_rng(8)
    F0 = rng.uniform(0.0, 200.0, (500, 33)).astype(np.float32); F1 = rng.uniform(0.0, 200.0, (480, 33)).astype(np.float32)
    F0[7] = 0.0
    A = fpfh.normalise(torch.from_numpy(F0)).numpy()
    want = F0.astype(np.float64) / (np.linalg.norm(F0.astype(np.float64), axis=1, keepdims=True) + 1e-6)
    assert A.dtype == np.float32 and np.all(np.abs(A - want) <= 4 * 2.0 ** -24) and not A[7].any()
    B = F1.astype(np.float64) / (np.linalg.norm(F1.astype(np.float64), axis=1, keepdims=True) + 1e-6)
    d2 = (want * want).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * want @ B.T
    i01, i10 = d2.argmin(1), d2.argmin(0)
    corr = fpfh.mutual_pairs(i01, i10).numpy()
    keep = np.flatnonzero(i10[i01] == np.arange(500))
    assert corr.dtype == np.int64 and np.array_equal(corr, np.stack([keep, i01[keep]], axis=1)) and 0 < len(keep) < 500
    assert fpfh.mutual_pairs(np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0, 2)


def test_host_check_program_builds_and_runs_clean():
    import os
    import subprocess
    from tests.conftest import ROOT
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lidarregistration_amd", "csrc"), "fpfh_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fpfh_host_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_refusals_and_scratch_sizes():
    L = _ext.lib()

    def call(**kw):
        a = dict(xyz=256, nrm=256, n=10, radius=1.0, max_nn=100, o64=256, o32=None, info=256, scratch=256, bytes=1 << 42)
        a.update(kw)
        rc = L.lr_fpfh(a["xyz"], a["nrm"], a["n"], a["radius"], a["max_nn"], a["o64"], a["o32"], a["info"], a["scratch"], a["bytes"], None)
        return rc, L.lr_last_error().decode()
    for kw, word in ((dict(radius=0.0), "radius"), (dict(radius=float("nan")), "radius"), (dict(radius=1e200), "radius"),
                     (dict(max_nn=1), "max_nn"), (dict(max_nn=129), "max_nn"), (dict(n=-1), "n must"), (dict(n=(1 << 22) + 1), "n must"),
                     (dict(xyz=None), "null xyz"), (dict(nrm=None), "null normals"), (dict(o64=None), "null out_f64 and out_f32"),
                     (dict(info=None), "null info"), (dict(scratch=None), "null scratch"), (dict(scratch=264), "aligned"),
                     (dict(bytes=L.lr_fpfh_scratch_bytes(10, 100) - 1), "scratch too small")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lr_fpfh:") and word in msg, (kw, msg)
    sb = L.lr_fpfh_scratch_bytes
    assert sb(-1, 100) == 0 and sb((1 << 22) + 1, 100) == 0 and sb(10, 1) == 0 and sb(10, 129) == 0
    prev = 0
    for n in (0, 1, 2, 257, 3000, 75000, 1 << 22):
        assert sb(n, 2) % 256 == 0 and sb(n, 2) <= sb(n, 128) and sb(n, 128) >= prev
        prev = sb(n, 128)
    n = 1 << 22
    assert sb(n, 128) > n * 128 * 4 + n * 33 * 8 > 1 << 31            # the lists alone pass 2^31 bytes: size_t throughout
