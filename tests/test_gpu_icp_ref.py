"""lr_icp and lr_icp_batch against the independent fp64 ICP of tests/icp_ref.py (k-d tree correspondences, SVD update) at full
cloud sizes, at radii from 5 cm to 10 m, far from the origin, with duplicate and NaN target rows, and with neighbours placed at the
walls of the kernel's hash grid (cell = max_dist, 27-cell search).  Needs an MI355X."""

import numpy as np
import pytest

from lidarregistration_amd import synth
from tests import icp_ref
from tests.conftest import Args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lr():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import FR, _ext, ransac
    _ext.lib()
    class NS: pass
    ns = NS(); ns.FR = FR; ns.ransac = ransac; ns.torch = torch; ns.ext = _ext
    return ns


def _start(T_gt, offset, deg, centre=0.0):
    """T_gt moved by `offset` and turned by `deg` about the vertical through `centre` (the middle of the clouds)."""
    a = np.radians(deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = np.full(3, float(centre))
    T0 = T_gt.copy()
    T0[:3, :3] = Rz @ T_gt[:3, :3]
    T0[:3, 3] = Rz @ (T_gt[:3, 3] - c) + c + np.array([offset, -0.5 * offset, 0.3 * offset])
    return T0


def _same(info, ref, T, Tr):
    """n_corr and iterations exact (iterations only where no convergence test of the reference came within 1e-12 of its 1e-6
    decision: there the last bit of the rmse decides); fitness, rmse and the rotation to fp64 summation-order noise.  The
    translation gets 1e-9 + 1e-12 |t|: the kernel solves each update from raw moments (sum p q^T - n c_p c_q^T), which cancel
    by |c|^2 / variance on clouds 10^3 m from the origin -- 1.6e-9 m on a 2 km translation was measured there."""
    assert info["n_corr"] == ref["n_corr"], (info, ref)
    if ref["margin"] > 1e-12:
        assert info["iterations"] == ref["iterations"], (info, ref)
    assert abs(info["fitness"] - ref["fitness"]) <= 1e-12
    assert abs(info["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-9
    assert np.abs(T[:3, :3] - Tr[:3, :3]).max() <= 1e-9
    assert np.abs(T[:3, 3] - Tr[:3, 3]).max() <= 1e-9 + 1e-12 * np.abs(Tr[:3, 3]).max()


def _shifted(n, seed, shift, noise=0.05):
    xyz0, xyz1, T_gt = synth.make_clouds(n, n, 0.6, seed, noise=noise)
    T = T_gt.copy()
    T[:3, 3] += shift - T_gt[:3, :3] @ np.full(3, shift)
    return (xyz0 + shift).astype(np.float32), (xyz1 + shift).astype(np.float32), T


@pytest.mark.parametrize("n,max_dist,shift", [(30000, 0.05, 0.0), (30000, 0.6, 1e3), (30000, 2.0, 0.0), (30000, 10.0, -1e3),
                                              (100000, 0.05, 1e3), (100000, 0.6, 0.0), (100000, 2.0, -1e3), (100000, 10.0, 0.0)])
def test_icp_full_size_against_reference(lr, n, max_dist, shift):
    """make_clouds spans about +-80 m around 0 (straddling zero on every axis); shift moves both clouds 10^3 m away."""
    xyz0, xyz1, T_gt = _shifted(n, n + int(max_dist * 10), shift, noise=min(0.05, max_dist / 4))
    T0 = _start(T_gt, min(0.5 * max_dist, 1.0), 1.0, shift) if max_dist >= 0.5 else _start(T_gt, 0.2 * max_dist, 0.005, shift)
    T, info = lr.ransac.icp_dev(xyz0, xyz1, T0, max_dist=max_dist)
    Tr, ref = icp_ref.icp(xyz0, xyz1, T0, max_dist=max_dist)
    _same(info, ref, T, Tr)
    assert info["n_corr"] > 0.05 * n


def test_icp_duplicates_and_nan_targets(lr):
    rng = np.random.default_rng(12)
    xyz0, xyz1, T_gt = synth.make_clouds(30000, 30000, 0.6, 77)
    dup = rng.choice(30000, 12000)
    xyz1 = np.concatenate([xyz1, xyz1[dup], xyz1[dup[:3000]]])
    xyz1 = xyz1[rng.permutation(len(xyz1))].astype(np.float32)
    xyz1[rng.choice(len(xyz1), 9, replace=False)] = np.nan
    xyz1[rng.choice(len(xyz1), 2, replace=False), 1] = np.nan
    for max_dist in (0.6, 2.0):
        T0 = _start(T_gt, 0.3, 1.0)
        T, info = lr.ransac.icp_dev(xyz0, xyz1, T0, max_dist=max_dist)
        Tr, ref = icp_ref.icp(xyz0, xyz1, T0, max_dist=max_dist)
        _same(info, ref, T, Tr)


def _cell(x, inv_cell):
    return np.floor(np.asarray(x, np.float64) * inv_cell)                       # icp_hist_kernel / icp_iter_kernel (fp64)


def _wall_probes(max_dist):
    """(p, q, label): a transformed source point p (fp64, placed by T_init) within a few ulps of a cell wall on `axes` axes, and a
    lone fp32 target q at |q - p| = max_dist (1 + j 2^-52) along axis 0, on a wall of its own, just past the next wall; on the
    other axes q sits on the wall p is a few ulps short of.  Also the same at max_dist (1 -+ 1e-9)."""
    c = float(max_dist)
    inv = 1.0 / c
    out = []
    for k in (7, -3, 40):
        W = np.float32(k * c)                                                   # an fp32 wall position (as close as fp32 gets)
        for axes in (1, 2, 3):
            for j in list(range(-4, 5)) + ["-1e-9", "+1e-9"]:
                f = 1.0 + (float(j) if isinstance(j, str) else j * 2.0 ** -52)
                q = np.array([W, np.float32((k + 1) * c), np.float32((2 - k) * c)], np.float32)
                p = q.astype(np.float64).copy()
                p[0] = float(q[0]) - c * f
                for b in range(1, axes):
                    p[b] = np.nextafter(np.nextafter(float(q[b]), -np.inf), -np.inf)    # two ulps short of q's wall
                out.append((p, q, f"k{k}-axes{axes}-j{j}"))
    return out, inv


@pytest.mark.parametrize("max_dist", [0.05, 0.6, 2.0, 10.0])
def test_icp_neighbours_on_cell_walls(lr, oracle, max_dist):
    """The contract's computed d2 < max_dist^2 decides, as in the brute-force oracle: the hash grid must find every such neighbour,
    whichever cell the rounded products p * (1 / max_dist) put it in.  One evaluation (max_iter 0) per probe."""
    probes, inv = _wall_probes(max_dist)
    n_in = n_far = 0
    for p, q, label in probes:
        T0 = np.eye(4); T0[:3, 3] = p                                           # source point (0, 0, 0): T_init carries it to p exactly
        src = np.zeros((1, 3), np.float32)
        tgt = np.concatenate([q[None, :], q[None, :] + np.float32(50 * max_dist)]).astype(np.float32)
        T, info = lr.ransac.icp_dev(src, tgt, T0, max_dist=max_dist, max_iter=0)
        _, einfo = oracle.icp(src, tgt, T0, max_dist=max_dist, max_iter=0)
        _, ref = icp_ref.icp(src, tgt, T0, max_dist=max_dist, max_iter=0)
        assert info["n_corr"] == einfo["n_corr"] == ref["n_corr"], (label, info, einfo, ref)
        assert info["inlier_rmse"] == einfo["inlier_rmse"], label
        d = np.abs(_cell(p, inv) - _cell(q.astype(np.float64), inv)).max()
        n_in += ref["n_corr"]
        n_far += d >= 1 and ref["n_corr"] == 1
    assert 0 < n_in < len(probes) and n_far > 0                                 # both sides of the radius, across cell walls


def test_icp_batch_against_reference(lr):
    """lr_register_batch with icp (max_dist 0.6), then lr_icp_batch again at 2.0 m, both per pair against the reference."""
    dev = lr.torch.device("cuda", 0)
    host = [synth.make_pair(N=30000, rho=0.5, s=0.9, seed=600 + k) for k in range(3)]
    pairs = [tuple(lr.torch.from_numpy(p[key]).to(dev) for key in ("xyz0", "xyz1", "feats0", "feats1")) for p in host]
    params = lr.FR.pair_params(Args(mode="MNN", codebase="open3D", iters=2000, ransac_n=3, o3d_conf=1.0, icp=True))
    ws = lr.ext.Workspace(30000, 30000, 32, 2000, max_pairs=len(pairs))
    out = lr.FR.register_batch_dev(pairs, params, ws=ws)
    lr.torch.cuda.synchronize()
    res = [lr.ext.PairResult.from_buffer_copy(out[k].cpu().numpy().tobytes()) for k in range(len(pairs))]
    for k, p in enumerate(host):
        r = res[k]
        T = np.array(r.T[:]).reshape(4, 4)
        Tr, ref = icp_ref.icp(p["xyz0"], p["xyz1"], T, max_dist=0.6)
        _same(dict(n_corr=r.icp.n_corr, iterations=r.icp.iterations, fitness=r.icp.fitness, inlier_rmse=r.icp.inlier_rmse), ref,
              np.array(r.T_icp[:]).reshape(4, 4), Tr)
    lr.ext.check(lr.ext.lib().lr_icp_batch(ws.handle, 2.0, 30, 1e-6, 1e-6, out.data_ptr(), None))
    lr.torch.cuda.synchronize()
    for k, p in enumerate(host):
        r = lr.ext.PairResult.from_buffer_copy(out[k].cpu().numpy().tobytes())
        Tr, ref = icp_ref.icp(p["xyz0"], p["xyz1"], np.array(res[k].T[:]).reshape(4, 4), max_dist=2.0)
        _same(dict(n_corr=r.icp.n_corr, iterations=r.icp.iterations, fitness=r.icp.fitness, inlier_rmse=r.icp.inlier_rmse), ref,
              np.array(r.T_icp[:]).reshape(4, 4), Tr)
