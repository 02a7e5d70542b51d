"""Every device entry point that fits a rotation -- lr_kabsch, RANSAC's minimal-sample fits, lr_refit, lr_teaser, lr_icp -- against the
40-digit reference of tests/rigid_hp.py on degenerate geometry.  Each sums in its own order, so each is checked on its own."""
import numpy as np
import pytest

from tests import rigid_hp as hp

pytestmark = pytest.mark.gpu

CASES = hp.kabsch_cases(0)
SMALL = [c for c in CASES if c[3] is None and c[1].shape[0] in (3, 4)]


@pytest.fixture(scope="module")
def lib():
    import torch
    from lidarregistration_amd import _ext, ransac, teaser
    _ext.build()
    assert torch.cuda.is_available()
    return ransac, teaser


def test_lr_kabsch_against_hp(lib):
    ransac, _ = lib
    for name, P, Q, w in CASES:
        hp.check(ransac.kabsch_dev(P, Q, w), hp.fit(P, Q, w), where=name)


@pytest.mark.parametrize("ns", [3, 4])
def test_ransac_minimal_sample_fit_against_hp(lib, ns):
    """m = sample_size with unique-index sampling: every hypothesis is a fit of exactly the m points (in some order), and with no
    pre-check and no local optimisation the returned model is one of them."""
    import torch
    ransac, _ = lib
    n_done = 0
    for name, P, Q, _ in SMALL:
        if P.shape[0] != ns:
            continue
        src = torch.from_numpy(P.astype(np.float32)).cuda()
        tgt = torch.from_numpy(Q.astype(np.float32)).cuda()
        T, info = ransac.ransac_dev(src, tgt, 32, sample_size=ns, use_elc=False, thr=0.6, seed=5, sampler=2, local_opt=0)
        assert info["best_h"] >= 0, name
        hp.check(T, hp.fit(P, Q), where=name)
        n_done += 1
    assert n_done >= 40


def _refit_scene(rng, n, offset, pole):
    """n source points, ~60 % inliers (noise <= 0.1, |error| < 0.5) and outliers displaced by >= 1.2 under thr = 0.6: no pair
    near the threshold."""
    if pole:
        P = hp.near_collinear(rng, n, 1e-3, length=4.0, offset=offset)
    else:
        P = np.c_[rng.uniform(-40, 40, (n, 2)), rng.uniform(-2, 8, n)] + offset
    R0, t0 = hp.random_rot(rng), rng.uniform(-3, 3, 3)
    Q = P @ R0.T + t0
    inl = rng.random(n) < 0.6
    e = rng.normal(size=(n, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    Q = Q + e * np.where(inl, rng.uniform(0.0, 0.1, n), rng.uniform(1.2, 5.0, n))[:, None]
    P32, Q32 = P.astype(np.float32), Q.astype(np.float32)
    T0 = np.eye(4); T0[:3, :3] = R0; T0[:3, 3] = t0
    d = np.linalg.norm(P32.astype(np.float64) @ R0.T + t0 - Q32.astype(np.float64), axis=1)
    assert np.all(np.abs(d - 0.6) > 1e-3)
    return P32, Q32, T0, d < 0.6


@pytest.mark.parametrize("kind", ["scene", "pole_at_80m"])
def test_lr_refit_against_hp(lib, kind):
    ransac, _ = lib
    rng = np.random.default_rng(11)
    P, Q, T0, inl = _refit_scene(rng, 30000 if kind == "scene" else 3000, hp.LIDAR_OFFSET if kind == "pole_at_80m" else 0.0,
                                 kind == "pole_at_80m")
    T, n = ransac.refit_dev(P, Q, np.arange(P.shape[0], dtype=np.int32), T0, thr=0.6)
    assert n == int(inl.sum())
    ref = hp.fit(P[inl].astype(np.float64), Q[inl].astype(np.float64))
    hp.check(T, ref, raw=True, where=kind)


def test_lr_teaser_degenerate_against_hp(lib):
    """Fully consistent sets (noise << beta): the clique is every point and GNC does not start, so R is the uncentred fit of the chain
    TIMs.  Collinear and coincident sets have rank-deficient H: R must still be a proper rotation attaining the optimum."""
    _, teaser = lib
    for name, a, b in hp.teaser_cases(0):
        T, info, clique = teaser.teaser_dev(a, b)
        assert info["status"] == 0, (name, info)
        assert np.array_equal(clique, np.arange(a.shape[0])), (name, clique)
        A, B = a.astype(np.float64), b.astype(np.float64)
        ref = hp.fit(np.roll(A, -1, 0) - A, np.roll(B, -1, 0) - B, centred=False)
        hp.check(T[:3, :3], ref, raw=True, where=name)
        res = np.linalg.norm(B - (A @ T[:3, :3].T + T[:3, 3]), axis=1)
        assert res.max() <= 0.3, (name, res.max())


def test_lr_icp_one_iteration_near_planar(lib):
    """A ground-plane grid at LiDAR range, one ICP step from a start within 1 cm of every pair: the pairing is the identity, and by
    the fit's rigid equivariance the result is the Kabsch fit of the pairs themselves."""
    ransac, _ = lib
    rng = np.random.default_rng(13)
    g = np.arange(-20.0, 20.0, 0.5)
    X, Y = np.meshgrid(g, g)
    P = np.c_[X.ravel(), Y.ravel(), np.full(X.size, -1.75) + rng.normal(0, 1e-4, X.size)] + hp.LIDAR_OFFSET
    R0, t0 = hp.rot((0.1, 0.2, 1.0), 0.4), np.array([1.0, -2.0, 0.1])
    P, Q = hp.move(P, R0, t0)
    Ti = np.eye(4); Ti[:3, :3] = hp.rot((1, -1, 0.5), 1e-4) @ R0; Ti[:3, 3] = t0 + 2e-3
    assert np.abs(P @ Ti[:3, :3].T + Ti[:3, 3] - Q).max() < 0.02
    T, info = ransac.icp_dev(P.astype(np.float32), Q.astype(np.float32), Ti, max_dist=0.2, max_iter=1)
    assert info["n_corr"] == P.shape[0] and info["iterations"] == 1
    hp.check(T, hp.fit(P, Q), raw=True, where="icp")
