"""The oracle's fp64 Kabsch (csrc/lr_contract.h, the text the kernels compile too) against a 40-digit SVD Kabsch (tests/rigid_hp.py) over thin, flat,
coincident, mirrored and far-offset geometry: the bit-identity of oracle and device cannot catch a flaw they share."""
import ctypes

import numpy as np
import pytest

from tests import rigid_hp as hp

CASES = hp.kabsch_cases(0)
UNWEIGHTED = [c for c in CASES if c[3] is None]


def _moments(oracle, P, Q):
    """orc_kabsch_moments: the raw-moment form (n, sum p, sum q, sum p q^T) the refit, the local optimisation and ICP use."""
    f64 = ctypes.POINTER(ctypes.c_double)
    sp, sq = np.ascontiguousarray(P.sum(0)), np.ascontiguousarray(Q.sum(0))
    spq = np.ascontiguousarray((P.T @ Q).reshape(9))
    T = np.empty(16)
    oracle.lib().orc_kabsch_moments(ctypes.c_double(float(P.shape[0])), sp.ctypes.data_as(f64), sq.ctypes.data_as(f64),
                                    spq.ctypes.data_as(f64), T.ctypes.data_as(f64))
    return T.reshape(4, 4)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_kabsch_points_against_hp(oracle, case):
    name, P, Q, w = case
    hp.check(oracle.kabsch(P, Q, w), hp.fit(P, Q, w), where=name)


@pytest.mark.parametrize("case", UNWEIGHTED, ids=[c[0] for c in UNWEIGHTED])
def test_oracle_kabsch_moments_against_hp(oracle, case):
    name, P, Q, _ = case
    hp.check(_moments(oracle, P, Q), hp.fit(P, Q), raw=True, where=name)


def test_near_collinear_sweep_three_and_four_points(oracle):
    """The band where Newton's root is accepted but the adjugate vector carried eps kappa^2: many seeds of 3- and 4-point samples,
    height / length from 3e-6 to 0.3 (the worst ratio angle / (eps kappa) was 1e5 before the Rayleigh-quotient pass)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in (3, 4):
        for h in np.geomspace(3e-6, 0.3, 11):
            for _ in range(12):
                P, Q = hp.move(hp.near_collinear(rng, n, h), hp.random_rot(rng), rng.uniform(-5, 5, 3))
                r = hp.check(oracle.kabsch(P, Q), hp.fit(P, Q), where=f"n={n} h={h:.2g}")
                worst = max(worst, r or 0.0)
    assert worst > 0.0


# ----------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_matches_numpy_svd_on_general_data():
    rng = np.random.default_rng(1)
    P = rng.uniform(-5, 5, (50, 3))
    R0 = hp.random_rot(rng)
    P, Q = hp.move(P, R0, rng.uniform(-5, 5, 3), rng, 0.01)
    ref = hp.fit(P, Q)
    cp, cq = P.mean(0), Q.mean(0)
    U, S, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    R = Vt.T @ np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    np.testing.assert_allclose(ref["R"], R, atol=1e-13)
    np.testing.assert_allclose(ref["t"], cq - R @ cp, atol=1e-12)
    np.testing.assert_allclose(ref["s"], S, rtol=1e-12)
    assert ref["d"] == 1 and abs(ref["kappa"] - S[0] / (S[1] + S[2])) <= 1e-12 * ref["kappa"]
    # the mirror image needs d = -1
    ref = hp.fit(P, P * np.array([-1.0, 1.0, 1.0]))
    assert ref["d"] == -1 and abs(np.linalg.det(ref["R"]) - 1.0) < 1e-14


@pytest.mark.parametrize("theta", [1e-9, 1e-4, 1.0, np.pi - 1e-7, np.pi])
def test_angle_helper_accurate_near_zero_and_pi(theta):
    """angle(R, R*) resolves 1e-9 rad next to the identity and next to a half turn (arccos((tr - 1) / 2) bottoms out at 1e-8)."""
    rng = np.random.default_rng(3)
    axis = rng.normal(size=3)
    Rs = hp.rot(axis, theta)
    ref = dict(Rmp=hp._mpm(Rs))
    for d in (1e-9, 1e-12):
        got = hp.angle(hp.rot(rng.normal(size=3), d) @ Rs, ref)
        assert abs(got - d) <= 1e-3 * d + 4 * hp.EPS, (theta, d, got)


def test_check_rejects_non_rotations_and_wrong_rolls():
    """(b) catches what a rank-deficient SVD completion produces -- the singular R = v1 u1^T of collinear points -- and a reflection;
    (a) catches a roll about a determined axis that (b) alone would miss."""
    P = hp.collinear_exact(4, 0, 1.0)
    P, Q = hp.move(P, hp.rot((1, 2, 3), 0.7), np.zeros(3))
    ref = hp.fit(P, Q)
    v1 = ref["R"][:, 0]
    T = np.eye(4); T[:3, :3] = np.outer(v1, [1.0, 0.0, 0.0]); T[:3, 3] = ref["cq"] - T[:3, :3] @ ref["cp"]
    with pytest.raises(AssertionError, match="R\\^T R"):
        hp.check(T, ref)
    rng = np.random.default_rng(2)
    P, Q = hp.move(rng.uniform(-5, 5, (10, 3)), hp.rot((0, 0, 1), 0.3), np.ones(3))
    ref = hp.fit(P, Q)
    T = np.eye(4); T[:3, :3] = ref["R"] @ np.diag([1.0, 1.0, -1.0]); T[:3, 3] = ref["cq"] - T[:3, :3] @ ref["cp"]
    with pytest.raises(AssertionError, match="det R"):
        hp.check(T, ref)
    T = np.eye(4); T[:3, :3] = hp.rot((1, 0, 0), 1e-12) @ ref["R"]; T[:3, 3] = ref["cq"] - T[:3, :3] @ ref["cp"]
    with pytest.raises(AssertionError, match="32 eps kappa"):
        hp.check(T, ref)
    T = np.eye(4); T[:3, :3] = ref["R"]; T[:3, 3] = ref["t"]
    assert hp.check(T, ref) <= 1.0
