"""High-precision reference for the fp64 rigid fits (lr_contract.h's Horn solver, lr_teaser.hip's SVD rotation) and the degenerate
inputs they must survive.

The input is exact fp64 data -- float32 clouds up-cast, which is what the kernels see -- and the reference works in mpmath at DPS
digits, so its own rounding is far below anything an fp64 solver can resolve.  Acceptance (eps = 2^-52):
  (a) where kappa * eps < 1e-3: angle(R, R*) <= 32 eps kappa (kappa_raw for paths that form H from raw moments);
  (b) always: R^T R = I and det R = 1 to 1e-12, finite, and f* - tr(R H) <= 32 eps sum w |p| |q|;
  (c) t = c_q - R c_p to 1e-12 (1 + |c|).
kappa = s1 / (s2 + d s3) is the conditioning of the rotation: a perturbation of H by e |H| moves R* by up to about e kappa.
"""
import numpy as np
from mpmath import mp

EPS = 2.0 ** -52
DPS = 40
ALPHA = 32.0              # the constant of (a) and (b)


def _mpm(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], np.float64)


def _det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def fit(P, Q, w=None, centred=True):
    """argmax_R tr(R H) over proper rotations, H = sum w (p - c_p)(q - c_q)^T (centred: Kabsch) or sum w p q^T (centred=False: the
    uncentred fit TEASER runs on its TIMs).  P, Q: [n,3] exact fp64 values.  Returns a dict of fp64 numbers:
      R, t (t = c_q - R* c_p; zero when uncentred), cp, cq, s (singular values, descending), d (sign det(V U^T)),
      kappa = s1 / (s2 + d s3), kappa_raw = sum w |p| |q| / (s2 + d s3) (inf where the denominator is 0), fstar = s1 + s2 + d s3,
      scale = sum w |p| |q| over the raw (uncentred) vectors, H (fp64 rounding of the exact H)."""
    with mp.workdps(DPS):
        P = np.asarray(P, np.float64).reshape(-1, 3)
        Q = np.asarray(Q, np.float64).reshape(-1, 3)
        n = P.shape[0]
        w = np.ones(n) if w is None else np.asarray(w, np.float64)
        Pm = [[mp.mpf(float(v)) for v in r] for r in P]
        Qm = [[mp.mpf(float(v)) for v in r] for r in Q]
        wm = [mp.mpf(float(v)) for v in w]
        W = mp.fsum(wm)
        if centred:
            cp = [mp.fsum(wm[i] * Pm[i][a] for i in range(n)) / W for a in range(3)]
            cq = [mp.fsum(wm[i] * Qm[i][a] for i in range(n)) / W for a in range(3)]
        else:
            cp = [mp.mpf(0)] * 3
            cq = [mp.mpf(0)] * 3
        H = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                H[a, b] = mp.fsum(wm[i] * (Pm[i][a] - cp[a]) * (Qm[i][b] - cq[b]) for i in range(n))
        U, S, Vt = mp.svd_r(H)
        V = Vt.T
        d = mp.mpf(1) if _det3(V * U.T) >= 0 else mp.mpf(-1)
        R = V * mp.diag([1, 1, d]) * U.T
        t = [cq[a] - mp.fsum(R[a, b] * cp[b] for b in range(3)) for a in range(3)]
        s = [S[0], S[1], S[2]]
        den = s[1] + d * s[2]
        scale = mp.fsum(wm[i] * mp.sqrt(mp.fsum(x * x for x in Pm[i])) * mp.sqrt(mp.fsum(x * x for x in Qm[i])) for i in range(n))
        kappa = float(s[0] / den) if den > 0 else float("inf")
        kappa_raw = float(scale / den) if den > 0 else float("inf")
        if s[0] == 0:
            kappa = float("inf")
        return dict(R=_np(R), Rmp=R, t=np.array([float(v) for v in t]), cp=np.array([float(v) for v in cp]),
                    cq=np.array([float(v) for v in cq]), s=np.array([float(v) for v in s]), d=int(d), kappa=kappa, kappa_raw=kappa_raw,
                    fstar=s[0] + s[1] + d * s[2], scale=float(scale), Hmp=H, H=_np(H))


def angle(R, ref):
    """Rotation angle of R R*^T in mpmath (atan2 of the skew and symmetric parts: accurate near 0 and near pi), plus the
    orthogonality defect |R^T R - I|_F so that a non-rotation cannot pass as a small angle."""
    with mp.workdps(DPS):
        Rm = _mpm(np.asarray(R, np.float64)[:3, :3])
        E = Rm * ref["Rmp"].T
        sk = mp.sqrt(mp.fsum((E[i, j] - E[j, i]) ** 2 for i in range(3) for j in range(3)) / 8)
        co = (E[0, 0] + E[1, 1] + E[2, 2] - 1) / 2
        orth = mp.sqrt(mp.fsum(x ** 2 for x in (Rm.T * Rm - mp.eye(3))))
        return float(mp.atan2(sk, co) + orth)


def check(T, ref, raw=False, where=""):
    """(a), (b) and (c) on a 4x4 (or 3x3 when the fit is uncentred) result against fit(...).  Returns the (a) ratio
    angle / (eps kappa) or None where (a) does not apply."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    assert np.all(np.isfinite(T)), f"{where}: non-finite result\n{T}"
    # (b) a proper rotation attaining the optimum
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, f"{where}: R^T R != I\n{R}"
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, f"{where}: det R = {np.linalg.det(R)}"
    with mp.workdps(DPS):
        Rm = _mpm(R)
        trRH = mp.fsum(Rm[i, j] * ref["Hmp"][j, i] for i in range(3) for j in range(3))
        gap = float(ref["fstar"] - trRH)
    assert gap <= ALPHA * EPS * ref["scale"], f"{where}: f* - tr(RH) = {gap:.3e} > {ALPHA * EPS * ref['scale']:.3e}"
    # (c) the translation follows from R
    if T.shape == (4, 4):
        c = ref["cq"] - R @ ref["cp"]
        assert np.abs(T[:3, 3] - c).max() <= 1e-12 * (1.0 + np.abs(ref["cp"]).max() + np.abs(ref["cq"]).max()), \
            f"{where}: t {T[:3, 3]} != c_q - R c_p {c}"
    # (a) forward error within the conditioning
    k = ref["kappa_raw"] if raw else ref["kappa"]
    if not (k * EPS < 1e-3):
        return None
    a = angle(R, ref)
    assert a <= ALPHA * EPS * k, f"{where}: angle {a:.3e} rad > 32 eps kappa = {ALPHA * EPS * k:.3e} (ratio {a / (EPS * k):.1f})"
    return a / (EPS * k)


# ----------------------------------------------------------------------------------------------------------------- generators
def rot(axis, theta):
    """Rodrigues in fp64."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def random_rot(rng):
    return rot(rng.normal(size=3), rng.uniform(0.1, np.pi - 0.1))


def move(P, R, t, rng=None, noise=0.0):
    """q = R p + t (+ noise), both sides rounded to float32 and up-cast: the kernels' input."""
    P = np.asarray(P, np.float64)
    Q = P @ R.T + t
    if noise:
        Q = Q + rng.normal(0, noise, Q.shape)
    return P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)


def near_collinear(rng, n, h, length=2.0, offset=None):
    """n points along a random line of the given length, scattered off it by h * length (the height / length ratio)."""
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    u = np.cross(d, rng.normal(size=3)); u /= np.linalg.norm(u)
    v = np.cross(d, u)
    s = rng.uniform(-0.5, 0.5, n) * length
    s[0], s[1] = -0.5 * length, 0.5 * length
    e = rng.normal(size=(n, 2)) * (h * length)
    P = s[:, None] * d + e[:, :1] * u + e[:, 1:] * v
    return P + (rng.uniform(-3, 3, 3) if offset is None else offset)


def collinear_exact(n, axis=0, step=1.0, start=(0.0, 0.0, 0.0)):
    """(k step) along a coordinate axis from start: exactly representable, exactly collinear after centring for n <= 4."""
    P = np.tile(np.asarray(start, np.float64), (n, 1))
    P[:, axis] += step * np.arange(n)
    return P


def coplanar(rng, n, ground=False, offset=None):
    """n points in a random plane, or on a ground plane z = const."""
    if ground:
        P = np.c_[rng.uniform(-20, 20, (n, 2)), np.full(n, -1.75)]
    else:
        nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
        u = np.cross(nrm, rng.normal(size=3)); u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        c = rng.uniform(-5, 5, (n, 2))
        P = c[:, :1] * u + c[:, 1:] * v
    return P + (0.0 if offset is None else offset)


def near_coplanar(rng, n, h, extent=20.0):
    """A ground-plane patch of the given extent whose height is scattered by h * extent (s3 / s1 ~ h^2)."""
    P = np.c_[rng.uniform(-0.5, 0.5, (n, 2)) * extent, np.full(n, -1.75)]
    P[:, 2] += rng.normal(size=n) * (h * extent)
    return P


def mirrored(rng, P):
    """Q = a rotation of P's mirror image: the best proper rotation has d = -1."""
    return (P * np.array([-1.0, 1.0, 1.0])) @ random_rot(rng).T + rng.uniform(-2, 2, 3)


LIDAR_OFFSET = np.array([80.0, -61.0, 2.5])


def kabsch_cases(seed=0):
    """(name, P, Q, w) over every generator: exact fp64 (float32-representable) coordinates."""
    rng = np.random.default_rng(seed)
    cases = []
    for n in (3, 4, 21, 2000):
        for h in (1e-8, 1e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3, 1e-2, 0.1, 0.3, 1.0):
            reps = 3 if n <= 4 else 1
            for r in range(reps):
                P = near_collinear(rng, n, h)
                cases.append((f"near_collinear n={n} h={h:g} #{r}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    for n in (3, 4, 21):
        for h in (1e-6, 1e-4, 1e-2):
            P = near_collinear(rng, n, h, length=30.0, offset=LIDAR_OFFSET)
            cases.append((f"lidar_offset near_collinear n={n} h={h:g}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    for n in (2, 3, 4):
        for axis in range(3):
            P = collinear_exact(n, axis, 0.5, (1.0, -2.0, 0.25))
            cases.append((f"collinear_exact axis={axis} n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
            Q = collinear_exact(n, (axis + 1) % 3, 0.5, (3.0, 0.5, -1.0))
            cases.append((f"collinear_exact both axis={axis} n={n}", P, Q, None))
    for n in (3, 21, 2000):
        P = near_collinear(rng, n, 0.0)
        cases.append((f"collinear n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    for n in (3, 4, 21, 2000):
        for ground in (False, True):
            P = coplanar(rng, n, ground)
            cases.append((f"coplanar ground={ground} n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3), rng, 0.01), None))
            P = coplanar(rng, n, ground, LIDAR_OFFSET)
            cases.append((f"lidar_offset coplanar ground={ground} n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3), rng, 0.01), None))
    for n in (4, 21, 2000):
        for h in (1e-8, 3e-7, 1e-5, 1e-3):
            P = near_coplanar(rng, n, h)
            cases.append((f"near_coplanar n={n} h={h:g}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    for n in (1, 3, 4, 21):
        P = np.tile(rng.uniform(-5, 5, 3), (n, 1))
        cases.append((f"coincident n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    P = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, -1.0, 0.5]])
    cases.append(("duplicate point n=3", *move(P, random_rot(rng), rng.uniform(-5, 5, 3)), None))
    for n in (3, 4, 21, 2000):
        P = rng.uniform(-5, 5, (n, 3))
        Q = mirrored(rng, P)
        cases.append((f"mirror n={n}", P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64), None))
        P = coplanar(rng, n)
        Q = mirrored(rng, P) + rng.normal(0, 0.01, P.shape)
        cases.append((f"mirror coplanar n={n}", P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64), None))
    for theta in (np.pi, np.pi - 1e-7, 1e-9, 0.0):
        for n in (3, 4, 21, 2000):
            P = rng.uniform(-5, 5, (n, 3))
            cases.append((f"angle={theta:.9g} n={n}", *move(P, rot(rng.normal(size=3), theta), rng.uniform(-5, 5, 3)), None))
        P = rng.uniform(-5, 5, (21, 3))
        cases.append((f"angle={theta:.9g} x-axis n=21", *move(P, rot((1, 0, 0), theta), np.zeros(3)), None))
    for n in (3, 21, 2000):
        P = rng.uniform(-20, 20, (n, 3)) + LIDAR_OFFSET
        cases.append((f"lidar_offset n={n}", *move(P, random_rot(rng), rng.uniform(-5, 5, 3), rng, 0.02), None))
    for n in (4, 21, 2000):
        P = rng.uniform(-5, 5, (n, 3))
        Pm, Qm = move(P, random_rot(rng), rng.uniform(-5, 5, 3), rng, 0.05)
        w = rng.uniform(0.1, 2.0, n)
        w[: n // 3] = 0.0
        cases.append((f"weights zeros n={n}", Pm, Qm, w))
        w = np.full(n, 1e-6)
        w[n // 2] = 1.0
        w[n // 2 + 1] = 1.0
        cases.append((f"weights dominant n={n}", Pm, Qm, w))
        w = np.zeros(n)
        w[:3] = 1.0
        cases.append((f"weights three live n={n}", Pm, Qm, w))
    return cases


def teaser_cases(seed=0):
    """(name, a, b) correspondence sets that are fully consistent (noise << beta): collinear, axis-aligned collinear, coplanar,
    coincident, and s2 / s1 and s3 / s1 on either side of the solver's 1e-14 rank branch.  float32."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, A, R=None, t=None):
        R = random_rot(rng) if R is None else R
        t = rng.uniform(-5, 5, 3) if t is None else t
        a, b = move(A, R, t)
        cases.append((name, a.astype(np.float32), b.astype(np.float32)))

    add("collinear_exact x n=4", collinear_exact(4, 0, 1.0, (0.0, 0.0, 0.0)))
    add("collinear_exact z n=6", collinear_exact(6, 2, 0.5, (1.0, 2.0, 0.0)))
    add("collinear_exact x identity n=4", collinear_exact(4, 0, 1.0, (0.0, 0.0, 0.0)), np.eye(3), np.zeros(3))
    add("collinear n=12", near_collinear(rng, 12, 0.0, length=10.0))
    add("near_collinear 1e-9 n=12", near_collinear(rng, 12, 1e-9, length=10.0))
    add("near_collinear 1e-6 n=12", near_collinear(rng, 12, 1e-6, length=10.0))
    add("near_collinear 1e-3 n=12", near_collinear(rng, 12, 1e-3, length=10.0))
    add("near_collinear 3e-7 n=12 (s2/s1 above 1e-14)", near_collinear(rng, 12, 3e-7, length=10.0))
    add("near_collinear 1e-8 n=12 (s2/s1 below 1e-14)", near_collinear(rng, 12, 1e-8, length=10.0))
    add("near_coplanar 3e-7 n=16 (s3/s1 above 1e-14)", near_coplanar(rng, 16, 3e-7))
    add("near_coplanar 1e-8 n=16 (s3/s1 below 1e-14)", near_coplanar(rng, 16, 1e-8))
    add("coplanar n=10", coplanar(rng, 10))
    add("coplanar ground n=30", coplanar(rng, 30, ground=True))
    add("coincident n=5", np.tile(rng.uniform(-5, 5, 3), (5, 1)))
    add("coincident pairs n=6", np.repeat(rng.uniform(-5, 5, (2, 3)), 3, axis=0))
    add("general n=10", rng.uniform(-5, 5, (10, 3)))
    return cases
