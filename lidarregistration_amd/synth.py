"""Synthetic FCGF-like pairs: there are no datasets or trained FCGF weights here (the network itself is
lidarregistration_amd.fcgf; with a checkpoint it computes real descriptors from a raw scan).

A pair is two clouds with a planted rigid motion and partial overlap ``rho``; descriptors are
32-d unit vectors (the reference L2-normalises FCGF output, Experiments/misc/fcgf.py:387-391)
whose partner rows are noisy copies (noise scale ``s``), so that feature-space NN recovers a
controllable fraction of true correspondences.
"""
import numpy as np


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _partner_perm(n0, n1, rho, rng):
    """Which rows of cloud 1 are partners of which rows of cloud 0 (K = floor(rho*min(n0,n1)))."""
    k = int(rho * min(n0, n1))
    src_rows = rng.permutation(n0)[:k]
    order1 = rng.permutation(n1)
    return k, src_rows, order1


def make_features(n0, n1, d=32, rho=0.5, s=1.2, seed=51):
    rng = np.random.default_rng(seed)
    k, src_rows, order1 = _partner_perm(n0, n1, rho, rng)
    F0 = _unit(rng.standard_normal((n0, d)))
    F1 = np.empty((n1, d), np.float32)
    F1[order1[:k]] = _unit(F0[src_rows] + s * rng.standard_normal((k, d)) / np.sqrt(d))
    F1[order1[k:]] = _unit(rng.standard_normal((n1 - k, d)))
    return F0, F1


def random_motion(rng, max_t_xy=30.0):
    yaw = rng.uniform(-np.pi, np.pi)
    roll, pitch = np.radians(rng.uniform(-2, 2, 2))
    cz, sz = np.cos(yaw), np.sin(yaw)
    cy, sy = np.cos(pitch), np.sin(pitch)
    cx, sx = np.cos(roll), np.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [rng.uniform(-max_t_xy, max_t_xy), rng.uniform(-max_t_xy, max_t_xy), rng.uniform(-0.5, 0.5)]
    return T


def make_clouds(n0, n1, rho=0.5, seed=51, clustered=False, noise=0.05):
    """xyz0 [n0,3] f32, xyz1 [n1,3] f32, T_gt 4x4 f64 with xyz1[partner] ~ R xyz0 + t.

    Uses the same partner permutation as ``make_features`` for the same (n0, n1, rho, seed).
    ``clustered`` concentrates x,y around a few centres so that GPF grid cells are unevenly filled.
    """
    rng = np.random.default_rng(seed)
    k, src_rows, order1 = _partner_perm(n0, n1, rho, rng)
    rng = np.random.default_rng(seed + 1000003)

    def box(n):
        if clustered:
            c = rng.uniform(-60, 60, (6, 2))
            xy = c[rng.integers(0, 6, n)] + rng.normal(0, 12.0, (n, 2))
            xy = np.clip(xy, -80, 80)
        else:
            xy = rng.uniform(-80, 80, (n, 2))
        return np.concatenate([xy, rng.uniform(-3, 5, (n, 1))], axis=1)

    xyz0 = box(n0)
    T = random_motion(rng)
    xyz1 = np.empty((n1, 3))
    xyz1[order1[:k]] = xyz0[src_rows] @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (k, 3))
    xyz1[order1[k:]] = box(n1 - k)
    return xyz0.astype(np.float32), xyz1.astype(np.float32), T


def make_pair(N=30000, D=32, rho=0.5, s=1.2, seed=51, N1=None, clustered=False):
    """dict(xyz0, xyz1, feats0, feats1, T_gt) -- BASELINE config #2 uses the defaults."""
    N1 = N if N1 is None else N1
    F0, F1 = make_features(N, N1, D, rho, s, seed)
    xyz0, xyz1, T = make_clouds(N, N1, rho, seed, clustered=clustered)
    return dict(xyz0=xyz0, xyz1=xyz1, feats0=F0, feats1=F1, T_gt=T)


def make_pair_dev(N=30000, D=32, rho=0.5, s=1.2, seed=51, device=None, noise=0.05, T_gt=None):
    """The recipe of ``make_pair`` drawn with torch's generator on `device` (milliseconds instead of a quarter second per
    30k-point pair, so a benchmark can hold hundreds of distinct pairs): same distributions, different numbers.
    T_gt: plant this 4x4 motion instead of a random one (the list-driven surrogate: a row's ground truth and overlap).
    Returns dict(xyz0, xyz1, feats0, feats1) of float32 device tensors and T_gt (4x4 float64 numpy)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    k = int(rho * N)

    def unit(x):
        return x / x.norm(dim=1, keepdim=True)

    def box(n):
        xy = torch.rand((n, 2), generator=g, device=device) * 160 - 80
        z = torch.rand((n, 1), generator=g, device=device) * 8 - 3
        return torch.cat([xy, z], dim=1)

    src_rows = torch.randperm(N, generator=g, device=device)[:k]
    order1 = torch.randperm(N, generator=g, device=device)
    F0 = unit(torch.randn((N, D), generator=g, device=device))
    F1 = torch.empty((N, D), device=device)
    F1[order1[:k]] = unit(F0[src_rows] + s * torch.randn((k, D), generator=g, device=device) / np.sqrt(D))
    F1[order1[k:]] = unit(torch.randn((N - k, D), generator=g, device=device))
    T = random_motion(np.random.default_rng(seed + 1000003)) if T_gt is None else np.asarray(T_gt, np.float64).reshape(4, 4)
    Tt = torch.from_numpy(T).to(device=device, dtype=torch.float32)
    xyz0 = box(N)
    xyz1 = torch.empty((N, 3), device=device)
    xyz1[order1[:k]] = xyz0[src_rows] @ Tt[:3, :3].T + Tt[:3, 3] + noise * torch.randn((k, 3), generator=g, device=device)
    xyz1[order1[k:]] = box(N - k)
    return dict(xyz0=xyz0.contiguous(), xyz1=xyz1.contiguous(), feats0=F0.contiguous(), feats1=F1.contiguous(), T_gt=T)


def _scan_frame(rng, n, pose, reach):
    """One frame of make_scan_pair's scene seen from `pose` (4x4, scene -> frame), in the frame's coordinates."""
    r = reach * rng.uniform(size=n) ** 2 + 1.5                       # density falls with range
    phi = rng.uniform(0, 2 * np.pi, size=n)
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros(n)], axis=1)
    world = (local - pose[:3, 3]) @ pose[:3, :3]                      # inverse of `pose`: scene coordinates of the returns
    x, y = world[:, 0], world[:, 1]
    z = 0.3 * np.sin(0.2 * x) * np.cos(0.15 * y) - 1.7
    wall = rng.uniform(size=n) < 0.35
    z = np.where(wall, z + rng.uniform(0, 6, size=n), z)
    x = np.where(wall, np.round(x / 7.0) * 7.0, x)
    world = np.stack([x, y, z], axis=1) + rng.normal(scale=0.02, size=(n, 3))
    return world @ pose[:3, :3].T + pose[:3, 3]


def make_scan_pair(n0=120000, n1=None, seed=51, forward=8.0, yaw_deg=5.0, reach=80.0):
    """Two raw LiDAR-like frames (float64, like the reference's cloud cache) of one scene seen from two poses `forward` metres and `yaw_deg`
    apart, and the 4x4 motion frame 0 -> frame 1: range-dependent density (most returns near the sensor), a rolling ground, facades on a
    7 m street grid.  What the overlap measure and the Open3D-style down-sampling are timed on (tools/overlap_bench.py)."""
    n1 = n0 if n1 is None else n1
    rng = np.random.default_rng(seed)
    a = np.radians(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [-forward, 0.3, 0.0]

    return _scan_frame(rng, n0, np.eye(4), reach), _scan_frame(rng, n1, T, reach), T


class SyntheticSessions:
    """A dataset of make_session drives with the members the balanced-set generator asks of a full dataset (balanced.py): load_PC,
    get_relative_motion, session_length, indexing_from, total_num_of_clouds, sessions_list, time_step, name, phase."""

    def __init__(self, sessions, name="Synthetic", phase="test", time_step=0.1):
        self.sessions = dict(sessions)                  # session index -> make_session's dict
        self.sessions_list = list(self.sessions)
        self.name, self.phase, self.time_step = name, phase, float(time_step)

    def indexing_from(self):
        return 0

    def session_length(self, session_ind):
        return len(self.sessions[session_ind]["clouds"])

    def total_num_of_clouds(self):
        return sum(len(s["clouds"]) for s in self.sessions.values())

    def load_PC(self, session_ind, i):
        return self.sessions[session_ind]["clouds"][i]

    def get_relative_motion(self, session_ind, i, j):
        """4x4 motion frame i -> frame j."""
        poses = self.sessions[session_ind]["poses"]
        return poses[j] @ np.linalg.inv(poses[i])


def make_session(n_frames=40, n_points=6000, seed=51, step=2.5, yaw_step_deg=1.5, reach=80.0):
    """A short synthetic drive: n_frames scans (float64 [n_points,3]) of make_scan_pair's static scene from poses `step` metres and
    `yaw_step_deg` apart along a curve whose curvature swings slowly, with a little pitch, roll and heave.  dict(clouds, poses): poses[i] maps scene coordinates to frame i, so
    frame i -> frame j is poses[j] @ inv(poses[i]).  SyntheticSessions({0: make_session(...)}) is a dataset without any download."""
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    pose = np.eye(4)
    for i in range(n_frames):
        poses.append(pose.copy())
        clouds.append(_scan_frame(rng, n_points, pose, reach))
        a = np.radians(yaw_step_deg * np.cos(2.0 * np.pi * i / 25.0))
        b, c = np.radians(0.3 * np.sin(0.5 * i)), np.radians(0.2 * np.cos(0.9 * i))      # a little pitch and roll: no motion field stays constant
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
        hop = np.eye(4)
        hop[:3, :3] = Rz @ Ry @ Rx
        hop[:3, 3] = [-step, 0.02 * np.sin(0.7 * i), 0.03 * np.sin(0.4 * i)]
        pose = hop @ pose
    return dict(clouds=clouds, poses=poses)
