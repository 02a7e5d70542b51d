"""Inputs of the PointDSC encoder tests: seeded weights under the reference's state-dict names and seeded correspondence sets.  Nothing
here is read from a file; tests/golden/make_golden_pdsc.py runs the reference on exactly these and records what it returns."""
import functools
import hashlib

import numpy as np

C = 128
GOLDEN = tuple((m, 12) for m in (1, 2, 3, 31, 32, 33, 64, 65, 129, 257, 1000)) + ((257, 1), (257, 2))
SIGMA_D = float(np.float32(1.2))    # the reference holds sigma_spat as a float32 parameter: this is the value its arithmetic sees
FEATURE_ROWS = 32          # rows of a golden case whose features are recorded


def golden_name(m, num_layers):
    return f"m{m}_L{num_layers}"


def _conv(rng, n_out, n_in, gain=1.0):
    """Conv1d(kernel 1) at Xavier scale (PointDSC.py:118), bias as torch's default range."""
    w = rng.standard_normal((n_out, n_in, 1)) * (gain * np.sqrt(2.0 / (n_in + n_out)))
    b = rng.uniform(-1.0, 1.0, n_out) / np.sqrt(n_in)
    return w.astype(np.float32), b.astype(np.float32)


def _bn(rng, n):
    """BatchNorm1d in inference mode with statistics that are not the identity."""
    return dict(weight=rng.uniform(0.5, 1.5, n).astype(np.float32), bias=(0.1 * rng.standard_normal(n)).astype(np.float32),
                running_mean=(0.2 * rng.standard_normal(n)).astype(np.float32), running_var=rng.uniform(0.5, 1.5, n).astype(np.float32),
                num_batches_tracked=np.int64(1000))


def weights(seed, num_layers, scale=1.0):
    """A full state dict of models.PointDSC.PointDSC(num_layers=num_layers) as float32 arrays (num_batches_tracked int64), in the model's
    own key order.  scale multiplies the q and k projections' weights and biases: the attention logits grow by scale^2, which is what
    stresses the online softmax (scaling every layer would only overflow the activations)."""
    rng = np.random.default_rng([seed, num_layers])
    sd = {"sigma": np.array([1.0], np.float32), "sigma_spat": np.array([SIGMA_D], np.float32)}

    def conv(name, n_out, n_in, gain=1.0):
        w, b = _conv(rng, n_out, n_in, gain)
        sd[name + ".weight"], sd[name + ".bias"] = w, (b * gain).astype(np.float32)

    def bn(name, n):
        for k, v in _bn(rng, n).items():
            sd[f"{name}.{k}"] = v

    conv("encoder.layer0", C, 6)
    for i in range(num_layers):
        p, q = f"encoder.blocks.PointCN_layer_{i}", f"encoder.blocks.NonLocal_layer_{i}"
        conv(p + ".0", C, C); bn(p + ".1", C)
        conv(q + ".fc_message.0", C // 2, C); bn(q + ".fc_message.1", C // 2)
        conv(q + ".fc_message.3", C // 2, C // 2); bn(q + ".fc_message.4", C // 2)
        conv(q + ".fc_message.6", C, C // 2)
        conv(q + ".projection_q", C, C, scale); conv(q + ".projection_k", C, C, scale); conv(q + ".projection_v", C, C)
    conv("classification.0", 32, C); conv("classification.2", 32, 32); conv("classification.4", 1, 32)
    return sd


@functools.lru_cache(maxsize=None)
def shared_weights(num_layers, scale=1.0):
    """weights(24, num_layers, scale), built once per process (read-only)."""
    sd = weights(24, num_layers, scale)
    for v in sd.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sd


def _motion(rng):
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return R, rng.uniform(-5.0, 5.0, 3) * np.array([1.0, 1.0, 0.1])


def _box(rng, m):
    return rng.uniform(-0.5, 0.5, (m, 3)) * np.array([80.0, 80.0, 6.0])


def planted(m, seed=0, inlier_ratio=0.2, noise=0.05):
    """m correspondences over an 80 x 80 x 6 m extent: a planted rigid motion on inlier_ratio of them (5 cm noise), the rest uniform."""
    rng = np.random.default_rng([seed, m, 1])
    R, t = _motion(rng)
    src = _box(rng, m)
    tgt = src @ R.T + t + noise * rng.standard_normal((m, 3))
    out = rng.random(m) >= inlier_ratio
    tgt[out] = _box(rng, int(out.sum()))
    return src.astype(np.float32), tgt.astype(np.float32)


def all_outliers(m, seed=0):
    return planted(m, seed, inlier_ratio=0.0)


def coincident(m, seed=0):
    """Every keypoint is one of five: most pairwise distances are exactly 0 on both sides."""
    src, tgt = planted(5, seed, inlier_ratio=1.0)
    pick = np.random.default_rng([seed, m, 2]).integers(0, 5, m)
    return src[pick].copy(), tgt[pick].copy()


def far_offset(m, seed=0):
    """The planted case moved by +1000 m in the source and -1000 m in the target: coordinates of 1e3 with differences of metres."""
    src, tgt = planted(m, seed)
    return (src + np.float32(1000.0)).astype(np.float32), (tgt - np.float32(1000.0)).astype(np.float32)


def nonfinite(m, seed=0):
    """The planted case with NaN / +Inf / -Inf in some rows: (src, tgt, indices of the dead rows, ascending)."""
    src, tgt = planted(m, seed)
    rng = np.random.default_rng([seed, m, 3])
    bad = np.sort(rng.choice(m, size=max(3, m // 16), replace=False))
    for n, i in enumerate(bad):
        (src if n & 1 else tgt)[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    return src, tgt, bad


def dead_block(m, lo, hi, keep=()):
    """The planted case with the rows lo .. hi-1 (but those in `keep`) dead as a block: NaN, +Inf, -Inf in turn, in src or tgt as
    nonfinite() places them: (src, tgt, indices of the dead rows, ascending)."""
    src, tgt = planted(m)
    bad = np.array([i for i in range(lo, hi) if i not in keep], np.int64)
    for n, i in enumerate(bad):
        (src if n & 1 else tgt)[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    return src, tgt, bad


# The attention plans above m = 8192 (pd_make_plan): the full 512-block grid, the first m of 7, 6, 4, 3 and 2 chunks and the contract's
# largest m at one layer (one attention pass is what the plan changes); the first m of 5 chunks -- the plan of the CLI's 12 000 rows -- at
# full depth.  Recorded by tests/golden/make_golden_pdsc_large.py.
LARGE = tuple((m, 1) for m in (8192, 8193, 9345, 13057, 16385, 21761, 32768)) + ((10881, 12),)


def large_case(m, num_layers):
    src, tgt = planted(m)
    return dict(name=golden_name(m, num_layers), m=m, num_layers=num_layers, src=src, tgt=tgt, sd=shared_weights(num_layers))


def conf_rows(m):
    """The rows of a large case whose fp64 confidence is recorded: 128 b + ((37 b + 32 w) mod 128) for every query block b and w = 0 .. 3
    -- four rows of every block, one per wave, the lane moving from block to block -- as far as they lie below m, and row m - 1."""
    b, w = np.meshgrid(np.arange((m + 127) // 128, dtype=np.int64), np.arange(4, dtype=np.int64), indexing="ij")
    rows = (128 * b + (37 * b + 32 * w) % 128).reshape(-1)
    return np.unique(np.concatenate([rows[rows < m], [m - 1]]))


def golden_case(m, num_layers):
    src, tgt = planted(m, seed=m + num_layers)
    return dict(name=golden_name(m, num_layers), m=m, num_layers=num_layers, src=src, tgt=tgt, sd=shared_weights(num_layers))


def feature_rows(m):
    """The rows of a golden case whose fp64 features are recorded: spread over the whole range, first and last included."""
    return np.unique(np.linspace(0, m - 1, min(m, FEATURE_ROWS)).round().astype(np.int64))


def checksum(case):
    """sha256 over the case's inputs and weights: a fixture belongs to the inputs it was recorded from."""
    h = hashlib.sha256()
    h.update(case["src"].tobytes()); h.update(case["tgt"].tobytes())
    for k, v in case["sd"].items():
        h.update(k.encode()); h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()
