"""The sparse ResUNetBN2C that fcgf.py (three dimensions) and dgr.py's inlier network (six) pack for liblidarreg.so: the plan of its 23
stages (csrc/lr_sparse.h: sp_stage_table) and the BatchNorm fold of a state dict into per-stage (W, scale, offset)."""
import numpy as np
import torch

BN_EPS = 1e-5              # MinkowskiBatchNorm wraps torch.nn.BatchNorm1d and keeps its default
N_STAGES = 23


def stage_plan(widths, nk_conv1, nk, cout_final):
    """The 23 stages in order: (conv module, norm module | None, offsets, Cin, Cout), widths = C1 C2 C3 C4 (down) T4 T3 T2 T1 (up):
    nk_conv1 offsets in conv1, nk in the other convolutions, one in the last two stages."""
    C1, C2, C3, C4, T4, T3, T2, T1 = widths
    plan = [("conv1", "norm1", nk_conv1, 1, C1)]

    def block(name, c):
        return [(f"{name}.conv1", f"{name}.norm1", nk, c, c), (f"{name}.conv2", f"{name}.norm2", nk, c, c)]

    plan += block("block1", C1)
    for i, (cin, cout) in zip((2, 3, 4), ((C1, C2), (C2, C3), (C3, C4))):
        plan += [(f"conv{i}", f"norm{i}", nk, cin, cout)] + block(f"block{i}", cout)
    for i, (cin, cout) in zip((4, 3, 2), ((C4, T4), (T4 + C3, T3), (T3 + C2, T2))):
        plan += [(f"conv{i}_tr", f"norm{i}_tr", nk, cin, cout)] + block(f"block{i}_tr", cout)
    plan += [("conv1_tr", None, 1, T2 + C1, T1), ("final", None, 1, T1, cout_final)]
    assert len(plan) == N_STAGES
    return plan


def packed_floats(plan):
    return sum(k * cin * cout + 2 * cout for _, _, k, cin, cout in plan)


def np64(sd, key, shape, what):
    if key not in sd:
        raise ValueError(f"{what}: missing key {key!r}")
    v = sd[key]
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    v = np.asarray(v, np.float64)
    if shape is not None:
        if v.shape != shape and not (v.size == int(np.prod(shape)) and v.squeeze().shape == tuple(s for s in shape if s != 1)):
            raise ValueError(f"{what}: {key} has shape {v.shape}, expected {shape}")
        v = v.reshape(shape)
    if not np.isfinite(v).all():
        raise ValueError(f"{what}: {key} holds a non-finite value")
    return v


def fold(sd, plan, what, strict, dtype=np.float32):
    """[(W [offsets,Cin,Cout], scale [Cout], offset [Cout])] per stage of `plan`, as `dtype`: BatchNorm folded in fp64 and rounded once
    (float64: not at all).  A 1x1 kernel may be [Cin,Cout] or [1,Cin,Cout]; a missing key, a wrong shape or a non-finite value is a
    ValueError that begins with `what` and names the key; strict: so is a key the plan does not know (num_batches_tracked apart)."""
    known, out = set(), []
    for conv, norm, k, cin, cout in plan:
        W = np64(sd, conv + ".kernel", (k, cin, cout), what)
        known.update((conv + ".kernel", "final.bias"))
        if norm:
            names = [f"{norm}.bn.{f}" for f in ("weight", "bias", "running_mean", "running_var")]
            g, b, mean, var = (np64(sd, nm, (cout,), what) for nm in names)
            known.update(names + [f"{norm}.bn.num_batches_tracked"])
            with np.errstate(invalid="ignore", divide="ignore"):
                scale = g / np.sqrt(var + BN_EPS)
                offset = (0.0 - mean) * scale + b
            if not (np.isfinite(scale).all() and np.isfinite(offset).all()):
                raise ValueError(f"{what}: {norm}.bn.running_var does not fold to a finite scale")
        else:
            scale = np.ones(cout)
            offset = np64(sd, "final.bias", (cout,), what) if conv == "final" else np.zeros(cout)
        out.append((W.astype(dtype), scale.astype(dtype), offset.astype(dtype)))
    extra = sorted(set(sd) - known) if strict else []
    if extra:
        raise ValueError(f"{what}: unexpected key {extra[0]!r}")
    return out


def pack(stages):
    """The flat float32 blob of a network's stages: per stage W, scale, offset."""
    return np.concatenate([np.concatenate([W.reshape(-1), s, o]) for W, s, o in stages]).astype(np.float32, copy=False)


def unpack(blob, plan):
    """pack() undone: the stages of a blob."""
    stages, at = [], 0
    for _, _, k3, cin, cout in plan:
        W = blob[at:at + k3 * cin * cout].reshape(k3, cin, cout); at += k3 * cin * cout
        stages.append((W, blob[at:at + cout], blob[at + cout:at + 2 * cout])); at += 2 * cout
    assert at == len(blob), (at, len(blob))
    return stages
