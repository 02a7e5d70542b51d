"""What the reference's GlobalRegistration returns on the golden cases of tests/dgr_cases.py, recorded -- not restated.

Runs only where the reference tree exists.  DGR/core/registration.py is imported as it is (plain torch, CPU) and GlobalRegistration is
called the way DeepGlobalRegistration.register calls it (deep_global_registration.py:415-421: break_threshold_ratio 1e-4,
quantization_size 2 * voxel).  Two observers, neither changing a value: the loss object handed in as `loss_fn` is the reference's own
HighDimSmoothL1Loss behind a wrapper that notes every value it returns (the first is loss_prev, then one per iteration), and
weighted_procrustes is wrapped to note the init.  Each case runs twice:
  * float32, as shipped;
  * torch's default dtype float64, so that the parameters, the loss and Adam run in float64.  weighted_procrustes ends in .float() and mixes
    that result with the default dtype, which raises in float64; the wrapper runs it on the float32 inputs and widens its result.
Stored per case in g27_dgr.npz: a checksum of the inputs, the init, and per run the losses of all iterations, iterations, break_count, the
final loss, R, t.

The generator asserts that every stable case has the same iterations and break_count in both precisions, and that at most one case is
marked unstable.

    python tests/golden/make_golden_dgr.py
"""
import os
import sys

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run(torch, cr, loss_mod, c, P, dtype):
    torch.set_default_dtype(dtype)
    torch.manual_seed(0)
    seen = {"losses": []}
    orig = cr.weighted_procrustes

    def watch_fit(X, Y, w, eps):
        R, t = orig(X.float(), Y.float(), w.float(), eps)
        seen["R0"], seen["t0"] = R.double().numpy().copy(), t.double().numpy().ravel().copy()
        return R.to(X.dtype), t.to(X.dtype)

    class Watch:
        def __init__(self, inner):
            self.inner, self.eps = inner, inner.eps

        def __call__(self, X, Y):
            v = self.inner(X, Y)
            seen["losses"].append(v.item())
            return v

    X, Y = torch.from_numpy(c["src"]).to(dtype), torch.from_numpy(c["tgt"]).to(dtype)
    w = torch.from_numpy(c["weights"]).to(dtype).reshape(-1, 1)
    cr.weighted_procrustes = watch_fit
    try:
        R, t, info = cr.GlobalRegistration(X, Y, weights=w, max_iter=P["max_iter"], max_break_count=P["max_break"], break_threshold_ratio=P["ratio"],
                                           loss_fn=Watch(loss_mod.HighDimSmoothL1Loss(w, P["quantization_size"])), quantization_size=P["quantization_size"])
    finally:
        cr.weighted_procrustes = orig
        torch.set_default_dtype(torch.float32)
    # losses[0] is loss_prev (the initial parameters, which iteration 0 evaluates again)
    return dict(R0=seen["R0"], t0=seen["t0"], losses=np.array(seen["losses"][1:], np.float64), iterations=int(info["iterations"]),
                break_count=int(info["break_count"]), loss=float(info["loss"]), R=R.double().numpy(), t=t.double().numpy().ravel())


def main():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(REF, "DGR"))
    import core.loss as loss_mod
    import core.registration as cr
    from tests import dgr_cases as cases
    assert len(cases.UNSTABLE) <= 1
    out = {}
    for name, *_ in cases.GOLDEN:
        c = cases.golden_case(name)
        r32 = run(torch, cr, loss_mod, c, cases.PARAMS, torch.float32)
        r64 = run(torch, cr, loss_mod, c, cases.PARAMS, torch.float64)
        assert np.array_equal(r32["R0"], r64["R0"]) and np.array_equal(r32["t0"], r64["t0"]), f"{name}: the two runs start apart"
        same = r32["iterations"] == r64["iterations"] and r32["break_count"] == r64["break_count"]
        print("" if same else f"{name}: the precisions stop apart\n", end="")
        out[name + "/sha256"] = np.array(cases.checksum(c))
        out[name + "/R0"], out[name + "/t0"] = r64["R0"], r64["t0"]
        for tag, r in (("f32", r32), ("f64", r64)):
            out[f"{name}/{tag}/losses"] = r["losses"]
            out[f"{name}/{tag}/iterations"], out[f"{name}/{tag}/break_count"] = np.int32(r["iterations"]), np.int32(r["break_count"])
            out[f"{name}/{tag}/loss"], out[f"{name}/{tag}/R"], out[f"{name}/{tag}/t"] = np.float64(r["loss"]), r["R"], r["t"]
        print(f"{name:9s} f32: it {r32['iterations']:4d} brk {r32['break_count']:3d}  f64: it {r64['iterations']:4d} brk {r64['break_count']:3d} loss {r64['loss']:.6f}  "
              f"fp32-vs-fp64: R {np.abs(r32['R'] - r64['R']).max():.2e} t {np.abs(r32['t'] - r64['t']).max():.2e} loss {abs(r32['loss'] - r64['loss']):.2e}")
    path = os.path.join(HERE, "g27_dgr.npz")
    np.savez_compressed(path, **out)
    print(len(cases.GOLDEN), "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
