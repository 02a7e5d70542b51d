"""What the reference's PointDSC encoder and classification head return on the golden cases of tests/pdsc_cases.py, recorded -- not
restated.

Runs only where the reference tree exists.  Experiments/models/PointDSC.py is imported as it is (plain torch, CPU); the model is built
with the case's num_layers and sigma_d, loaded with pdsc_cases.weights through load_state_dict (strict) and put in eval mode.  What is run
is the part the project builds, through the model's own modules: the compatibility matrix (the operations of :151-153), model.encoder
(:155) and model.classification (:171), on
corr_pos = [src, tgt] - its column mean (demo_registration.py:107-108).  Each case runs twice, in float64 and in float32.  Stored per
case in g24_pdsc.npz: the fp64 confidence of every row, the fp64 features of pdsc_cases.feature_rows(m), the reference's OWN
fp32-vs-fp64 max abs deviation of the features (over all rows) and of the confidence -- the yardstick of the device tests -- and a
checksum of the inputs and weights (the tests rebuild both from their seeds and compare it).

    python tests/golden/make_golden_pdsc.py
"""
import os
import sys

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run(model, torch, src, tgt, dtype):
    model = model.to(dtype)
    src_keypts, tgt_keypts = torch.from_numpy(src)[None].to(dtype), torch.from_numpy(tgt)[None].to(dtype)
    corr_pos = np.concatenate([src, tgt], axis=-1).astype(np.float64)
    corr_pos = torch.from_numpy(corr_pos - corr_pos.mean(0))[None].float().to(dtype)      # (the demo hands the model float32)
    pair_dist = lambda x: (x[:, :, None, :] - x[:, None, :, :]).norm(dim=-1)
    with torch.no_grad():
        d = pair_dist(src_keypts) - pair_dist(tgt_keypts)
        compat = (1.0 - d ** 2 / model.sigma_spat ** 2).clamp(min=0)          # the operations of PointDSC.py:151-153, in their order
        corr_features = model.encoder(corr_pos.permute(0, 2, 1), compat).permute(0, 2, 1)
        confidence = model.classification(corr_features.permute(0, 2, 1)).squeeze(1)
    return corr_features[0].double().numpy(), confidence[0].double().numpy()


def main():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    from models.PointDSC import PointDSC
    from tests import pdsc_cases
    torch.manual_seed(0)
    out = {}
    for m, num_layers in pdsc_cases.GOLDEN:
        c = pdsc_cases.golden_case(m, num_layers)
        model = PointDSC(in_dim=6, num_layers=num_layers, num_channels=128, sigma_d=pdsc_cases.SIGMA_D)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c["sd"].items()}, strict=True)
        model.eval()
        f32, c32 = run(model, torch, c["src"], c["tgt"], torch.float32)
        f64, c64 = run(model, torch, c["src"], c["tgt"], torch.float64)
        n = c["name"]
        out[n + "/conf"] = c64
        out[n + "/feat"] = f64[pdsc_cases.feature_rows(m)]
        out[n + "/dev_feat"] = np.float64(np.abs(f32 - f64).max())
        out[n + "/dev_conf"] = np.float64(np.abs(c32 - c64).max())
        out[n + "/sha256"] = np.array(pdsc_cases.checksum(c))
        print(f"{n:12s} max|feat| {np.abs(f64).max():8.3f}  fp32-vs-fp64: features {out[n + '/dev_feat']:.2e}, confidence {out[n + '/dev_conf']:.2e}")
    path = os.path.join(HERE, "g24_pdsc.npz")
    np.savez_compressed(path, **out)
    print(len(pdsc_cases.GOLDEN), "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
