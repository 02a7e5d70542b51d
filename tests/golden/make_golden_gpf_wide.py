"""G29: the reference's find_2nn / nn_to_mutual / calc_distance_ratio_in_feature_space / Grid_Prioritized_Filter on 33-wide descriptors
(runs only where the reference tree exists).

Nothing from the reference is copied: this script IMPORTS Experiments/algorithms/matching.py, calls it on a seeded synthetic pair
(tests/wide_cases.reg_pair: synth.make_pair's clouds, its descriptors taken to 33 numbers by a seeded Gaussian matrix) and stores the seed,
the shape and the reference's lists and scores.

    python tests/golden/make_golden_gpf_wide.py            # rewrites tests/golden/g29_gpf_wide.npz

The reference orders a cell's pairs with torch.argsort, which is unstable: a near-tie in the normalised ratio may be ordered either way.
The seed is the first one, counted up from SEED0, at which (checked here, on the CPU, before anything is written) no two pairs of the list
have the same normalised ratio in float32 (the only case in which an unstable sort is free to choose), none are closer than 1e-7 (about
two float32 steps at 1) in a float64 evaluation, and no ratio's float32 value differs from the float64 one by more than 1e-6.
"""
import os
import sys
import warnings

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

warnings.filterwarnings("ignore")

N, D, SEED0 = 1500, 33, 290
CONFIGS = [(0.5, 10), (2.0, 6)]          # (GPF_factor, GPF_grid_wid)
BB_CAPS = [200, 10 ** 9]                 # GPF_max_matches of the BB_first form (the second: returned before the grid filter)


class A:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    from algorithms import matching as M

    from tests import wide_cases

    for seed in range(SEED0, SEED0 + 50):
        p = wide_cases.reg_pair(N, D, seed)
        F0, F1 = np.array(p["feats0"]), np.array(p["feats1"])
        t0, t1, x0 = torch.from_numpy(F0), torch.from_numpy(F1), torch.from_numpy(np.array(p["xyz0"]))
        i0, i1, i2, _ = M.find_2nn(t0, t1)
        ratio = M.calc_distance_ratio_in_feature_space(t0, t1, i0, i1, i2).numpy()
        A64, B64 = F0.astype(np.float64), F1.astype(np.float64)
        r64 = np.sqrt(((A64 - B64[i1.numpy()]) ** 2).sum(1)) / (np.sqrt(((A64 - B64[i2.numpy()]) ** 2).sum(1)) + 1e-6)
        norm = (r64 - r64.min()) / (r64.max() - r64.min())
        gaps = np.diff(np.sort(norm))
        r32 = (ratio - ratio.min()) / (ratio.max() - ratio.min())
        if gaps.min() > 1e-7 and len(np.unique(r32)) == len(r32) and np.abs(ratio - r64).max() < 1e-6:
            break
    else:
        raise SystemExit(f"no seed in {SEED0}..{SEED0 + 49} without a near-tie in the ratio")
    out = dict(shape=np.array([N, D, seed]), idx1=i1.numpy().astype(np.int32), idx2=i2.numpy().astype(np.int32), ratio_nn=ratio.astype(np.float32))
    m0, m1, m2 = M.nn_to_mutual(t0, t1, i0, i1, i2)
    out.update(mnn_idx0=m0.numpy().astype(np.int32), mnn_idx1=m1.numpy().astype(np.int32), mnn_idx2=m2.numpy().astype(np.int32))
    out["ratio_mnn"] = M.calc_distance_ratio_in_feature_space(t0, t1, m0, m1, m2).numpy().astype(np.float32)
    for k, (factor, wid) in enumerate(CONFIGS):
        g = M.Grid_Prioritized_Filter(t0, t1, i0, i1, i2, x0, A(GPF_factor=factor, GPF_grid_wid=wid, GPF_max_matches=10 ** 9))
        out[f"gpf{k}_cfg"] = np.array([factor, wid], np.float64)
        for name, v in zip(("idx0", "idx1", "idx2"), g[:3]):
            out[f"gpf{k}_{name}"] = np.asarray(v).astype(np.int32)
        out[f"gpf{k}_score"] = np.asarray(g[6]).astype(np.float32)
        print("gpf", factor, wid, "kept", len(g[0]))
    for k, cap in enumerate(BB_CAPS):
        g = M.Grid_Prioritized_Filter(t0, t1, i0, i1, i2, x0, A(GPF_factor=2.0, GPF_grid_wid=10, GPF_max_matches=cap), BB_first=True)
        out[f"gpfbb{k}_cap"] = np.array(cap)
        out[f"gpfbb{k}_idx0"] = np.asarray(g[0]).astype(np.int32); out[f"gpfbb{k}_idx1"] = np.asarray(g[1]).astype(np.int32)
        out[f"gpfbb{k}_has_score"] = np.array(g[6] is not None)
        if g[6] is not None:
            out[f"gpfbb{k}_score"] = np.asarray(g[6]).astype(np.float32)
        print("gpf bb_first", cap, "kept", len(g[0]))
    print("seed", seed, "mutual", len(m0), "of", N)
    np.savez_compressed(os.path.join(HERE, "g29_gpf_wide.npz"), **out)


if __name__ == "__main__":
    main()
