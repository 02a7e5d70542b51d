"""G28: the reference's find_nn / find_2nn / nn_to_mutual on descriptors wider than 32 (runs only where the reference tree exists).

Nothing from the reference is copied: this script IMPORTS Experiments/algorithms/matching.py, calls it on seeded synthetic descriptors
(lidarregistration_amd.synth.make_features: unit rows, planted partners at noise 0.5, well separated from the random rest) and stores
the seeds, shapes and the reference's index lists.

    python tests/golden/make_golden_nn_wide.py            # rewrites tests/golden/g28_nn_wide.npz

For every width the seed is the first one, counted up from the width's start value, at which the reference agrees on every row with a
float64 numpy evaluation of the same distances (first and second neighbour): the fixture then holds no row whose answer depends on float32
rounding, and the test's tolerance rule (tests/test_nn_wide_cpu.py) is not needed on it.
"""
import os
import sys
import warnings

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

warnings.filterwarnings("ignore")

CASES = {"d33": (1500, 1300, 33, 2800), "d64": (1100, 1400, 64, 6400), "d128": (900, 1000, 128, 12800)}


def top2_f64(F0, F1):
    A, B = F0.astype(np.float64), F1.astype(np.float64)
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    order = np.argsort(d2, axis=1, kind="stable")
    return order[:, 0], order[:, 1]


def main():
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    from algorithms import matching as M

    from lidarregistration_amd import synth

    out = {}
    for tag, (n0, n1, d, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 50):
            F0, F1 = synth.make_features(n0, n1, d, 0.5, 0.5, seed)
            t0, t1 = torch.from_numpy(F0), torch.from_numpy(F1)
            i0, i1, i2, _ = M.find_2nn(t0, t1)
            j0, j1, none = M.find_nn(t0, t1, return_2nd=False)
            assert none is None and torch.equal(i1, j1) and torch.equal(i0, j0)
            e1, e2 = top2_f64(F0, F1)
            if np.array_equal(i1.numpy(), e1) and np.array_equal(i2.numpy(), e2):
                break
        else:
            raise SystemExit(f"{tag}: no seed in {seed0}..{seed0 + 49} at which the reference equals the float64 evaluation")
        m0, m1, m2 = M.nn_to_mutual(t0, t1, i0, i1, i2)
        b0, b1 = M.nn_to_mutual(t0, t1, i0, i1)
        assert torch.equal(m0, b0) and torch.equal(m1, b1)
        out[f"{tag}_shape"] = np.array([n0, n1, d, seed])
        out[f"{tag}_idx1"] = i1.numpy().astype(np.int32)
        out[f"{tag}_idx2"] = i2.numpy().astype(np.int32)
        out[f"{tag}_m0"] = m0.numpy().astype(np.int32)
        out[f"{tag}_m1"] = m1.numpy().astype(np.int32)
        out[f"{tag}_m2"] = m2.numpy().astype(np.int32)
        print(tag, "seed", seed, "mutual", len(m0), "of", n0)
    np.savez_compressed(os.path.join(HERE, "g28_nn_wide.npz"), **out)


if __name__ == "__main__":
    main()
