"""What the reference's spectral matching returns on the cases of tests/sm_cases.py, recorded -- not restated.

Runs only where the reference tree exists.  Experiments/baseline_scripts/baseline_3DMatch.py is imported as it is, with empty stand-in
modules for what its other functions need and this machine lacks (open3d, config, datasets.ThreeDMatch, datasets.dataloader); SM() itself
(:19-53) and rigid_transform_3d (models/common.py:7-45) are plain torch and run on the CPU.  Every case marked `golden` is run at the
settings of baseline_KITTI.py:51-52 (inlier_threshold 0.6) with the case's top_ratio.  Only outputs are stored, in g16_sm.npz: the
labels bit-packed, the 4x4 as float32, K, and a checksum of the inputs (the tests rebuild the inputs from their seeds and compare it).

    python tests/golden/make_golden_sm.py
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def reference_sm():
    for name in ("open3d", "config", "datasets", "datasets.ThreeDMatch", "datasets.dataloader"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["config"].str2bool = lambda v: str(v).lower() in ("true", "1")
    sys.modules["datasets.ThreeDMatch"].ThreeDMatchTest = None
    sys.modules["datasets.dataloader"].get_dataloader = None
    sys.modules["datasets"].__path__ = []
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    sys.path.insert(0, os.path.join(REF, "Experiments", "baseline_scripts"))
    import baseline_3DMatch
    return baseline_3DMatch.SM


def main():
    import torch
    sys.path.insert(0, ROOT)
    from tests import sm_cases
    SM = reference_sm()
    out = {}
    for c in sm_cases.cases():
        if not c["golden"]:
            continue
        a, b = torch.from_numpy(c["a"])[None], torch.from_numpy(c["b"])[None]
        corr = torch.cat([a[0], b[0]], dim=-1)[:, None, :]        # [M,1,6]: SM() subtracts its own transpose (3DMatch.py:20)
        args = types.SimpleNamespace(inlier_threshold=c["thr"])
        with torch.no_grad():
            T, labels = SM(corr, a, b, args, top_ratio=c["ratio"])
        labels = labels[0].numpy() > 0.5
        n = c["name"]
        out[n + "/labels"] = np.packbits(labels)
        out[n + "/T"] = T[0].numpy().astype(np.float32)
        out[n + "/K"] = np.int32(labels.sum())
        out[n + "/sha256"] = np.array(sm_cases.checksum(c))
        print(f"{n:28s} M={len(c['a']):5d} K={int(labels.sum()):4d}")
    path = os.path.join(HERE, "g16_sm.npz")
    np.savez_compressed(path, **out)
    print(len(out) // 4, "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
