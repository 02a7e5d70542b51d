"""What the reference's overlap measure returns on the pairs of tests/overlap_cases.py::golden_cases, recorded -- not restated.

Runs only where the reference tree exists.  BalancedDatasetGenerator/GenerateBalancedSet.py is imported as it is, with stand-in modules for
what this machine lacks (open3d, matplotlib, easydict, datasets.*); its own overlap_fraction (:155-179) and calc_GT_overlap (:186-205) are
called unbound on a namespace object, with its own apply_transformation (utils/tools_3d.py), NN (scipy's cKDTree) and downsample.

What the fixture pins: the reference's transform, its scipy search, its threshold np.sqrt(2) * voxel_size with the strict `<`, both
fractions and the numerator they share.  What it does NOT pin: the down-sampling -- Open3D is not available, so the stand-in for
o3d.geometry.PointCloud.voxel_down_sample is the restatement tests/overlap_cpu.py::voxel_mean (the recalled part of the contract).

Only outputs are stored, in g17_overlap.npz: the two fractions, |A_|, |B_| and a checksum of the inputs (the tests rebuild the inputs
from their seeds and compare it).

    python tests/golden/make_golden_overlap.py
"""
import functools
import os
import sys
import types

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SIZES = []


def reference_generator():
    from tests import overlap_cpu

    class PointCloud:
        points = None

        @staticmethod
        def voxel_down_sample(x, voxel_size):
            out = PointCloud()
            out.points = overlap_cpu.voxel_mean(np.asarray(x.points), voxel_size)["cent"]
            SIZES.append(len(out.points))
            return out

    for name in ("open3d", "matplotlib", "matplotlib.pyplot", "easydict", "datasets", "datasets.KITTI", "datasets.ApolloSouthbay",
                 "datasets.NuScenes", "datasets.LyftLEVEL5"):
        sys.modules[name] = types.ModuleType(name)
    o3d = sys.modules["open3d"]
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda x: np.asarray(x))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["easydict"].EasyDict = lambda d: types.SimpleNamespace(**d)
    sys.modules["datasets"].__path__ = []
    sys.path.insert(0, os.path.join(REF, "BalancedDatasetGenerator"))
    import GenerateBalancedSet
    cls = GenerateBalancedSet.BalancedSetGenerator
    ns = types.SimpleNamespace(config=types.SimpleNamespace(overlap_measure="symmetric"))
    for f in ("downsample", "NN", "make_open3d_point_cloud", "overlap_fraction", "calc_GT_overlap"):
        setattr(ns, f, functools.partial(getattr(cls, f), ns))
    return ns


def main():
    sys.path.insert(0, ROOT)
    from tests import overlap_cases
    gen = reference_generator()
    out = {}
    for name, p in overlap_cases.golden_cases().items():
        del SIZES[:]
        if p["T"] is None:
            frac, sym = gen.overlap_fraction(p["A"], p["B"])
        else:
            frac, sym = gen.calc_GT_overlap(p["A"], p["B"], p["T"], return_both=True)
        out[name + "/frac"] = np.float64(frac)
        out[name + "/frac_sym"] = np.float64(sym)
        out[name + "/n0_ds"] = np.int32(SIZES[0])
        out[name + "/n1_ds"] = np.int32(SIZES[1])
        out[name + "/sha256"] = np.array(overlap_cases.checksum(p["A"], p["B"], p["T"]))
        print(f"{name:18s} |A_|={SIZES[0]:6d} |B_|={SIZES[1]:6d} frac={frac:.6f} sym={sym:.6f}")
    path = os.path.join(HERE, "g17_overlap.npz")
    np.savez_compressed(path, **out)
    print(len(out) // 5, "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
