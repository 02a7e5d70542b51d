"""What the reference's Z-only refinement returns on the pairs of tests/refine_z_cases.py::golden_cases, recorded -- not restated.

Runs only where the reference tree exists.  BalancedDatasetGenerator/GenerateBalancedSet.py is imported as it is, with the stand-in modules
of make_golden_overlap.py for what this machine lacks; its own refine_motion_Z_only (:257-291) is called unbound on a namespace object,
with its own NN (scipy's cKDTree, :149-153) and apply_transformation (utils/tools_3d.py).  The loop's locals are read without touching its
text: NN is wrapped (the first repeat's `ind`), and the module's `np` is a pass-through that notes the size of what np.median is given
(the valid count) and the scalar np.abs is given (mean_z_dist) in every repeat.

Only outputs are stored, in g18_refine_z.npz, per case: dz, the per-repeat mean_z_dist and valid count, the first repeat's ind, the
largest valid |z_dist| of the first repeat (the tolerance's scale) and a checksum of the inputs.  The inputs must keep every decision
1e-8 away from its threshold (check_conditions, asserted here and in tests/test_refine_z_cpu.py), so that the last-bit differences
between the reference's matrix product and the contract's transform cannot flip one.

tests/golden/g20_refine_z_large.npz holds the same for the 120 000-raw-point scan pair (tests/large_cases.py::golden_case, 75 199 x 74 958
centroids; seed 51, the generator's default, met every margin: no other seed was tried), with a SHA-256 of the first repeat's ind in place
of the array.  Its conditions are checked on the restatement over nn_tree (tests/refine_z_cpu.py), which the brute-force search cannot
serve at this size.  It is written by a call of its own, so that g18_refine_z.npz keeps its bytes:

    python tests/golden/make_golden_refine_z.py
    python tests/golden/make_golden_refine_z.py large
"""
import functools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LOG = dict(ind=[], nvalid=[], means=[], zmax=[])


class NumpyTap:
    """numpy, except that median and abs note what the refinement loop hands them."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def median(w):
        LOG["nvalid"].append(len(w))
        return np.median(w)

    @staticmethod
    def abs(x):
        if np.ndim(x) == 0:
            LOG["means"].append(float(x))
        elif not LOG["zmax"]:
            LOG["zmax"].append(float(np.max(np.abs(x))))
        return np.abs(x)


def reference_generator():
    sys.path.insert(0, HERE)
    import make_golden_overlap
    make_golden_overlap.reference_generator()                # the stand-in modules and the import path
    import GenerateBalancedSet
    GenerateBalancedSet.np = NumpyTap()
    cls = GenerateBalancedSet.BalancedSetGenerator
    ns = types.SimpleNamespace()

    def NN(A, B):
        d, ind = cls.NN(ns, A, B)
        LOG["ind"].append(np.array(ind))
        return d, ind
    ns.NN = NN
    ns.refine_motion_Z_only = functools.partial(cls.refine_motion_Z_only, ns)
    return ns


def record(gen, p):
    """The reference's refinement on one pair: (dz, per-repeat means)."""
    for v in LOG.values():
        del v[:]
    raw = np.array(p["T"], np.float64)
    res = gen.refine_motion_Z_only(raw.copy(), p["A"].copy(), p["B"].copy(), p["gate"])
    means = np.array(LOG["means"])
    dz = 0
    for m in means:
        dz -= m                                              # (:284, the same subtractions)
    assert len(means) == len(LOG["nvalid"]) == len(LOG["ind"]) and res[2, 3] == raw[2, 3] + dz
    return dz, means


def main_large():
    sys.path.insert(0, ROOT)
    from tests import large_cases, refine_z_cases
    gen = reference_generator()
    name, p = large_cases.GOLDEN_NAME, large_cases.golden_case()
    dz, means = record(gen, p)
    mine, trace = large_cases.golden_trace()
    margins = refine_z_cases.check_conditions(p, name, trace=trace)
    out = {name + "/dz": np.float64(dz), name + "/means": means, name + "/nvalid": np.array(LOG["nvalid"], np.int32),
           name + "/zmax": np.float64(LOG["zmax"][0]), name + "/sha256": np.array(refine_z_cases.checksum(p["A"], p["B"], p["T"])),
           name + "/ind0_sha256": np.array(large_cases.index_hash(LOG["ind"][0]))}
    print(f"{name:18s} n0={len(p['A']):6d} n1={len(p['B']):6d} repeats={len(means):2d} valid={LOG['nvalid'][0]:6d} dz={dz:+.9f} "
          f"restated {mine['dz']:+.9f} (diff {mine['dz'] - dz:+.2e}) margins nn {margins[0]:.1e} gate {margins[1]:.1e} stop {margins[2]:.1e}")
    path = os.path.join(HERE, "g20_refine_z_large.npz")
    np.savez_compressed(path, **out)
    print("1 case ->", path, os.path.getsize(path), "bytes")


def main():
    sys.path.insert(0, ROOT)
    from tests import refine_z_cases, refine_z_cpu
    gen = reference_generator()
    out = {}
    for name, p in refine_z_cases.golden_cases().items():
        dz, means = record(gen, p)
        margins = refine_z_cases.check_conditions(p, name)
        mine = refine_z_cpu.refine_z(p["A"], p["B"], p["T"], p["gate"])
        out[name + "/dz"] = np.float64(dz)
        out[name + "/means"] = means
        out[name + "/nvalid"] = np.array(LOG["nvalid"], np.int32)
        out[name + "/ind0"] = LOG["ind"][0].astype(np.int32)
        out[name + "/zmax"] = np.float64(LOG["zmax"][0])
        out[name + "/sha256"] = np.array(refine_z_cases.checksum(p["A"], p["B"], p["T"]))
        print(f"{name:18s} n0={len(p['A']):6d} n1={len(p['B']):6d} repeats={len(means):2d} valid={LOG['nvalid'][0]:6d} dz={dz:+.9f} "
              f"restated {mine['dz']:+.9f} (diff {mine['dz'] - dz:+.2e}) margins nn {margins[0]:.1e} gate {margins[1]:.1e} stop {margins[2]:.1e}")
    path = os.path.join(HERE, "g18_refine_z.npz")
    np.savez_compressed(path, **out)
    print(len(out) // 6, "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main_large() if sys.argv[1:] == ["large"] else main()
