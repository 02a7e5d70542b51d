"""Generate tests/golden/g15_filter_edges.npz by IMPORTING the reference (runs only where the reference tree exists).

Nothing from the reference is copied: this script calls its ``Grid_Prioritized_Filter``
(Experiments/algorithms/matching.py:100-205) on every cloud of ``tests/filter_edges.py`` -- the cell-edge clouds, the wide clouds,
the water-filling cases -- once with ``BB_first=False`` at the cloud's factor and once with ``BB_first=True`` at its cap, and stores
the OUTPUTS only: the kept idx0 / idx1 / idx2 and the bits of the returned scores.  The inputs are rebuilt from seeds by the tests;
a checksum of them is stored so that a drifting builder is noticed.

    python tests/golden/make_golden_filter_edges.py
"""
import os
import sys
import warnings

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

warnings.filterwarnings("ignore")


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(4)
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    from algorithms import matching as M

    from tests import filter_edges as fe

    out = {}
    t = torch.from_numpy
    for name, build in fe.all_clouds().items():
        c = build()
        G = c["G"]
        out[f"{name}_sha"] = np.frombuffer(bytes.fromhex(fe.checksum(c)), np.uint8)
        out[f"{name}_cfg"] = np.array([G, c["factor"], c["cap"]], np.float64)
        for tag, kw, bb_first in (("gpf", dict(GPF_factor=c["factor"]), False), ("bbf", dict(GPF_max_matches=c["cap"]), True)):
            a = Args(GPF_grid_wid=G, **kw)
            r = M.Grid_Prioritized_Filter(t(c["F0"]), t(c["F1"]), t(c["i0"]), t(c["i1"]), t(c["i2"]), t(c["xyz0"]), a, BB_first=bb_first)
            for k in range(3):
                out[f"{name}_{tag}_idx{k}"] = r[k].numpy().astype(np.int32)
            assert r[6] is not None
            out[f"{name}_{tag}_score"] = r[6].numpy().astype(np.float32).view(np.uint32)
        print(name, G, len(c["i1"]), len(out[f"{name}_gpf_idx0"]), len(out[f"{name}_bbf_idx0"]))
    np.savez_compressed(os.path.join(HERE, "g15_filter_edges.npz"), **out)


if __name__ == "__main__":
    main()
