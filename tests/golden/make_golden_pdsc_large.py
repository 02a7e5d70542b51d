"""The fp64 outputs of the PointDSC encoder on the large cases of tests/pdsc_cases.LARGE, recorded -- a test cannot restate them: the
numpy restatement takes 12 s in fp64 at m = 8 193 with one layer and grows as m^2 x layers.

The cases are the attention plans above m = 8 192 (pd_make_plan of csrc/lr_pdsc.hip): the full 512-block grid, the first m of every
smaller chunk count and the contract's largest m at one layer, the 5-chunk plan at 12 layers.  Inputs and weights are rebuilt from their
seeds (pdsc_cases.large_case).  Per case g25_pdsc_large.npz holds: the checksum of inputs and weights (the tests rebuild both and
compare), the fp64 features of pdsc_cases.feature_rows(m), the fp64 confidence of pdsc_cases.conf_rows(m) (four rows of every query
block, one per wave, and the last row), and two yardsticks, each a max abs distance over ALL rows between an fp32 evaluation of the
reference's formula and the fp64 one (pdsc_cpu.encode_slabbed, float64):
    d32_feat,  d32_conf     pdsc_cpu.encode_slabbed in float32: numpy's blocked sums
    d32t_feat, d32t_conf    pdsc_cpu.encode_tiled32: the softmax in the contract's order (E6) -- key tiles of 32 in sequence behind one
                            running maximum inside each chunk of the plan, 512 tiles at m = 32 768
None of these comes from the device.

The cases run in separate processes (--jobs, default 4, two BLAS threads each).  Run time 6 min 36 s on 8 cores with --jobs 4 (per
case, each in its own process: 19 - 25 s up to m = 9 345, 51 s / 79 s / 147 s at 13 057 / 16 385 / 21 761, 329 s at 32 768, 393 s
for m = 10 881 at 12 layers), peak memory 2.4 GB in the largest process (m = 32 768: the fp64 slabs of 512 x 32 768 differences),
1.3 - 1.8 GB in the others.

    python tests/golden/make_golden_pdsc_large.py [--jobs N]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def record(case):
    """One case in a process of its own: the entries of the .npz and the line to print."""
    import resource

    import numpy as np
    sys.path.insert(0, ROOT)
    from tests import pdsc_cases, pdsc_cpu
    m, num_layers = case
    c = pdsc_cases.large_case(m, num_layers)
    n, t0 = c["name"], time.time()
    run = lambda fn, **kw: fn(c["src"], c["tgt"], c["sd"], num_layers, pdsc_cases.SIGMA_D, **kw)
    f64, c64 = run(pdsc_cpu.encode_slabbed, dtype=np.float64)
    f32, c32 = run(pdsc_cpu.encode_slabbed, dtype=np.float32)
    ft, ct = run(pdsc_cpu.encode_tiled32)
    dist = lambda a, b: np.float64(np.abs(a.astype(np.float64) - b).max())
    out = {n + "/sha256": np.array(pdsc_cases.checksum(c)),
           n + "/feat": f64[pdsc_cases.feature_rows(m)], n + "/conf": c64[pdsc_cases.conf_rows(m)],
           n + "/d32_feat": dist(f32, f64), n + "/d32_conf": dist(c32, c64), n + "/d32t_feat": dist(ft, f64), n + "/d32t_conf": dist(ct, c64)}
    assert np.isfinite(f64).all() and np.isfinite(c64).all()
    line = (f"{n:12s} plan {pdsc_cpu.plan(m)}: max|feat| {np.abs(f64).max():7.3f}, max|conf| {np.abs(c64).max():7.3f}; fp32 blocked: features "
            f"{out[n + '/d32_feat']:.2e}, confidence {out[n + '/d32_conf']:.2e}; fp32 tiled: {out[n + '/d32t_feat']:.2e}, {out[n + '/d32t_conf']:.2e}; "
            f"{time.time() - t0:.0f} s, peak {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GB")
    return out, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "2" if a.jobs > 1 else str(os.cpu_count()))
    os.environ.setdefault("OPENBLAS_NUM_THREADS", os.environ["OMP_NUM_THREADS"])
    os.environ.setdefault("MKL_NUM_THREADS", os.environ["OMP_NUM_THREADS"])
    import multiprocessing

    import numpy as np
    sys.path.insert(0, ROOT)
    from tests import pdsc_cases
    t0 = time.time()
    todo = sorted(pdsc_cases.LARGE, key=lambda c: -c[0] * c[0] * c[1])          # the longest first
    out = {}
    with multiprocessing.get_context("spawn").Pool(a.jobs) as pool:
        for entries, line in pool.imap_unordered(record, todo):
            out.update(entries)
            print(line, flush=True)
    path = os.path.join(HERE, "g25_pdsc_large.npz")
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(len(todo), "cases ->", path, os.path.getsize(path), "bytes;", f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
