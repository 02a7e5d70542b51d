"""BASELINE config #1: one synthetic 5k-point pair through the whole path (plumbing demo).

    python demo_registration.py --algo RANSAC --mode MMN --iters 1000
    python demo_registration.py --descriptor fpfh --mode GPF --n 120000 --iters 50000

The reference's demo_registration.py is a PointDSC viewer without RANSAC flags (Experiments/demo_registration.py:61-67);
this one exercises FR() with the reference's flag names and prints the recovered motion next to the ground truth.
--descriptor fpfh (the reference's --descriptor fpfh, :37-44,93-95) needs no descriptors and no weights: it registers two raw synthetic
scan frames of --n points from the points alone -- fpfh.Extractor on both (voxel --voxel_size), then FR() on the 33-wide rows with
--mode / --codebase as given (a wide workspace behind it).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--algo", default="RANSAC", choices=["RANSAC"])
    p.add_argument("--codebase", default="GC", choices=["open3D", "GC"])
    p.add_argument("--mode", default="MMN", choices=["MMN", "MNN", "GPF", "no_filter"])
    p.add_argument("--iters", type=int, default=1000)
    p.add_argument("--n", type=int, default=5000)
    p.add_argument("--seed", type=int, default=51)
    p.add_argument("--fast_rejection", default="ELC")
    p.add_argument("--GPF_factor", type=float, default=2.0)
    p.add_argument("--GPF_grid_wid", type=int, default=10)
    p.add_argument("--descriptor", default="synthetic", choices=["synthetic", "fpfh"])
    p.add_argument("--voxel_size", type=float, default=0.3)
    args = p.parse_args(argv)
    import torch
    from lidarregistration_amd import metrics, synth
    np.set_printoptions(precision=4, suppress=True)
    if args.descriptor == "fpfh":
        return fpfh_demo(args, metrics, synth)
    from algorithms.FR import FR
    pr = synth.make_pair(N=args.n, rho=0.5, s=0.9, seed=args.seed)
    t = torch.from_numpy
    T, elapsed, _, _, n_init, ir_init, n_filt, ir_filt = FR(t(pr["xyz0"]), t(pr["xyz1"]), t(pr["feats0"]), t(pr["feats1"]), args, pr["T_gt"])
    print(f"{n_init} nn pairs ({ir_init:.3f} inliers), {n_filt} filtered pairs ({ir_filt:.3f} inliers), {elapsed*1e3:.2f} ms")
    print("estimated motion:\n", T, "\nground truth:\n", pr["T_gt"])
    print(f"RE = {metrics.rotation_error_deg(T, pr['T_gt']):.4f} deg, TE = {metrics.translation_error_cm(T, pr['T_gt']):.3f} cm")
    return T


def fpfh_demo(args, metrics, synth):
    from time import time
    from algorithms.FR import FR
    from lidarregistration_amd import fpfh
    A, B, T_gt = synth.make_scan_pair(args.n, seed=args.seed)
    t0 = time()
    ex = fpfh.Extractor(args.voxel_size)
    p0, F0, _ = ex.extract(A)
    p1, F1, _ = ex.extract(B)
    extract_s = time() - t0
    T, elapsed, _, _, n_init, ir_init, n_filt, ir_filt = FR(p0, p1, F0, F1, args, T_gt)
    print(f"{p0.shape[0]} x {p1.shape[0]} points after down-sampling (FPFH in {extract_s*1e3:.2f} ms), {n_init} nn pairs ({ir_init:.3f} inliers), "
          f"{n_filt} filtered pairs ({ir_filt:.3f} inliers), {elapsed*1e3:.2f} ms")
    print("estimated motion:\n", T, "\nground truth:\n", T_gt)
    print(f"RE = {metrics.rotation_error_deg(T, T_gt):.4f} deg, TE = {metrics.translation_error_cm(T, T_gt):.3f} cm")
    return T


if __name__ == "__main__":
    main()
