"""What the reference's BBR-F loop computes on the pairs of tests/bbrf_cases.py::golden_cases, recorded -- not restated.

Runs only where the reference tree exists.  FCGF_FAST/net/BBR_F.py is imported as it is, with a stand-in `open3d` module (only
calc_normals, which is not called here, touches it), and its own BBR_F_step is driven 100 times with its own parameters (float32) and
torch's Adam, as BBR_F (:289-309) does; the normals are given.  record_in_logs (:243-259) compares an array with [] and raises under
the installed numpy: it is replaced, as a module attribute, by a stand-in that appends -- bookkeeping, no arithmetic.  prerun_gpu is
tapped for the pair lists, and the parameters' .grad is read after the first backward through a wrapped optimizer step.

Only outputs are stored, in g19_bbrf.npz, per case: the 100 x 6 parameter log, the losses, the pair counts, iteration 0's pair list and
six gradients, the argmin, the final 4x4 (:312-319) and a checksum of the inputs.

    python tests/golden/make_golden_bbrf.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_ITER = 100


def reference_module():
    sys.path.insert(0, HERE)
    from make_golden_overlap import REF
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    sys.path.insert(0, os.path.join(REF, "FCGF_FAST", "net"))
    import BBR_F

    def record_in_logs(angles_np, trans_np, theta, phi, psi, trans_x, trans_y, trans_z):
        angles_np.append([theta.item(), phi.item(), psi.item()]); trans_np.append([trans_x.item(), trans_y.item(), trans_z.item()])
        return angles_np, trans_np
    BBR_F.record_in_logs = record_in_logs
    return BBR_F


def run(ref, p):
    import torch
    pairs, grads = [], []
    prerun = ref.prerun_gpu

    def tap(*a):
        inds = prerun(*a)
        pairs.append((inds["HARD_BEST_BUDDY_PAIRS"]["A"].numpy().copy(), inds["HARD_BEST_BUDDY_PAIRS"]["B"].numpy().copy()))
        return inds
    ref.prerun_gpu = tap
    try:
        t = lambda X: torch.tensor(X, requires_grad=False)
        A, nA, B, nB = t(p["A"]), t(p["nA"]), t(p["B"]), t(p["nB"])
        prm = [torch.tensor([0.0], requires_grad=True) for _ in range(6)]
        opt = torch.optim.Adam([{"params": prm[:3], "lr": 2e-4}, {"params": prm[3:], "lr": 2e-4}])
        step = opt.step

        def wrapped(*a, **k):
            if not grads:
                grads.append([float(q.grad.item()) for q in prm])
            return step(*a, **k)
        opt.step = wrapped
        loss_np, angles_np, trans_np = [], [], []
        for _ in range(N_ITER):
            opt, loss_np, angles_np, trans_np = ref.BBR_F_step(A, B, nA, nB, *prm, opt, angles_np, trans_np, loss_np)
    finally:
        ref.prerun_gpu = prerun
    ind = int(np.argmin(loss_np))
    B_to_A = np.eye(4)
    B_to_A[:3, :3] = ref.euler_angles_to_rotation_matrix(np.array(angles_np[ind]), deg_or_rad="rad")
    B_to_A[:3, 3] = trans_np[ind]
    order = np.argsort(pairs[0][0], kind="stable")
    return dict(params=np.concatenate([np.array(angles_np), np.array(trans_np)], axis=1), loss=np.array(loss_np),
                npairs=np.array([len(a) for a, _ in pairs], np.int32), pairs0=np.stack([pairs[0][0][order], pairs[0][1][order]], axis=1).astype(np.int32),
                grad0=np.array(grads[0]), argmin=np.int32(ind), T=np.linalg.inv(B_to_A))


def main():
    sys.path.insert(0, ROOT)
    from tests import bbrf_cases
    ref = reference_module()
    out = {}
    for name, p in bbrf_cases.golden_cases().items():
        gap = bbrf_cases.check_conditions(p)
        g = run(ref, p)
        mine, log, trace = bbrf_cases.golden_run(name)
        for k, v in g.items():
            out[f"{name}/{k}"] = v
        out[name + "/sha256"] = np.array(bbrf_cases.checksum(p["A"], p["nA"], p["B"], p["nB"]))
        two = np.sort(g["loss"])[:2]
        print(f"{name:16s} n0={len(p['A'])} n1={len(p['B'])} nn gap {gap:.1e} argmin {int(g['argmin'])} (restated {mine['best_iter']}) "
              f"two lowest losses {two[1] - two[0]:.1e} apart; max |param diff| {np.abs(log[:, :6] - g['params']).max():.2e} "
              f"max |loss diff| {np.abs(log[:, 6] - g['loss']).max():.2e} pair counts differ in {(log[:, 7] != g['npairs']).sum()} iterations")
    path = os.path.join(HERE, "g19_bbrf.npz")
    np.savez_compressed(path, **out)
    print(len(bbrf_cases.golden_cases()), "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
