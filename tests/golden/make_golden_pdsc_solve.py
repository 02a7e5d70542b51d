"""What the reference's PointDSC tail returns on the golden cases of tests/pdsc_solve_cases.py, recorded -- not restated.

Runs only where the reference tree exists.  Experiments/models/PointDSC.py is imported as it is (plain torch, CPU).  What is run is the
model's own pick_seeds (:199-217), cal_seed_trans (:234-336, with knn and rigid_transform_3d of models/common.py and
cal_leading_eigenvector :338-358) and post_refinement (:403-438), in the order of forward (:156-186), on the case's features and
confidence.  The neighbour lists and the weights are what cal_seed_trans hands to rigid_transform_3d (the call is observed, not
changed).  Each case runs in float32 and in float64 (torch.set_default_dtype(float64): rigid_transform_3d builds torch.eye in the
default type).  Stored per case in g26_pdsc_solve.npz, from the fp64 run: seeds, neighbour lists, weights, seed transforms, counts, the
best seed, labels, the unrefined and the refined transform, whether the power loop left early; the reference's OWN fp32-vs-fp64 max abs
deviation per quantity -- the yardstick of the device tests -- and a checksum of the inputs.

The generator asserts, for every case it stores: the two precisions pick the same seeds, count the same inliers for every seed and choose
the same best seed, and at least 95 % of the seeds have the same neighbour set.

    python tests/golden/make_golden_pdsc_solve.py
"""
import os
import sys

import numpy as np

REF = os.environ.get("LIDARREG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run(torch, F, mod, model, c, dtype):
    torch.set_default_dtype(dtype)
    model = model.to(dtype)
    src, tgt = torch.from_numpy(c["src"])[None].to(dtype), torch.from_numpy(c["tgt"])[None].to(dtype)
    feat, conf = torch.from_numpy(c["feat"])[None].to(dtype), torch.from_numpy(c["conf"])[None].to(dtype)
    seen = {"close": []}
    fit, close = mod.rigid_transform_3d, torch.allclose

    def watch_fit(A, B, weights=None, weight_threshold=0):
        seen.setdefault("weights", weights.detach().clone())
        return fit(A, B, weights, weight_threshold)

    def watch_knn(x, k, ignore_self=False, normalized=True):
        seen["knn_all"] = knn(x, k, ignore_self, normalized)
        return seen["knn_all"]

    def watch_close(*a, **kw):
        seen["close"].append(bool(close(*a, **kw)))
        return seen["close"][-1]

    knn = mod.knn
    mod.rigid_transform_3d, mod.knn, torch.allclose = watch_fit, watch_knn, watch_close
    try:
        with torch.no_grad():
            normed = F.normalize(feat, p=2, dim=-1)
            src_dist = torch.norm(src[:, :, None, :] - src[:, None, :, :], dim=-1)
            seeds = model.pick_seeds(src_dist, conf, R=model.nms_radius, max_num=int(conf.shape[1] * model.ratio))
            seed_trans, fitness, final_trans, final_labels = model.cal_seed_trans(seeds, normed, src, tgt)
            early = any(seen["close"])
            refined = model.post_refinement(final_trans, src, tgt)
    finally:
        mod.rigid_transform_3d, mod.knn, torch.allclose = fit, knn, close
        torch.set_default_dtype(torch.float32)
    m = conf.shape[1]
    s = seeds[0].numpy().astype(np.int64)
    return dict(seeds=s, knn=seen["knn_all"][0].numpy()[s], weights=seen["weights"].double().numpy(), seed_T=seed_trans[0].double().numpy(),
                counts=np.rint(fitness[0].double().numpy() * m).astype(np.int64), best=int(fitness[0].argmax()),
                labels=final_labels[0].numpy().astype(np.uint8), T_best=final_trans[0].double().numpy(), T=refined[0].double().numpy(), early=early)


def main():
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(REF, "Experiments"))
    import models.PointDSC as mod
    from tests import pdsc_solve_cases as cases
    torch.manual_seed(0)
    P = cases.PARAMS
    out = {}
    for name, m, _, _ in cases.GOLDEN:
        c = cases.golden_case(name)
        model = mod.PointDSC(in_dim=6, num_layers=1, num_channels=128, num_iterations=P["num_iterations"], ratio=P["ratio"],
                             inlier_threshold=P["inlier_threshold"], sigma_d=P["sigma_d"], k=P["k"], nms_radius=P["nms_radius"])
        model.eval()
        r32 = run(torch, F, mod, model, c, torch.float32)
        r64 = run(torch, F, mod, model, c, torch.float64)
        assert np.array_equal(r32["seeds"], r64["seeds"]), f"{name}: the precisions pick different seeds"
        assert np.array_equal(r32["counts"], r64["counts"]) and r32["best"] == r64["best"], f"{name}: the precisions count differently"
        same_set = np.array([set(a) == set(b) for a, b in zip(r32["knn"], r64["knn"])])
        same_order = np.array([np.array_equal(a, b) for a, b in zip(r32["knn"], r64["knn"])])
        assert same_set.mean() >= 0.95, f"{name}: only {same_set.mean():.3f} of the seeds have equal neighbour sets"
        # weights compared neighbour by neighbour (the order of near-equal similarities may differ between the precisions)
        w32 = np.stack([w[np.argsort(i)] for w, i in zip(r32["weights"], r32["knn"])])
        w64 = np.stack([w[np.argsort(i)] for w, i in zip(r64["weights"], r64["knn"])])
        dev = lambda a, b: np.float64(np.abs(a - b).max()) if a.size else np.float64(0)
        out[name + "/seeds"] = r64["seeds"].astype(np.int32)
        out[name + "/knn"] = r64["knn"].astype(np.int16)
        out[name + "/weights"] = r64["weights"]
        out[name + "/seed_T"] = r64["seed_T"]
        out[name + "/counts"] = r64["counts"].astype(np.int32)
        out[name + "/best"] = np.int32(r64["best"])
        out[name + "/labels"] = np.packbits(r64["labels"])
        out[name + "/T_best"], out[name + "/T"] = r64["T_best"], r64["T"]
        out[name + "/early"] = np.bool_(r64["early"])
        out[name + "/same_set"], out[name + "/same_order"] = np.float64(same_set.mean()), np.float64(same_order.mean())
        out[name + "/dev_weights"] = dev(w32[same_set], w64[same_set])
        out[name + "/dev_seed_T"] = dev(r32["seed_T"][same_set], r64["seed_T"][same_set])
        out[name + "/dev_T_best"], out[name + "/dev_T"] = dev(r32["T_best"], r64["T_best"]), dev(r32["T"], r64["T"])
        out[name + "/sha256"] = np.array(cases.checksum(c))
        top = int((r64["counts"] == r64["counts"].max()).sum())
        print(f"{name:8s} seeds {len(r64['seeds']):4d} best {r64['best']:4d} count {r64['counts'].max():4d} ({top} seeds at the top) early {r64['early']!s:5s} "
              f"sets {same_set.mean():.3f} order {same_order.mean():.3f}  fp32-vs-fp64: weights {out[name + '/dev_weights']:.2e} seed T "
              f"{out[name + '/dev_seed_T']:.2e} T_best {out[name + '/dev_T_best']:.2e} T {out[name + '/dev_T']:.2e}")
    path = os.path.join(HERE, "g26_pdsc_solve.npz")
    np.savez_compressed(path, **out)
    print(len(cases.GOLDEN), "cases ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
