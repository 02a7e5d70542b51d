"""One call of every entry point of liblidarreg.so that launches kernels, at dim 32 and dim 3, and every branch of the RANSAC and NN launch plans: the
workload behind profiles/host_context_trace.txt, profiles/prims_trace.txt, profiles/ransac_split_trace.txt, profiles/nn_split_trace.txt and profiles/corrset_shared_trace.txt.  Run it under `rocprofv3 --kernel-trace -- python tools/entry_point_trace.py`, once per library
(LIDARREG_LIB names an alternate build), and compare the two kernel traces with tools/trace_compare.py."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lidarregistration_amd import FR, _ext, dgr, matching, overlap, pointdsc, ransac, sm, synth, teaser, voxel
from tests import pdsc_cases
from types import SimpleNamespace as Args      # (FR.pair_params supplies the reference's defaults for what is not given)

t = torch.from_numpy
SIZES = [(3000, 2500), (2000, 2500), (2500, 1800)]
host = [synth.make_pair(N=n0, N1=n1, rho=0.5, s=0.9, seed=610 + k) for k, (n0, n1) in enumerate(SIZES)]
dev = [tuple(t(p[key]).cuda() for key in ("xyz0", "xyz1", "feats0", "feats1")) for p in host]
A, B, FA, FB = dev[0]

# the pair pipeline: MNN / open3D and GPF / GC
for kw in (dict(mode="MNN", codebase="open3D", ransac_n=3, o3d_conf=1.0), dict(mode="GPF", codebase="GC", prosac=True)):
    FR.read_result(FR.register_pair_dev(A, B, FA, FB, FR.pair_params(Args(iters=2048, **kw))))
# a ragged batch of three with the ICP stage inside, then the ICP stage on its own
params = FR.pair_params(Args(mode="MNN", codebase="open3D", iters=2048, ransac_n=3, o3d_conf=1.0, icp=True))
ws = _ext.Workspace(3000, 2500, 32, 2048, max_pairs=3)
out = FR.register_batch_dev(dev, params, ws=ws)
_ext.check(_ext.lib().lr_icp_batch(ws.handle, 0.6, 30, 1e-6, 1e-6, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
torch.cuda.synchronize()
# every operator once
i1, i2, _, _ = matching.nn_top2_dev(FA, FB, want_2nd=True, want_dist=True)
_, o0, o1, _ = matching.mutual_dev(FA, FB, i1, i2)
gpf = Args(GPF_grid_wid=7, GPF_factor=0.5, GPF_max_matches=300)
matching.Grid_Prioritized_Filter(FA, FB, None, i1, i2, A, gpf)
matching.Grid_Prioritized_Filter(FA, FB, None, i1, i2, A, gpf, BB_first=True)
T, _ = ransac.ransac_dev(A[o0.long()], B[o1.long()], 2048, want_mask=True)
ransac.refit_dev(A, B, i1, T)
ransac.icp_dev(A, B, T)
# descriptors narrower than 32: the coordinates themselves
FR.read_result(FR.register_pair_dev(A, B, A.contiguous(), B.contiguous(), FR.pair_params(Args(mode="MNN", codebase="open3D", iters=2048, ransac_n=3, o3d_conf=1.0))))
matching.nn_top2_dev(A, B)
# the cloud-level primitives: lr_voxel_dedup, lr_voxel_mean, lr_overlap, lr_overlap_batch over three ragged pairs
clouds = [(t(p["xyz0"]).double(), t(p["xyz1"]).double(), p["T_gt"]) for p in host]
voxel.sparse_quantize(clouds[0][0] / 0.3)
overlap.voxel_mean_dev(clouds[0][0], 0.3, clouds[0][2])
overlap.overlap_dev(*clouds[0])
overlap.overlap_batch_dev(clouds)
# the correspondence-set solvers over the mutual pairs, cut to three ragged sets: lr_sm_batch, lr_teaser_batch
src, tgt = A[o0.long()].contiguous(), B[o1.long()].contiguous()
sets = [len(src), 300, 65]
sm.sm_batch_dev([src[:m] for m in sets], [tgt[:m] for m in sets])
teaser.teaser_batch_dev([src[:m] for m in sets], [tgt[:m] for m in sets])
# the rest of that family on the same sets, batched and through the single-pair entry points: lr_pdsc_encode, lr_pdsc_solve (fed the
# encoder's outputs; with the trace arrays), lr_pdsc_register at two layers of synthetic weights, lr_dgr_refine (with the log)
S, G = [src[:m] for m in sets], [tgt[:m] for m in sets]
model = pointdsc.PointDSCModel.from_state_dict(pdsc_cases.shared_weights(2), 2)
enc = model.encoder.encode_batch(S, G)
pointdsc.solve_batch(S, G, [f for f, _, _ in enc], [c for _, c, _ in enc])
model.register_batch(S, G)
pointdsc.solve(S[0], G[0], *model.encoder.encode(S[0], G[0]), trace=True)
model.register(S[0], G[0])
dgr.refine_batch(S, G, max_iter=30)
dgr.refine(S[0], G[0], log=True, max_iter=30)
torch.cuda.synchronize()
# the branches of the RANSAC launch plan (lr_ransac_run) the calls above do not reach
gc = dict(mode="MNN", codebase="GC", prosac=True, iters=4096)      # GC defaults: exit rule (batches of 1 024, then 3 072 ids), PROSAC, ELC, LO + polish
ws5 = _ext.Workspace(3000, 2500, 32, 4096, max_pairs=5)
FR.register_batch_dev(dev + dev[:2], FR.pair_params(Args(**gc)), ws=ws5)      # more than four pairs, a batch of >= 2 048 ids: the pilot-ordered passes
FR.register_batch_dev(dev, FR.pair_params(Args(**gc)), ws=ws5)                # three pairs: eight helper groups per pair in the local optimisation
for kw in (dict(fast_rejection="SPRT"), dict(fast_rejection="NONE"), dict(GC_LO=False)):      # second model list; no pre-check; polish only
    FR.read_result(FR.register_pair_dev(A, B, FA, FB, FR.pair_params(Args(**gc, **kw))))
FR.read_result(FR.register_pair_dev(A, B, FA, FB, FR.pair_params(Args(mode="MNN", codebase="open3D", iters=2048, ransac_n=4, o3d_conf=1.0))))
ransac.ransac_dev(A[o0.long()], B[o1.long()], 2048, confidence=0.99, batch=512)      # the caller's batch length
torch.cuda.synchronize()
# the branches of the NN launch plans (lr_nn16_plan_fwd / lr_nn16_plan_rev) and of the form hint the calls above do not reach
big = synth.make_pair(N=3000, N1=8192, rho=0.5, s=0.9, seed=640)
G0, G1 = t(big["feats0"]).cuda(), t(big["feats1"]).cuda()
matching.nn_top2_dev(G0, G1, want_2nd=True)       # 256 column tiles: four forward strips on 256 CUs (the pairs above: one)
matching.nn_top2_dev(G0, G1, want_2nd=False)
for name, value in (("nn_sample_stride", 1), ("nn_sample_stride", 64), ("nn_blocks", 1), ("rev_strips", 1), ("rev_strips", 64)):
    ws1 = matching.workspace(3000, 8192)
    ws1.set_option(name, value)
    j1, j2, _, _ = matching.nn_top2_dev(G0, G1)
    matching.mutual_dev(G0, G1, j1, j2)            # a caller's list: the unseeded reverse pass
    ws1.set_option(name, 0)
# the form hint of single-pair calls: unknown and then one reading (both forms), two readings that agree (one form), a miss (the norms change)
unit = [F / F.norm(dim=1, keepdim=True) for F in (FA, FB)]
spread = [F * torch.linspace(0.5, 3.0, len(F), device=F.device)[:, None] for F in unit]
for U0, U1 in [unit] * 3 + [spread] * 3:
    matching.nn_top2_dev(U0, U1)
    torch.cuda.synchronize()      # (the hint is what the previous call's range kernel left in host memory)
print("entry_point_trace: done")
