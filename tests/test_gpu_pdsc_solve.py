"""PointDSC's tail on the GPU (csrc/lr_pdsc_solve.hip), all through the C ABI (lidarregistration_amd.pointdsc's ctypes calls): every stage
against the numpy restatement (tests/pdsc_solve_cpu.py) FED WITH THE DEVICE'S OWN UPSTREAM OUTPUT, and the whole against the recording of
the reference's tail (tests/golden/g26_pdsc_solve.npz).

Rules, none derived from what the kernels return:
  * seeds: exact.
  * kNN, by band B = 4 x 128 x 2^-24 (the fp32 dot product of two unit vectors of 128 channels errs by at most 128 x 2^-24; two such sides
    of a comparison and the fp32 normalisation make the factor 4): every returned neighbour lies within B of the fp64 k'-th similarity,
    every row clearer than that is present, no self, no dead row, no row twice, descending within B.
  * weights: max(4 x yardstick, 16 x 2^-23 x max|w|), the yardstick the fp32 restatement's distance to the fp64 one on the same lists.
  * seed transforms: the device fit is fp64 on fp32 inputs, so is the restatement's (SVD Kabsch): 1e-12 x kappa x (1 + |centroid|) with
    kappa = s1 / (s2 + sign s3) of the covariance, the conditioning of the rotation; seeds with kappa > 1e8 are only held to a proper rotation.
  * counts, labels: exact given the device's transforms, except for rows whose fp64 residual lies within 1e-9 of the threshold.
  * best seed: the first of the largest device count; refinement: 1e-9 x (1 + max|T|) of the restatement started from the device's T_best
    (where the last fit's kappa is above 1e6 -- two inliers -- a proper rotation of the same weighted cost to 1e-9).
  * golden: max(4 x the reference's own fp32-vs-fp64 deviation, 16 x 2^-23 x max|reference|) (§16.3's rule); per-seed quantities on the seeds
    whose device neighbour set equals the recorded one, at least 95 % of them.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, pointdsc
from tests import pdsc_cases
from tests import pdsc_solve_cases as cases
from tests import pdsc_solve_cpu as cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g26_pdsc_solve.npz"))
P = cases.PARAMS
B = 4 * 128 * 2.0 ** -24
THR_BAND = 1e-9
NAMES = [c[0] for c in cases.GOLDEN]


def host(t):
    return t.cpu().numpy()


def run(c, trace=True, **kw):
    """lr_pdsc_solve on a case: dict of host arrays."""
    T, labels, info = pointdsc.solve(c["src"], c["tgt"], c["feat"], c["conf"], trace=trace, **dict(P, **kw.pop("params", {})), **kw)
    out = dict(info, T=T, labels=host(labels), seeds=host(info["seeds"]).astype(np.int64))
    out.pop("raw_trace", None)
    for k in ("knn", "weights", "seed_T", "counts"):
        if k in out:
            out[k] = host(out[k])
    return out


def rule(yard, ref):
    return max(4 * yard, 16 * 2.0 ** -23 * float(np.abs(ref).max(initial=0.0)))


def check_knn(c, live, fn, seeds, knn, k):
    kp = min(k, int(live.sum()) - 1)
    assert (knn[:, kp:] == -1).all()
    knn = knn[:, :kp]
    for lo in range(0, len(seeds), 256):
        s = cpu.sims(fn, live, seeds[lo:lo + 256])
        kth = -np.partition(-s, kp - 1, axis=1)[:, kp - 1]
        got = knn[lo:lo + 256]
        gs = np.take_along_axis(s, got, 1)
        assert np.isfinite(gs).all(), "a dead row or the seed itself among the neighbours"
        assert (np.sort(got, axis=1)[:, 1:] != np.sort(got, axis=1)[:, :-1]).all(), "a row twice"
        assert (gs >= kth[:, None] - B).all()
        present = np.zeros_like(s, bool)
        np.put_along_axis(present, got, True, 1)
        assert present[s > kth[:, None] + B].all(), "a row clearer than the band is missing"
        assert (gs[:, :-1] >= gs[:, 1:] - B).all()
    return knn


def kappa(A, Bp, w):
    w = w.astype(np.float64)
    den = w.sum() + 1e-6
    ca, cb = (A * w[:, None]).sum(0) / den, (Bp * w[:, None]).sum(0) / den
    H = ((A - ca) * w[:, None]).T @ (Bp - cb)
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    gap = s[1] + d * s[2]
    return (s[0] / gap if gap > 0 else np.inf), float(np.abs(ca).max())


def stagewise(tag, c, d, count_rows=None, **params):
    """Every stage of the device result d against the restatement fed with the device's own upstream output."""
    p = dict(P, **params)
    src, tgt, feat, conf = (c[k][:d["m"]] for k in ("src", "tgt", "feat", "conf"))
    m = d["m"]
    live = cpu.live_rows(src, tgt, feat, conf)
    assert d["dead"] == m - live.sum() and d["status"] == 0
    seeds = cpu.pick_seeds(src, conf, live, p["nms_radius"], p["ratio"])
    assert d["n_seeds"] == len(seeds) and np.array_equal(d["seeds"], seeds)
    fn = cpu.normalize(feat, live)
    knn = check_knn(c, live, fn, seeds, d["knn"].astype(np.int64), p["k"])
    kp = knn.shape[1]
    # S5, S6 on the device's lists
    w64 = cpu.seed_weights(fn, src, tgt, knn, p["sigma"], p["sigma_d"], p["num_iterations"])
    w32 = cpu.seed_weights(cpu.normalize32(feat, live), src, tgt, knn, p["sigma"], p["sigma_d"], p["num_iterations"], np.float32)
    bw = rule(float(np.abs(w32 - w64).max()), w64)
    dw = float(np.abs(d["weights"][:, :kp] - w64).max())
    assert not d["weights"][:, kp:].any() and dw <= bw, (dw, bw)
    # S7 on the device's weights
    worst, skipped = 0.0, 0
    for s in range(len(seeds)):
        A, Bp, w = src[knn[s]].astype(np.float64), tgt[knn[s]].astype(np.float64), d["weights"][s, :kp]
        T = d["seed_T"][s]
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-9 and np.array_equal(T[3], [0, 0, 0, 1])
        kap, cen = kappa(A, Bp, w)
        if not kap <= 1e8:
            skipped += 1
            continue
        dT = np.abs(T - cpu.fit(A, Bp, w)).max()
        worst = max(worst, dT / (1e-12 * kap * (1 + cen)))
        assert dT <= 1e-12 * kap * (1 + cen), (s, dT, kap)
    # S8 on the device's transforms
    rows = np.arange(len(seeds)) if count_rows is None else count_rows
    inexact = 0
    for lo in range(0, len(rows), 64):
        r = cpu.residuals(d["seed_T"][rows[lo:lo + 64]], src[live], tgt[live])
        lo_c, hi_c = (r < p["inlier_threshold"] - THR_BAND).sum(1), (r < p["inlier_threshold"] + THR_BAND).sum(1)
        got = d["counts"][rows[lo:lo + 64]]
        assert ((lo_c <= got) & (got <= hi_c)).all()
        inexact += int((lo_c != hi_c).sum())
    best = int(np.argmax(d["counts"]))
    assert (d["best_rank"], d["best_index"], d["best_count"]) == (best, seeds[best], d["counts"][best])
    assert np.array_equal(d["T_best"], d["seed_T"][best])
    r = cpu.residuals(d["T_best"], np.where(live[:, None], src, 0), np.where(live[:, None], tgt, 0))
    sure = np.abs(r - p["inlier_threshold"]) > THR_BAND
    assert np.array_equal(d["labels"][:m][sure], (live & (r < p["inlier_threshold"]))[sure]) and not d["labels"][m:].any()
    assert d["n_labels"] == d["labels"].sum() == d["best_count"]
    # S9 from the device's T_best
    last = []
    T, rounds = cpu.refine(d["T_best"], src, tgt, live, p["refine_threshold"], p["refine_iters"], last)
    dR = float(np.abs(d["T"] - T).max())
    assert d["refine_rounds"] == rounds
    kap = kappa(*last)[0] if last else 1.0
    if kap <= 1e6:
        assert dR <= 1e-9 * (1 + np.abs(T).max()), (dR, rounds, kap)
    else:                                              # (two inliers, collinear ones: the rotation about their axis is free; S7 promises a proper rotation of the same cost)
        R = d["T"][:3, :3]
        cost = lambda X: float((last[2] * ((last[0] @ X[:3, :3].T + X[:3, 3] - last[1]) ** 2).sum(1)).sum())
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9 and abs(cost(d["T"]) - cost(T)) <= 1e-9 * (1 + cost(T)), (kap, cost(d["T"]), cost(T))
    print(f"{tag}: {len(seeds)} seeds, k' {kp}; weights {dw:.2e} of {bw:.2e}; seed T worst {worst:.3f} of its bound ({skipped} seeds beyond kappa 1e8); "
          f"{inexact} counts with a row in the threshold band; best {best} ({d['best_count']}); refined {dR:.2e}, {rounds} fits")


# ---- the golden cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_golden(name):
    c = cases.golden_case(name)
    m = c["m"]
    assert str(GOLD[name + "/sha256"]) == cases.checksum(c)
    d = run(c)
    stagewise(name, c, d)
    g = {k: GOLD[f"{name}/{k}"] for k in ("seeds", "knn", "weights", "seed_T", "counts", "best", "labels", "T_best", "T", "dev_weights", "dev_seed_T", "dev_T_best", "dev_T")}
    rec_seeds = g["seeds"].astype(np.int64)
    assert set(rec_seeds) == set(d["seeds"])           # (the order inside a group of equal keys is S2's, which stagewise() holds exactly)
    row = {int(s): i for i, s in enumerate(d["seeds"])}
    at = np.array([row[int(s)] for s in rec_seeds])
    kp = g["knn"].shape[1]
    knn = d["knn"][at][:, :kp]
    same = np.array([set(a) == set(b) for a, b in zip(g["knn"], knn)])
    assert same.mean() >= 0.95
    order = lambda w_, k_: np.stack([a[np.argsort(b)] for a, b in zip(w_, k_)])
    dw = float(np.abs(order(g["weights"][same], g["knn"][same]) - order(d["weights"][at][same][:, :kp], knn[same])).max())
    dT = float(np.abs(g["seed_T"][same] - d["seed_T"][at][same]).max())
    dB, dR = float(np.abs(g["T_best"] - d["T_best"]).max()), float(np.abs(g["T"] - d["T"]).max())
    bw, bT = rule(float(g["dev_weights"]), g["weights"]), rule(float(g["dev_seed_T"]), g["seed_T"])
    bB, bR = rule(float(g["dev_T_best"]), g["T_best"]), rule(float(g["dev_T"]), g["T"])
    print(f"{name}: {same.mean():.3f} of the seeds with the recorded neighbour set; |device - fp64 recording| / allowed: weights {dw:.2e} / {bw:.2e}, "
          f"seed T {dT:.2e} / {bT:.2e}, T_best {dB:.2e} / {bB:.2e}, T {dR:.2e} / {bR:.2e}")
    assert dw <= bw and dT <= bT
    # the best seed is the recording's -- or, where the reference's argsort ordered a group of equal keys otherwise than S2 does, its twin
    rec_best = rec_seeds[int(g["best"])]
    assert d["best_index"] == rec_best or (name == "m1000" and c["conf"][d["best_index"]] == c["conf"][rec_best] and abs(d["best_index"] - rec_best) == 1)
    assert d["best_count"] == g["counts"].max()
    assert dB <= bB and dR <= bR
    # labels: equal, except where the recorded residual is within the transform's bound (times the lever arm) of the threshold
    r = cpu.residuals(g["T_best"], c["src"], c["tgt"])
    sure = np.abs(r - P["inlier_threshold"]) > bB * (1 + np.abs(c["src"]).sum(1))
    assert np.array_equal(d["labels"][sure], np.unpackbits(g["labels"])[:m][sure]) and sure.mean() > 0.99


# ---- shapes of the kernel's plan -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain(m, seed=0):
    c = cases.case(m, seed=seed)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("m", (20, 32, 33, 129, 1289, 1290))
def test_plan_edges(m):
    """ps_make_plan: one key chunk up to m = 32, two from 33 on; one seed block of 128 up to 1 289 rows (128 seeds), two from 1 290 on (129);
    m = 20: k' = m - 1 = 19."""
    want = {20: (1, 1), 32: (1, 1), 33: (1, 2), 129: (1, 5), 1289: (1, 7), 1290: (2, 7)}[m]        # (41 tiles of 32 keys in 7 chunks of 6)
    pl = cpu.plan(cpu.n_seeds(m, P["ratio"]), m)
    assert (pl["nsb"], pl["chunks"]) == want
    d = run(plain(m))
    stagewise(f"m = {m}", plain(m), d)
    assert d["knn"].shape[1] == P["k"] and (m >= 41 or (d["knn"][:, m - 1:] == -1).all())


def test_all_neighbours_k_64_and_small_k():
    c = plain(257)
    for k in (64, 1, 7):
        d = run(c, params=dict(k=k))
        stagewise(f"k = {k}", c, d, k=k)


def test_largest_size():
    """m = 32 768, 3 276 seeds in 26 seed blocks x 8 chunks of 4 096 keys, against the slabbed restatement (counts on every 16th seed and on
    every seed at the top count)."""
    m = 32768
    c = plain(m)
    assert cpu.plan(cpu.n_seeds(m, P["ratio"]), m) == dict(nsb=26, chunks=8, per=4096)
    d = run(c)
    assert d["n_seeds"] == 3276
    rows = np.union1d(np.arange(0, 3276, 16), np.flatnonzero(d["counts"] == d["counts"].max())[:64])
    stagewise("m = 32 768", c, d, count_rows=rows)
    assert d["best_count"] > 0.15 * m


def test_live_count_below_m():
    c = plain(1000)
    m_dev = torch.tensor([300], dtype=torch.int32, device="cuda")
    d = run(c, m_dev=m_dev)
    assert d["m"] == 300
    stagewise("m_dev 300 of 1 000", c, d)
    assert host(pointdsc.solve_batch.last_raw[1][0])[30:100].tolist() == [-1] * 70        # seeds_out: -1 from n_seeds to (int)(m ratio)
    short = {k: (v[:300] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    e = run(short)
    assert np.array_equal(d["T"], e["T"]) and np.array_equal(d["labels"][:300], e["labels"]) and np.array_equal(d["seeds"], e["seeds"])


def test_dead_rows():
    """NaN / Inf in src, tgt, conf and a feature row -- the best candidate (largest confidence) and a row that would be a neighbour among them."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in plain(700).items()}
    clean = run(plain(700))
    first = int(clean["seeds"][0])
    nb = int(clean["knn"][1, 0])
    dead = sorted({first, nb, 5, 699})
    c["src"][first, 2] = np.nan; c["feat"][nb, 64] = np.inf; c["conf"][5] = np.nan; c["tgt"][699, 0] = -np.inf
    d = run(c)
    assert d["dead"] == len(dead) and d["n_seeds"] == int((700 - len(dead)) * P["ratio"])
    assert not np.isin(dead, d["seeds"]).any() and not np.isin(dead, d["knn"]).any() and not d["labels"][dead].any()
    stagewise("dead rows", c, d)
    assert np.isfinite(d["T"]).all() and np.abs(d["T"] - clean["T"]).max() < 1e-2       # (at most four of ~140 inliers with 5 cm noise are gone)


def test_all_dead_and_too_few():
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in plain(64).items()}
    c["conf"][:] = np.nan
    d = run(c)
    assert (d["status"], d["dead"], d["n_seeds"], d["best_rank"], d["best_index"], d["n_labels"]) == (1, 64, 0, -1, -1, 0)
    assert np.array_equal(d["T"], np.eye(4)) and np.array_equal(d["T_best"], np.eye(4)) and not d["labels"].any()
    for m in (1, 5, 9):
        d = run(plain(m))
        assert (d["status"], d["m"], d["n_seeds"], d["refine_rounds"]) == (2, m, 0, 0) and np.array_equal(d["T"], np.eye(4)) and not d["labels"].any()


def test_all_outliers():
    c = cases.all_outliers(1000)
    d = run(c)
    stagewise("all outliers", c, d)
    assert d["best_count"] < 20 and np.isfinite(d["T"]).all()


def test_parameters():
    c = plain(500)
    for kw in (dict(ratio=0.5), dict(ratio=1.0, k=16), dict(nms_radius=5.0), dict(nms_radius=0.0), dict(num_iterations=1), dict(num_iterations=50, sigma=0.7),
               dict(refine_iters=0), dict(refine_iters=1), dict(inlier_threshold=0.1, refine_threshold=0.3), dict(sigma_d=0.3)):
        d = run(c, params=kw)
        stagewise(str(kw), c, d, **kw)
    assert run(c, params=dict(refine_iters=0))["refine_rounds"] == 0


# ---- bits ------------------------------------------------------------------------------------------------------------------------------------
def _bits(d):
    return [np.ascontiguousarray(d[k]).tobytes() for k in ("T", "T_best", "labels", "seeds")] + [tuple(d[k] for k in ("status", "m", "dead", "n_seeds", "best_rank", "best_index", "best_count", "n_labels", "refine_rounds"))]


def test_same_bits_on_every_run_and_over_any_scratch():
    c = plain(3000)
    a, b, z = run(c, poison=0x00), run(c, poison=0xFF), run(c)
    for k in ("knn", "weights", "seed_T", "counts"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], z[k]), k
    assert _bits(a) == _bits(b) == _bits(z)


def test_ragged_batch_is_the_single_calls():
    ms = (0, 5, 1000, 41, 300)
    cs = [plain(m) if m else dict(src=np.zeros((0, 3), np.float32), tgt=np.zeros((0, 3), np.float32), feat=np.zeros((0, 128), np.float32), conf=np.zeros(0, np.float32)) for m in ms]
    for poison in (0x00, 0xFF):
        out = pointdsc.solve_batch(*[[c[k] for c in cs] for k in ("src", "tgt", "feat", "conf")], poison=poison, **P)
        for k, (c, m) in enumerate(zip(cs, ms)):
            T, labels, info = out[k]
            got = dict(info, T=T, labels=host(labels), seeds=host(info["seeds"]).astype(np.int64))
            assert _bits(got) == _bits(run(c, trace=False)), (k, m)
        assert [o[2]["status"] for o in out] == [1, 2, 0, 0, 0]


def _untouched(t, fill):
    return bool((t == fill).all())


def test_null_outputs():
    c = plain(300)
    full = run(c)
    for wl, ws in ((False, None), (None, False), (False, False)):
        d = run(c, trace=False, want_labels=wl, want_seeds=ws, poison=0xFF)
        labels, seeds = pointdsc.solve_batch.last_raw
        assert np.array_equal(d["T"], full["T"]) and d["n_labels"] == full["n_labels"]
        assert _untouched(labels[0], 255) if wl is False else np.array_equal(d["labels"], full["labels"])
        assert _untouched(seeds[0], -7) if ws is False else np.array_equal(host(seeds[0])[:30], full["seeds"])
    cs = [plain(300), plain(41)]
    both = pointdsc.solve_batch(*[[c[k] for c in cs] for k in ("src", "tgt", "feat", "conf")], **P)
    out = pointdsc.solve_batch(*[[c[k] for c in cs] for k in ("src", "tgt", "feat", "conf")], want_labels=[False, True], want_seeds=[True, False], **P)
    labels, seeds = pointdsc.solve_batch.last_raw
    assert _untouched(labels[0], 255) and torch.equal(out[1][1], both[1][1]) and torch.equal(out[0][2]["seeds"], both[0][2]["seeds"]) and _untouched(seeds[1], -7)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(out, both))


# ---- register ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(num_layers=2):
    return pointdsc.PointDSCModel.from_state_dict(pdsc_cases.shared_weights(num_layers), num_layers, cases.SIGMA_D, **{k: v for k, v in P.items() if k not in ("sigma_d", "sigma")})


def test_register_is_encode_then_solve_bit_for_bit():
    """Random encoder weights give seeds without meaning; what is pinned is the bytes."""
    mdl = model()
    assert mdl.solve_kw["sigma"] == 1.0 and mdl.solve_kw["sigma_d"] == cases.SIGMA_D
    ms = (700, 0, 33, 129)
    pairs = [pdsc_cases.planted(m) if m else (np.zeros((0, 3), np.float32),) * 2 for m in ms]
    for poison in (0x00, 0xFF):
        out = mdl.register_batch([p[0] for p in pairs], [p[1] for p in pairs], poison=poison, want_feat=[True, True, False, True], want_conf=[False, True, True, True])
        for k, ((src, tgt), m) in enumerate(zip(pairs, ms)):
            T, labels, info = out[k]
            if m == 0:
                assert info["status"] == 1
                continue
            feat, conf = mdl.encoder.encode(src, tgt)
            T1, labels1, info1 = pointdsc.solve(src, tgt, feat, conf, **mdl.solve_kw)
            assert np.array_equal(T, T1) and torch.equal(labels, labels1) and torch.equal(info["seeds"], info1["seeds"]), (k, m)
            assert all(np.array_equal(info[x], info1[x]) for x in ("T_best", "status", "n_seeds", "best_index", "best_count", "refine_rounds"))
            if k != 2:
                assert torch.equal(info["feat"], feat)
            if k != 0:
                assert torch.equal(info["conf"], conf)
            single = mdl.register(src, tgt, poison=poison)
            assert np.array_equal(single[0], T) and torch.equal(single[1], labels)
    r = mdl.forward(dict(src_keypts=torch.from_numpy(pairs[0][0])[None], tgt_keypts=torch.from_numpy(pairs[0][1])[None], testing=True))
    assert r["final_trans"].shape == (1, 4, 4) and r["final_labels"].shape == (1, 700) and r["final_trans"].dtype == torch.float32
    assert np.array_equal(host(r["final_trans"][0]), out[0][0].astype(np.float32))


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_call_can_be_captured_into_a_graph():
    """One lr_pdsc_solve (m = 700, an m_dev buffer) recorded on a side stream and replayed on other inputs and live counts gives the bytes of
    the eager calls, whatever the scratch held."""
    L = _ext.lib()
    m = 700
    configs = [(cases.case(m, seed=s), live) for s, live in ((1, 700), (2, 129), (3, 0))]
    dev = dict(src=torch.empty((m, 3), dtype=torch.float32, device="cuda"), tgt=torch.empty((m, 3), dtype=torch.float32, device="cuda"),
               feat=torch.empty((m, 128), dtype=torch.float32, device="cuda"), conf=torch.empty(m, dtype=torch.float32, device="cuda"))
    m_dev = torch.empty(1, dtype=torch.int32, device="cuda")
    labels = torch.empty(m, dtype=torch.uint8, device="cuda"); seeds = torch.empty(70, dtype=torch.int32, device="cuda")
    res = torch.zeros(ctypes.sizeof(_ext.PdscSolveResult), dtype=torch.uint8, device="cuda")
    sc = torch.empty(L.lr_pdsc_solve_scratch_bytes(m), dtype=torch.uint8, device="cuda")
    p = pointdsc.solve_params(**P)
    s = torch.cuda.Stream()

    def call():
        _ext.check(L.lr_pdsc_solve(dev["src"].data_ptr(), dev["tgt"].data_ptr(), m, m_dev.data_ptr(), dev["feat"].data_ptr(), dev["conf"].data_ptr(), ctypes.byref(p),
                                   res.data_ptr(), labels.data_ptr(), seeds.data_ptr(), None, None, None, None, sc.data_ptr(), sc.numel(), s.cuda_stream))

    def load(cfg, poison):
        c, live = cfg
        for k, t in dev.items():
            t.copy_(torch.from_numpy(c[k]))
        m_dev.fill_(live); labels.fill_(7); seeds.fill_(7); res.fill_(0x55); sc.fill_(poison)
        torch.cuda.synchronize()

    def outputs():
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (res, labels, seeds)]
    eager = []
    for cfg in configs:
        load(cfg, 0x00); call(); eager.append(outputs())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for k, (cfg, want) in list(enumerate(zip(configs, eager)))[::-1] + [(0, (configs[0], eager[0]))]:
        load(cfg, 0xFF if k & 1 else 0x00); g.replay()
        assert outputs() == want, k
    for (c, live), e in zip(configs, eager):
        r = _ext.PdscSolveResult.from_buffer_copy(e[0])
        assert (r.status, r.m, r.n_seeds) == (0 if live else 1, live, int(live * 0.1))
        if live:
            d = run({k: (v[:live] if isinstance(v, np.ndarray) else v) for k, v in c.items()}, trace=False)
            assert np.array_equal(np.array(r.T).reshape(4, 4), d["T"]) and np.array_equal(np.frombuffer(e[1], np.uint8)[:live], d["labels"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    L = _ext.lib()
    m = 64
    c = plain(m)
    t = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("src", "tgt", "feat", "conf")}
    res = torch.zeros(ctypes.sizeof(_ext.PdscSolveResult), dtype=torch.uint8, device="cuda")
    need = L.lr_pdsc_solve_scratch_bytes(m)
    sc = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def solve(p=None, m_=m, res_=res, scp=None, scn=need, **repl):
        a = {k: v.data_ptr() for k, v in t.items()}
        a.update(repl)
        p = p or pointdsc.solve_params(**P)
        return L.lr_pdsc_solve(a["src"], a["tgt"], m_, None, a["feat"], a["conf"], ctypes.byref(p), None if res_ is None else res_.data_ptr(), None, None, None, None, None, None,
                               sc.data_ptr() if scp is None else scp, scn, None)

    def refused(rc, word):
        err = L.lr_last_error().decode()
        assert rc == -1 and word in err, (rc, err)
    assert solve() == 0
    torch.cuda.synchronize()
    before = res.cpu().numpy().tobytes()
    for name, bad in (("num_iterations", 0), ("num_iterations", 1001), ("k", 0), ("k", 65), ("refine_iters", -1), ("refine_iters", 1001), ("ratio", 0.0), ("ratio", 1.5),
                      ("ratio", float("nan")), ("nms_radius", -1.0), ("nms_radius", float("inf")), ("inlier_threshold", 0.0), ("refine_threshold", float("nan")),
                      ("sigma_d", 0.0), ("sigma", -1.0), ("sigma", float("inf"))):
        refused(solve(pointdsc.solve_params(**dict(P, **{name: bad}))), name)
    p = pointdsc.solve_params(**P); p.struct_size = 56
    refused(solve(p), "struct_size")
    refused(solve(src=None), "null point array"); refused(solve(feat=None), "null feat"); refused(solve(conf=None), "null conf")
    refused(solve(feat=t["feat"].data_ptr() + 4), "aligned")
    refused(solve(res_=None), "null pointer"); refused(solve(m_=-1), "negative"); refused(solve(m_=32769), "32768")
    refused(solve(scn=need - 1), "lr_pdsc_solve_scratch_bytes"); refused(solve(scp=sc.data_ptr() + 128), "256-byte aligned")
    refused(L.lr_pdsc_solve(t["src"].data_ptr(), t["tgt"].data_ptr(), m, None, t["feat"].data_ptr(), t["conf"].data_ptr(), None, res.data_ptr(), None, None, None, None, None, None,
                            sc.data_ptr(), need, None), "null params")
    pp = lambda *v: (ctypes.c_void_p * len(v))(*v)
    args = lambda n: (n, pp(t["src"].data_ptr()), pp(t["tgt"].data_ptr()), (ctypes.c_int32 * 1)(m), None, pp(t["feat"].data_ptr()), pp(t["conf"].data_ptr()),
                      ctypes.byref(pointdsc.solve_params(**P)), res.data_ptr(), None, None, sc.data_ptr(), need, None)
    refused(L.lr_pdsc_solve_batch(*args(0)), "npairs"); refused(L.lr_pdsc_solve_batch(*args(65)), "npairs")
    a = list(args(1)); a[5] = None
    refused(L.lr_pdsc_solve_batch(*a), "null pointer")
    # register: the tail's params, the encoder's params and weights, its own scratch size
    mdl = model()
    enc = mdl.encoder
    rneed = L.lr_pdsc_register_scratch_bytes(m)
    rsc = torch.empty(rneed, dtype=torch.uint8, device="cuda")

    def register(ep=None, sp=None, wb=None, scn=rneed):
        return L.lr_pdsc_register(t["src"].data_ptr(), t["tgt"].data_ptr(), m, None, enc.weights.data_ptr(), enc.weights.numel() * 4 if wb is None else wb,
                                  ctypes.byref(ep or enc.params), ctypes.byref(sp or pointdsc.solve_params(**P)), res.data_ptr(), None, None, None, None,
                                  rsc.data_ptr(), scn, None)
    assert register() == 0
    refused(register(sp=pointdsc.solve_params(**dict(P, k=99))), "k must")
    refused(register(ep=_ext.PdscParams(num_layers=0)), "num_layers"); refused(register(wb=16), "weights_bytes")
    refused(register(scn=rneed - 1), "lr_pdsc_register_scratch_bytes")
    assert L.lr_pdsc_solve_scratch_bytes(-1) == 0 and L.lr_pdsc_solve_scratch_bytes(32769) == 0 and L.lr_pdsc_register_scratch_bytes(32769) == 0
    assert L.lr_version() == 103
    torch.cuda.synchronize()
    assert solve() == 0
    torch.cuda.synchronize()
    assert res.cpu().numpy().tobytes() == before        # no refused call launched anything that wrote
