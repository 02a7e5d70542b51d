"""`python -m test --algo PointDSC --chosen_snapshot DIR` end to end on the GPU: a snapshot directory in the reference's layout (config.json,
models/model_best.pkl) written by the test from pdsc_cases.shared_weights, four small synthetic pairs.  The weights are random, so the
transforms mean nothing; what is pinned is that the run completes, writes its files with finite rows, and that every pair's transform
is PointDSCModel.register's on the same correspondences (to the 16 decimals of coarse_motions.txt)."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import pdsc_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_LAYERS = 2


@pytest.fixture()
def cli(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(ROOT, "Experiments"))
    mod = importlib.import_module("test")
    yield mod
    sys.path.remove(os.path.join(ROOT, "Experiments"))


def write_snapshot(d):
    os.makedirs(d / "models")
    # (inlier_threshold and sigma_d as a 3DMatch snapshot holds them: the CLI overrides both)
    cfg = dict(in_dim=6, num_layers=NUM_LAYERS, num_channels=128, num_iterations=10, ratio=0.1, k=40, inlier_threshold=0.1, sigma_d=0.1, descriptor="fcgf")
    (d / "config.json").write_text(json.dumps(cfg))
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in pdsc_cases.shared_weights(NUM_LAYERS).items()}, str(d / "models" / "model_best.pkl"))
    return str(d)


def test_cli_runs_pointdsc_end_to_end(cli, tmp_path):
    from lidarregistration_amd import _ext, io_lists, pointdsc, synth
    snap = write_snapshot(tmp_path / "snapshot")
    n, N, num_node = 4, 3000, 2000
    stats = cli.main(["--dataset", "synthetic", "--num_pairs", str(n), "--synthetic_n", str(N), "--algo", "PointDSC", "--chosen_snapshot", snap,
                      "--num_node", str(num_node), "--batch", "3"])
    d = sorted((tmp_path / "outputs").iterdir())[-1]
    for f in ("raw_stats.npy", "raw_stats.columns.txt", "log.txt", "coarse_motions.txt"):
        assert (d / f).exists(), f
    raw = np.load(d / "raw_stats.npy")
    assert raw.shape == (n, 22) and np.array_equal(raw, stats, equal_nan=True)
    filled = [0, 1, 2, 9, 10, 11, 12, 13, 14, 15, 17, 19, 20, 21]
    assert np.isfinite(raw[:, filled]).all() and (raw[:, 9] > 0).all() and (raw[:, 17] == num_node).all()
    assert "PointDSC" in (d / "log.txt").read_text()
    ids, T = io_lists.read_coarse_motions(str(d / "coarse_motions.txt"))
    # the same correspondences, the same model, one pair at a time
    model = pointdsc.load_snapshot(snap)
    assert model.encoder.num_layers == NUM_LAYERS and model.solve_kw["inlier_threshold"] == 0.6 and model.solve_kw["nms_radius"] == 0.6
    assert model.solve_kw["sigma_d"] == float(np.float32(1.2)) and model.solve_kw["sigma"] == 1.0
    dev = torch.device("cuda", torch.cuda.current_device())

    class A:
        seed = 51
    A.num_node = num_node
    for i in range(n):
        p = synth.make_pair_dev(N=N, seed=51 + i, device=dev)
        ws = _ext.Workspace(p["feats0"].shape[0], p["feats1"].shape[0], p["feats0"].shape[1], 1)
        i0, i1, cnt = pointdsc.correspondences_dev(p["xyz0"], p["xyz1"], p["feats0"], p["feats1"], A, ws, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ws.close()
        assert int(cnt[0]) == num_node and len(torch.unique(i0)) == num_node
        Ti, labels, info = model.register(p["xyz0"][i0.long()], p["xyz1"][i1.long()])
        assert info["status"] == 0 and info["n_seeds"] == num_node // 10
        assert np.abs(T[i] - Ti).max() <= 1e-15, i     # (coarse_motions.txt holds 16 decimals)


def test_cli_refuses_what_is_not_built(cli, tmp_path, capsys):
    snap = write_snapshot(tmp_path / "snapshot")
    with pytest.raises(SystemExit):
        cli.main(["--dataset", "synthetic", "--algo", "PointDSC", "--chosen_snapshot", snap, "--solver", "RANSAC"])
    assert "--solver RANSAC is not built" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--dataset", "synthetic", "--algo", "PointDSC"])
    assert "--chosen_snapshot" in capsys.readouterr().err
    assert cli.get_args(["--dataset", "synthetic"]).algo == "RANSAC"          # the default stays
