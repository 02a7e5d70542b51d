"""`python -m test --fcgf_weights_file CHECKPOINT` end to end on the GPU: raw scans from a cloud cache, the FCGF descriptors computed on
the device (no feature cache), the RANSAC path behind them.  The checkpoint is random (tests/fcgf_cases.py), so recall means nothing
and is not asserted: the stats rows and the per-pair 4x4 motions must be there and finite."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from lidarregistration_amd import harness, io_lists, synth
from tests import fcgf_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cli(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(ROOT, "Experiments"))
    mod = importlib.import_module("test")
    yield mod
    sys.path.remove(os.path.join(ROOT, "Experiments"))


def test_cli_computes_the_descriptors_from_the_cloud_cache(cli, tmp_path, monkeypatch):
    raw0, raw1, T = synth.make_scan_pair(n0=6000, seed=8)
    name = io_lists.DATASET_NAMES["A"]
    clouds, sets = tmp_path / "clouds", tmp_path / "sets"
    io_lists.save_ref_cloud(str(clouds / name), 4, 10, raw0); io_lists.save_ref_cloud(str(clouds / name), 4, 11, raw1)
    os.makedirs(sets / name)
    with open(sets / name / "test.txt", "w") as f:
        f.write("session_ind i j " + " ".join(f"mot{k}" for k in range(16)) + "\n")
        for i, j, M in ((10, 11, T), (11, 10, np.linalg.inv(T))):
            f.write(f"4 {i} {j} " + " ".join("%.17g" % v for v in M.reshape(-1)) + "\n")
    ck = tmp_path / "fcgf.pth"
    torch.save({"state_dict": {k: torch.as_tensor(v) for k, v in fcgf_cases.make_state_dict(0, 5).items()}, "epoch": 1}, ck)
    monkeypatch.setenv("LIDARREG_CLOUD_CACHE", str(clouds)); monkeypatch.setenv("LIDARREG_BALANCED_SETS", str(sets))
    monkeypatch.delenv("LIDARREG_FEATURE_CACHE", raising=False)
    stats = cli.main(["--dataset", "A", "--algo", "RANSAC", "--mode", "MNN", "--iters", "2000", "--batch", "2", "--fcgf_weights_file", str(ck)])
    d = sorted((tmp_path / "outputs").iterdir())[-1]
    raw = np.load(d / "raw_stats.npy")
    ids, Ts = io_lists.read_coarse_motions(str(d / "coarse_motions.txt"))
    assert raw.shape == (2, 22) and np.array_equal(raw, stats, equal_nan=True)
    assert raw[:, 19:22].tolist() == [[4, 10, 11], [4, 11, 10]] and ids.tolist() == [[4, 10, 11], [4, 11, 10]]
    assert Ts.shape == (2, 4, 4) and np.isfinite(Ts).all() and np.allclose(Ts[:, 3], [0, 0, 0, 1])
    assert "fcgf_weights_file = " + str(ck) in (d / "log.txt").read_text()
    # the source behind the flag: the extractor's rows, nothing from a feature cache
    from lidarregistration_amd import fcgf
    src = harness.RefCloudSource(io_lists.read_pair_list(str(sets / name / "test.txt")), str(clouds / name), None, extractor=fcgf.FCGF.from_checkpoint(str(ck)))
    p = src.get(0)
    assert p["feats0"].shape == (p["xyz0"].shape[0], 32) and np.allclose(np.linalg.norm(p["feats0"], axis=1), 1.0, atol=1e-5)
    assert 0.5 * len(raw0) < p["xyz0"].shape[0] < len(raw0)
