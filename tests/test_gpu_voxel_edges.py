"""The voxel hash (csrc/lr_voxel.hip) on the clouds of tests/voxel_edges.py, held to the plain definition: floor, the first index of
every cell, ascending.  Needs an MI355X."""
import numpy as np
import pytest

from tests import voxel_edges as ve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voxel():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from lidarregistration_amd import _ext, voxel
    _ext.lib()
    return voxel


def _held(voxel, coords):
    cells, sel = voxel.sparse_quantize(coords, return_index=True)
    ec, es = ve.dedup_ref(coords)
    assert np.array_equal(sel.cpu().numpy(), es), (len(sel), len(es))
    assert np.array_equal(cells.cpu().numpy(), ec)
    only = voxel.sparse_quantize(coords, return_index=False)
    assert np.array_equal(only.cpu().numpy(), ec)
    return es


def test_voxel_long_merged_probe_chains(voxel):
    p = ve.probe_chain_cloud()
    sel = _held(voxel, p["coords"])
    assert sel.max() < 12500


@pytest.mark.parametrize("name", ["first_is_0", "first_is_49999"])
def test_voxel_one_heavily_contended_cell(voxel, name):
    sel = _held(voxel, ve.contention_clouds()[name])
    assert len(sel) == (1 if name == "first_is_0" else 50000)


def test_voxel_cell_limits_and_negative_floors(voxel):
    _held(voxel, ve.limit_cloud())


@pytest.mark.parametrize("name", list(ve.stride_clouds()))
def test_voxel_compaction_strides(voxel, name):
    _held(voxel, ve.stride_clouds()[name])


def test_voxel_wrong_device_is_refused(voxel):
    """lr_voxel_dedup takes caller-owned scratch: with another device current it refuses (LR_EINVAL, before any launch) instead of
    running its kernels on foreign pointers.  n == 0 takes no scratch and stays LR_OK.  The wrong device is the test hook's."""
    import torch
    from lidarregistration_amd import _ext
    L = _ext.lib()
    n = 1000
    c = torch.from_numpy(np.random.default_rng(3).uniform(-40, 40, (n, 3))).cuda()
    scratch = torch.empty(int(L.lr_voxel_dedup_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    sel = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        return L.lr_voxel_dedup(c.data_ptr(), n, sel.data_ptr(), cnt.data_ptr(), None, scratch.data_ptr(), scratch.numel(), st)
    assert call() == 0
    L.lr_debug_fake_current_device(torch.cuda.current_device() + 1)
    try:
        assert call() == -1 and b"device" in L.lr_last_error()
        assert L.lr_voxel_dedup(None, 0, None, cnt.data_ptr(), None, None, L.lr_voxel_dedup_scratch_bytes(0), st) == 0      # (null scratch)
    finally:
        L.lr_debug_fake_current_device(-1)
    assert int(cnt.item()) == 0
    assert call() == 0
    assert np.array_equal(sel[:int(cnt.item())].cpu().numpy(), ve.dedup_ref(c.cpu().numpy())[1])
