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
