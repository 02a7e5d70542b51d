"""lr_workspace_create_wide without a device: every refusal returns before the first HIP call, with the argument's name in
lr_last_error; the narrow constructors still refuse 33 with their own text."""
import ctypes

import pytest

from lidarregistration_amd import _ext


@pytest.fixture(scope="module")
def L():
    _ext.build()
    return _ext.lib()


def create_wide(L, pairs, n0, n1, dim, iters, out=True):
    h = ctypes.c_void_p()
    rc = L.lr_workspace_create_wide(ctypes.byref(h) if out else None, pairs, n0, n1, dim, iters)
    assert not h.value
    return rc, L.lr_last_error()


@pytest.mark.parametrize("dim", [32, 1, 0, -5])
def test_narrow_dims_are_sent_to_the_narrow_constructor(L, dim):
    rc, err = create_wide(L, 1, 100, 100, dim, 10)
    assert rc == -1 and b"dim" in err
    if dim >= 1:
        assert b"use lr_workspace_create" in err


@pytest.mark.parametrize("dim", [129, 4096])
def test_too_wide(L, dim):
    rc, err = create_wide(L, 1, 100, 100, dim, 10)
    assert rc == -1 and b"dim must lie in 33..128" in err


def test_pair_and_size_limits_and_null(L):
    assert create_wide(L, 1, 100, 100, 33, 10, out=False) == (-1, b"lr_workspace_create_wide: null output (ws)")
    for pairs in (0, 65, -1):
        rc, err = create_wide(L, pairs, 100, 100, 33, 10)
        assert rc == -1 and b"max_pairs" in err
    rc, err = create_wide(L, 1, 0, 100, 64, 10)
    assert rc == -1 and b"max_n0" in err
    rc, err = create_wide(L, 1, 100, -3, 64, 10)
    assert rc == -1 and b"max_n1" in err
    rc, err = create_wide(L, 1, 100, 100, 64, -1)
    assert rc == -1 and b"max_iters" in err
    rc, err = create_wide(L, 1, 1 << 22, 100, 128, 10)
    assert rc == -4 and b"max_n0" in err and b"2^22" in err      # LR_ESIZE
    rc, err = create_wide(L, 64, 100, 1 << 22, 128, 10)
    assert rc == -4 and b"max_n1" in err


def test_old_constructors_keep_their_refusal(L):
    h = ctypes.c_void_p()
    assert L.lr_workspace_create(ctypes.byref(h), 10, 10, 33, 10) == -1 and b"1 to 32" in L.lr_last_error()
    assert L.lr_workspace_create_batch(ctypes.byref(h), 4, 10, 10, 33, 10) == -1 and b"1 to 32" in L.lr_last_error()
    assert L.lr_version() == 103


def test_fits_keeps_the_kinds_apart():
    class W(_ext.Workspace):
        def __init__(self, dim, wide):      # (no device: only what fits() reads)
            self.max_n0 = self.max_n1 = 100; self.dim = dim; self.max_iters = 10; self.is_wide = wide; self._h = None
    assert W(33, True).fits(50, 50, 33, 5) and not W(33, True).fits(50, 50, 32, 5) and not W(33, True).fits(50, 50, 34, 5)
    assert W(32, False).fits(50, 50, 32, 5) and not W(32, False).fits(50, 50, 33, 5)
    # only the kind differs (a handle of the other constructor under the same numbers): the width alone does not make it fit
    assert not W(33, False).fits(50, 50, 33, 5) and not W(32, True).fits(50, 50, 32, 5)
