"""corrset.BatchCall builds the argument tuple of every correspondence-set entry point (lr_teaser, lr_sm, lr_pdsc_encode, lr_pdsc_solve,
lr_pdsc_register, lr_dgr_refine and their _batch forms) from one description per family: the tuple against the argtypes of _ext.py, the
NULLs of the `want` selectors and of omitted inputs, the output tensors' shapes and fills.  No GPU: the buffers are CPU tensors and nothing is
launched (the library is asked for *_scratch_bytes / *_weights_bytes only)."""
import ctypes

import numpy as np
import pytest
import torch

from lidarregistration_amd import _ext, corrset, dgr, pointdsc, sm, teaser
from tests import pdsc_cases

MS = [0, 1, 5]
RATIO, K, MAX_ITER = 0.5, 7, 9                  # seeds / trace rows int(m RATIO): 0, 0, 2; trace columns; log rows
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
PP, IP = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32)
cap = lambda m: int(m * RATIO)
# per family: the solver, and per output (name, dtype, fill, rows(m), columns or None)
FAMILIES = {
    "teaser": (teaser.SOLVER, [("clique", I32, -1, int, None)]),
    "sm": (sm.SOLVER, [("eig", F32, -1.0, int, None), ("labels", U8, 255, int, None)]),
    "encode": (pointdsc.ENCODE, [("feat", F32, -1.0, int, 128), ("conf", F32, -1.0, int, None)]),
    "solve": (pointdsc.SOLVE, [("labels", U8, 255, int, None), ("seeds", I32, -7, cap, None)]),
    "register": (pointdsc.REGISTER, [("feat", F32, -1.0, int, 128), ("conf", F32, -1.0, int, None), ("labels", U8, 255, int, None), ("seeds", I32, -7, cap, None)]),
    "dgr": (dgr.SOLVER, []),
}
# the single-only outputs: (keyword, [(dtype, fill, rows(m), columns or None)])
EXTRAS = {"solve": ("trace", [(I32, -7, cap, K), (F32, -7.0, cap, K), (F64, -7.0, cap, 16), (I32, -7, cap, None)]),
          "dgr": ("log", [(F64, np.nan, lambda m: MAX_ITER, 10)])}


@pytest.fixture(scope="module")
def blob():
    b = torch.from_numpy(pointdsc.pack(pdsc_cases.shared_weights(1), 1))
    assert b.numel() * 4 == _ext.lib().lr_pdsc_weights_bytes(1)
    return b


def build(name, ms, blob, single=False, **kw):
    """The BatchCall of a family over pairs of ms rows, with every optional input given unless kw says otherwise."""
    rng = np.random.default_rng(len(ms))
    pts = lambda: [rng.standard_normal((m, 3)).astype(np.float32) for m in ms]
    if name in ("encode", "register"):
        enc = _ext.PdscParams(num_layers=1)
        kw.update(blob=blob.data_ptr(), blob_bytes=blob.numel() * 4,
                  params=(enc,) if name == "encode" else (enc, pointdsc.solve_params(ratio=RATIO, k=K)))
    if name == "solve":
        kw = dict(dict(feat=[np.zeros((m, 128), np.float32) for m in ms], conf=[np.zeros(m, np.float32) for m in ms], ratio=RATIO, k=K), **kw)
    if name == "dgr":
        kw = dict(dict(weights=[np.ones(m, np.float32) for m in ms], T_inits=[np.eye(4)] * len(ms), max_iter=MAX_ITER), **kw)
    return corrset.BatchCall(FAMILIES[name][0], pts(), pts(), single=single, device="cpu", **kw)


def layout(call):
    """(the entry point's argtypes, the position of the first per-pair output): the outputs follow the result block, which follows
    the last params struct."""
    types = call._fn.argtypes
    structs = [i for i, t in enumerate(types) if isinstance(t, type(PP)) and issubclass(t._type_, ctypes.Structure)]
    assert len(structs) == len(call.solver.params)
    return types, structs[-1] + 2


def entries(a):
    return [a[k] for k in range(len(a))]


@pytest.mark.parametrize("single", [False, True], ids=["batch", "single"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_arguments_follow_the_argtypes(name, single, blob):
    solver, outs = FAMILIES[name]
    ms = [5] if single else MS
    n = len(ms)
    m_devs = [torch.tensor([m], dtype=I32) for m in ms]
    call = build(name, ms, blob, single, m_devs=m_devs)
    types, o0 = layout(call)
    assert call._fn is getattr(_ext.lib(), solver.single if single else solver.batch)
    assert len(call._args) + 1 == len(types)                       # (+ the stream)
    for i, (t, a) in enumerate(zip(types, call._args)):
        if t in (ctypes.c_int, ctypes.c_size_t):
            assert type(a) is int, (i, a)
        if t is PP:
            assert a is None or (isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p and len(a) == n), (i, a)
        if t is IP:
            assert entries(a) == ms
    assert (IP in types) == (not single)
    # the pairs, the live counts and every extra input are there, in the ABI's order
    first = 0 if single else 1
    given = [call.srcs, call.tgts, None, m_devs, *call.inputs]
    for i, ts in enumerate(given):
        if ts is not None:
            a = call._args[first + i]
            assert ([a] if single else entries(a)) == [t.data_ptr() or None for t in ts], i
    assert (call._args[2] == ms[0] if single else call._args[0] == n) and len(call.inputs) == len(solver.inputs)
    assert call._args[o0 - 1] == call.res.data_ptr() and call.res.numel() == n * ctypes.sizeof(solver.result)
    assert call._args[-2:] == (call.scratch.data_ptr(), call.scratch.numel())
    assert call.scratch.numel() == max(getattr(_ext.lib(), solver.scratch_bytes)(max(ms)) * n, 256)
    # the outputs: max(rows, 1) rows of the documented fill, all of them passed
    assert len(call.outs) == len(outs) == len(solver.outputs)
    for i, (oname, dtype, fill, rows, cols) in enumerate(outs):
        assert solver.outputs[i].name == oname
        for k, m in enumerate(ms):
            t = call.outs[i][k]
            assert t.dtype == dtype and tuple(t.shape) == (max(rows(m), 1),) + (() if cols is None else (cols,)) and bool((t == fill).all()), (oname, k)
        a = call._args[o0 + i]
        assert ([a] if single else entries(a)) == [t.data_ptr() for t in call.outs[i]]
    # the single-only outputs are NULL unless asked for
    n_extra = len(EXTRAS[name][1]) if name in EXTRAS else 0
    assert len(solver.extras) == n_extra and len(call._args) == o0 + len(outs) + (n_extra if single else 0) + 2
    if single:
        assert call._args[o0 + len(outs):-2] == (None,) * n_extra and call.extras is None


@pytest.mark.parametrize("single", [False, True], ids=["batch", "single"])
@pytest.mark.parametrize("name", sorted(n for n in FAMILIES if FAMILIES[n][1]))
def test_want_selectors_put_null_where_they_say(name, single, blob):
    solver, outs = FAMILIES[name]
    ms = [5] if single else MS
    for i, (oname, _, fill, _, _) in enumerate(outs):
        call = build(name, ms, blob, single, **{"want_" + oname: False})
        _, o0 = layout(call)
        assert call._args[o0 + i] is None and all(call._args[o0 + j] is not None for j in range(len(outs)) if j != i)
        assert all(bool((t == fill).all()) for t in call.outs[i])                   # (the tensors exist all the same, with their fill)
        for want in ([False] * len(ms), [k % 2 == 0 for k in range(len(ms))]):
            call = build(name, ms, blob, single, **{"want_" + oname: want})
            a = call._args[o0 + i]
            assert ([a] if single else entries(a)) == [t.data_ptr() if ok else None for t, ok in zip(call.outs[i], want)]
    call = build(name, ms, blob, single, outputs=False)
    _, o0 = layout(call)
    assert call.outs == [None] * len(outs) and call._args[o0:o0 + len(outs)] == (None,) * len(outs)


@pytest.mark.parametrize("single", [False, True], ids=["batch", "single"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_omitted_inputs_are_null(name, single, blob):
    ms = [5] if single else MS
    first = 0 if single else 1
    call = build(name, ms, blob, single)
    assert call._args[first + 3] is None                                              # no m_devs at all
    some = [None if k % 2 == 0 else torch.tensor([m], dtype=I32) for k, m in enumerate(ms)]
    call = build(name, ms, blob, single, m_devs=some)
    a = call._args[first + 3]
    assert ([a] if single else entries(a)) == [t if t is None else t.data_ptr() for t in some]
    if name == "dgr":
        call = build(name, ms, blob, single, weights=None, T_inits=None)
        assert call._args[first + 4] is None and call._args[first + 5] is None and call.inputs == [None, None]
        Ts = [None if k % 2 == 0 else np.eye(4) for k in range(len(ms))]
        call = build(name, ms, blob, single, weights=[None] * len(ms), T_inits=Ts)
        w, T = call._args[first + 4], call._args[first + 5]
        assert ([w] if single else entries(w)) == [None] * len(ms)
        assert ([T] if single else entries(T)) == [t if t is None else t.data_ptr() for t in call.inputs[1]]
        assert all(t is None or (t.dtype == F64 and tuple(t.shape) == (16,)) for t in call.inputs[1]) and [t is None for t in call.inputs[1]] == [t is None for t in Ts]


@pytest.mark.parametrize("name", sorted(EXTRAS))
def test_single_only_outputs(name, blob):
    flag, extras = EXTRAS[name]
    call = build(name, [5], blob, True, **{flag: True})
    _, o0 = layout(call)
    tail = call._args[o0 + len(FAMILIES[name][1]):-2]
    assert tail == tuple(t.data_ptr() for t in call.extras) and len(tail) == len(extras)
    for t, (dtype, fill, rows, cols) in zip(call.extras, extras):
        assert t.dtype == dtype and tuple(t.shape) == (max(rows(5), 1),) + (() if cols is None else (cols,))
        assert bool(torch.isnan(t).all() if np.isnan(fill) else (t == fill).all())
    with pytest.raises(AssertionError, match=FAMILIES[name][0].extras_msg):
        build(name, MS, blob, False, **{flag: True})
    build(name, MS, blob, False, **{flag: False})                                       # (not asked for: the batched call is built)
