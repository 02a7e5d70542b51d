"""CPU-side checks of the C-ABI library: it builds for gfx950, loads, and exports every symbol the header declares.
No compute call is made here (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from lidarregistration_amd import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    return _ext.build()


def test_header_symbols_are_exported(libpath):
    hdr = open(os.path.join(ROOT, "include", "lidarreg.h")).read()
    declared = sorted(set(re.findall(r"LR_API\s+[\w\s\*]+?\b(lr_\w+)\s*\(", hdr)))
    assert declared, "no LR_API declarations found"
    assert sorted(_ext.SYMBOLS) == declared
    L = ctypes.CDLL(libpath)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/lidarreg.h but not exported"


def test_version_and_error_string(libpath):
    L = _ext.lib()
    assert L.lr_version() >= 100
    assert isinstance(L.lr_last_error(), bytes)


def test_struct_layouts_match_header():
    # sizes the C side static-asserts implicitly through its field order (include/lidarreg.h); both params structs start with struct_size
    R, P = _ext.RansacParams, _ext.PairParams
    assert ctypes.sizeof(R) == 72 and R.struct_size.offset == 0 and R.sample_size.offset == 4 and R.seed.offset == 24
    assert R.sampler.offset == 40 and R.scoring.offset == 48 and R.local_opt.offset == 52 and R.lo_rounds.offset == 56 and R.min_iters.offset == 68
    assert ctypes.sizeof(_ext.RansacResult) == 40
    assert ctypes.sizeof(_ext.PairResult) == 496
    assert ctypes.sizeof(P) == 112 and P.struct_size.offset == 0 and P.mode.offset == 4 and P.ransac.offset == 16 and P.gpf_factor.offset == 96
    # the Python mirror fills the sizes in (positional arguments start at sample_size, as before)
    r = R(3, 1, 0.36, 50000, 51)
    assert (r.struct_size, r.sample_size, r.use_elc, r.iters, r.seed) == (72, 3, 1, 50000, 51)
    p = P()
    assert p.struct_size == 112 and p.ransac.struct_size == 72
    p.ransac = r
    assert p.ransac.struct_size == 72 and p.ransac.iters == 50000


def test_params_from_another_header_version_are_rejected():
    """A caller built against lr_version 101 (no struct_size: the struct started with sample_size = 3 or 4; 64 / 96 bytes) is turned
    away before anything is read past the end of its shorter struct.  Checked before any HIP call: safe without a device."""
    L = _ext.lib()
    assert L.lr_version() == 103
    r = _ext.RansacParams(3, 1, 0.36, 1000, 51)
    r.struct_size = 3                                   # what an old caller's first field would hold
    one = ctypes.c_void_p(1)                            # non-null dummies: the size check comes before any dereference of them
    assert L.lr_ransac(one, one, one, 10, None, ctypes.byref(r), one, one, None) == -1
    assert b"struct_size" in L.lr_last_error() and b"lr_version 103" in L.lr_last_error()
    p = _ext.PairParams()
    p.mode = 1
    p.struct_size = 96
    pp = (ctypes.c_void_p * 1)(1)
    ip = (ctypes.c_int32 * 1)(10)
    assert L.lr_register_batch(one, 1, pp, pp, pp, pp, ip, ip, 32, ctypes.byref(p), one, None) == -1 and b"lr_pair_params.struct_size is 96" in L.lr_last_error()
    assert L.lr_register_pair(one, one, one, one, one, 10, 10, 32, ctypes.byref(p), one, None) == -1 and b"struct_size" in L.lr_last_error()


def test_bad_arguments_are_reported_not_crashed(libpath):
    L = _ext.lib()
    h = ctypes.c_void_p()
    # argument validation happens before any HIP call, so this is safe without a device
    assert L.lr_workspace_create(ctypes.byref(h), 0, 10, 32, 10) == -1
    assert b"positive" in L.lr_last_error()
    assert L.lr_workspace_create(ctypes.byref(h), 10, 10, 33, 10) == -1 and b"1 to 32" in L.lr_last_error()      # wider than FCGF's 32: refused
    assert L.lr_workspace_create(ctypes.byref(h), 10, 10, 0, 10) == -1
    assert L.lr_feat_ratio(None, None, 32, 4, None, None, None, None, None) == -1


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "lidarregistration_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f"{f} imports the oracle"
                assert "liboracle" not in text, f"{f} references the oracle library"


def test_mode_aliases_and_defaults():
    from lidarregistration_amd import FR as fr
    from tests.conftest import Args
    p = fr.pair_params(Args(mode="MMN", codebase="GC", iters=None))
    assert p.mode == _ext.LR_MODE_MNN and p.ransac.iters == 500000 and p.ransac.sample_size == 3 and p.ransac.use_elc == 1
    assert abs(p.ransac.confidence - 0.999) < 1e-6 and p.refit == 0 and p.ransac.local_opt == 1     # GC: LO + final LSQ inside the RANSAC call
    p = fr.pair_params(Args(mode="GPF", codebase="open3D", iters=1000, GPF_factor=0.5, GPF_grid_wid=4))
    assert p.mode == _ext.LR_MODE_GPF and p.ransac.sample_size == 4 and p.gpf_factor == 0.5 and p.gpf_grid_wid == 4 and p.refit == 1
    assert abs(p.refit_thr2 - 0.36) < 1e-15 and abs(p.ransac.thr2 - 0.36) < 1e-7
    with pytest.raises(AssertionError):
        fr.pair_params(Args(mode="bogus"))


def test_pair_params_follow_the_reference_flags():
    """args namespace (Experiments/test.py:294-313) -> lr_pair_params, no device needed."""
    from lidarregistration_amd import FR
    from tests.conftest import Args
    p = FR.pair_params(Args(mode="GPF", codebase="GC", iters=None, prosac=True, GPF_factor=1.5, GPF_grid_wid=12))
    assert (p.mode, p.refit, p.gpf_grid_wid, p.gpf_factor) == (_ext.LR_MODE_GPF, 0, 12, 1.5)
    r = p.ransac
    assert (r.sample_size, r.use_elc, r.iters, r.sampler, r.scoring, r.local_opt) == (3, 1, 500000, 1, 2, 1)       # FR.py:65-67, GC_RANSAC.py:19-37
    assert (r.lo_rounds, r.lo_trials, r.lo_max_calls, r.min_iters) == (0, 0, 0, 0) and abs(r.effective_thr2() - 0.81) < 1e-6   # library defaults; (3/2 * 0.6)^2
    assert abs(r.confidence - 0.999) < 1e-7 and abs(r.thr2 - 0.36) < 1e-7
    p = FR.pair_params(Args(mode="MMN", codebase="GC", iters=1000, prosac=False, fast_rejection="NONE", GC_conf=0.9))
    assert (p.mode, p.ransac.sampler, p.ransac.use_elc, p.ransac.iters) == (_ext.LR_MODE_MNN, 2, 0, 1000)     # uniform, unique indices
    assert abs(p.ransac.confidence - 0.9) < 1e-7
    # --GC_LO False: only the final least squares (GC_RANSAC.py:36-37); flags the HIP path does not implement are refused
    assert FR.pair_params(Args(codebase="GC", GC_LO=False)).ransac.local_opt == 2
    # ... but gcransac_python.cpp:518-521,553-556 honour that switch only in the branches with a pre-verification (:571-591 do not)
    assert FR.pair_params(Args(codebase="GC", GC_LO=False, fast_rejection="NONE")).ransac.local_opt == 1
    assert FR.pair_params(Args(codebase="GC", lo_trials=5, lo_max_calls=3, min_iters=100)).ransac.lo_trials == 5
    import pytest
    assert FR.pair_params(Args(codebase="GC", fast_rejection="SPRT")).ransac.use_elc == 2
    with pytest.raises(NotImplementedError):
        FR.pair_params(Args(codebase="GC", spatial_coherence_weight=0.1))
    FR.pair_params(Args(codebase="open3D", fast_rejection="SPRT", spatial_coherence_weight=0.1))      # GC-only flags: ignored, as in FR.py:70-97
    with pytest.raises(AssertionError):
        FR.pair_params(Args(codebase="GC", fast_rejection="bogus"))
    p = FR.pair_params(Args(mode="no_filter", codebase="open3D", iters=2000))
    r = p.ransac
    assert (p.mode, p.refit, r.sample_size, r.use_elc, r.sampler, r.scoring) == (_ext.LR_MODE_NO_FILTER, 1, 4, 1, 0, 0)   # FR.py:128-137
    assert abs(r.confidence - 0.9995) < 1e-7 and r.local_opt == 0
    with pytest.raises(AssertionError):
        FR.pair_params(Args(mode="bogus"))
    with pytest.raises(AssertionError):
        FR.pair_params(Args(codebase="other"))


def test_no_ablation_switches_in_the_shipped_kernels():
    """The library's .hip files carry no development variants: the ablation switches of rounds 3-5 (LR_PB_EXP bits, geometric
    schedule, per-wave rounds, ...) are rebuilt from history by tools/pb_variant.sh; the NN files (lr_nn16*.hip, lr_nn16_dev.h) keep ONE
    switch between them, the statistics probe of the filter pass."""
    csrc = os.path.join(ROOT, "lidarregistration_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, f)).read()
            for word in ("LR_PB_EXP", "LR_PB_GEO", "LR_PB_JOINT", "LR_PB_P1FOLD", "LR_PB_PRIO"):
                assert word not in text, f"{f} still carries the development switch {word}"
    nn_files = sorted(f for f in os.listdir(csrc) if (f.startswith("lr_nn16") and f.endswith(".hip")) or f == "lr_nn16_dev.h")
    assert {"lr_nn16.hip", "lr_nn16_pass.hip", "lr_nn16_exact.hip", "lr_nn16_rev.hip", "lr_nn16_dev.h"} <= set(nn_files), nn_files
    nn = "\n".join(open(os.path.join(csrc, f)).read() for f in nn_files)
    conds = re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b.*$", nn, flags=re.M)
    assert len(conds) <= 6, conds
    assert any("LR_PB_PROBE" in c for c in conds)


def test_the_scoring_contract_has_one_text():
    """The fp32 scoring arithmetic lives in lr_contract.h alone: the 2^20 fixed-point scale is spelled out only there, and neither side keeps a
    winner ordering of its own (the oracle's model_better, the kernels' better) next to lr_score_better."""
    csrc = os.path.join(ROOT, "lidarregistration_amd", "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))] + [os.path.join(ROOT, "oracle", "oracle.c")]
    assert len(files) >= 10
    for path in files:
        text, name = open(path).read(), os.path.basename(path)
        assert ("1048576" in text) == (name == "lr_contract.h"), f"{name}: the fixed-point scale belongs to lr_contract.h (LR_SCORE_SCALE) alone"
        assert "model_better" not in text, f"{name} still carries model_better"
        assert not re.search(r"__device__[^;{}()]*\bbetter\s*\(", text), f"{name} still defines a device-side better()"


# lr_teaser_scratch_bytes / lr_sm_scratch_bytes at m = 0, 1, 63, 64, 65, 257, 4097, 32768, as the library returned them BEFORE the two back
# ends got a shared front end (csrc/lr_corrset.h): constants read from that build, so that a moved align helper cannot shift an arena
SCRATCH_M = (0, 1, 63, 64, 65, 257, 4097, 32768)
SCRATCH_BYTES = {"lr_teaser_scratch_bytes": (12032, 12032, 12032, 12032, 26368, 87808, 7124736, 407650560),
                 "lr_sm_scratch_bytes": (3328, 3328, 3328, 3328, 6912, 20736, 1231872, 2490624)}


@pytest.mark.parametrize("fn", sorted(SCRATCH_BYTES))
def test_corrset_scratch_sizes_unchanged(libpath, fn):
    f = getattr(_ext.lib(), fn)
    assert tuple(f(m) for m in SCRATCH_M) == SCRATCH_BYTES[fn]


# lr_voxel_dedup_scratch_bytes(n), lr_voxel_mean_scratch_bytes(n), lr_overlap_scratch_bytes(n, n) around the block size, the table's
# doublings and the largest cloud, as the library returned them BEFORE the voxel and overlap kernels got a shared cell table and shared
# primitives (csrc/lr_cells.h, csrc/lr_prims.h): constants read from that build, so that the one capacity rule cannot shift an arena
CELLS_N = (0, 1, 255, 256, 257, 511, 512, 513, 4097, 30000, 4194304)
CELLS_BYTES = {"lr_voxel_dedup_scratch_bytes": (13580, 13580, 14596, 14604, 14864, 15880, 15888, 28436, 218444, 938140, 121701384),
               "lr_voxel_mean_scratch_bytes": (24320, 24320, 40704, 40704, 43776, 60160, 60160, 83712, 642816, 3593216, 486605568),
               "lr_overlap_scratch_bytes": (56576, 56576, 95232, 95232, 101632, 140288, 140288, 187648, 1449216, 8168192, 1107428352)}


@pytest.mark.parametrize("fn", sorted(CELLS_BYTES))
def test_cell_table_scratch_sizes_unchanged(libpath, fn):
    f = getattr(_ext.lib(), fn)
    call = (lambda n: f(n, n)) if fn == "lr_overlap_scratch_bytes" else f
    assert tuple(call(n) for n in CELLS_N) == CELLS_BYTES[fn]
    if fn != "lr_voxel_dedup_scratch_bytes":
        assert call(4194305) == 0                       # one point more than a cloud may have: refused


# lr_nn3_scratch_bytes(n, n), lr_refine_z_scratch_bytes(n, n), lr_bbrf_scratch_bytes(n, n, 100), lr_normals_scratch_bytes(n) and
# lr_balanced_select_scratch_bytes(n) around the block size, the run length, past 65 536 points and at the largest cloud, as the library
# returned them BEFORE the cloud-level entry points got one scratch front end (csrc/lr_scratch.h): constants read from that build, so
# that the one align helper cannot shift an arena
CLOUD_N = (0, 1, 255, 256, 257, 4097, 30000, 65537, 4194304)
CLOUD_BYTES = {"lr_nn3_scratch_bytes": (17920, 17920, 25344, 25344, 26112, 198400, 1441280, 3148544, 201392896),
               "lr_refine_z_scratch_bytes": (27392, 27392, 45056, 45056, 46848, 388096, 2770432, 6042624, 386016256),
               "lr_bbrf_scratch_bytes": (38144, 38144, 66304, 66304, 68864, 628736, 4566016, 9973504, 637930240),
               "lr_normals_scratch_bytes": (17920, 17920, 25344, 25344, 26112, 198400, 1441280, 3148544, 201392896),
               "lr_balanced_select_scratch_bytes": (33792, 35328, 46080, 46080, 47616, 231936, 1474560, 3181056, 201360384)}
CLOUD_ARGS = {"lr_nn3_scratch_bytes": lambda n: (n, n), "lr_refine_z_scratch_bytes": lambda n: (n, n), "lr_bbrf_scratch_bytes": lambda n: (n, n, 100)}


@pytest.mark.parametrize("fn", sorted(CLOUD_BYTES))
def test_cloud_level_scratch_sizes_unchanged(libpath, fn):
    f, args = getattr(_ext.lib(), fn), CLOUD_ARGS.get(fn, lambda n: (n,))
    assert tuple(f(*args(n)) for n in CLOUD_N) == CLOUD_BYTES[fn]
    assert f(*args(4194305)) == 0                       # one point more than a cloud may have: refused
