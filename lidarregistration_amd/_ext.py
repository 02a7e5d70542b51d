"""ctypes binding of liblidarreg.so (the C ABI in include/lidarreg.h).

There is no fallback: if the library is missing or a call fails, an exception is raised.  PyTorch
is only used by the callers for device memory and streams; no torch type crosses this boundary.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("LIDARREG_LIB") or os.path.join(CSRC, "liblidarreg.so")      # LIDARREG_LIB: development hook (alternate builds)

LR_MODE_NO_FILTER, LR_MODE_MNN, LR_MODE_GPF = 0, 1, 2

SYMBOLS = [
    "lr_version", "lr_last_error", "lr_workspace_create", "lr_workspace_destroy", "lr_workspace_bytes", "lr_workspace_poison",
    "lr_nn_top2", "lr_nn_to_mutual", "lr_feat_ratio", "lr_gpf", "lr_gpf_bb_first", "lr_ransac", "lr_refit", "lr_icp", "lr_kabsch",
    "lr_register_pair", "lr_workspace_lists", "lr_workspace_timing", "lr_workspace_timing_read",
    "lr_workspace_create_batch", "lr_register_batch", "lr_workspace_lists_at", "lr_inlier_mask", "lr_workspace_mask_at",
    "lr_voxel_dedup_scratch_bytes", "lr_voxel_dedup", "lr_workspace_option", "lr_workspace_stage_times", "lr_icp_batch", "lr_workspace_lists_batch",
    "lr_workspace_clock", "lr_debug_fake_current_device",
    "lr_teaser_scratch_bytes", "lr_teaser", "lr_teaser_batch", "lr_teaser_timing", "lr_teaser_stage_times",
    "lr_sm_scratch_bytes", "lr_sm", "lr_sm_batch",
    "lr_voxel_mean_scratch_bytes", "lr_voxel_mean", "lr_overlap_scratch_bytes", "lr_overlap", "lr_overlap_batch",
    "lr_nn3_scratch_bytes", "lr_nn3", "lr_refine_z_scratch_bytes", "lr_refine_z",
    "lr_bbrf_scratch_bytes", "lr_bbrf", "lr_normals_scratch_bytes", "lr_normals", "lr_normals2", "lr_symicp_scratch_bytes", "lr_symicp",
    "lr_balanced_select_scratch_bytes", "lr_balanced_select",
    "lr_pdsc_weights_bytes", "lr_pdsc_scratch_bytes", "lr_pdsc_encode", "lr_pdsc_encode_batch",
    "lr_pdsc_solve_scratch_bytes", "lr_pdsc_solve", "lr_pdsc_solve_batch",
    "lr_pdsc_register_scratch_bytes", "lr_pdsc_register", "lr_pdsc_register_batch",
    "lr_fcgf_weights_bytes", "lr_fcgf_scratch_bytes", "lr_fcgf_extract", "lr_fcgf_batch_scratch_bytes", "lr_fcgf_extract_batch", "lr_debug_fcgf_batch_stop_after",
    "lr_dgr_scratch_bytes", "lr_dgr_refine", "lr_dgr_refine_batch",
    "lr_dgr_inlier_weights_bytes", "lr_dgr_inlier_scratch_bytes", "lr_dgr_inlier",
    "lr_dgr_inlier_batch_scratch_bytes", "lr_dgr_inlier_batch",
    "lr_nn_wide_scratch_bytes", "lr_nn_wide", "lr_fpfh_scratch_bytes", "lr_fpfh", "lr_workspace_create_wide", "lr_debug_workspace_rev",
]

# lr_workspace_option ids (include/lidarreg.h).  DEFAULT_OPTIONS is applied to every Workspace this module creates (a hook for
# tuning experiments and for the test that no option changes a result; the library itself reads no environment variable).
OPTIONS = {"nn_blocks": 1, "nn_blocks_batch": 2, "nn_sample_stride": 3, "rev_strips": 4, "nn_second_auto": 5, "clock_probe": 6}
DEFAULT_OPTIONS = {}


class LidarRegError(RuntimeError):
    pass


class RansacParams(ctypes.Structure):
    """lr_ransac_params.  Positional arguments start at sample_size: struct_size (the first field of the C struct) is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("sample_size", ctypes.c_int32), ("use_elc", ctypes.c_int32), ("thr2", ctypes.c_float),
                ("iters", ctypes.c_int32), ("seed", ctypes.c_uint64), ("confidence", ctypes.c_float), ("batch", ctypes.c_int32),
                ("sampler", ctypes.c_int32), ("prosac_growth", ctypes.c_int32), ("scoring", ctypes.c_int32), ("local_opt", ctypes.c_int32),
                ("lo_rounds", ctypes.c_int32), ("lo_trials", ctypes.c_int32), ("lo_max_calls", ctypes.c_int32), ("min_iters", ctypes.c_int32)]

    def __init__(self, *args, **kw):
        kw.pop("struct_size", None)          # (always this build's size: an explicit keyword used to end in ctypes' opaque "duplicate values" TypeError)
        super().__init__(ctypes.sizeof(type(self)), *args, **kw)

    def effective_thr2(self):
        """The squared threshold the estimator really tests inliers against: scoring 2 (MSAC as GC-RANSAC runs it) uses the
        truncated threshold (3/2 thr)^2 -- what lr_inlier_mask has to be given to reproduce the estimator's own inlier set."""
        return float(self.thr2) * 2.25 if self.scoring == 2 else float(self.thr2)


class RansacResult(ctypes.Structure):
    _fields_ = [("best_h", ctypes.c_int64), ("best_count", ctypes.c_uint32), ("pad0", ctypes.c_uint32),
                ("best_ssq", ctypes.c_uint64), ("n_valid", ctypes.c_int64), ("n_ids", ctypes.c_int64)]


class IcpResult(ctypes.Structure):
    _fields_ = [("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double), ("n_corr", ctypes.c_int32),
                ("iterations", ctypes.c_int32)]


class PairResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("T_ransac", ctypes.c_double * 16), ("ransac", RansacResult),
                ("n_corr", ctypes.c_int32), ("n_refit", ctypes.c_int32), ("n_nn_fixed", ctypes.c_int32),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32 * 8), ("T_icp", ctypes.c_double * 16), ("icp", IcpResult)]


class PairParams(ctypes.Structure):
    """lr_pair_params.  struct_size (here and in the nested lr_ransac_params) is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("mode", ctypes.c_int32), ("refit", ctypes.c_int32), ("ransac", RansacParams),
                ("gpf_grid_wid", ctypes.c_int32), ("icp", ctypes.c_int32), ("gpf_factor", ctypes.c_double),
                ("refit_thr2", ctypes.c_double)]

    def __init__(self, *args, **kw):
        kw.pop("struct_size", None)
        super().__init__(ctypes.sizeof(type(self)), *args, **kw)
        if self.ransac.struct_size == 0:
            self.ransac.struct_size = ctypes.sizeof(RansacParams)


class KeywordParams(ctypes.Structure):
    """A params struct filled by keyword over its DEFAULTS; struct_size (always this build's size: a passed one is dropped) is filled in."""
    DEFAULTS = {}

    def __init__(self, **kw):
        kw.pop("struct_size", None)
        super().__init__(struct_size=ctypes.sizeof(type(self)), **{**self.DEFAULTS, **kw})


class TeaserParams(KeywordParams):
    """lr_teaser_params with the reference's settings (TEASER_plus_plus.py:78-93) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_iterations", ctypes.c_int32), ("noise_bound", ctypes.c_double),
                ("cbar2", ctypes.c_double), ("kcore_threshold", ctypes.c_double), ("gnc_factor", ctypes.c_double),
                ("cost_threshold", ctypes.c_double), ("node_budget", ctypes.c_int64), ("time_budget_ms", ctypes.c_double),
                ("rotation_tim_graph", ctypes.c_int32), ("estimate_scaling", ctypes.c_int32)]
    DEFAULTS = dict(max_iterations=10000, noise_bound=0.3, cbar2=1.0, kcore_threshold=0.5, gnc_factor=1.4, cost_threshold=1e-16,
                    node_budget=10 ** 7, time_budget_ms=10000.0)


class TeaserResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("status", ctypes.c_int32), ("K", ctypes.c_int32), ("exact", ctypes.c_int32),
                ("max_core", ctypes.c_int32), ("lb", ctypes.c_int32), ("pad0", ctypes.c_int32), ("nodes", ctypes.c_uint64),
                ("gnc_iters", ctypes.c_int32), ("n_rot_inliers", ctypes.c_int32), ("n_trans_inliers", ctypes.c_int32),
                ("pad1", ctypes.c_int32)]


class SmParams(KeywordParams):
    """lr_sm_params with the settings the reference runs SM() with (baseline_KITTI.py:51-52) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("iterations", ctypes.c_int32), ("inlier_threshold", ctypes.c_double),
                ("top_ratio", ctypes.c_double)]
    DEFAULTS = dict(iterations=10, inlier_threshold=0.6, top_ratio=0.05)


class SmResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("status", ctypes.c_int32), ("K", ctypes.c_int32), ("m", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("weight_sum", ctypes.c_double)]


class OverlapParams(KeywordParams):
    """lr_overlap_params with the reference's settings (GenerateBalancedSet.py:171,175) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("voxel_size", ctypes.c_double), ("radius", ctypes.c_double)]
    DEFAULTS = dict(voxel_size=1.0, radius=0.0)


class OverlapResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("n0_ds", ctypes.c_int32), ("n1_ds", ctypes.c_int32), ("n_overlap", ctypes.c_int32),
                ("n0_dropped", ctypes.c_int32), ("n1_dropped", ctypes.c_int32), ("frac", ctypes.c_double), ("frac_sym", ctypes.c_double)]


class Nn3Params(KeywordParams):
    """lr_nn3_params; cell 0 = automatic (the result does not depend on it); struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("cell", ctypes.c_double)]


class RefineZParams(KeywordParams):
    """lr_refine_z_params with the reference's settings (GenerateBalancedSet.py:264-265, voxel 0.3 at :298) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_repeats", ctypes.c_int32), ("xy_gate", ctypes.c_double), ("min_change", ctypes.c_double),
                ("cell", ctypes.c_double)]
    DEFAULTS = dict(max_repeats=10, xy_gate=0.3, min_change=1e-6, cell=0.0)


class RefineZResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("repeats", ctypes.c_int32), ("n_valid", ctypes.c_int32), ("n0_dropped", ctypes.c_int32),
                ("n1_dropped", ctypes.c_int32), ("reserved", ctypes.c_int32), ("dz", ctypes.c_double), ("last_step", ctypes.c_double)]


class BbrfParams(KeywordParams):
    """lr_bbrf_params with the reference's settings (BBR_F.py:271-275, torch.optim.Adam's defaults) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_iter", ctypes.c_int32), ("angles_lr", ctypes.c_double), ("trans_lr", ctypes.c_double),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("cell", ctypes.c_double)]
    DEFAULTS = dict(n_iter=100, angles_lr=2e-4, trans_lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, cell=0.0)


class BbrfResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("B_to_A", ctypes.c_double * 16), ("status", ctypes.c_int32), ("best_iter", ctypes.c_int32),
                ("best_loss", ctypes.c_double), ("n_pairs_best", ctypes.c_int32), ("iters_run", ctypes.c_int32)]


class SymicpParams(KeywordParams):
    """lr_symicp_params; max_dist is two of the refinement tester's voxels, the rest as chosen in DESIGN.md §23; struct_size is filled in.
    T_init: the address of a device float64 4x4, or None."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_iter", ctypes.c_int32), ("max_dist", ctypes.c_double), ("min_cos", ctypes.c_double),
                ("eps_rot", ctypes.c_double), ("eps_trans", ctypes.c_double), ("piv_eps", ctypes.c_double), ("cell", ctypes.c_double),
                ("T_init", ctypes.c_void_p)]
    DEFAULTS = dict(n_iter=30, max_dist=0.6, min_cos=0.7, eps_rot=1e-5, eps_trans=1e-4, piv_eps=1e-9, cell=0.0, T_init=None)


class SymicpResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("B_to_A", ctypes.c_double * 16), ("status", ctypes.c_int32), ("iters_run", ctypes.c_int32),
                ("converged", ctypes.c_int32), ("n_pairs", ctypes.c_int32), ("mean_sq", ctypes.c_double)]


class SelectParams(KeywordParams):
    """lr_select_params with the reference's threshold (GenerateBalancedSet.py:474) as default; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_request", ctypes.c_int32), ("thresh", ctypes.c_double), ("resume", ctypes.c_int32),
                ("max_rounds", ctypes.c_int32)]
    DEFAULTS = dict(n_request=0, thresh=0.1, resume=0, max_rounds=0)


class SelectResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("n_selected", ctypes.c_int32), ("attempts", ctypes.c_int64), ("misses", ctypes.c_int64),
                ("consumed", ctypes.c_int64), ("rounds", ctypes.c_int32), ("rescales", ctypes.c_int32), ("lo", ctypes.c_double * 6),
                ("hi", ctypes.c_double * 6)]


class PdscParams(KeywordParams):
    """lr_pdsc_params with the settings of the reference's CLI (config.py:34, sigma_spat for Lidar) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_layers", ctypes.c_int32), ("sigma_d", ctypes.c_double)]
    DEFAULTS = dict(num_layers=12, sigma_d=1.2)


class PdscResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("m", ctypes.c_int32), ("dead", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PdscSolveParams(KeywordParams):
    """lr_pdsc_solve_params with the reference's Lidar settings (config.py, test.py:338-339, PointDSC.py:415-418) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_iterations", ctypes.c_int32), ("k", ctypes.c_int32), ("refine_iters", ctypes.c_int32),
                ("ratio", ctypes.c_double), ("nms_radius", ctypes.c_double), ("inlier_threshold", ctypes.c_double),
                ("refine_threshold", ctypes.c_double), ("sigma_d", ctypes.c_double), ("sigma", ctypes.c_double)]
    DEFAULTS = dict(num_iterations=10, k=40, refine_iters=20, ratio=0.1, nms_radius=0.6, inlier_threshold=0.6, refine_threshold=1.2,
                    sigma_d=1.2, sigma=1.0)


class PdscSolveResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("T_best", ctypes.c_double * 16), ("status", ctypes.c_int32), ("m", ctypes.c_int32),
                ("dead", ctypes.c_int32), ("n_seeds", ctypes.c_int32), ("best_rank", ctypes.c_int32), ("best_index", ctypes.c_int32),
                ("best_count", ctypes.c_int32), ("n_labels", ctypes.c_int32), ("refine_rounds", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class FcgfParams(KeywordParams):
    """lr_fcgf_params with the reference's network (LidarFeatureExtractor.py:71-76) as default; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("conv1_kernel_size", ctypes.c_int32), ("tap", ctypes.c_int32)]
    DEFAULTS = dict(conv1_kernel_size=5, tap=0)


class FcgfResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("n", ctypes.c_int32), ("n_tap", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DgrParams(KeywordParams):
    """lr_dgr_params with GlobalRegistration's defaults (DGR/core/registration.py:135-144, :163-164) as defaults; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_iter", ctypes.c_int32), ("max_break", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("quantization_size", ctypes.c_double), ("lr", ctypes.c_double), ("gamma", ctypes.c_double), ("ratio", ctypes.c_double),
                ("clip", ctypes.c_double), ("wsum_threshold", ctypes.c_double)]
    DEFAULTS = dict(max_iter=1000, max_break=20, quantization_size=1.0, lr=0.1, gamma=0.999, ratio=1e-5, clip=0.0, wsum_threshold=0.0)


class DgrResult(ctypes.Structure):
    _fields_ = [("T", ctypes.c_double * 16), ("loss", ctypes.c_double), ("w1", ctypes.c_double), ("iterations", ctypes.c_int32),
                ("break_count", ctypes.c_int32), ("L", ctypes.c_int32), ("status", ctypes.c_int32)]


class DgrInlierParams(KeywordParams):
    """lr_dgr_inlier_params with ResUNetBN2C's widths (DGR/model/resunet.py:662-665) as default; struct_size is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("tap", ctypes.c_int32), ("widths", ctypes.c_int32 * 8)]
    DEFAULTS = dict(tap=0, widths=(32, 64, 128, 256, 128, 64, 64, 64))

    def __init__(self, **kw):
        if "widths" in kw:
            kw["widths"] = (ctypes.c_int32 * 8)(*[int(w) for w in kw["widths"]])
        else:
            kw["widths"] = (ctypes.c_int32 * 8)(*self.DEFAULTS["widths"])
        super().__init__(**kw)


class DgrInlierResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("n", ctypes.c_int32), ("n_tap", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(DgrInlierParams) == 40 and ctypes.sizeof(DgrInlierResult) == 16
assert ctypes.sizeof(DgrParams) == 64 and ctypes.sizeof(DgrResult) == 160
assert ctypes.sizeof(FcgfParams) == 12 and ctypes.sizeof(FcgfResult) == 16
assert ctypes.sizeof(PdscSolveParams) == 64 and ctypes.sizeof(PdscSolveResult) == 304
assert ctypes.sizeof(PdscParams) == 16 and ctypes.sizeof(PdscResult) == 16
assert ctypes.sizeof(SelectParams) == 24 and ctypes.sizeof(SelectResult) == 136
assert ctypes.sizeof(BbrfParams) == 56 and ctypes.sizeof(BbrfResult) == 280
assert ctypes.sizeof(SymicpParams) == 64 and ctypes.sizeof(SymicpResult) == 280
assert ctypes.sizeof(Nn3Params) == 16 and ctypes.sizeof(RefineZParams) == 32 and ctypes.sizeof(RefineZResult) == 40
assert ctypes.sizeof(OverlapParams) == 24 and ctypes.sizeof(OverlapResult) == 40
assert ctypes.sizeof(TeaserParams) == 72 and ctypes.sizeof(TeaserResult) == 176
assert ctypes.sizeof(SmParams) == 24 and ctypes.sizeof(SmResult) == 152
assert ctypes.sizeof(PairResult) == 496 and ctypes.sizeof(RansacParams) == 72 and ctypes.sizeof(PairParams) == 112

_lib = None


def build(force=False):
    """hipcc --offload-arch=gfx950 -> csrc/liblidarreg.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "lidarreg.h"))
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4", "liblidarreg.so"])
    return LIB_PATH


def lib():
    """Load the HIP library; raises LidarRegError when it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LidarRegError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # torch ships its own libamdhip64; it must be in the process before this library is, so that both use the same
        # HIP runtime (loaded the other way round, the library binds to a second runtime that sees no device)
        import torch  # noqa: F401
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise LidarRegError(f"cannot load {LIB_PATH}: {e}") from e
        L.lr_last_error.restype = ctypes.c_char_p
        L.lr_workspace_bytes.restype = ctypes.c_size_t
        for name in SYMBOLS:
            if name.endswith("_scratch_bytes"):
                getattr(L, name).restype = ctypes.c_size_t
        L.lr_workspace_bytes.argtypes = [ctypes.c_void_p]
        L.lr_workspace_poison.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.lr_workspace_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.lr_workspace_destroy.argtypes = [ctypes.c_void_p]
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.lr_nn_top2.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]
        L.lr_nn_to_mutual.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lr_feat_ratio.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.lr_gpf.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, vp, vp]
        L.lr_gpf_bb_first.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp, ci, ctypes.c_double, vp, vp, vp, vp, vp, vp, vp]
        L.lr_ransac.argtypes = [vp, vp, vp, ci, vp, ctypes.POINTER(RansacParams), vp, vp, vp]
        L.lr_refit.argtypes = [vp, vp, ci, vp, vp, vp, ctypes.c_double, vp, vp, vp]
        L.lr_icp.argtypes = [vp, vp, ci, vp, ci, vp, ctypes.c_double, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp]
        L.lr_kabsch.argtypes = [vp, vp, vp, ci, vp, vp]
        L.lr_icp_batch.argtypes = [vp, ctypes.c_double, ci, ctypes.c_double, ctypes.c_double, vp, vp]
        L.lr_register_pair.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(PairParams), vp, vp]
        L.lr_workspace_lists.argtypes = [vp, ci, vp, vp, vp, vp, vp]
        L.lr_workspace_lists_at.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
        L.lr_workspace_lists_batch.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
        L.lr_inlier_mask.argtypes = [vp, vp, vp, ci, vp, ctypes.c_float, vp, vp, vp]
        L.lr_workspace_mask_at.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, vp]
        L.lr_voxel_dedup_scratch_bytes.argtypes = [ci]
        L.lr_voxel_dedup.argtypes = [vp, ci, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_workspace_create_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ci, ci, ci, ci, ci]
        L.lr_workspace_create_wide.argtypes = [ctypes.POINTER(ctypes.c_void_p), ci, ci, ci, ci, ci]
        L.lr_debug_workspace_rev.argtypes = [vp, ci, ci, vp, vp]
        pp, ip = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32)
        L.lr_register_batch.argtypes = [vp, ci, pp, pp, pp, pp, ip, ip, ci, ctypes.POINTER(PairParams), vp, vp]
        L.lr_workspace_option.argtypes = [vp, ci, ci]
        L.lr_workspace_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float * 8), ctypes.POINTER(ci)]
        L.lr_workspace_timing.argtypes = [vp, ci]
        if hasattr(L, "lr_workspace_clock"):      # (absent only from older builds loaded through the LIDARREG_LIB development hook)
            L.lr_workspace_clock.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong), ci]
        L.lr_teaser_scratch_bytes.argtypes = [ci]
        L.lr_teaser.argtypes = [vp, vp, ci, vp, ctypes.POINTER(TeaserParams), vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_teaser_batch.argtypes = [ci, pp, pp, ip, pp, ctypes.POINTER(TeaserParams), vp, pp, vp, ctypes.c_size_t, vp]
        L.lr_teaser_timing.argtypes = [ci]
        L.lr_teaser_stage_times.argtypes = [ctypes.POINTER(ctypes.c_float * 4)]
        L.lr_sm_scratch_bytes.argtypes = [ci]
        L.lr_sm.argtypes = [vp, vp, ci, vp, ctypes.POINTER(SmParams), vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_sm_batch.argtypes = [ci, pp, pp, ip, pp, ctypes.POINTER(SmParams), vp, pp, pp, vp, ctypes.c_size_t, vp]
        dp = ctypes.c_double
        L.lr_voxel_mean_scratch_bytes.argtypes = [ci]
        L.lr_voxel_mean.argtypes = [vp, ci, vp, dp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_overlap_scratch_bytes.argtypes = [ci, ci]
        L.lr_overlap.argtypes = [vp, ci, vp, ci, vp, ctypes.POINTER(OverlapParams), vp, vp, ctypes.c_size_t, vp]
        L.lr_overlap_batch.argtypes = [ci, pp, ip, pp, ip, pp, ctypes.POINTER(OverlapParams), vp, vp, ctypes.c_size_t, vp]
        L.lr_nn3_scratch_bytes.argtypes = [ci, ci]
        L.lr_nn3.argtypes = [vp, ci, vp, ci, ctypes.POINTER(Nn3Params), vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_refine_z_scratch_bytes.argtypes = [ci, ci]
        L.lr_refine_z.argtypes = [vp, ci, vp, ci, vp, ctypes.POINTER(RefineZParams), vp, vp, ctypes.c_size_t, vp]
        L.lr_bbrf_scratch_bytes.argtypes = [ci, ci, ci]
        L.lr_bbrf.argtypes = [vp, vp, ci, vp, vp, ci, ctypes.POINTER(BbrfParams), vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_normals_scratch_bytes.argtypes = [ci]
        L.lr_normals.argtypes = [vp, ci, dp, ci, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_normals2.argtypes = [vp, ci, dp, ci, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_symicp_scratch_bytes.argtypes = [ci, ci]
        L.lr_symicp.argtypes = [vp, vp, ci, vp, vp, ci, ctypes.POINTER(SymicpParams), vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_balanced_select_scratch_bytes.argtypes = [ci]
        L.lr_balanced_select.argtypes = [vp, vp, vp, ci, ci, vp, ctypes.c_longlong, ctypes.POINTER(SelectParams), vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_pdsc_weights_bytes.restype = ctypes.c_size_t
        L.lr_pdsc_weights_bytes.argtypes = [ci]
        L.lr_pdsc_scratch_bytes.argtypes = [ci]
        L.lr_pdsc_encode.argtypes = [vp, vp, ci, vp, vp, ctypes.c_size_t, ctypes.POINTER(PdscParams), vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lr_pdsc_encode_batch.argtypes = [ci, pp, pp, ip, pp, vp, ctypes.c_size_t, ctypes.POINTER(PdscParams), vp, pp, pp, vp, ctypes.c_size_t, vp]
        sz, ps = ctypes.c_size_t, ctypes.POINTER(PdscSolveParams)
        L.lr_pdsc_solve_scratch_bytes.argtypes = [ci]
        L.lr_pdsc_register_scratch_bytes.argtypes = [ci]
        L.lr_pdsc_solve.argtypes = [vp, vp, ci, vp, vp, vp, ps, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        L.lr_pdsc_solve_batch.argtypes = [ci, pp, pp, ip, pp, pp, pp, ps, vp, pp, pp, vp, sz, vp]
        L.lr_pdsc_register.argtypes = [vp, vp, ci, vp, vp, sz, ctypes.POINTER(PdscParams), ps, vp, vp, vp, vp, vp, vp, sz, vp]
        L.lr_pdsc_register_batch.argtypes = [ci, pp, pp, ip, pp, vp, sz, ctypes.POINTER(PdscParams), ps, vp, pp, pp, pp, pp, vp, sz, vp]
        L.lr_fcgf_weights_bytes.restype = ctypes.c_size_t
        L.lr_fcgf_weights_bytes.argtypes = [ci]
        L.lr_fcgf_scratch_bytes.argtypes = [ci]
        L.lr_fcgf_extract.argtypes = [vp, vp, ci, vp, sz, ctypes.POINTER(FcgfParams), vp, vp, vp, vp, sz, vp]
        L.lr_fcgf_batch_scratch_bytes.argtypes = [ci, ci]
        L.lr_debug_fcgf_batch_stop_after.argtypes = [ci]
        L.lr_fcgf_extract_batch.argtypes = [ci, pp, pp, ip, vp, sz, ctypes.POINTER(FcgfParams), vp, pp, vp, sz, vp]
        pd = ctypes.POINTER(DgrParams)
        L.lr_dgr_scratch_bytes.argtypes = [ci]
        L.lr_dgr_refine.argtypes = [vp, vp, ci, vp, vp, vp, pd, vp, vp, vp, sz, vp]
        L.lr_dgr_refine_batch.argtypes = [ci, pp, pp, ip, pp, pp, pp, pd, vp, vp, sz, vp]
        w8 = ctypes.POINTER(ctypes.c_int32 * 8)
        L.lr_dgr_inlier_weights_bytes.restype = ctypes.c_size_t
        L.lr_dgr_inlier_weights_bytes.argtypes = [w8]
        L.lr_dgr_inlier_scratch_bytes.argtypes = [ci, w8]
        L.lr_dgr_inlier.argtypes = [vp, ci, vp, sz, ctypes.POINTER(DgrInlierParams), vp, vp, vp, vp, sz, vp]
        L.lr_dgr_inlier_batch_scratch_bytes.argtypes = [ci, ci, w8]
        L.lr_dgr_inlier_batch.argtypes = [ci, pp, ip, vp, sz, ctypes.POINTER(DgrInlierParams), vp, pp, vp, sz, vp]
        L.lr_nn_wide_scratch_bytes.argtypes = [ci, ci, ci]
        L.lr_nn_wide.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, sz, vp]
        L.lr_fpfh_scratch_bytes.argtypes = [ci, ci]
        L.lr_fpfh.argtypes = [vp, vp, ci, dp, ci, vp, vp, vp, vp, sz, vp]
        L.lr_workspace_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ci)]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise LidarRegError(f"liblidarreg error {rc}: {lib().lr_last_error().decode()}")


class Workspace:
    """Owns one lr_workspace: device scratch for one in-flight pair, or -- max_pairs > 1 -- for one in-flight batch of pairs
    registered by a single lr_register_batch call."""

    def __init__(self, max_n0, max_n1, dim=32, max_iters=50000, max_pairs=1, _wide=False):
        self._h = ctypes.c_void_p()
        self.max_n0, self.max_n1, self.dim, self.max_iters = int(max_n0), int(max_n1), int(dim), int(max_iters)
        self.max_pairs = int(max_pairs)
        self.is_wide = bool(_wide)
        create = lib().lr_workspace_create_wide if self.is_wide else lib().lr_workspace_create_batch
        check(create(ctypes.byref(self._h), self.max_pairs, self.max_n0, self.max_n1, self.dim, self.max_iters))
        for name, value in DEFAULT_OPTIONS.items():
            self.set_option(name, value)

    @classmethod
    def wide(cls, max_n0, max_n1, dim, max_iters=50000, max_pairs=1):
        """A wide workspace (lr_workspace_create_wide): descriptors of 33..128 numbers.  Workspace(dim=33) itself keeps refusing."""
        return cls(max_n0, max_n1, dim, max_iters, max_pairs, _wide=True)

    @classmethod
    def for_dim(cls, max_n0, max_n1, dim, max_iters=50000, max_pairs=1):
        """The workspace kind that serves descriptors `dim` wide: narrow up to 32, wide from 33."""
        return cls(max_n0, max_n1, dim, max_iters, max_pairs, _wide=int(dim) > 32)

    def set_option(self, name, value):
        """Tuning option of this workspace (OPTIONS; none changes a result)."""
        check(lib().lr_workspace_option(self._h, OPTIONS[name], int(value)))

    def stage_times(self):
        """(sums in ms [whole call, forward NN, forward filter pass, reverse filter pass, RANSAC gen+score, reverse NN], timed calls)
        since lr_workspace_timing(ws, 1); the stream must be synchronised."""
        out = (ctypes.c_float * 8)(); n = ctypes.c_int()
        check(lib().lr_workspace_stage_times(self._h, out, ctypes.byref(n)))
        return list(out[:6]), n.value

    def timing(self, enable):
        check(lib().lr_workspace_timing(self._h, int(bool(enable))))

    def clock(self, reset=False):
        """(MHz, shader cycles, 100 MHz ticks) of the filter-pass blocks since the last reset (option clock_probe); the streams that used the
        workspace must be synchronised."""
        mhz = ctypes.c_double(); cyc = ctypes.c_ulonglong(); tk = ctypes.c_ulonglong()
        check(lib().lr_workspace_clock(self._h, ctypes.byref(mhz), ctypes.byref(cyc), ctypes.byref(tk), int(bool(reset))))
        return mhz.value, cyc.value, tk.value

    @property
    def handle(self):
        return self._h

    def fits(self, n0, n1, dim, iters):
        return n0 <= self.max_n0 and n1 <= self.max_n1 and dim == self.dim and iters <= self.max_iters and (dim > 32) == self.is_wide

    @property
    def nbytes(self):
        return lib().lr_workspace_bytes(self._h)

    def poison(self, byte, stream=None):
        """Test hook: fill the scratch arena with one byte value (results must not depend on it)."""
        check(lib().lr_workspace_poison(self._h, int(byte), stream))

    def close(self):
        if self._h:
            lib().lr_workspace_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
