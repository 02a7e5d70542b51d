/*
 * lidarreg.h -- C ABI of liblidarreg.so (hand-written HIP for gfx950 / MI355X).
 *
 * Drop-in boundary for the registration hot path of AmnonDrory/LidarRegistration.  Each entry point
 * names the reference interface it replaces (paths relative to the reference tree).  Conventions:
 *
 *   - every data pointer is a caller-owned DEVICE pointer (e.g. torch tensor .data_ptr()), contiguous,
 *     row-major; the library allocates nothing behind the caller's back except inside an explicit
 *     lr_workspace;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all calls are asynchronous on
 *     it and do not synchronise with the host; the data-path entry points only launch kernels (and
 *     1-D memsets) on that stream, so a caller may capture them in a HIP graph and replay it on new
 *     data in the same buffers (timing off: lr_workspace_timing records events);
 *   - return value 0 = LR_OK, negative = error (lr_last_error() gives the text); nothing throws;
 *   - 4x4 transforms are row-major float64, column-vector convention, cloud 0 -> cloud 1
 *     (the reference's pygcransac binding returns the transpose, GC_RANSAC.py:55 -- not here);
 *   - a workspace may be used by one stream at a time; use one workspace per in-flight pair;
 *   - a workspace belongs to the device that was current when it was created (hipGetDevice); every entry point that takes one returns
 *     LR_EINVAL -- before launching anything -- when another device is current or the stream belongs to another device.  The library
 *     holds gfx950 code objects only: lr_workspace_create refuses any other architecture (gcnArchName) and sizes its launches from the
 *     device's compute-unit count (multiProcessorCount).
 */
#ifndef LIDARREG_H
#define LIDARREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR_API __attribute__((visibility("default")))

enum { LR_OK = 0, LR_EINVAL = -1, LR_ENOMEM = -2, LR_EHIP = -3, LR_ESIZE = -4 };

/* filter modes of FR(): Experiments/algorithms/FR.py:48-56 ("MNN" | "GPF" | "no_filter") */
enum { LR_MODE_NO_FILTER = 0, LR_MODE_MNN = 1, LR_MODE_GPF = 2 };

typedef struct lr_workspace lr_workspace;

/* RANSAC knobs.  Replaces the parameter dict of GC_RANSAC.py:12-37 and the keyword arguments of
 * FR.py:128-137, with explicit flags instead of the reference's sentinel overloading.            */
typedef struct lr_ransac_params {
    uint32_t struct_size;   /* = sizeof(lr_ransac_params) of the header the caller was built against; every entry point that
                               takes the struct checks it first and returns LR_EINVAL on a mismatch (lr_version 102)   */
    int32_t  sample_size;   /* 3 = GC-RANSAC minimal solver, 4 = FR.py:134 ransac_n                  */
    int32_t  use_elc;       /* pre-verification (--fast_rejection, GC_RANSAC.py:29-34): 0 none; 1 edge-length check of the
                               sample, similarity 0.9 (preemption_edge_length.h:82); 2 SPRT on the estimated model
                               (gcransac_python.cpp:534-568, min_inlier_ratio_for_sprt 0.1): Wald's sequential test over
                               the first 256 correspondences, design (eps, delta, A) updated between batches          */
    float    thr2;          /* squared inlier threshold; (2*voxel)^2 = 0.36 (FR.py:85,95)             */
    int32_t  iters;         /* hypothesis ids 0..iters-1 (--iters, FR.py:65-67)                       */
    uint64_t seed;          /* Philox4x32-10 key; sample of hypothesis h = philox(seed, h)            */
    float    confidence;    /* early exit (--GC_conf / FR.py:136): ids are evaluated in batches of `batch`; after a
                               batch ending at id e the run stops when e >= log(1-confidence) / log(1 - (inl/M)^sample_size)
                               for the best model so far.  >= 1 (or <= 0): every id is evaluated.             */
    int32_t  batch;         /* batch length of the early-exit test, constant; 0 -> 1024, 8192, 65536, ... (eightfold) */
    int32_t  sampler;       /* 0: uniform WITH replacement (Open3D's RANSAC, FR.py:128-137); 2: uniform, unique indices
                               (GC_RANSAC.py:19 'sampler': 0 -> GC-RANSAC's UniformSampler); 1: PROSAC (--prosac,
                               GC_RANSAC.py:24,39-43): the correspondences must come best quality first; hypothesis id h =
                               PROSAC draw h+1: sample_size-1 indices uniformly from the first n-1 correspondences plus the
                               n-th, n from the growth function of Chum & Matas 2005 (as in USAC / GC-RANSAC's
                               prosac_sampler.h); ids past prosac_growth fall back to uniform sampling over all
                               correspondences.  Samplers 1 and 2 reject a draw with a repeated index (the id is consumed
                               like a failed pre-check)                                                              */
    int32_t  prosac_growth; /* T_N of the growth function (0 -> 100000, GC-RANSAC's default)          */
    int32_t  scoring;       /* which model wins: 0 = more inliers, then lower squared-error sum (Open3D: fitness, then
                               inlier RMSE); 1 = MSAC, the truncated quadratic cost: larger sum over inliers of (thr2 - d^2),
                               evaluated as count * (uint32)(thr2 * 2^20) - best_ssq; 2 = MSAC as GC-RANSAC runs it
                               (MSACScoringFunction behind gcransac_python.cpp:507-512; --codebase GC): inlier test, cost, exit
                               rule, local optimisation, final least squares and inlier mask all use the TRUNCATED threshold
                               (3/2 thr)^2 = 2.25 thr2 (upstream-recalled) -- i.e. scoring 1 at 1.5 x the threshold */
    int32_t  local_opt;     /* 0: none -- the winning minimal-sample model is returned (Open3D); 1: GC-RANSAC's local
                               optimisation (--GC_LO True, GC_RANSAC.py:36-37; gcransac_python.cpp:418-423,508-515): every new
                               best model is re-estimated by an inner RANSAC over its inliers (<= 10 rounds of 20 least-squares
                               fits on 21 inliers each, scored over all correspondences; spatial coherence weight 0), at the
                               granularity of the early-exit batches, plus the final iterated least squares; 2: the final
                               iterated least squares over the inliers only (--GC_LO False)                           */
    /* Three settings of gcransac_python.cpp:513-517 (553-556, 579-582) whose meaning lives in the un-vendored library; 0 = default.
     * `max_local_optimization_number = 20` (50 without a pre-verification) admits two readings -- least-squares fits per round of
     * one optimisation (lo_trials) or optimisations per run (lo_max_calls); both are knobs, both default to that number.         */
    int32_t  lo_rounds;     /* rounds of one local optimisation (upstream max_graph_cut_number), default 10             */
    int32_t  lo_trials;     /* least-squares fits per round, 1..20, default 20                                          */
    int32_t  lo_max_calls;  /* local optimisations per run, default 20 (use_elc != 0) / 50 (use_elc == 0)               */
    int32_t  min_iters;     /* the exit rule is not consulted before this many ids (min_iteration_number), default 20 / 50;
                               only matters with batches shorter than that                                              */
} lr_ransac_params;

/* Written to device memory by lr_ransac / lr_register_pair. */
typedef struct lr_ransac_result {
    int64_t  best_h;        /* winning hypothesis id, -1 when none had an inlier                     */
    uint32_t best_count;    /* its inlier count over the M correspondences                            */
    uint32_t pad0;          /* diagnostic: see lr_pair_result.reserved[1] (0 unless a hand-off wait of the local optimisation timed out) */
    uint64_t best_ssq;      /* sum over its inliers of (uint32)(d^2 * 2^20)                           */
    int64_t  n_valid;       /* hypotheses that passed the pre-check and were scored                   */
    int64_t  n_ids;         /* hypothesis ids examined before the run stopped (== iters without early exit) */
} lr_ransac_result;

/* Written by lr_icp / lr_register_pair(icp != 0). */
typedef struct lr_icp_result {
    double   fitness;       /* correspondences within max_dist / source points, last evaluation       */
    double   inlier_rmse;   /* sqrt(mean squared distance) over those correspondences                  */
    int32_t  n_corr;
    int32_t  iterations;    /* transform updates applied                                               */
} lr_icp_result;

/* Per-pair result block of lr_register_pair (device memory, 496 bytes). */
typedef struct lr_pair_result {
    double   T[16];         /* final transform (after the LS refit when refit != 0)                   */
    double   T_ransac[16];  /* winning minimal-sample model before the refit                          */
    lr_ransac_result ransac;
    int32_t  n_corr;        /* correspondences after filtering (num_pairs_filtered, FR.py:60)         */
    int32_t  n_refit;       /* inliers used by the refit (FR.py:104-108): the NUMBER of pairs within refit_thr2 of T_ransac, also under the
                               weights of refit = 3 (not their weight sum) and when the refit left T = T_ransac (unweighted: fewer than 3
                               of them); 0 when there was no model (status 1)                          */
    int32_t  n_nn_fixed;    /* NN rows/cols that needed the exact sqrt tie-break path                 */
    int32_t  status;        /* 0 ok, 1 = no valid hypothesis (T = identity, GC_RANSAC.py:51-52)       */
    int32_t  reserved[8];   /* [0]: diagnostic, like n_nn_fixed -- (model, correspondence) evaluations of the scoring passes in ppm of
                               scanning every list in full (0: not recorded); may differ between runs (the pilot among models with
                               equal head counts depends on scheduling), no result does.  [1]: diagnostic -- waits of the local optimisation's
                               helper-block hand-off that hit their 0.2 s bound (low 16 bits: the master block recomputed a scoring job alone;
                               high 16 bits: a helper block left without a job); integer sums make the result the same either way, a non-zero
                               value means time was lost (also in lr_ransac_result.pad0).  [2]: diagnostic -- a single-pair call launched only the form of the
                               filter pass the previous calls' norms asked for and this pair's asked for the other (bit 0: forward, bit 1: reverse pass):
                               every row then went through the exact scan, correct but slow; two calls in a row must agree before a form is launched
                               alone.  [3..7]: 0                                                                                  */
    double   T_icp[16];     /* T refined by point-to-point ICP (test.py:183-189) when icp != 0, else = T */
    lr_icp_result icp;
} lr_pair_result;

typedef struct lr_pair_params {
    uint32_t struct_size;   /* = sizeof(lr_pair_params), checked like lr_ransac_params.struct_size (which must be set too) */
    int32_t  mode;          /* LR_MODE_*                                                             */
    int32_t  refit;         /* 0 none; 1: LS refit on the ORIGINAL NN pairs within thr (FR.py:99-111, codebase open3D);
                               2: on the FILTERED pairs RANSAC ran on (GC-RANSAC's final least squares over its inliers);
                               3: as 1 but weighted by the inverse feature distance of each pair (DGR register_FCGF,
                                  DGR/core/deep_global_registration.py:531-537)                                  */
    lr_ransac_params ransac;
    /* GPF (matching.py:100-205), only read when mode == LR_MODE_GPF */
    int32_t  gpf_grid_wid;  /* --GPF_grid_wid, default 10                                            */
    int32_t  icp;           /* 1: refine T by ICP (max distance 0.6 m, 30 updates, 1e-6 criteria; test.py:183-189) */
    double   gpf_factor;    /* --GPF_factor,   default 2.0 (a Python float in the reference)         */
    double   refit_thr2;    /* fp64 squared threshold of the refit's inlier test, (2*0.3)**2 (FR.py:105) */
} lr_pair_params;

/* ---- library ------------------------------------------------------------------------------- */
LR_API int         lr_version(void);    /* 100 * major + minor; 103: lr_workspace_clock, LR_OPT_CLOCK_PROBE, lr_debug_fake_current_device, device checks; 102: params structs start with struct_size (72 / 112 bytes), descriptors of 1..32 dimensions; 101: lr_ransac_params 64 bytes / lr_pair_params 96 bytes (round 3), lr_icp_batch */
LR_API const char *lr_last_error(void);

/* Scratch for clouds up to (max_n0, max_n1) points x dim (1 <= dim <= 32; matching.py:22-65 takes any width: 33..128 go to lr_workspace_create_wide, or to lr_nn_wide, which takes no workspace) and up to max_iters hypotheses. */
LR_API int    lr_workspace_create(lr_workspace **ws, int max_n0, int max_n1, int dim, int max_iters);
/* The same for up to max_pairs (<= 64) pairs registered by ONE call of lr_register_batch: max_pairs arenas of identical
 * layout in one allocation.  The single-pair entry points below work on such a workspace too (they use arena 0).        */
LR_API int    lr_workspace_create_batch(lr_workspace **ws, int max_pairs, int max_n0, int max_n1, int dim, int max_iters);
/* The same for descriptors of 33..128 numbers (FPFH's 33): a WIDE workspace.  Its NN stage is the exact f32 matrix-core kernel of
 * lr_nn_wide with the pair as a grid dimension, both directions and the norms once per call (no f16 filter pass: none of its operand
 * copies is allocated, lr_workspace_bytes says what is).  A wide workspace is a workspace: lr_nn_top2 (idx2 = NULL: the top-1 form),
 * lr_nn_to_mutual, lr_gpf, lr_gpf_bb_first, lr_register_pair / _batch in every mode with either sampler and refit 0, 1 or 2,
 * lr_icp_batch, the *_lists* / *_mask_at accessors, the timing events, LR_OPT_NN_SECOND_AUTO and lr_workspace_poison work on it with
 * dim == its dim, and give what the oracle gives at that width.  Refused on it with LR_EINVAL, by name and before any launch:
 * refit == 3, and a pair with n1 < 2 in a call that reads the second neighbour (lr_gpf*, mode GPF, the PROSAC sampler).
 * Limits of max_pairs / max_n0 / max_n1 / max_iters as lr_workspace_create_batch; refusals are LR_EINVAL / LR_ESIZE before any HIP
 * call, lr_last_error naming the argument; dim 1..32: "use lr_workspace_create".                                                   */
LR_API int    lr_workspace_create_wide(lr_workspace **ws, int max_pairs, int max_n0, int max_n1, int dim, int max_iters);
LR_API int    lr_workspace_destroy(lr_workspace *ws);
/* Test hook (no reference counterpart): copies the reverse-NN list of pair `pair` out of the arena, as the last call with a reverse
 * direction (lr_nn_to_mutual, lr_gpf*, lr_register_pair / _batch in mode MNN or GPF) left it: rev[j] = the nearest cloud-0 row of
 * cloud-1 row j, -1 where no query points at j (j < n1 <= max_n1; device memory).                                                  */
LR_API int    lr_debug_workspace_rev(lr_workspace *ws, int pair, int n1, int32_t *rev, void *stream);
LR_API size_t lr_workspace_bytes(const lr_workspace *ws);
/* Test hook (no reference counterpart): fill the scratch arena with one byte value; results must not depend on it. */
LR_API int    lr_workspace_poison(lr_workspace *ws, int byte, void *stream);
/* Test hook (no reference counterpart): the entry points take `device` for the current device from now on (-1: ask HIP again), so that a
 * one-GPU box can exercise the wrong-device refusal above. */
LR_API int    lr_debug_fake_current_device(int device);
/* Tuning options of a workspace (no reference counterpart; NONE of them changes a result, tests/test_gpu_parity.py; the library
 * reads no environment variable).  value 0 restores the default.                                                          */
enum {
    LR_OPT_NN_BLOCKS        = 1,  /* a single-pair filter pass is cut into column strips so that it launches about this many blocks (512) */
    LR_OPT_NN_BLOCKS_BATCH  = 2,  /* the same for a batched call, over all its pairs (3072)                                  */
    LR_OPT_NN_SAMPLE_STRIDE = 3,  /* the filter pass samples every k-th column tile for its start thresholds (default: strip tiles / 32, at most 32) */
    LR_OPT_REV_STRIPS       = 4,  /* column strips offered to each row block of the reverse NN pass (default 48 / pairs, within 2..8) */
    LR_OPT_NN_SECOND_AUTO   = 5,  /* 1: lr_register_pair / _batch compute the second neighbour only when a stage of the call reads it */
    LR_OPT_CLOCK_PROBE      = 6   /* 1: the filter-pass blocks sum their shader cycles and 100 MHz ticks into the workspace (lr_workspace_clock) */
};
LR_API int    lr_workspace_option(lr_workspace *ws, int option, int value);
/* Measurement hook (no reference counterpart): the shader clock the filter-pass blocks ran at since the last reset, *mhz = 100 * cycles / ticks
 * (0 when nothing was recorded: LR_OPT_CLOCK_PROBE off).  The caller has synchronised the streams that used the workspace.  Any pointer may be NULL. */
LR_API int    lr_workspace_clock(lr_workspace *ws, double *mhz, unsigned long long *cycles, unsigned long long *ticks, int reset);

/* ---- a1/a2: find_nn / find_2nn  (Experiments/algorithms/matching.py:6-65) ------------------------
 * For every row of F0 [n0,dim] the nearest and second nearest row of F1 [n1,dim] under L2, first
 * minimal value wins.  idx2/s1/s2 may be NULL.  s = sqrt(max(d2,1e-30)) as matching.py:30.        */
LR_API int lr_nn_top2(lr_workspace *ws, const float *F0, int n0, const float *F1, int n1, int dim,
                      int32_t *idx1, int32_t *idx2, float *s1, float *s2, void *stream);

/* ---- a3-a5: nn_to_mutual / mark_best_buddies  (matching.py:67-87, 207-239) -----------------------
 * Runs the reverse NN (F1 -> F0) and intersects: is_bb[i] = (rev[idx1[i]] == i).  The surviving
 * pairs are written in ascending i (torch coalesce order) to out_idx0/out_idx1[/out_idx2]; their
 * number to *n_out (device int32).  is_bb, out_* and idx2 may be NULL.                             */
LR_API int lr_nn_to_mutual(lr_workspace *ws, const float *F0, int n0, const float *F1, int n1, int dim,
                           const int32_t *idx1, const int32_t *idx2,
                           uint8_t *is_bb, int32_t *out_idx0, int32_t *out_idx1, int32_t *out_idx2,
                           int32_t *n_out, void *stream);

/* ---- a6: calc_distance_ratio_in_feature_space  (matching.py:89-98) ------------------------------- */
LR_API int lr_feat_ratio(const float *F0, const float *F1, int dim, int m,
                         const int32_t *i0, const int32_t *i1, const int32_t *i2, float *out, void *stream);

/* ---- a7: Grid_Prioritized_Filter, BB_first=False  (matching.py:100-205) --------------------------
 * idx1/idx2 are the NN lists of all n0 rows; xyz0 [n0,3].  Kept pairs (ascending i) go to out_*,
 * their count to *n_out (device), their score (norm_feat_dist, matching.py:124,134) to out_score. */
LR_API int lr_gpf(lr_workspace *ws, const float *F0, int n0, const float *F1, int n1, int dim,
                  const int32_t *idx1, const int32_t *idx2, const float *xyz0,
                  int grid_wid, double factor,
                  int32_t *out_idx0, int32_t *out_idx1, int32_t *out_idx2, float *out_score,
                  int32_t *n_out, void *stream);

/* ---- a7, BB_first=True  (matching.py:109-113,126; the reference's TEASER wrapper, TEASER_plus_plus.py:109-110) ----
 * Mutual pairs first, then the grid filter over them with TOTAL_NUM = max_matches and no best-buddy shift.
 * *has_score (device int32) is 0 when the mutual set was already <= max_matches (the reference returns None). */
LR_API int lr_gpf_bb_first(lr_workspace *ws, const float *F0, int n0, const float *F1, int n1, int dim,
                           const int32_t *idx1, const int32_t *idx2, const float *xyz0,
                           int grid_wid, double max_matches,
                           int32_t *out_idx0, int32_t *out_idx1, int32_t *out_idx2, float *out_score,
                           int32_t *n_out, int32_t *has_score, void *stream);

/* ---- a10/a12: RANSAC over M correspondences src[i] <-> tgt[i]  ([M,3] float32 each) ---------------
 * Replaces pygcransac.findRigidTransform(x1y1z1, x2y2z2, ...) (GC_RANSAC.py:46-49; native side
 * gcransac_python.cpp:404-416) and o3d registration_ransac_based_on_correspondence (FR.py:128-137).
 * m_dev, if not NULL, is a device int32 holding the live M (<= m).  Writes T_out[16] and *res, and leaves a copy of the model on
 * the workspace, where lr_inlier_mask(T = NULL) reads it (one device-to-device copy of 128 bytes on the call's stream).          */
LR_API int lr_ransac(lr_workspace *ws, const float *src, const float *tgt, int m, const int32_t *m_dev,
                     const lr_ransac_params *p, double *T_out, lr_ransac_result *res, void *stream);

/* The inlier mask findRigidTransform returns next to the pose (gcransac_python.cpp:594-603): mask[c] = 1 when
 * |T src[c] - tgt[c]|^2 < thr2 in the fp32 arithmetic of the scoring kernel; *n_inliers (device, may be NULL) their number.
 * T is a DEVICE pointer (e.g. T_out of lr_ransac); with T = NULL the model of the last lr_ransac / lr_register_pair on ws.  */
LR_API int lr_inlier_mask(lr_workspace *ws, const float *src, const float *tgt, int m, const double *T, float thr2,
                          uint8_t *mask, int32_t *n_inliers, void *stream);
/* ... over the filtered pairs (corr_idx0[c], corr_idx1[c]) of pair `pair` of the last lr_register_pair / lr_register_batch,
 * with that pair's RANSAC model (lr_pair_result.T_ransac); mask has room for n0 entries, the first n_corr are written.      */
LR_API int lr_workspace_mask_at(lr_workspace *ws, int pair, const float *xyz0, const float *xyz1, int n0, float thr2,
                                uint8_t *mask, int32_t *n_inliers, void *stream);

/* ---- a11: LS refit on the original NN pairs within thr of T_in  (FR.py:99-111) --------------------
 * Pairs (i, idx1[i]), i < n0, with |T_in xyz0[i] - xyz1[idx1[i]]|^2 < thr2 (fp64, strict) are the inliers; a row with idx1[i] < 0
 * has no partner and is skipped.  *n_inliers (device, may be NULL) = their number; T_out = T_in when there are fewer than 3.  */
LR_API int lr_refit(lr_workspace *ws, const float *xyz0, int n0, const float *xyz1, const int32_t *idx1,
                    const double *T_in, double thr2, double *T_out, int32_t *n_inliers, void *stream);

/* ---- f1: point-to-point ICP refinement (Experiments/test.py:183-189; Open3D registration_icp) ---------------
 * src = xyz0 [n0,3], tgt = xyz1 [n1,3] float32, T_init[16] device float64.  Open3D defaults: max_iter 30,
 * rel_fitness = rel_rmse = 1e-6.                                                                   */
LR_API int lr_icp(lr_workspace *ws, const float *xyz0, int n0, const float *xyz1, int n1, const double *T_init,
                  double max_dist, int max_iter, double rel_fitness, double rel_rmse,
                  double *T_out, lr_icp_result *res, void *stream);

/* The same refinement for EVERY pair of the last lr_register_batch call on this workspace, as one set of launches: the
 * harness runs ICP after the timed registration and times it on its own (Experiments/test.py:183-193, stats columns 11-14).
 * Starts from that call's final transforms (still in the arenas), over the clouds that call was given (they must still be
 * alive); fills T_icp / icp of out[k], k < npairs of that call (out = the result blocks of that call, or a copy).       */
LR_API int lr_icp_batch(lr_workspace *ws, double max_dist, int max_iter, double rel_fitness, double rel_rmse,
                        lr_pair_result *out, void *stream);

/* ---- a13: least-squares rigid fit of n point pairs  (models/common.py:7-45) -------------------------
 * P, Q [n,3] float64, optional weights w [n]; T_out[16].                                           */
LR_API int lr_kabsch(const double *P, const double *Q, const double *w, int n, double *T_out, void *stream);

/* ---- a9: FR() end to end on device  (Experiments/algorithms/FR.py:16-119) -------------------------
 * NN -> filter (mode) -> RANSAC -> optional refit, one call, no host synchronisation.             */
LR_API int lr_register_pair(lr_workspace *ws, const float *xyz0, const float *xyz1,
                            const float *F0, const float *F1, int n0, int n1, int dim,
                            const lr_pair_params *p, lr_pair_result *out, void *stream);

/* ---- a9 for many pairs: what Experiments/test.py:165-167 does pair after pair (one FR() per list row), as ONE sequence of
 * kernel launches over `npairs` pairs: every kernel of the path is launched once with the pair as a grid dimension, so the
 * GPU is filled by the batch instead of by many concurrent streams.  xyz0/xyz1/F0/F1/n0/n1 are HOST arrays of length npairs
 * (device pointers / cloud sizes, which may differ from pair to pair); out is a DEVICE array of npairs result blocks.  The
 * result of pair k is bit-identical to lr_register_pair on that pair.
 * ONE CALL IN FLIGHT PER WORKSPACE: the call's descriptor table and scratch arenas belong to the workspace, so a second call on
 * the same workspace -- from any stream -- may only be enqueued behind the first on the SAME stream; concurrent batches need one
 * workspace each (bench.py: one per stream).  The *_at accessors read pair < npairs of the LAST call only.                  */
LR_API int lr_register_batch(lr_workspace *ws, int npairs, const float *const *xyz0, const float *const *xyz1,
                             const float *const *F0, const float *const *F1, const int32_t *n0, const int32_t *n1, int dim,
                             const lr_pair_params *p, lr_pair_result *out, void *stream);

/* Copies the correspondence lists of the last lr_register_pair on this workspace into caller-owned
 * device buffers (any may be NULL): the NN lists over all n0 rows (FR.py's corres_idx1_orig / idx1_2nd_orig)
 * and the filtered lists, of which the first out->n_corr entries are live (buffers sized n0).     */
LR_API int lr_workspace_lists(lr_workspace *ws, int n0, int32_t *nn_idx1, int32_t *nn_idx2,
                              int32_t *corr_idx0, int32_t *corr_idx1, void *stream);
/* ... and of pair `pair` of the last lr_register_batch */
LR_API int lr_workspace_lists_at(lr_workspace *ws, int pair, int n0, int32_t *nn_idx1, int32_t *nn_idx2,
                                 int32_t *corr_idx0, int32_t *corr_idx1, void *stream);
/* ... and of its first `npairs` pairs at once: buffers [npairs][width] int32, row k = pair k (what the harness reads for the
 * statistics of Experiments/test.py:200-208 after a batched call: one strided copy per list)                             */
LR_API int lr_workspace_lists_batch(lr_workspace *ws, int npairs, int width, int32_t *nn_idx1, int32_t *nn_idx2,
                                    int32_t *corr_idx0, int32_t *corr_idx1, void *stream);

/* ---- f2: voxel de-duplication of a raw cloud -- ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) as the
 * reference's loaders call it (Experiments/dataloader/generic_balanced_loader.py:62-63; voxel_size 0.3).
 * coords [n,3] float64 device = xyz / voxel_size (the division is the caller's, as in the reference); one point per occupied
 * integer cell floor(coords) is kept -- the first in input order -- and the kept point indices are written to sel in ascending
 * order, their number to *n_sel (device).  cells (optional, [n,3] int32) receives the integer cell of every kept point.
 * Points with a non-finite coordinate or |cell| >= 2^20 are dropped.  scratch: lr_voxel_dedup_scratch_bytes(n) device bytes, memory
 * of the current device (checked, like the stream: LR_EINVAL, before any launch; n == 0 takes no scratch and checks none).       */
LR_API size_t lr_voxel_dedup_scratch_bytes(int n);
LR_API int    lr_voxel_dedup(const double *coords, int n, int32_t *sel, int32_t *n_sel, int32_t *cells, void *scratch,
                             size_t scratch_bytes, void *stream);

/* ---- t1: TEASER++ global registration over M correspondences src[i] <-> tgt[i]  ([M,3] float32 device arrays) ----------------
 * Replaces the reference's TEASER++ back end (Experiments/algorithms/TEASER_plus_plus.py:78-126, --algo TEASER; TEASER++ is not
 * vendored, so parity with it is unpinned and the following is the contract, restated in tests/teaser_cpu.py):
 *  1. consistency graph: i ~ j (i != j) iff | |a_i - a_j| - |b_i - b_j| | <= 2 noise_bound sqrt(cbar2), in fp64 on the promoted
 *     inputs (differences, (dx*dx + dy*dy) + dz*dz, no FMA, correctly rounded sqrt); the device adjacency is bit-identical to it;
 *  2. a maximum clique, ascending indices, the same set on every run.  K-core shortcut: when the maximum core number exceeds
 *     kcore_threshold * M the vertices of maximum core number are returned instead (1.0 disables it).  The search is bounded by
 *     node_budget branch nodes and time_budget_ms of device clock; when either runs out the best clique found so far is
 *     returned with exact = 0 (the GPU form of the reference's 10 s kill, TEASER_plus_plus.py:14-59);
 *  3. rotation: GNC-TLS on the K chain TIMs A_k = a[c_(k+1) mod K] - a[c_k] (B_k on b), noise bound 2 noise_bound (nb2 =
 *     4 noise_bound^2 cbar2), gnc_factor, max_iterations, cost_threshold; the weighted uncentred fit R = V diag(1,1,det(VU^T)) U^T
 *     of H = sum w A B^T = U S V^T; where H has rank <= 1 (collinear or coincident points, s2 <= 1e-14 s1) the optimum is not unique
 *     and R is any proper rotation attaining it (R = I for H = 0); TIM k is a rotation inlier iff its final weight >= 0.5;
 *  4. translation: per axis adaptive voting over x = b - R a of the rotation-inlier clique points with range noise_bound (endpoints
 *     sorted by value, entries before exits, then index; first minimum of sum_in (x - mean)^2 + noise_bound |out|); a point is a
 *     translation inlier iff it lies within noise_bound of the estimate on all three axes;
 *  5. K < 3 or fewer than 3 rotation inliers: status 1 and T = identity (GC_RANSAC.py:51-52).
 * Other TEASER++ modes (scale estimation, other TIM graphs / rotation solvers / clique modes) are not built and refused.          */
typedef struct lr_teaser_params {
    uint32_t struct_size;        /* = sizeof(lr_teaser_params), checked like lr_ransac_params.struct_size                        */
    int32_t  max_iterations;     /* GNC iterations, 10000 (TEASER_plus_plus.py)                                                   */
    double   noise_bound;        /* beta, VOXEL_SIZE = 0.3                                                                        */
    double   cbar2;              /* 1                                                                                             */
    double   kcore_threshold;    /* 0.5 (upstream default, recalled); in (0, 1], 1.0 disables the shortcut                      */
    double   gnc_factor;         /* 1.4, > 1                                                                                      */
    double   cost_threshold;     /* 1e-16                                                                                         */
    int64_t  node_budget;        /* branch nodes of the exact search, >= 1                                                        */
    double   time_budget_ms;     /* device-clock budget of the exact search, (0, 3.6e6]                                           */
    int32_t  rotation_tim_graph; /* 0 = CHAIN (the only graph built)                                                              */
    int32_t  estimate_scaling;   /* 0 (scale estimation is not built)                                                             */
} lr_teaser_params;

/* Written to device memory by lr_teaser / lr_teaser_batch (176 bytes). */
typedef struct lr_teaser_result {
    double   T[16];              /* cloud 0 -> cloud 1, row-major; identity when status = 1                                      */
    int32_t  status;             /* 0 ok, 1 = fewer than 3 clique points or rotation inliers                                      */
    int32_t  K;                  /* clique size                                                                                   */
    int32_t  exact;              /* 1: the search was not cut by a budget (also with the k-core shortcut); 0: it was              */
    int32_t  max_core;           /* maximum core number of the graph                                                              */
    int32_t  lb;                 /* size of the best greedy clique (0 when the shortcut fired)                                   */
    int32_t  pad0;
    uint64_t nodes;              /* branch nodes of the exact search                                                              */
    int32_t  gnc_iters;          /* GNC iterations run (0: all residuals below nb2 / 2 at the start)                              */
    int32_t  n_rot_inliers;
    int32_t  n_trans_inliers;
    int32_t  pad1;
} lr_teaser_result;

/* Caller-owned device scratch per pair for up to max_m correspondences (0 when max_m is outside 0..32768).  Test hook: after a
 * call, the consistency graph of pair k is readable at byte 256 of its arena (scratch + k * lr_teaser_scratch_bytes(max m)): row
 * i < M is ceil(max m / 64) uint64 words apart, bit j of word j / 64 set iff i ~ j (words past ceil(M / 64) are not written).     */
LR_API size_t lr_teaser_scratch_bytes(int max_m);
/* m_dev, if not NULL, is a device int32 holding the live M (clamped to 0..m).  clique_out (nullable, room for m int32) receives the
 * clique, ascending; result->K entries are live.  scratch: >= lr_teaser_scratch_bytes(m) bytes, 256-byte aligned, memory of the
 * current device (checked, like the stream: LR_EINVAL, before any launch; a short scratch and m > 32768 are LR_ESIZE).          */
LR_API int lr_teaser(const float *src, const float *tgt, int m, const int32_t *m_dev, const lr_teaser_params *p,
                     lr_teaser_result *result, int32_t *clique_out, void *scratch, size_t scratch_bytes, void *stream);
/* npairs (1..64) independent problems in one sequence of launches (the pair is a grid dimension); src/tgt/m/m_dev/clique_out are
 * HOST arrays of length npairs (m_dev and clique_out, and their entries, may be NULL), carried by value into a setup kernel (no
 * copy: graph-capturable); results is a DEVICE array of npairs blocks; scratch >= npairs * lr_teaser_scratch_bytes(max m).  The
 * result of pair k is bit-identical to lr_teaser on that pair.                                                                   */
LR_API int lr_teaser_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                           const lr_teaser_params *p, lr_teaser_result *results, int32_t *const *clique_out, void *scratch,
                           size_t scratch_bytes, void *stream);
/* Measurement hook: with timing on, every lr_teaser / _batch call records events between its four stages (graph, clique, rotation,
 * translation); lr_teaser_stage_times gives those of the last call in ms (after synchronising its stream).  Process-wide.        */
LR_API int lr_teaser_timing(int enable);
LR_API int lr_teaser_stage_times(float out[4]);

/* ---- s1: spectral matching over M correspondences src[i] <-> tgt[i]  ([M,3] float32 device arrays) -------------------------------
 * Replaces SM() of the reference's baseline survey (Experiments/baseline_scripts/baseline_3DMatch.py:19-53; run with inlier_threshold
 * 0.6 and top_ratio 0.05 by baseline_KITTI.py:51-52) and the weighted fit it ends in (Experiments/models/common.py:7-45).  The M x M
 * compatibility matrix is never stored: every power iteration re-evaluates it.  Contract (restated in tests/sm_cpu.py):
 *  1. compatibility (3DMatch.py:20-37): c(i,j) = max(0, 4.5 - d^2 / (2 sigma^2)), sigma = inlier_threshold / 3, d = |a_i - a_j| - |b_i - b_j|,
 *     in fp32 on the direct differences: (dx*dx + dy*dy) + dz*dz, correctly rounded sqrt, d = la - lb, fmaf(d*d, -1/(2 sigma^2), 4.5), no
 *     other fusion.  c(i,i) = 0 by INDEX: a duplicated correspondence gets 4.5.  Deviation: a correspondence with a non-finite
 *     coordinate has compatibility 0 with everything (the reference propagates NaN into every output);
 *  2. power iteration (3DMatch.py:40-44): v = 1; `iterations` times v <- C v, v <- v / (|v|_2 + 1e-6).  Row sums are fp32 over column
 *     chunks in ascending order, the chunks and the norm are summed in fp64 in a fixed order;
 *  3. selection (3DMatch.py:47-49): K = (int)((double)M * top_ratio), Python's int(M * top_ratio); the K largest v under (value descending,
 *     index ascending) -- torch's argsort leaves ties open, this pins them; labels in {0,1};
 *  4. fit (3DMatch.py:52, common.py:7-45): weights w_i = v_i label_i, centroids divided by (sum w + 1e-6), covariance of the centred
 *     points, all fp64 in a fixed order, rotation by the Horn solver of csrc/lr_contract.h (= V diag(1,1,det) U^T of common.py:36-41);
 *  5. K < 3 or sum w = 0: status 1 and T = identity.
 * The same input gives the same bits on every run, whatever the scratch held, alone or as pair k of a batch (on devices with the same
 * number of compute units: it sizes the column chunks, i.e. the order of the fp32 sums).                                        */
typedef struct lr_sm_params {
    uint32_t struct_size;        /* = sizeof(lr_sm_params), checked like lr_ransac_params.struct_size                              */
    int32_t  iterations;         /* power iterations, 10 (3DMatch.py:41); 1..1000                                                   */
    double   inlier_threshold;   /* 0.6 (baseline_KITTI.py:51); sigma = inlier_threshold / 3                                        */
    double   top_ratio;          /* 0.05 (baseline_KITTI.py:52; SM()'s own default is 0.1); in (0, 1]                               */
} lr_sm_params;

/* Written to device memory by lr_sm / lr_sm_batch (152 bytes). */
typedef struct lr_sm_result {
    double   T[16];              /* cloud 0 -> cloud 1, row-major; identity when status = 1                                        */
    int32_t  status;             /* 0 ok, 1 = fewer than 3 selected correspondences or all of weight 0                              */
    int32_t  K;                  /* selected correspondences                                                                        */
    int32_t  m;                  /* live correspondence count the call ran on                                                       */
    int32_t  reserved;           /* 0                                                                                               */
    double   weight_sum;         /* sum of the weights w_i                                                                          */
} lr_sm_result;

/* Caller-owned device scratch per pair for up to max_m correspondences (0 when max_m is outside 0..32768). */
LR_API size_t lr_sm_scratch_bytes(int max_m);
/* m_dev, if not NULL, is a device int32 holding the live M (clamped to 0..m); K is then formed on the device.  eig_out (nullable,
 * float32[m]) receives the final v, labels_out (nullable, uint8[m]) the labels; entries at and past the live count are written 0.
 * scratch: >= lr_sm_scratch_bytes(m) bytes, 256-byte aligned, memory of the current device (checked, like the stream: LR_EINVAL).
 * Every refusal (short scratch, m > 32768, iterations / top_ratio out of range, struct_size) is LR_EINVAL, before any launch.  */
LR_API int lr_sm(const float *src, const float *tgt, int m, const int32_t *m_dev, const lr_sm_params *p, lr_sm_result *result,
                 float *eig_out, uint8_t *labels_out, void *scratch, size_t scratch_bytes, void *stream);
/* npairs (1..64) independent problems in one sequence of launches (the pair is a grid dimension); src/tgt/m/m_dev/eig_out/labels_out are
 * HOST arrays of length npairs (m_dev, eig_out and labels_out, and their entries, may be NULL), carried by value into a setup kernel (no
 * copy, no host synchronisation: graph-capturable); results is a DEVICE array of npairs blocks; scratch >= npairs *
 * lr_sm_scratch_bytes(max m).  The result of pair k is bit-identical to lr_sm on that pair.                                       */
LR_API int lr_sm_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                       const lr_sm_params *p, lr_sm_result *results, float *const *eig_out, uint8_t *const *labels_out, void *scratch,
                       size_t scratch_bytes, void *stream);

/* ---- f5: voxel-grid down-sampling (one centroid per voxel) and the pair overlap measure -----------------------------------------
 * lr_voxel_mean replaces Open3D's PointCloud.voxel_down_sample as the reference calls it (BalancedDatasetGenerator/
 * GenerateBalancedSet.py:143-147 `downsample`; FCGF_FAST/net/refinement_tester.py:69-73) -- NOT lr_voxel_dedup, which is
 * MinkowskiEngine's "keep the first point of a cell".  lr_overlap / lr_overlap_batch replace overlap_fraction and calc_GT_overlap
 * (GenerateBalancedSet.py:155-205), the batch serving one source frame against many candidates (find_farthest_overlapping_partner,
 * :321-371).  Contract (restated in tests/overlap_cpu.py).  All arithmetic is fp64, no fused multiply-add.  Items marked
 * (recalled) come from memory of Open3D 0.13, which is neither vendored by the reference nor available to this project: unpinned.
 *  C1 input: xyz [n,3] float64 on the device.  An optional T[16] (device, fp64, row-major) is applied first,
 *     p_a = ((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3] (the expression of lr_icp); T == NULL is the identity: no arithmetic is done
 *     on the point.  Deviation: a point with a non-finite coordinate after the transform is dropped and counted (Open3D would carry
 *     NaN into the bounds).
 *  C2 cells (recalled: PointCloud::VoxelDownSample): lo_a = min of p_a over the kept points, vmb_a = lo_a - voxel * 0.5, cell
 *     c_a = (int)floor((p_a - vmb_a) / voxel) -- a division, so c_a >= 0.  A cloud is refused with status 2 and no output unless
 *     (hi_a - vmb_a) / voxel < 2^21 on every axis.
 *  C3 output: one row per occupied cell, rows by ascending index of the cell's first point (scan order, like lr_voxel_dedup; Open3D's
 *     order is that of an unordered_map, unspecified).  Per row: first = that index; count; centroid = the sum (from +0) of the cell's
 *     points in ascending point index, left to right, per axis, then divided by (double)count -- the order in which Open3D's
 *     AccumulatedPoint::AddPoint sees them (recalled).  The same bits on every run, whatever the scratch held; no floating-point atomics.
 *  C4 overlap: A_ = C3(T A, voxel), B_ = C3(B, voxel); r = radius, or fl(sqrt 2) * voxel when radius == 0 (np.sqrt(2) * voxel_size,
 *     in double on the host); n_overlap = #{ a in A_ : exists b in B_ with sqrt((dx dx + dy dy) + dz dz) < r }, strict, d = a - b per
 *     axis, sqrt correctly rounded; frac = n_overlap / |A_|; frac_sym = min(frac, n_overlap / |B_|) -- the SAME A->B numerator in both,
 *     the reference's own definition (GenerateBalancedSet.py:176-178).  |A_| == 0 or |B_| == 0: status 1, both fractions 0, n_overlap 0
 *     (the reference divides by zero); a refused cloud (C2): status 2, likewise, and its n?_ds is 0.  Only existence within r is
 *     asked, so the result does not depend on any order.
 *  C5 refusals, all LR_EINVAL before any launch, lr_last_error naming the argument: wrong struct_size; voxel_size not positive and
 *     finite; radius negative or not finite, or not 0 and outside voxel_size / 16 .. 4 voxel_size (one centroid per voxel bounds what
 *     a search cell of edge r holds: 0.5 and 3 voxel are served, a radius far from the voxel size is not); n < 0 or n > 4194304;
 *     npairs outside 1..64; null pointers where n > 0 (the scratch and the result / info block are always needed); short or
 *     misaligned (256 bytes) scratch; scratch that is not memory of the current gfx950 device, or a stream of another device.
 *     n == 0 is legal (status 1).                                                                                                   */
typedef struct lr_overlap_params {
    uint32_t struct_size;        /* = sizeof(lr_overlap_params), checked like lr_ransac_params.struct_size                          */
    uint32_t reserved;           /* 0                                                                                               */
    double   voxel_size;         /* 1.0 (GenerateBalancedSet.py:171)                                                                */
    double   radius;             /* 0: fl(sqrt 2) * voxel_size (:175)                                                               */
} lr_overlap_params;

/* Written to device memory by lr_overlap / lr_overlap_batch (40 bytes). */
typedef struct lr_overlap_result {
    int32_t  status;             /* 0 ok, 1 = a down-sampled cloud is empty, 2 = a cloud exceeds 2^21 cells on an axis              */
    int32_t  n0_ds, n1_ds;       /* |A_|, |B_|                                                                                      */
    int32_t  n_overlap;
    int32_t  n0_dropped, n1_dropped;     /* points with a non-finite coordinate                                                     */
    double   frac, frac_sym;     /* overlap_frac, overlap_frac_symmetric (:177-178)                                                 */
} lr_overlap_result;

/* Caller-owned device scratch for a cloud of n points (0 when n is outside 0..4194304). */
LR_API size_t lr_voxel_mean_scratch_bytes(int n);
/* GenerateBalancedSet.py:143-147 / refinement_tester.py:69-73 (o3d voxel_down_sample), with the transform of :197 / :243 folded in.
 * cent [n,3] float64, cent_f32 [n,3] float32 (the float32 rounding of cent: what lr_icp consumes), counts [n], first [n]: nullable,
 * room for n rows, info[0] rows are written.  info: device int32[4] = { rows, dropped, status, 0 }; status 1 = no point kept,
 * 2 = refused (C2): no row is written.  scratch: >= lr_voxel_mean_scratch_bytes(n), 256-byte aligned.  Asynchronous on `stream`.      */
LR_API int lr_voxel_mean(const double *xyz, int n, const double *T, double voxel_size, double *cent, float *cent_f32,
                         int32_t *counts, int32_t *first, int32_t *info, void *scratch, size_t scratch_bytes, void *stream);
/* Scratch PER PAIR for clouds of up to max_n0 / max_n1 points (0 when either is outside 0..4194304). */
LR_API size_t lr_overlap_scratch_bytes(int max_n0, int max_n1);
/* GenerateBalancedSet.py:155-179 overlap_fraction (T == NULL) and :186-205 calc_GT_overlap (T = GT_mot, applied to cloud 0).
 * result: device block.  scratch >= lr_overlap_scratch_bytes(n0, n1).                                                               */
LR_API int lr_overlap(const double *xyz0, int n0, const double *xyz1, int n1, const double *T, const lr_overlap_params *p,
                      lr_overlap_result *result, void *scratch, size_t scratch_bytes, void *stream);
/* npairs (1..64) pairs in one sequence of launches (the pair and the cloud are grid dimensions) -- the candidate loop of
 * GenerateBalancedSet.py:321-371.  xyz0/n0/xyz1/n1/T are HOST arrays of length npairs (T, and its entries, may be NULL), carried by
 * value into a setup kernel (no copy, no host synchronisation: graph-capturable); results is a DEVICE array of npairs blocks; scratch
 * >= npairs * lr_overlap_scratch_bytes(max n0, max n1).  The result of pair k is bit-identical to lr_overlap on that pair.          */
LR_API int lr_overlap_batch(int npairs, const double *const *xyz0, const int32_t *n0, const double *const *xyz1, const int32_t *n1,
                            const double *const *T, const lr_overlap_params *p, lr_overlap_result *results, void *scratch,
                            size_t scratch_bytes, void *stream);

/* ---- f6: the exact 3-D nearest neighbour and the Z-only refinement of a ground-truth motion ------------------------------------------
 * lr_nn3 replaces the balanced-set generator's NN (GenerateBalancedSet.py:149-153: cKDTree(B).query(A, k = 1)) -- unbounded and exact,
 * unlike the radius-bounded searches of lr_icp and lr_overlap; lr_refine_z replaces refine_motion_Z_only (:257-291).  Contract (restated
 * in tests/refine_z_cpu.py).  All arithmetic is fp64, no fused multiply-add.
 *  N1 inputs: xyz0 [n0,3] (queries), xyz1 [n1,3] (target), float64 on the device, n in 0 .. 4194304.
 *  N2 distance: d2(i,j) = (dx dx + dy dy) + dz dz on the differences a - b per axis.
 *  N3 outputs: idx[i] = the j of the least d2 over the finite target points, the LOWEST j on equal computed d2; dist[i] = the correctly
 *     rounded square root of that d2.
 *  N4 a target point with a non-finite coordinate is never a neighbour; a non-finite query gets idx -1, dist +inf.  Both kinds are
 *     counted in info (the reference raises ValueError).
 *  N5 n1 == 0 or no finite target: every idx -1, every dist +inf, status 1.  Legal.
 *  N6 cell: edge of the search grid's cells.  0 = automatic: the finest edge E 2^(-k/2), k = 0 .. 80, E the longest edge of the
 *     target's bounding box, whose grid over that box has at most max(4096, 4 n1) cells.  cell > 0: that edge, doubled until the grid
 *     has at most that many cells.  A tuning knob only: THE RESULT DOES NOT DEPEND ON IT.
 *  Z  lr_refine_z: A_ = T A by C1 above (T == NULL: A as it is), dz = 0; the target's grid is built once.  Each of up to max_repeats
 *     repeats: (1) ind = N(A_, B); (2) pair i is valid iff ind >= 0 and sqrt(dx dx + dy dy) <= xy_gate (root correctly rounded,
 *     non-strict); (3) z_i = A_z - B_z, w_i = 1 / |z_i| (+inf at 0); (4) med = numpy's median of the valid w: the middle element, or
 *     (lo + hi) / 2 of the two middle ones -- found by an exact radix select on the bit patterns; (5) w_i = min(w_i, med);
 *     (6) mean = S(w z) / S(w), the products rounded separately, S the fixed two-level sum: the terms sit at their source index (an
 *     invalid pair is +0.0), every run of 1024 consecutive indices is summed left to right from +0, then the run sums left to right;
 *     (7) every A_z becomes fl(A_z - mean), dz = fl(dz - mean); (8) stop after this repeat if |mean| < min_change.
 *     Deviations: no valid pair -> status 1, dz stays as accumulated, the loop stops (the reference takes the median of nothing: NaN);
 *     med == +inf (at least half the valid pairs coincide in z) -> status 2, the step is 0, the loop stops (the reference computes
 *     inf * 0 = NaN).  The same bits on every run, whatever the scratch held; no floating-point atomics; no host synchronisation
 *     (the repeats of a finished call return at their first instruction): graph-capturable.
 *  Refusals, all LR_EINVAL before any launch, lr_last_error naming the argument: wrong struct_size; cell negative or not finite;
 *     max_repeats outside 1..64; xy_gate not positive and finite; min_change negative or not finite; n0 / n1 outside 0..4194304; null
 *     pointers where n > 0 (scratch, info / result always needed); short or misaligned (256 bytes) scratch; scratch that is not memory
 *     of the current gfx950 device, or a stream of another device.                                                                   */
typedef struct lr_nn3_params {
    uint32_t struct_size;        /* = sizeof(lr_nn3_params)                                                                         */
    uint32_t reserved;           /* 0                                                                                               */
    double   cell;               /* 0 = automatic (N6)                                                                              */
} lr_nn3_params;

typedef struct lr_refine_z_params {
    uint32_t struct_size;        /* = sizeof(lr_refine_z_params)                                                                    */
    int32_t  max_repeats;        /* 10 (MAX_REPEATS, :264); 1..64                                                                   */
    double   xy_gate;            /* voxel_size (:273)                                                                               */
    double   min_change;         /* 1e-6 (MIN_CHANGE, :265)                                                                         */
    double   cell;               /* 0 = automatic (N6)                                                                              */
} lr_refine_z_params;

/* Written to device memory by lr_refine_z (40 bytes). */
typedef struct lr_refine_z_result {
    int32_t  status;             /* 0 ok, 1 = a repeat had no valid pair, 2 = a repeat's median weight was +inf                     */
    int32_t  repeats;            /* repeats run, the stopping one included                                                          */
    int32_t  n_valid;            /* valid pairs of the last repeat                                                                  */
    int32_t  n0_dropped, n1_dropped;     /* points with a non-finite coordinate (cloud 0: after T)                                  */
    int32_t  reserved;           /* 0                                                                                               */
    double   dz;                 /* what to add to the motion's [2,3] (:289)                                                        */
    double   last_step;          /* mean_z_dist of the last repeat (0 with status 1 / 2)                                            */
} lr_refine_z_result;

/* Caller-owned device scratch for n0 queries against n1 target points (0 when either is outside 0..4194304). */
LR_API size_t lr_nn3_scratch_bytes(int n0, int n1);
/* idx [n0] int32, dist [n0] float64: device.  info: device int32[4] = { status (N5), non-finite queries, non-finite target points,
 * queries resolved by the second phase (a statistic) }.  Asynchronous on `stream`.                                                   */
LR_API int lr_nn3(const double *xyz0, int n0, const double *xyz1, int n1, const lr_nn3_params *p, int32_t *idx, double *dist,
                  int32_t *info, void *scratch, size_t scratch_bytes, void *stream);
LR_API size_t lr_refine_z_scratch_bytes(int n0, int n1);
/* T: device, fp64, row-major 4x4, nullable; result: device block.  scratch >= lr_refine_z_scratch_bytes(n0, n1).                    */
LR_API int lr_refine_z(const double *xyz0, int n0, const double *xyz1, int n1, const double *T, const lr_refine_z_params *p,
                       lr_refine_z_result *result, void *scratch, size_t scratch_bytes, void *stream);

/* ---- f7: Best-Buddies refinement (BBR-F) and hybrid-search point normals on the exact nearest neighbour -------------------------------
 * lr_bbrf replaces FCGF_FAST/net/BBR_F.py:267-322 (100 Adam steps on six pose parameters over the mutual nearest neighbours of two
 * clouds under a symmetric point-to-plane loss); lr_normals replaces its calc_normals (:236-241, Open3D estimate_normals with
 * KDTreeSearchParamHybrid).  Contract (restated in tests/bbrf_cpu.py).  All arithmetic is fp64, no fused multiply-add;
 * (PQ) of two 3x3 matrices is (P[a][0] Q[0][b] + P[a][1] Q[1][b]) + P[a][2] Q[2][b]; M.v of a matrix and a vector is
 * (M[a][0] x + M[a][1] y) + M[a][2] z; u.v is (u0 v0 + u1 v1) + u2 v2.  The parameters p = (theta, phi, psi, tx, ty, tz), Adam's
 * moments and the powers of beta start at 0, 0 and 1.  For iteration k = 0 .. n_iter - 1:
 *  B1 log row k = (p, loss, n_pairs) of this iteration.
 *  B2 W = Rz(psi) (Ry(phi) Rx(theta)), Rx = [1 0 0; 0 c -s; 0 s c], Ry = [c 0 s; 0 1 0; -s 0 c], Rz = [c -s 0; s c 0; 0 0 1]
 *     (BBR_F.py:69-85).  sin and cos are fixed polynomials: z = x x; q = c_17, q = q z + c_k for k = 15, 13 .. 3, sin x = x + (x z) q;
 *     q = c_16, q = q z + c_k for k = 14, 12 .. 2, cos x = 1 + z q; c_k = fl(+-1 / k!), the Taylor signs (truncation below 2^-60 on
 *     |x| <= 0.5).  The derivative matrices are dW/dtheta = Rz (Ry dRx), dW/dphi = Rz (dRy Rx), dW/dpsi = dRz (Ry Rx) with
 *     dRx = [0 0 0; 0 -s -c; 0 c -s], dRy = [-s 0 c; 0 0 0; -c 0 -s], dRz = [-s -c 0; c -s 0; 0 0 0].
 *  B3 B'_j = (W.B_j) + t per axis (C1 of lr_overlap), nB'_j = W.nB_j.  A never moves.
 *  B4 f = N(A, B'), r = N(B', A) by contract N of lr_nn3; (i, f_i) is a pair iff f_i >= 0 and r[f_i] == i.
 *  B5 per pair: s = -1 if nA_i.nB'_j < 0, else +1; m = nA_i + s nB'_j; d = A_i - B'_j; dot = d.m; term = |dot| if |dot| > 1e-15, else
 *     1e-15.  loss = S(terms) / n_pairs, S the two-level sum Z6 of lr_refine_z over the source index i (a non-pair is +0.0).
 *  B6 gradient: a pair with fl(dot dot) < 1e-30 contributes +0.0; else g = sg e, sg = -1 if dot < 0, else +1, with
 *     e = -m_a for t_a and e = d.(s (dW/dq.nB_j)) - (dW/dq.B_j).m for an angle q.  grad = S(g) / n_pairs, six sums.
 *  B7 Adam (torch's rule), t = k + 1: pw1 = pw1 beta1, pw2 = pw2 beta2; m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2)(g g);
 *     p = p - (lr / (1 - pw1)) (m / (sqrt(v) / sqrt(1 - pw2) + eps)); roots and quotients correctly rounded.  An angle that then is
 *     not within [-0.5, 0.5]: status 3, the loop stops.
 *  B8 best_iter = the first iteration of least loss (a NaN loss is never the least); B_to_A = [W t; 0 1] from that row's parameters by
 *     B2; T = [W^T, -(W^T.t); 0 1].  No iteration with a pair: the identity, best_iter -1, best_loss +inf.
 *  Deviations from the reference: parameters and moments are fp64 (float32 there); an iteration without a pair logs loss +inf, sets
 *     status 1 and stops the loop with the best so far (the reference takes the mean of nothing); the inverse is the rigid one.
 *  Log rows past iters_run are +0.0.  The same bits on every run, whatever the scratch held; no floating-point atomics; no host
 *  synchronisation (the launches of a finished call return at their first instruction): graph-capturable.
 *  Refusals, all LR_EINVAL before any launch, lr_last_error naming the argument: wrong struct_size; n_iter outside 1..1000; a learning
 *     rate or eps not positive and finite; a beta outside [0, 1); cell negative or not finite; n0 / n1 outside 0..4194304; null pointers
 *     where n > 0 (scratch and result always needed); short or misaligned (256 bytes) scratch; scratch that is not memory of the
 *     current gfx950 device, or a stream of another device.  n0 == 0 or n1 == 0 is legal (status 1).
 *  Normals [upstream-recalled from Open3D 0.13, parity unpinned]: the neighbours of point i are the at most max_nn finite points of
 *     least (d2, index) with d2 <= fl(radius radius), d2 by N2, i itself included.  Fewer than 3: (0, 0, 1).  Else the sums of x, y, z,
 *     xx, xy, xz, yy, yz, zz over the neighbours in (d2, index) order from +0, each divided by their number, cov(a,b) = E[ab] - E[a] E[b];
 *     eigenvectors by 8 sweeps of cyclic Jacobi over (0,1), (0,2), (1,2) -- a_pq != 0: th = (a_qq - a_pp) / (2 a_pq),
 *     t = sign(th) / (|th| + sqrt(th th + 1)) (sign(0) = +1), c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0,
 *     (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), the same on the columns p, q of V (from the identity) -- the normal is the column
 *     of V with the least diagonal entry (the lowest index on ties) divided by its norm sqrt((xx + yy) + zz); a norm that is not > 0
 *     gives (0, 0, 1).  The sign is the solver's.  A non-finite point gets (0, 0, 1) and is counted in info.                         */
typedef struct lr_bbrf_params {
    uint32_t struct_size;        /* = sizeof(lr_bbrf_params)                                                                        */
    int32_t  n_iter;             /* 100 (BBR_F.py:272); 1..1000                                                                     */
    double   angles_lr, trans_lr;        /* 2e-4 each (:273-274)                                                                    */
    double   beta1, beta2, eps;  /* 0.9, 0.999, 1e-8 (torch.optim.Adam's defaults)                                                  */
    double   cell;               /* 0 = automatic (N6)                                                                              */
} lr_bbrf_params;

/* Written to device memory by lr_bbrf (280 bytes). */
typedef struct lr_bbrf_result {
    double   T[16];              /* A -> B, row-major                                                                               */
    double   B_to_A[16];
    int32_t  status;             /* 0 ok, 1 = an iteration had no pair, 3 = an angle left [-0.5, 0.5]                               */
    int32_t  best_iter;          /* -1: none                                                                                        */
    double   best_loss;
    int32_t  n_pairs_best;
    int32_t  iters_run;          /* log rows written, the stopping one included                                                     */
} lr_bbrf_result;

/* Caller-owned device scratch (0 when n0 / n1 is outside 0..4194304 or n_iter outside 1..1000). */
LR_API size_t lr_bbrf_scratch_bytes(int n0, int n1, int n_iter);
/* xyzA, nrmA [n0,3], xyzB, nrmB [n1,3]: device float64; result: device block; log: device float64 [n_iter, 8], nullable.           */
LR_API int lr_bbrf(const double *xyzA, const double *nrmA, int n0, const double *xyzB, const double *nrmB, int n1,
                   const lr_bbrf_params *params, lr_bbrf_result *result, double *log, void *scratch, size_t scratch_bytes, void *stream);
LR_API size_t lr_normals_scratch_bytes(int n);
/* normals_out [n,3] device float64; info: device int32[4] = { 1 if no finite point, non-finite points, points with fewer than 3
 * neighbours, 0 }.  radius positive and finite, max_nn in 1..32.                                                                  */
LR_API int lr_normals(const double *xyz, int n, double radius, int max_nn, double *normals_out, int32_t *info, void *scratch,
                      size_t scratch_bytes, void *stream);
/* lr_normals and, where n_nb_out (device int32 [n], nullable) is given, the number of neighbours every point took: 0 .. max_nn, the point
 * itself included, 0 for a non-finite point.  A default (0, 0, 1) cannot be told from a true one without it.  Same kernels, normals, info
 * and scratch (lr_normals_scratch_bytes) as lr_normals.                                                                            */
LR_API int lr_normals2(const double *xyz, int n, double radius, int max_nn, double *normals_out, int32_t *n_nb_out, int32_t *info,
                       void *scratch, size_t scratch_bytes, void *stream);

/* ---- f9: symmetric ICP on the exact nearest neighbour (f8 is the balanced-set selection below) -----------------------------------------
 * lr_symicp is the third refinement of FCGF_FAST/net/refinement_tester.py:75-93.  The reference shells out to trimesh2's mesh_align
 * (net/symmetric_icp.py:47-82), a binary outside its tree: [upstream-recalled, parity unpinned].  The contract is the algorithm of the
 * paper behind that binary (Rusinkiewicz, A Symmetric Objective Function for ICP, 2019), restated in tests/symicp_cpu.py; DESIGN.md §23.
 * All arithmetic is fp64, no fused multiply-add, only + - x / sqrt; products, M.v and u.v associate as in f7; the cross product is
 * (u x v)_x = u_y v_z - u_z v_y, cyclically.  A is fixed, B moves.  (W, t) starts at the identity, or at the upper 3 x 4 of T_init.
 * For iteration k = 0 .. n_iter - 1:
 *  Y1 B'_j = (W.B_j) + t, nB'_j = W.nB_j.
 *  Y2 f = N(A, B'), r = N(B', A) by contract N of lr_nn3.  Forward candidates (i, f_i) for every i with f_i >= 0; backward candidates
 *     (r_j, j) for every j with r_j >= 0 and f[r_j] != j (a mutual pair counts once).
 *  Y3 a candidate (i, j), p = B'_j, q = A_i, d = p - q, dot = nA_i.nB'_j, is accepted iff p, q, nA_i, nB'_j are finite,
 *     d.d <= fl(max_dist max_dist) and |dot| >= min_cos.  s = -1 if dot < 0, else +1; n = nA_i + s nB'_j; row c = [(p + q) x n ; n],
 *     b = -(d.n).
 *  Y4 28 sums and an integer count: c_a c_b (a <= b, row-major), c_a b, b b; a rejected or absent candidate is +0.0.  Order: the index
 *     space in runs of 1024; in a run lane l = 0 .. 63 adds its 16 consecutive terms in order from +0.0; the lanes fold
 *     v[l] = v[l] + v[l + h] for h = 32, 16, 8, 4, 2, 1; the run sums are added in run order from +0.0; the forward total over i and the
 *     backward total over j separately, total = fwd + bwd.
 *  Y5 fewer than 6 accepted pairs: status 1, stop, the pose stays.  Cholesky H = L L^T, j ascending: d_j = H_jj - L_j0^2 - .. (k
 *     ascending); unless d_j > piv_eps H_jj (a NaN fails): status 2 (singular), stop, the pose stays.  L_jj = sqrt(d_j),
 *     L_ij = (H_ij - L_i0 L_j0 - ..) / L_jj; y_i = (g_i - L_i0 y_0 - ..) / L_ii; x_i = (y_i - L_(i+1)i x_(i+1) - .. - L_5i x_5) / L_ii,
 *     i descending.  x = (a, tt).  A non-finite x: status 3, stop, the pose stays.
 *  Y6 c = 1 / sqrt(1 + a.a); R[u][v] = (D_uv + c S_uv) + (c c / (1 + c)) (a_u a_v), D = c I, S = [0 -a2 a1; a2 0 -a0; -a1 a0 0];
 *     dW = R R; dt = R.(c tt); W = dW W; t = (dW.t) + dt.  No re-orthonormalisation.
 *  Y7 log row k = (n_pairs, S(b b) / n_pairs (0 without a pair), a.a, dt.dt, 0, 0, 0, 0) (a.a and dt.dt 0 on a status stop).  If
 *     a.a <= fl(eps_rot eps_rot) and dt.dt <= fl(eps_trans eps_trans): converged = 1, stop.  Rows past iters_run are +0.0.
 *  Result: B_to_A = [W t; 0 1] of the last pose, T = [W^T, -(W^T.t); 0 1], iters_run (the stopping iteration included), converged,
 *     status, the last n_pairs and mean square.  The same bits on every run, whatever the scratch held; no floating-point atomics; no
 *     host synchronisation: graph-capturable.
 *  Refusals, all LR_EINVAL before any launch, lr_last_error naming the argument: wrong struct_size; n_iter outside 1..1000; max_dist,
 *     piv_eps, eps_rot, eps_trans not positive and finite; min_cos outside [0, 1]; cell negative or not finite; n0 / n1 outside
 *     0..4194304; null pointers where n > 0 (scratch and result always needed); short or misaligned (256 bytes) scratch; scratch that
 *     is not memory of the current gfx950 device, or a stream of another device.  n0 == 0 or n1 == 0 is legal (status 1).          */
typedef struct lr_symicp_params {
    uint32_t struct_size;        /* = sizeof(lr_symicp_params)                                                                      */
    int32_t  n_iter;             /* 30; 1..1000                                                                                     */
    double   max_dist;           /* two voxels: 0.6 at the refinement tester's 0.3                                                  */
    double   min_cos;            /* 0.7; [0, 1]                                                                                     */
    double   eps_rot, eps_trans; /* 1e-5 (tan of the half step's angle), 1e-4 (m)                                                   */
    double   piv_eps;            /* 1e-9                                                                                            */
    double   cell;               /* 0 = automatic (N6)                                                                              */
    const double *T_init;        /* device, fp64, row-major 4x4, nullable: the start B -> A                                         */
} lr_symicp_params;

/* Written to device memory by lr_symicp (280 bytes). */
typedef struct lr_symicp_result {
    double   T[16];              /* A -> B, row-major                                                                               */
    double   B_to_A[16];
    int32_t  status;             /* 0 ok, 1 = fewer than 6 pairs, 2 = singular normal equations, 3 = a non-finite step              */
    int32_t  iters_run;          /* log rows written, the stopping one included                                                     */
    int32_t  converged;
    int32_t  n_pairs;            /* of the last iteration                                                                           */
    double   mean_sq;            /* S(b b) / n_pairs of the last iteration                                                          */
} lr_symicp_result;

/* Caller-owned device scratch (0 when n0 / n1 is outside 0..4194304). */
LR_API size_t lr_symicp_scratch_bytes(int n0, int n1);
/* xyzA, nrmA [n0,3], xyzB, nrmB [n1,3]: device float64; result: device block; log: device float64 [n_iter, 8], nullable.           */
LR_API int lr_symicp(const double *xyzA, const double *nrmA, int n0, const double *xyzB, const double *nrmB, int n1,
                     const lr_symicp_params *params, lr_symicp_result *result, double *log, void *scratch, size_t scratch_bytes, void *stream);

/* ---- f8: balanced-set selection -----------------------------------------------------------------------------------------------------
 * lr_balanced_select replaces the rejection loop of BalancedDatasetGenerator/GenerateBalancedSet.py (select_balanced_set :544-562 around
 * select_sample :466-507 and to_points_in_hyper_cube :456-464).  Contract S (restated in tests/balanced_cpu.py).  All
 * arithmetic is fp64, no fused multiply-add.  State: an alive flag per candidate, n_sel[s] per session (from 0), the constant n_cands[s]
 * (the candidates session s had at load).  For attempt k with the draw r_k[6]:
 *   S1  m_c / M_c = the least / greatest value of column c of `fields` over the alive candidates; p_ic = (f_ic - m_c) / (M_c - m_c).
 *   S2  q_c = (r_c - p_ic) (r_c - p_ic); s = ((((q_0 + q_1) + q_2) + q_3) + q_4) + q_5; d_i = sqrt(s), correctly rounded.
 *   S3  the group: the alive candidates with d_i < thresh, strictly.  Empty: a miss -- the attempt is consumed, the state stays.
 *   S4  fullness_i = (double)n_sel[s_i] / (double)n_cands[s_i]; selected: the lexicographic minimum of (fullness_i, d_i, i) over the group.
 *   S5  n_sel[s]++, the candidate dies and its index is appended to `out`; the next attempt sees S1 over the rest.
 * Stop (result.status): 0 = n_request candidates are selected (with n_request 0: at once, nothing consumed); 1 = the draws of this call
 * are used up; 2 = a column's M_c - m_c is not a positive finite number (one alive candidate, a constant column, a non-finite field: the
 * reference divides by zero there and never ends) -- before the first attempt, or straight after the commit that caused it, which is
 * kept and counted (also when it was the n_request-th); 3 = a session id outside 0..n_sessions-1, n_cands[s] < 1 for a session that
 * occurs, or a resumed state that does not add up; 4 = params.max_rounds rounds ran (only with max_rounds > 0).  After status 1 or 4
 * the state is left in the caller's buffers -- alive, n_sel, out, result -- and a call with resume = 1 and the draws from
 * result.consumed on continues exactly where this one stopped (the scratch need not be kept).                                       */
#define LR_SELECT_MAX_ROUNDS 65536
typedef struct lr_select_params {
    uint32_t struct_size;        /* = sizeof(lr_select_params)                                                                      */
    int32_t  n_request;          /* candidates to select in all, over every resumed call: 0..n                                      */
    double   thresh;             /* 0.1 (GenerateBalancedSet.py:474); positive and finite                                           */
    int32_t  resume;             /* 0: every candidate alive, every count 0; 1: alive, n_sel, out and result hold an earlier call's */
    int32_t  max_rounds;         /* 0: as many rounds as the draws can need (<= 65536, else the call is refused); else 1..65536     */
} lr_select_params;

/* Device block, read and written by lr_balanced_select (136 bytes). */
typedef struct lr_select_result {
    int32_t  status;
    int32_t  n_selected;         /* entries of `out`, over every resumed call                                                       */
    int64_t  attempts, misses;   /* draws consumed / of them without a selection, over every resumed call                           */
    int64_t  consumed;           /* draws of THIS call consumed                                                                     */
    int32_t  rounds;             /* rounds that did something, over every resumed call                                              */
    int32_t  rescales;           /* commits after which a column's least or greatest value was another one                          */
    double   lo[6], hi[6];       /* m_c, M_c over the alive candidates                                                              */
} lr_select_result;

/* Caller-owned device scratch (0 when n is outside 0..4194304). */
LR_API size_t lr_balanced_select_scratch_bytes(int n);
/* fields [n,6] float64, session [n] int32 (dense ids 0..n_sessions-1), n_cands [n_sessions] int32, draws [n_draws,6] float64, alive [n]
 * uint8, n_sel [n_sessions] int32, out [n_request] int32, result: all device memory.  n 0..4194304, n_sessions 1..65536, n_draws 0..2^40.
 * No host synchronisation; capturable into a graph.                                                                                 */
LR_API int lr_balanced_select(const double *fields, const int32_t *session, const int32_t *n_cands, int n, int n_sessions,
                              const double *draws, long long n_draws, const lr_select_params *params, uint8_t *alive, int32_t *n_sel,
                              int32_t *out, lr_select_result *result, void *scratch, size_t scratch_bytes, void *stream);

/* ---- p1: PointDSC's SC-NonLocal correspondence encoder and confidence head over M correspondences src[i] <-> tgt[i] -------------
 * Replaces NonLocalNet (Experiments/models/PointDSC.py:9-77), the spatial-consistency matrix it attends with (:150-153) and the
 * classification head (:107-113, :171) in inference mode: a 128-d feature and an inlier logit per correspondence.  The M x M
 * matrices (compatibility, logits, softmax weights) are never stored.  Seed picking, the neural spectral matching, the per-seed fits
 * and post_refinement are p2 below.  Contract (restated in tests/pdsc_cpu.py):
 *  E1 a correspondence with a non-finite coordinate is dead (deviation: the reference propagates NaN into every output): its key gets
 *     weight 0 in every softmax, its feature is 0 and its confidence -inf, and it does not enter the mean of E2;
 *  E2 corr_pos = [src, tgt] - column mean over the live rows (demo_registration.py:107-108): the sums in fp64 (thread t of 1024 adds
 *     rows t, t + 1024, ... in ascending order, then the halving tree s[t] += s[t + h], h = 512 .. 1), mean = sum / count, the
 *     subtraction in fp64, rounded to fp32 once;
 *  E3 compat(i,j) = max(0, 1 - d^2 / sigma_d^2), d = |s_i - s_j| - |t_i - t_j|, in fp32 on the direct differences of the given
 *     coordinates: (dx*dx + dy*dy) + dz*dz, correctly rounded sqrt, fmaxf(0, fmaf(d*d, (float)(-1 / sigma_d^2), 1));
 *  E4 per layer, fp32: h = relu(bn(conv(feat))) (PointCN); q, k, v = conv(h); w = softmax_j(compat(i,j) * (q_i . k_j * (float)(1/sqrt(128))))
 *     over the live j (all of them: a zero compatibility still weighs exp(0 - max)); message_i = sum_j w_ij v_j;
 *     feat = h + fc_message(message) (128 -> 64 -> 64 -> 128, bn + relu after the first two).  BatchNorm is folded: every layer is
 *     y = scale * (W x) + offset, the dot product an fmaf chain over ascending input channel;
 *  E5 confidence = conv(relu(conv(relu(conv(feat))))), 128 -> 32 -> 32 -> 1;
 *  E6 no floating-point atomics; a row's softmax runs over key tiles of 32 in ascending order inside each of up to 8 key chunks (their
 *     number a function of the pair's live M alone), the chunks are merged in ascending order; the same input gives the same bits on every
 *     run, whatever the scratch held, alone or as pair k of a batch.
 * Parity with the reference is to a tolerance (torch's order of summation is unspecified): tests/test_gpu_pdsc.py.
 *
 * Weights: one flat fp32 device blob of lr_pdsc_weights_bytes(num_layers) bytes, 16-byte aligned, the caller's.  A block is { Wt[in][out] (the conv's
 * weight transposed), scale[out], offset[out] }; the blob is: layer0 (in 8: the 6 inputs and two zero rows, out 128); then per layer
 * PointCN (128, 128), q|k|v as one layer (128, 384; scale 1, offset = the biases), fc_message 0 (128, 64), 3 (64, 64), 6 (64, 128);
 * then the head: (128, 32), (32, 32), (32, 1).  With a BatchNorm behind the conv, scale = gamma / sqrt(var + eps) and
 * offset = (bias - mean) * scale + beta, folded in fp64 and rounded once; without, scale = 1 and offset = bias.                   */
typedef struct lr_pdsc_params {
    uint32_t struct_size;        /* = sizeof(lr_pdsc_params), checked like lr_ransac_params.struct_size                            */
    int32_t  num_layers;         /* 12 (config.py:34); 1..16                                                                        */
    double   sigma_d;            /* 1.2 for Lidar (the reference's sigma_spat); positive and finite                                 */
} lr_pdsc_params;

/* Written to device memory by lr_pdsc_encode / _batch (16 bytes). */
typedef struct lr_pdsc_result {
    int32_t  status;             /* 0 ok, 1 = no live correspondence                                                                */
    int32_t  m;                  /* live correspondence count the call ran on (m_dev clamped to 0..m)                               */
    int32_t  dead;               /* of those, correspondences with a non-finite coordinate                                          */
    int32_t  reserved;           /* 0                                                                                               */
} lr_pdsc_result;

/* Bytes of the weight blob (0 when num_layers is outside 1..16). */
LR_API size_t lr_pdsc_weights_bytes(int num_layers);
/* Caller-owned device scratch per pair for up to max_m correspondences (0 when max_m is outside 0..32768); linear in max_m. */
LR_API size_t lr_pdsc_scratch_bytes(int max_m);
/* m_dev, if not NULL, is a device int32 holding the live M (clamped to 0..m).  feat_out (nullable, float32 [m,128]) receives the
 * features, conf_out (nullable, float32 [m]) the logits; rows at and past the live count are written 0, dead rows 0 / -inf; with m = 0
 * nothing is stored.  scratch: >= lr_pdsc_scratch_bytes(m) bytes, 256-byte aligned, memory of the current device (checked, like the
 * stream: LR_EINVAL).  Every refusal (struct_size, num_layers / sigma_d out of range, a short or misaligned weight blob, short scratch, m > 32768) is
 * LR_EINVAL, before any launch.  No host synchronisation, no allocation.                                                           */
LR_API int lr_pdsc_encode(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, size_t weights_bytes,
                          const lr_pdsc_params *p, lr_pdsc_result *result, float *feat_out, float *conf_out, void *scratch,
                          size_t scratch_bytes, void *stream);
/* npairs (1..64) independent pairs under one set of weights in one sequence of launches (the pair is a grid dimension);
 * src/tgt/m/m_dev/feat_out/conf_out are HOST arrays of length npairs (m_dev, feat_out and conf_out, and their entries, may be NULL),
 * carried by value into a setup kernel; results is a DEVICE array of npairs blocks; scratch >= npairs * lr_pdsc_scratch_bytes(max m).
 * The result of pair k is bit-identical to lr_pdsc_encode on that pair.                                                            */
LR_API int lr_pdsc_encode_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                const float *weights, size_t weights_bytes, const lr_pdsc_params *p, lr_pdsc_result *results,
                                float *const *feat_out, float *const *conf_out, void *scratch, size_t scratch_bytes, void *stream);

/* ---- p2: PointDSC's tail: seeds, neural spectral matching, per-seed fits, hypothesis selection, post refinement ------------------
 * Replaces pick_seeds (Experiments/models/PointDSC.py:199-217), cal_seed_trans (:234-336), cal_leading_eigenvector (:338-358) and
 * post_refinement (:403-438) with rigid_transform_3d and knn of models/common.py:7-69, in inference mode, on the features and the
 * confidence lr_pdsc_encode returns.  Contract (restated in tests/pdsc_solve_cpu.py); m = m_dev clamped to 0..m:
 *  S1 a row is dead if E1 holds, if its conf is not finite or if its feature row holds a non-finite value; live = m - dead.  A dead row is
 *     never a seed, never a neighbour, never counted; its label is 0 (deviation: the reference propagates NaN).
 *  S2 local_max(i): for all live j, conf_i >= conf_j or |s_i - s_j| >= (float)nms_radius, the distance by E3's fp32 expression.
 *     key_i = conf_i if local_max(i), else 0 (the reference's scores * is_local_max: a maximum of negative score sorts BEHIND the zeros).
 *     Seeds: the first n_seeds live rows by descending key, ASCENDING INDEX ON EQUAL KEYS (the reference's argsort leaves ties open);
 *     n_seeds = (int)((double)live * ratio), and 0 when live < 2.  n_seeds = 0: status 2, the identity, labels 0 (the reference raises).
 *  S3 fn = f / max(|f|, 1e-12) in fp32 (F.normalize): |f| = sqrtf(t), t from p_l = f[2l] f[2l] + f[2l+1] f[2l+1], l = 0..63, by the
 *     butterfly p_l = p_l + p_(l^d), d = 32, 16, 8, 4, 2, 1 (every l ends with the same value).
 *  S4 per seed s: the k' = min(k, live - 1) live rows j != s of largest sim(s,j), by descending sim, ascending index on ties (deviation:
 *     the reference takes k + 1 and drops the first, assuming it is s itself).  sim(s,j) in fp32: acc = 0; for c = 0..63:
 *     acc = fmaf(fn_j[64+c], fn_s[64+c], fmaf(fn_j[c], fn_s[c], acc)) -- the chain of v_mfma_f32_32x32x2_f32.  No M x M or n_seeds x M
 *     matrix is stored.
 *  S5 per seed, over its neighbours a, b in S4's order, fp32: dot = fmaf chain of fn_a[c] fn_b[c] over c = 0..127 from 0;
 *     M_ab = fmaxf(0, fmaf(1 - dot, (float)(-1 / sigma^2), 1)) * compat_E3(a, b), M_aa = 0.
 *  S6 v = 1; num_iterations times (deviation: the reference leaves early when ALL seeds of the call pass allclose): u_a = fmaf chain of
 *     M_ab v_b over ascending b from 0; v = u / (sqrtf(B(u u)) + 1e-6f), B the butterfly of S3 over the lanes a (0 past k').  Then
 *     w = v / (B(v) + 1e-6f).
 *  S7 fit (rigid_transform_3d, its + 1e-6 kept): fp64 on the fp32 inputs, every sum from 0 in ascending order of a:
 *     W = sum w, ca = sum(w a) / (W + 1e-6), cb alike, H_xy = sum (w (a_x - ca_x)) (b_y - cb_y); R, t by lr_rt_from_cov (Horn's closed form
 *     of lr_kabsch).  A rank-deficient H still gives a proper rotation -- an eigenvector of the largest eigenvalue of Horn's matrix, from the
 *     Jacobi path; H = 0 gives R = I and t = cb - ca.
 *  S8 count_s = #{live j : sqrt(dx dx + dy dy + dz dz) < inlier_threshold}, fp64 without fused multiply-add, d = (((R_x0 s_x + R_x1 s_y) +
 *     R_x2 s_z) + t_x) - t_jx.  Best: the FIRST seed in seed order of largest count.  labels = that seed's inliers (final_labels).
 *  S9 refinement, on the device: T = T_best, previous = 0; up to refine_iters rounds: residuals d by S8's expression, inliers d <
 *     refine_threshold; their number equal to previous: stop; else previous = it, weights 1 / (1 + (d / refine_threshold)^2), S7's fit over
 *     the inliers with every sum in the fixed tree of E2.
 * S10 no floating-point atomics; the same input gives the same bits on every run, whatever the scratch held, alone or as pair k of a batch.
 * The kNN's work plan (seed blocks of 128 x up to 8 chunks of keys) is a function of n_seeds and m alone and changes no result.          */
typedef struct lr_pdsc_solve_params {
    uint32_t struct_size;        /* = sizeof(lr_pdsc_solve_params)                                                                  */
    int32_t  num_iterations;     /* 10 (PointDSC.py:94); 1..1000                                                                    */
    int32_t  k;                  /* 40; 1..64                                                                                       */
    int32_t  refine_iters;       /* 20 (:416-418); 0 = no refinement; 0..1000                                                       */
    double   ratio;              /* 0.1; (0, 1]                                                                                     */
    double   nms_radius;         /* 0.6 for Lidar; >= 0, finite                                                                     */
    double   inlier_threshold;   /* 0.6; positive and finite                                                                        */
    double   refine_threshold;   /* 1.2: what the reference hard-codes whenever its threshold is not 0.10 (:415-418)                */
    double   sigma_d;            /* 1.2 (sigma_spat); positive and finite                                                           */
    double   sigma;              /* 1.0: the state dict's learned `sigma`; positive and finite                                      */
} lr_pdsc_solve_params;

/* Written to device memory by lr_pdsc_solve / _batch / lr_pdsc_register / _batch (304 bytes). */
typedef struct lr_pdsc_solve_result {
    double   T[16];              /* src -> tgt, row-major, after the refinement                                                     */
    double   T_best[16];         /* the best seed's transform, before it                                                            */
    int32_t  status;             /* 0 ok, 1 = no live correspondence, 2 = no seed (T = T_best = the identity, labels 0)             */
    int32_t  m;                  /* m_dev clamped to 0..m                                                                           */
    int32_t  dead;               /* of those, dead rows (S1)                                                                        */
    int32_t  n_seeds;
    int32_t  best_rank;          /* position of the best seed in seed order, -1: none                                               */
    int32_t  best_index;         /* its row, -1: none                                                                               */
    int32_t  best_count;         /* its count (S8)                                                                                  */
    int32_t  n_labels;           /* labels set                                                                                      */
    int32_t  refine_rounds;      /* fits the refinement ran                                                                         */
    int32_t  reserved[3];        /* 0                                                                                               */
} lr_pdsc_solve_result;

/* Caller-owned device scratch per pair for up to max_m correspondences (0 when max_m is outside 0..32768). */
LR_API size_t lr_pdsc_solve_scratch_bytes(int max_m);
/* feat [m,128] and conf [m]: device float32, what lr_pdsc_encode wrote.  labels_out (nullable, uint8 [m]): S8's labels, 0 at and past the
 * live count.  seeds_out (nullable, int32 [(int)(m * ratio)]): the seeds in order, -1 at and past n_seeds.  Trace outputs of this entry
 * only, all nullable, rows at and past n_seeds not written: knn_out int32 [n_seeds][k] (S4's order, -1 past k'), weight_out float32
 * [n_seeds][k] (w of S6, 0 past k'), seedT_out float64 [n_seeds][16], count_out int32 [n_seeds].  Refusals: LR_EINVAL before any launch,
 * lr_last_error naming the argument (struct_size, a parameter out of range, null feat / conf with m > 0, and the front end's).  No host
 * synchronisation, no allocation: graph-capturable.                                                                                */
LR_API int lr_pdsc_solve(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *feat, const float *conf,
                         const lr_pdsc_solve_params *p, lr_pdsc_solve_result *result, uint8_t *labels_out, int32_t *seeds_out,
                         int32_t *knn_out, float *weight_out, double *seedT_out, int32_t *count_out, void *scratch, size_t scratch_bytes,
                         void *stream);
/* npairs (1..64) ragged pairs; the arrays are HOST arrays of length npairs (m_dev, labels_out, seeds_out and their entries may be NULL);
 * scratch >= npairs * lr_pdsc_solve_scratch_bytes(max m).  Pair k is bit-identical to lr_pdsc_solve on that pair.                   */
LR_API int lr_pdsc_solve_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                               const float *const *feat, const float *const *conf, const lr_pdsc_solve_params *p,
                               lr_pdsc_solve_result *results, uint8_t *const *labels_out, int32_t *const *seeds_out, void *scratch,
                               size_t scratch_bytes, void *stream);
/* Encode, then solve, in one call on one scratch of npairs * lr_pdsc_register_scratch_bytes(max m) bytes: bit-identical to lr_pdsc_encode
 * followed by lr_pdsc_solve.  feat_out / conf_out are nullable (the scratch holds them then).                                       */
LR_API size_t lr_pdsc_register_scratch_bytes(int max_m);
LR_API int lr_pdsc_register(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, size_t weights_bytes,
                            const lr_pdsc_params *ep, const lr_pdsc_solve_params *sp, lr_pdsc_solve_result *result, float *feat_out,
                            float *conf_out, uint8_t *labels_out, int32_t *seeds_out, void *scratch, size_t scratch_bytes, void *stream);
LR_API int lr_pdsc_register_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                  const float *weights, size_t weights_bytes, const lr_pdsc_params *ep, const lr_pdsc_solve_params *sp,
                                  lr_pdsc_solve_result *results, float *const *feat_out, float *const *conf_out, uint8_t *const *labels_out,
                                  int32_t *const *seeds_out, void *scratch, size_t scratch_bytes, void *stream);

/* ---- n1: the FCGF feature extractor: ResUNetBN2C(in_channels = 1, out_channels = 32, conv1_kernel_size 3 | 5, normalize_feature),
 * inference mode, D = 3, hyper-cube regions (Experiments/misc/fcgf.py:621-851, :864-867): what the reference runs on MinkowskiEngine
 * for every pair (Experiments/datasets/LidarFeatureExtractor.py:71-81, :166-181).  MinkowskiEngine is not part of the reference tree:
 * its convolution semantics are upstream-recalled; the one table that would change if a recalled convention were wrong is idx(o) of F2.
 * Contract (restated twice in tests/fcgf_cpu.py, once on torch's dense convolutions in tests/test_fcgf_cpu.py).
 * Input: coords [n,3] int32 integer voxel cells at tensor stride 1 (lr_voxel_dedup's `cells`), feat_in [n] float32 or NULL = all ones
 * (generic_balanced_loader.py:81), 0 <= n <= 2^20.  Output: feat_out [n,32] float32, row i for input row i, and lr_fcgf_result.
 *  F1  levels: level 0 = the input rows in input order.  Level l+1 = the distinct floor(c / 2^(l+1)) * 2^(l+1) over level l (floor
 *      division: -1 -> -2), its rows by ascending (x, y, z), lexicographic on the biased 21-bit fields of the packed key (cell + 2^20):
 *      independent of the input order and of the hash.  Three coarse levels.
 *  F2  stride-1 convolution, K = 2h+1, tensor stride t, output set = input set: out[u] = sum_o in[u + o t] W[idx(o)], o in {-h..h}^3,
 *      absent neighbours contribute nothing; W is [K^3, Cin, Cout] (MinkowskiEngine 0.5's `kernel`);
 *      idx(o) = (o_x+h) + K (o_y+h) + K^2 (o_z+h), x fastest [upstream-recalled].  1x1: in[u] W, the kernel [Cin,Cout] or [1,Cin,Cout].
 *  F3  stride-2 convolution (K = 3, level l -> l+1): out[v] = sum_o in[v + o t] W[idx(o)], t the input's tensor stride, v a level-(l+1) cell.
 *  F4  transposed stride-2 convolution (K = 3, level l+1 -> l) onto the EXISTING level-l set, the transpose of F3's map:
 *      out[u] = sum_{o : u - o t in level l+1} in[u - o t] W[idx(o)].
 *  F5  fp32 throughout; per output element ONE fmaf chain from +0 over ascending idx(o) and, inside an offset, ascending input channel;
 *      an absent neighbour is a zero operand or skipped (the same bits with finite weights).  v_mfma_f32_32x32x2_f32 is this chain bit
 *      for bit: the contract is bit-exact.  No floating-point atomics.
 *  F6  epilogue: y = fmaf(scale, acc, offset); then `+ residual` (one fp32 add) where the stage has one; then ReLU where it has one
 *      (y > 0 ? y : 0, a NaN stays).  BatchNorm (eps 1e-5) folded in fp64 and rounded once: scale = gamma / sqrt(var + eps),
 *      offset = (0 - mean) scale + beta; no BatchNorm: scale 1, offset = bias or 0.
 *  F7  stages (BN = fold, R = ReLU, +r = residual = the block's input): 1 conv1 BN (no ReLU: fcgf.py:801-803); 2-3 block1: BN R, BN +r R;
 *      4 / 7 / 10 conv2 / conv3 / conv4 (F3) BN, each followed by its block (5-6, 8-9, 11-12) as block1; 13 conv4_tr (F4) BN, 14-15
 *      block4_tr; 16 conv3_tr on cat(up, s4) BN, 17-18 block3_tr; 19 conv2_tr on cat(up, s2) BN, 20-21 block2_tr; 22 conv1_tr 1x1 on
 *      cat(up, s1), 96 -> 64, R, no BN; 23 final 1x1 64 -> 32 + bias.  cat puts the up path's channels first.  Channels 32 / 64 / 128 /
 *      256 down, 128 / 64 / 64 / 64 up.
 *  F8  s = fmaf chain of the 32 squares from 0 in ascending channel; out = f / (sqrtf(s) + 1e-8f), root and division correctly rounded.
 *  F9  a duplicate coordinate: status 2; |cell| >= 2^20 - 2 on an axis: status 3 (it wins over 2); either way feat_out's n rows are 0
 *      (a tap stores no rows: n_tap = 0).  A non-finite feat_in is carried.  n = 0: status 0, nothing stored but the result block.
 *  F10 the same input gives the same bits on every run whatever the scratch held; permuting the input rows permutes the output rows;
 *      adding a multiple of 8 to every cell of an axis changes no bit.
 *  F11 weights: one flat float32 device blob of lr_fcgf_weights_bytes(conv1_kernel_size) bytes, 16-byte aligned: per stage in F7's order
 *      { W[K^3][Cin][Cout], scale[Cout], offset[Cout] }.
 *  F12 refusals: LR_EINVAL before any launch, lr_last_error naming the argument: struct_size, conv1_kernel_size not 3 or 5, tap outside
 *      0..23, n outside 0..2^20, null / short / misaligned weights, null result / coords / feat_out, and the scratch, stream and device
 *      rules of every entry point with a caller-owned scratch.                                                                         */
typedef struct lr_fcgf_params {
    uint32_t struct_size;        /* = sizeof(lr_fcgf_params)                                                                        */
    int32_t  conv1_kernel_size;  /* 5 (LidarFeatureExtractor.py:75); 3 or 5                                                         */
    int32_t  tap;                /* 0: the network.  s = 1..23: stop behind stage s and store ITS activations [n_tap, Cout] in feat_out
                                    (which the caller sizes for n x 256) and its level's cells in tap_coords                        */
} lr_fcgf_params;

/* Written to device memory by lr_fcgf_extract (16 bytes). */
typedef struct lr_fcgf_result {
    int32_t  status;             /* 0 ok, 2 = duplicate coordinate, 3 = a cell at or past the range limit                           */
    int32_t  n;
    int32_t  n_tap;              /* rows stored in feat_out: n, or the rows of the tapped stage's level; 0 on status 2 / 3          */
    int32_t  reserved;           /* 0                                                                                               */
} lr_fcgf_result;

/* Bytes of the weight blob (0 when conv1_kernel_size is not 3 or 5). */
LR_API size_t lr_fcgf_weights_bytes(int conv1_kernel_size);
/* Caller-owned device scratch for up to max_n cells (0 when max_n is outside 0..2^20); a constant plus a multiple of max_n rounded up to 64. */
LR_API size_t lr_fcgf_scratch_bytes(int max_n);
/* tap_coords: nullable, int32 [n,3], written by a tap only.  scratch: >= lr_fcgf_scratch_bytes(n) bytes, 256-byte aligned, memory of the
 * current device (checked, like the stream).  No host synchronisation, no allocation.  It initialises its tables with three memsets of
 * a few bytes per cell and is NOT tested under graph capture: a caller who replays graphs uses lr_fcgf_extract_batch (n2), which is
 * kernel launches only and is.                                                                                   */
LR_API int lr_fcgf_extract(const int32_t *coords, const float *feat_in, int n, const float *weights, size_t weights_bytes,
                           const lr_fcgf_params *p, lr_fcgf_result *result, float *feat_out, int32_t *tap_coords, void *scratch,
                           size_t scratch_bytes, void *stream);

/* ---- n2: the FCGF feature extractor on up to 64 clouds in one call: one sequence of launches for all of them, as the reference batches
 * the two clouds of a pair into one sparse tensor (LidarFeatureExtractor.py:166-181).  coords / feat_in / n / feat_out are HOST arrays of
 * length nclouds, carried by value in a kernel-argument table (nothing the caller must keep alive); feat_in, and any entry of it, may be
 * NULL = ones.  The weight blob is n1's (F11).  DESIGN.md §18.7.
 *  B1  sizes: 1 <= nclouds <= 64; 0 <= n[b] <= 2^20; sum of n <= 2^20; p->tap must be 0 (a batch has no tap).
 *  B2  for every cloud b, feat_out[b] [n_b,32] and results[b] hold exactly the bytes lr_fcgf_extract writes for that cloud alone
 *      ({status, n = n_b, n_tap = status ? 0 : n_b, reserved = 0}), whatever else is in the batch, at whichever position, and whatever the
 *      scratch held.  The one deviation: the range limit is |cell| >= 2^18 - 2 on an axis (status 3), where n1's is 2^20 - 2: a cell's
 *      key carries its cloud (6 bits) next to three 19-bit fields.  n_b = 0: status 0, only the result block is written.
 *  B3  the status is per cloud.  A cloud with status 2 or 3 (3 wins, as in F9) has its n_b rows set to 0, takes no part in the maps and
 *      changes no bit of another cloud's output.  The same cell in two clouds is not a duplicate.
 *  B4  refusals: LR_EINVAL before any launch, lr_last_error naming the argument and, where it applies, the cloud: struct_size,
 *      conv1_kernel_size, tap != 0, nclouds outside 1..64, an n[b] outside its range or a sum above 2^20, a null coords[b] / feat_out[b]
 *      with n[b] > 0, null results, null / misaligned / short weights, and the scratch, stream and device rules of n1.
 *  B5  no host synchronisation, no allocation, graph-capturable; integer atomics only.                                                */
/* Caller-owned device scratch for nclouds clouds of total_n cells together (0 when nclouds is outside 1..64 or total_n outside 0..2^20). */
LR_API size_t lr_fcgf_batch_scratch_bytes(int nclouds, int total_n);
/* results: device, [nclouds].  scratch: >= lr_fcgf_batch_scratch_bytes(nclouds, sum of n) bytes, 256-byte aligned. */
LR_API int lr_fcgf_extract_batch(int nclouds, const int32_t *const *coords, const float *const *feat_in, const int32_t *n,
                                 const float *weights, size_t weights_bytes, const lr_fcgf_params *p, lr_fcgf_result *results,
                                 float *const *feat_out, void *scratch, size_t scratch_bytes, void *stream);
/* Bench hook, like lr_debug_fake_current_device not for production: one unsynchronised process-wide word.  stage = 1..23 makes every
 * later lr_fcgf_extract_batch of the process end behind that stage: it still returns LR_OK and writes the result blocks (status as
 * found), but stores NO features (1: the maps and conv1, what tools/fcgf_bench.py times for the maps / convolutions split of a batch,
 * which has no tap); 0 restores the contract.  Set it, time, and set it back with no other caller of the library running.         */
LR_API int lr_debug_fcgf_batch_stop_after(int stage);

/* ---- n3: Deep Global Registration's inlier network: ResUNetBN2C(in_channels = 1, out_channels = 1, conv1_kernel_size = 3,
 * normalize_feature = False, D = 6), inference mode, hyper-cube regions (DGR/config.py:81-83, DGR/core/deep_global_registration.py:
 * 140-149, DGR/model/resunet.py:419-665): one inlier logit per correspondence, a 6-D cell (cell of the point in cloud 0, cell of its
 * match in cloud 1; deep_global_registration.py:382).  The reference runs it on MinkowskiEngine; as for n1 the semantics are
 * upstream-recalled and the contract below is the specification (restated twice in tests/dgr6_cpu.py).
 * Input: coords [n,6] int32 cells at tensor stride 1, the feature of every row is 1 (inlier_feature_type 'ones'), 0 <= n <= 131072.
 * Output: logit_out [n] float32, row i for input row i, and lr_dgr_inlier_result.
 * The contract is F1 - F7, F9, F10 and F12 of n1 read in six dimensions (o in {-1,0,1}^6, three coarse levels, the same 23 stages), with:
 *  I1  offsets: K = 3 everywhere, conv1 included; idx(o) = sum_a (o_a + 1) 3^a, axis 0 fastest [upstream-recalled, as F2]; W is
 *      [729, Cin, Cout].
 *  I2  levels and keys: a coarse level's rows are in ascending lexicographic order of the six cells, axis 0 most significant,
 *      independent of the input order and of the hash.  Cells are taken relative to the call's origin, origin_a = 8 floor(min_a / 8)
 *      per axis (computed on the device), and packed into six 10-bit fields (cell - origin + 8).  Extent limit: cell_a - origin_a <= 1007
 *      on every axis, which admits every cloud whose extent max_a - min_a + 1 is at most 1001 cells on each axis (300 m at 0.3 m voxels)
 *      and, with min_a a multiple of 8, 1008 cells.  A wider extent: status 3; a duplicate 6-D coordinate: status 2; 3 wins over 2;
 *      either way logit_out's n entries are 0 (a tap stores no rows: n_tap = 0).  n = 0: status 0, only the result block is written.
 *      The origin is a multiple of 8, so F10 holds: adding a multiple of 8 to every cell of an axis changes no bit.
 *  I3  arithmetic: F5 unchanged: per output element ONE fp32 fmaf chain from +0 over ascending idx(o) and, inside an offset, ascending
 *      input channel; no floating-point atomics.
 *  I4  stages: F7's table with 729 offsets for stages 1 - 21 and the widths of I5; 22 conv1_tr 1x1 on cat(up, s1), T2 + C1 -> T1, ReLU,
 *      no BatchNorm; 23 final 1x1, T1 -> 1: one fmaf chain over the T1 channels from +0, then one add of the bias.  There is no F8: the
 *      output is the logit.  The sigmoid (deep_global_registration.py:390) is the caller's.
 *  I5  widths: C1 C2 C3 C4 (down) and T4 T3 T2 T1 (up), each a multiple of 32 in 32 .. 256; ResUNetBN2C is 32 64 128 256, 128 64 64 64.
 *      Weights: one flat float32 device blob of lr_dgr_inlier_weights_bytes(widths) bytes, 16-byte aligned, per stage in order
 *      { W[K^6][Cin][Cout], scale[Cout], offset[Cout] } (F6's fold; final: scale 1, offset = bias).
 * Refusals (F12): LR_EINVAL before any launch, lr_last_error naming the argument: struct_size, a width out of range, tap outside 0..23,
 * n outside 0..131072, null / short / misaligned weights, null result / coords / logit_out, and the scratch, stream and device rules. */
typedef struct lr_dgr_inlier_params {
    uint32_t struct_size;        /* = sizeof(lr_dgr_inlier_params)                                                                  */
    int32_t  tap;                /* 0: the network.  s = 1..23: stop behind stage s and store ITS activations [n_tap, Cout] in logit_out
                                    (which the caller sizes for n x the largest width) and its level's cells in tap_coords          */
    int32_t  widths[8];          /* I5: C1 C2 C3 C4 T4 T3 T2 T1                                                                     */
} lr_dgr_inlier_params;

/* Written to device memory by lr_dgr_inlier (16 bytes). */
typedef struct lr_dgr_inlier_result {
    int32_t  status;             /* 0 ok, 2 = duplicate coordinate, 3 = an axis wider than the extent limit                         */
    int32_t  n;
    int32_t  n_tap;              /* entries / rows stored in logit_out: n, or the rows of the tapped stage's level; 0 on status 2 / 3 */
    int32_t  reserved;           /* 0                                                                                               */
} lr_dgr_inlier_result;

/* Bytes of the weight blob (0 when a width is out of range or widths is null). */
LR_API size_t lr_dgr_inlier_weights_bytes(const int32_t widths[8]);
/* Caller-owned device scratch for up to max_n rows (0 when max_n is outside 0..131072 or a width is out of range): a constant plus a
 * multiple of max_n rounded up to 64; the ten dense gather tables [rows][729] are 29 160 bytes of it per row.                        */
LR_API size_t lr_dgr_inlier_scratch_bytes(int max_n, const int32_t widths[8]);
/* tap_coords: nullable, int32 [n,6], written by a tap only.  scratch: >= lr_dgr_inlier_scratch_bytes(n, p->widths) bytes, 256-byte
 * aligned, memory of the current device (checked, like the stream).  Kernel launches only: no host synchronisation, no allocation.   */
LR_API int lr_dgr_inlier(const int32_t *coords, int n, const float *weights, size_t weights_bytes, const lr_dgr_inlier_params *p,
                         lr_dgr_inlier_result *result, float *logit_out, int32_t *tap_coords, void *scratch, size_t scratch_bytes,
                         void *stream);

/* ---- n4: the inlier network on up to 8 pairs' correspondence sets in one call: one sequence of launches over the concatenated rows.
 * coords / n / logit_out are HOST arrays of length npairs, carried by value in a kernel-argument table (nothing the caller must keep
 * alive).  The weight blob and the params struct are n3's.  DESIGN.md §20.7.
 *  P1  sizes: 1 <= npairs <= 8; 0 <= n[k] <= 131072; sum of n <= 131072; p->tap must be 0 (a batch has no tap).  A cell's key carries its
 *      pair in bits 60 .. 62, above the six 10-bit fields; bit 63 stays clear (with a fourth tag bit, tag 15 and six fields of 1023 --
 *      a neighbour query -- would be the table's empty-slot word), hence 8 pairs.
 *  P2  for every pair k, logit_out[k] [n_k] and results[k] hold exactly the bytes lr_dgr_inlier writes for that pair alone ({status,
 *      n = n_k, n_tap = status ? 0 : n_k, reserved = 0}), whatever else is in the batch, at whichever position, and whatever the scratch
 *      held.  There is no deviation in the limits: every pair has its own origin 8 floor(min_a / 8) (six integer minima per pair on the
 *      device), so I2's extent limit of 1007 and F10 hold per pair, wherever each pair lies.  n_k = 0: status 0, only the result block is
 *      written.  (I3 fixes the chain of an output element by idx(o) and the channel, not by the order of the rows, and the tag makes
 *      every pair's maps its own.)
 *  P3  the status is per pair; 3 (extent) wins over 2 (duplicate).  A refused pair has its n_k logits set to 0, takes no part in the maps
 *      and changes no bit of another pair's output.  The same 6-D cell in two pairs is not a duplicate; no pair finds another's cell.
 *  P4  refusals: LR_EINVAL before any launch, lr_last_error naming the argument and, where it applies, the pair: struct_size, a width,
 *      tap != 0, npairs outside 1..8, an n[k] outside its range or a sum above 131072, null coords / n / logit_out / results, a null
 *      coords[k] / logit_out[k] with n[k] > 0, null / misaligned / short weights, and the scratch, stream and device rules of n3.
 *  P5  kernel launches only: no host synchronisation, no allocation, graph-capturable; integer atomics only.                          */
/* Caller-owned device scratch for npairs pairs of total_n rows together (0 when npairs is outside 1..8, total_n outside 0..131072 or a
 * width is out of range).                                                                                                          */
LR_API size_t lr_dgr_inlier_batch_scratch_bytes(int npairs, int total_n, const int32_t widths[8]);
/* results: device, [npairs].  scratch: >= lr_dgr_inlier_batch_scratch_bytes(npairs, sum of n, p->widths) bytes, 256-byte aligned. */
LR_API int lr_dgr_inlier_batch(int npairs, const int32_t *const *coords, const int32_t *n, const float *weights, size_t weights_bytes,
                               const lr_dgr_inlier_params *p, lr_dgr_inlier_result *results, float *const *logit_out,
                               void *scratch, size_t scratch_bytes, void *stream);

/* ---- d1: Deep Global Registration's robust pose refinement over M weighted correspondences src[i] <-> tgt[i] -----------------------
 * Replaces what DeepGlobalRegistration.register does once it has the inlier weights (DGR/core/deep_global_registration.py:403-435): the
 * weight-sum decision and GlobalRegistration (DGR/core/registration.py:16-64, :116-194) under HighDimSmoothL1Loss (DGR/core/loss.py:42-61):
 * up to 1000 Adam iterations over a 6-D rotation (a, b) and a translation t, the whole loop in one launch.  Contract (restated in
 * tests/dgr_cpu.py); m = m_dev clamped to 0..m; fp64 throughout, no fused multiply-add, only + - * / sqrt, products and dot
 * products associated as in f7 ((u0 v0 + u1 v1) + u2 v2; M v likewise):
 *  G1 row i < m is live iff its six coordinates and its weight are finite, w_i > 0 and w_i >= clip.  weights == NULL: every weight is 1.
 *     Live rows are compacted in index order; L = their number; w1 = S(w).
 *  G2 S: thread t of 1024 adds entries t, t + 1024, ... of the compacted list in ascending order from +0.0, then s[t] = s[t] + s[t + h]
 *     for h = 512 .. 1.
 *  G3 p = (a, b, t), nine numbers.  With T_init: its first two columns as they are (not re-orthonormalised) and its translation.
 *     Without: wn = w / (w1 + 2^-23); mom = { S(wn), S(wn X_a), S(wn Y_a), S((wn X_a) Y_b) }; T = lr_rt_from_moments(mom) of lr_contract.h;
 *     every entry rounded to float32 and widened (the reference's weighted_procrustes ends in .float()).
 *  G4 R(p) (ortho2rotation): x = a / max(|a|, 1e-8); n2 = max(x.x, 1e-8); c = (x.b) / n2; u = b - c x; y = u / max(|u|, 1e-8); z = x X y;
 *     R = [x y z] (columns).  max(v, 1e-8) = v < 1e-8 ? 1e-8 : v (a NaN stays one).
 *  G5 r = ((R X_i + t) - Y_i) / q, q = quantization_size; s = r.r; l_i = 0.5 s if s < 1, else 0.5 (sqrt(s + 2^-23) - 0.5); loss = S(w l) / w1.
 *  G6 g_i = (((k_i w_i) / w1) / q) r, k_i = 1 if s < 1, else 0.5 / sqrt(s + 2^-23); dt = S(g); G[a][b] = S(g[a] X[b]); then through G4 on
 *     one lane, with Gx, Gy, Gz the columns of G: Gx += y X Gz; Gy += Gz X x; du = (Gy - y (y.Gy)) / |u| (Gy / 1e-8 where |u| < 1e-8);
 *     dc = -(du.x); Gx -= c du; t1 = dc / n2; Gx += t1 b; db = du + t1 x; where x.x >= 1e-8: dn2 = -((dc (x.b)) / (n2 n2)), Gx += (2 dn2) x;
 *     da = (Gx - x (x.Gx)) / |a| (Gx / 1e-8 where |a| < 1e-8).  grad = (da, db, dt).
 *  G7 Adam, f7's B7 on the nine parameters: beta = (0.9, 0.999), eps = 1e-8, step size lr, and lr = lr gamma after every step.
 *  G8 for i = 0 .. max_iter - 1: evaluate loss and grad at p (log row i = p, loss); loss not finite: status 3, stop; loss < 1e-7: stop;
 *     the Adam step; a parameter not finite: status 3, stop; if |loss_prev - loss| < loss_prev ratio: break_count += 1 (cumulative, never
 *     reset) and stop once break_count >= max_break; loss_prev = loss.  loss_prev starts as iteration 0's loss, so iteration 0 counts
 *     whenever its loss and ratio are > 0.  iterations = i at the stop, max_iter - 1 without one; loss = the last evaluated;
 *     T = [R(p) t; 0 1] of the parameters after the last step (status 3: of the initial parameters).
 *  G9 status 1: L == 0; status 2: w1 < wsum_threshold (the caller's safeguard is due; DGR passes max(4000, m) clip, :407).  Both: the
 *     identity, nothing run, iterations = break_count = 0, loss = 0, log all +0.0.
 * G10 no floating-point atomics; the same input gives the same bits on every run, whatever the scratch held, alone or as pair k of a batch.
 * Deviations: parameters and moments are fp64 (the reference's are float32); non-finite rows and rows with w <= 0 are dead (the reference
 * propagates NaN and lets negative weights pull); the SVD failure of :428 cannot happen.                                             */
typedef struct lr_dgr_params {
    uint32_t struct_size;        /* = sizeof(lr_dgr_params)                                                                         */
    int32_t  max_iter;           /* 1000 (registration.py:138); 1..1000                                                             */
    int32_t  max_break;          /* 20 (max_break_count); >= 1                                                                      */
    int32_t  reserved;           /* 0                                                                                               */
    double   quantization_size;  /* q; DGR passes 2 * voxel_size (:419); positive and finite                                        */
    double   lr;                 /* 0.1 (:163); positive and finite                                                                 */
    double   gamma;              /* 0.999 (:164); (0, 1]                                                                            */
    double   ratio;              /* break_threshold_ratio: 1e-5, DGR passes 1e-4 (:418); >= 0, finite                               */
    double   clip;               /* clip_weight_thresh; >= 0, finite                                                                */
    double   wsum_threshold;     /* G9; >= 0, finite                                                                                */
} lr_dgr_params;

/* Written to device memory by lr_dgr_refine / _batch (160 bytes). */
typedef struct lr_dgr_result {
    double   T[16];              /* src -> tgt, row-major                                                                           */
    double   loss;               /* the last evaluated loss                                                                         */
    double   w1;                 /* S(w) over the live rows                                                                         */
    int32_t  iterations;         /* G8                                                                                              */
    int32_t  break_count;
    int32_t  L;                  /* live rows                                                                                       */
    int32_t  status;             /* 0 refined, 1 no live row, 2 w1 < wsum_threshold, 3 a non-finite loss or parameter               */
} lr_dgr_result;

/* Caller-owned device scratch per pair for up to max_m correspondences (0 when max_m is outside 0..32768). */
LR_API size_t lr_dgr_scratch_bytes(int max_m);
/* weights (nullable): device float32 [m].  T_init (nullable): device float64 [16], row-major 4x4.  log_out (nullable, this entry only):
 * device float64 [max_iter][10], row i = the nine parameters iteration i was evaluated at and its loss, rows past the last evaluated one
 * +0.0.  Refusals: LR_EINVAL before any launch, lr_last_error naming the argument (struct_size, a parameter out of range, m > 32768, and
 * the front end's).  No host synchronisation, no allocation: graph-capturable.                                                       */
LR_API int lr_dgr_refine(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, const double *T_init,
                         const lr_dgr_params *p, lr_dgr_result *result, double *log_out, void *scratch, size_t scratch_bytes, void *stream);
/* npairs (1..64) ragged pairs; the arrays are HOST arrays of length npairs (m_dev, weights, T_init and their entries may be NULL);
 * scratch >= npairs * lr_dgr_scratch_bytes(max m).  Pair k is bit-identical to lr_dgr_refine on that pair.                           */
LR_API int lr_dgr_refine_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                               const float *const *weights, const double *const *T_init, const lr_dgr_params *p, lr_dgr_result *results,
                               void *scratch, size_t scratch_bytes, void *stream);

/* ---- a1/a2 for descriptors of 33..128 numbers (FPFH's 33, matching.py:22-65 takes any width) -------
 * The same contract as lr_nn_top2, at the wider dim, bit for bit oracle/oracle.c's orc_nn_top2: norm and dot are fmaf chains over
 * k = 0..dim-1 from +0, d2 = fmaf(-2, dot, n0[i] + n1[j]), s = sqrtf(fmaxf(d2, 1e-30f)); ascending (s, j), the first minimal value wins
 * for the first and for the second neighbour; with n1 = 1 the second is -1 / inf (n1 = 0: the first too).  fmaxf drops a NaN, so a
 * non-finite row never puts a NaN into a comparison (its distances are 1e-15 or inf, as the oracle's).  A stand-alone entry point: it
 * takes no workspace, and the f16 filter path behind lr_nn_top2 stays 32 wide.  Exact f32 on v_mfma_f32_32x32x2_f32, no n0 x n1 matrix.
 * idx2 / s1 / s2 may be NULL.  Caller-owned device scratch, 256-byte aligned (lr_nn_wide_scratch_bytes: 0 when n0 or n1 is outside
 * 0..4194304 or dim outside 33..128); its content on entry does not matter.  Refusals: LR_EINVAL before any launch and before anything
 * is written, lr_last_error naming the argument -- dim 1..32 ("use lr_nn_top2"), dim > 128, n0 / n1 out of range, a null array, and the
 * scratch front end's.  No host synchronisation, no allocation: graph-capturable.                                                    */
LR_API size_t lr_nn_wide_scratch_bytes(int n0, int n1, int dim);
LR_API int lr_nn_wide(const float *F0, int n0, const float *F1, int n1, int dim, int32_t *idx1, int32_t *idx2, float *s1, float *s2,
                      void *scratch, size_t scratch_bytes, void *stream);

/* ---- FPFH descriptors (Experiments/demo_registration.py:37-44, datasets/KITTI.py:85-93, misc/cal_fpfh.py:22-26 -> Open3D 0.13
 * compute_fpfh_feature, not vendored: PARITY UNPINNED, the algorithm is upstream-recalled) -------------------------------------------
 * xyz, normals: device float64 [n,3]; out_f64 / out_f32: device [n,33], either may be NULL (not both); info: device int32 [4].
 * The contract -- fp64, every operation a single IEEE operation in the written order, no libm call beyond sqrt; tests/fpfh_cpu.py
 * restates it and the device equals it bit for bit; out_f32 is the cast of out_f64:
 *   F1 lists    per point its at most max_nn finite points of least (d2, index) with d2 <= fl(radius radius), in that order,
 *               d2 = ((qx-px)^2 + (qy-py)^2) + (qz-pz)^2 (lr_normals' rule); the point itself is among them.  Entry 0 is skipped (literally,
 *               as Open3D does -- with exact duplicates it may be the duplicate); k = len - 1; len <= 1: the row is all zeros.  A
 *               non-finite point has no list, is in no list and gets a zero row
 *   F2 pair     of (p1, n1), (p2, n2): d = p2 - p1, L = sqrt((dx dx + dy dy) + dz dz), a1 = ((n1x dx + n1y dy) + n1z dz) / L, a2 likewise
 *               with n2; if |a1| < |a2|: the normals swap, d = -d, f3 = -a2, else f3 = a1 (Open3D's acos(|a1|) > acos(|a2|) on the
 *               arguments); v = d x n1, |v| = sqrt(v.v), v = v / |v| per component; w = n1 x v; f2 = v.n2; y = w.n2, x = n1.n2 (dots and
 *               cross products in the form (a0 b0 + a1 b1) + a2 b2 and a1 b2 - a2 b1, ...).  L == 0 or |v| == 0: bins 5, 5, 5 (the
 *               features (0, 0, 0), still counted)
 *   F3 bins     angle: floor(11 (atan2(y, x) + pi) / (2 pi)) clamped to 0..10, decided without the angle: with (x', y') = (-x, -y) and
 *               the edge directions (c_e, s_e) = (cos, sin)(2 pi e / 11) as tabulated fp64 literals, e = 1..10: y < 0: #{ e <= 5 :
 *               c_e y' - s_e x' >= 0 }; y > 0: 5 + #{ e >= 6 : the same }; y = +0, x < 0: 10; y = -0, x < 0: 0; otherwise 5.
 *               f2, f3: #{ e in 1..10 : (11 (f + 1)) 0.5 >= e } (= the clamped floor)
 *   F4 SPFH     integer counts per bin (the list's entries 1.., three bins each, at 0.., 11.., 22..) times (100 / k): one multiplication
 *               (not Open3D's repeated +=: the order of the entries does not matter)
 *   F5 FPFH     F[j] = sum over the entries 1.. in list order of spfh[entry][j] / d2(entry), a serial chain per (point, j) from +0;
 *               entries with d2 == 0 are skipped; g = the sum of F over each 11-block in j order from +0;
 *               out[j] = F[j] (g != 0 ? 100 / g : 0) + spfh[self][j]
 *   F6 info     [0] 0 ok, 1 no finite point; [1] non-finite points; [2] zero rows (len <= 1, the non-finite ones included);
 *               [3] lists that are full (len == max_nn)
 * 2 <= max_nn <= 128, 0 <= n <= 4194304 (the grid's limit; all index arithmetic is size_t: n max_nn 4 passes 2^31), radius positive and
 * finite.  Caller-owned device scratch, 256-byte aligned (lr_fpfh_scratch_bytes: 0 outside those ranges); its content on entry does not
 * matter.  Refusals: LR_EINVAL before any launch, lr_last_error naming the argument.  Stages, each a kernel of its own: the 3-D grid of
 * lr_nn3 at cell radius (1 + 2^-16), the lists (built once into scratch), SPFH, FPFH.  No host synchronisation, no allocation, no
 * floating-point atomics: graph-capturable.  Not built: normals on the raw cloud averaged by the down-sampling (the demo's order), and
 * several clouds per call.                                                                                                           */
LR_API size_t lr_fpfh_scratch_bytes(int n, int max_nn);
LR_API int lr_fpfh(const double *xyz, const double *normals, int n, double radius, int max_nn, double *out_f64, float *out_f32,
                   int32_t *info, void *scratch, size_t scratch_bytes, void *stream);

/* ---- measurement hook for bench.py: duration of the last NN distance kernel(s) on this workspace,
 * from HIP events recorded on the launch stream.  Enable, run, synchronise, then read.            */
LR_API int lr_workspace_timing(lr_workspace *ws, int enable);
LR_API int lr_workspace_timing_read(lr_workspace *ws, float *nn_ms, float *ransac_ms, int *n_samples);
/* Stage times of the timed lr_register_pair / _batch calls since lr_workspace_timing(ws, 1), sums in ms over *n_samples calls
 * (read after synchronising the stream): out[0] whole call; out[1] forward NN = find_nn of matching.py:22-65 incl. the second
 * neighbour (norms + f16 copies, filter pass, exact verification); out[2] / out[3] the forward / reverse filter-pass launch;
 * out[4] hypothesis generation + scoring of the first RANSAC batch; out[5] the reverse NN (ordering, filter pass, exact
 * verification; 0 with --mode no_filter); out[6..7] reserved (0).  The registration time FR.py:117
 * bills -- filter + RANSAC + refit + the second neighbour's surcharge, matching.py:12-18 -- is out[0] - out[1] + that surcharge.  */
LR_API int lr_workspace_stage_times(lr_workspace *ws, float out[8], int *n_samples);

#ifdef __cplusplus
}
#endif
#endif /* LIDARREG_H */
