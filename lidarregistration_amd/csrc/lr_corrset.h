// The front end the correspondence-set solvers share (lr_teaser.hip, lr_sm.hip; not part of the ABI): a batched call takes per-pair
// correspondence sets a[i] <-> b[i] with an optional live count on the device, nullable per-pair outputs and one caller-owned scratch
// of npairs arenas.  What differs between the back ends is their params, their arena layout and their kernels.  The align and arena
// pointer helpers, the refusal macro and the scratch checks are those of every caller-owned scratch (lr_scratch.h).
#pragma once
#include "lr_scratch.h"

#define CS_MAX_M 32768               // correspondences per pair
// One pair of a batched call.  The table travels BY VALUE into the back end's setup kernel (no host copy, graph-capturable):
// 64 entries of 48 bytes, next to the back end's own arguments, stay below the 4 KB kernel-argument limit.
struct cs_desc {
    const float *a, *b;
    const int32_t *m_dev;
    void *out0, *out1;               // nullable outputs (TEASER: clique, none; SM: eigenvector, labels)
    int32_t m, pad;
};
struct cs_desc_table { cs_desc d[LR_MAX_BATCH]; };
static_assert(sizeof(cs_desc_table) + 256 <= 4096, "the descriptor table no longer fits the kernel arguments");

#ifdef __HIPCC__
// the pair's live count: m_dev clamped to 0..m
__device__ __forceinline__ int cs_live_m(const cs_desc &d) { const int v = d.m_dev ? *d.m_dev : d.m; return v < 0 ? 0 : (v < d.m ? v : d.m); }
#endif

// What the front needs to know of a back end: its batched entry point by name, what the call's scratch takes as the messages word it
// ("npairs * lr_x_scratch_bytes(max m)"), its *_scratch_bytes, and what a short scratch and m > CS_MAX_M return (include/lidarreg.h
// documents it per back end: TEASER LR_ESIZE, SM LR_EINVAL)
struct cs_backend { const char *who, *scratch_fn; size_t (*scratch_bytes)(int); int size_code; };
struct cs_front {
    cs_desc_table t;                 // the call's pairs, zero entries behind them
    int mx, n_cus;                   // largest m of the call; compute units of the device the scratch lives on
    size_t per;                      // bytes per arena: scratch_bytes(mx)
};

// The checks of a batched call, after the back end's own params check and before any launch; the scratch's (lr_check_scratch) come last.
static inline int cs_check_batch(const cs_backend &be, int npairs, const float *const *src, const float *const *tgt, const int32_t *m,
                                 const int32_t *const *m_dev, void *const *out0, void *const *out1, const void *results,
                                 void *scratch, size_t scratch_bytes, void *stream, cs_front *f)
{
    const char *who = be.who;
    LR_REFUSE_UNLESS(npairs >= 1 && npairs <= LR_MAX_BATCH, LR_EINVAL, "npairs must lie in 1..64");
    LR_REFUSE_UNLESS(src && tgt && m && results && scratch, LR_EINVAL, "null pointer");
    f->mx = 0;
    for (int k = 0; k < npairs; ++k) {
        LR_REFUSE_UNLESS(m[k] >= 0, LR_EINVAL, "negative correspondence count");
        LR_REFUSE_UNLESS(m[k] <= CS_MAX_M, be.size_code, "more than 32768 correspondences");
        LR_REFUSE_UNLESS(m[k] == 0 || (src[k] && tgt[k]), LR_EINVAL, "null point array");
        f->t.d[k] = cs_desc{ src[k], tgt[k], m_dev ? m_dev[k] : nullptr, out0 ? out0[k] : nullptr, out1 ? out1[k] : nullptr, m[k], 0 };
        f->mx = m[k] > f->mx ? m[k] : f->mx;
    }
    for (int k = npairs; k < LR_MAX_BATCH; ++k) f->t.d[k] = cs_desc{ nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0 };
    f->per = be.scratch_bytes(f->mx);
    return lr_check_scratch(who, scratch, scratch_bytes, f->per * (size_t)npairs, be.scratch_fn, be.size_code, stream, &f->n_cus);
}
