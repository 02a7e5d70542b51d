// The front end the correspondence-set back ends share (lr_teaser.hip, lr_sm.hip, lr_pdsc.hip, lr_pdsc_solve.hip, lr_dgr.hip; not part
// of the ABI): a batched call takes per-pair correspondence sets a[i] <-> b[i] with an optional live count on the device, nullable
// per-pair outputs and one caller-owned scratch of npairs arenas.  What differs between the back ends is their params, their arena
// layout and their kernels; the device section holds what those kernels read of a pair in the same way: the live count, a row with its
// finiteness, and the length difference d(i,j) of the compatibility measures (SM's c, PointDSC's E3).  The align and arena
// pointer helpers, the refusal macro and the scratch checks are those of every caller-owned scratch (lr_scratch.h).
#pragma once
#include "lr_scratch.h"
#include <float.h>

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
// row i of a pair, r = (a_i, b_i); true iff all six are finite (false for NaN and inf).  A back end's further conditions (a weight, a
// confidence, a feature) stay at its call site.
__device__ __forceinline__ bool cs_load_row(const float *a, const float *b, int i, float (&r)[6])
{
    a += (size_t)3 * i; b += (size_t)3 * i;
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = b[0]; r[4] = b[1]; r[5] = b[2];
    bool ok = true;
    for (int k = 0; k < 6; ++k) ok = ok && fabsf(r[k]) <= FLT_MAX;
    return ok;
}
// d = |a_i - a_j| - |b_i - b_j| of the row p = (a_i, b_i) and another one's six scalars, in the contracts' fp32 order: direct
// differences, (dx dx + dy dy) + dz dz, two correctly rounded square roots, then the subtraction (-ffp-contract=off: nothing is fused)
__device__ __forceinline__ float cs_len_diff(const float (&p)[6], float a0, float a1, float a2, float b0, float b1, float b2)
{
    const float ax = p[0] - a0, ay = p[1] - a1, az = p[2] - a2, bx = p[3] - b0, by = p[4] - b1, bz = p[5] - b2;
    const float la = sqrtf((ax * ax + ay * ay) + az * az), lb = sqrtf((bx * bx + by * by) + bz * bz);
    return la - lb;
}
// PointDSC's E3 for one (query, key): max(0, 1 + nk d^2), nk = (float)(-1 / sigma_d^2)
__device__ __forceinline__ float cs_compat(const float (&p)[6], float a0, float a1, float a2, float b0, float b1, float b2, float nk)
{
    const float d = cs_len_diff(p, a0, a1, a2, b0, b1, b2);
    return fmaxf(0.0f, fmaf(d * d, nk, 1.0f));
}
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
