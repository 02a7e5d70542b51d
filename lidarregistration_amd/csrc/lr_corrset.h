// The front end the correspondence-set solvers share (lr_teaser.hip, lr_sm.hip; not part of the ABI): a batched call takes per-pair
// correspondence sets a[i] <-> b[i] with an optional live count on the device, nullable per-pair outputs and one caller-owned scratch
// of npairs arenas.  What differs between the back ends is their params, their arena layout and their kernels.
#pragma once
#include "lr_internal.h"

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

static inline size_t cs_al(size_t x) { return (x + 255) & ~size_t(255); }
#ifdef __HIPCC__
// the pair's live count: m_dev clamped to 0..m
__device__ __forceinline__ int cs_live_m(const cs_desc &d) { const int v = d.m_dev ? *d.m_dev : d.m; return v < 0 ? 0 : (v < d.m ? v : d.m); }
// byte `off` of pair `pair`'s arena; A = the back end's kernel arguments { char *base; size_t stride; ... }
template <typename T, typename A> __device__ __forceinline__ T *cs_ptr(const A &g, int pair, size_t off) { return reinterpret_cast<T *>(g.base + (size_t)pair * g.stride + off); }
#endif

// What the front needs to know of a back end: its batched entry point and *_scratch_bytes (by name, for the messages), and what a short
// scratch and m > CS_MAX_M return (include/lidarreg.h documents it per back end: TEASER LR_ESIZE, SM LR_EINVAL)
struct cs_backend { const char *who, *scratch_fn; size_t (*scratch_bytes)(int); int size_code; };
struct cs_front {
    cs_desc_table t;                 // the call's pairs, zero entries behind them
    int mx, n_cus;                   // largest m of the call; compute units of the device the scratch lives on
    size_t per;                      // bytes per arena: scratch_bytes(mx)
};

#define CS_REQUIRE(cond, code, msg) do { if (!(cond)) { lr_set_error("%s: " msg, be.who); return code; } } while (0)
// The checks of a batched call, after the back end's own params check and before any launch.  The last one is the device rule of
// every entry point: the scratch is memory of the current device, a gfx950, and the stream belongs to it.
static inline int cs_check_batch(const cs_backend &be, int npairs, const float *const *src, const float *const *tgt, const int32_t *m,
                                 const int32_t *const *m_dev, void *const *out0, void *const *out1, const void *results,
                                 void *scratch, size_t scratch_bytes, void *stream, cs_front *f)
{
    CS_REQUIRE(npairs >= 1 && npairs <= LR_MAX_BATCH, LR_EINVAL, "npairs must lie in 1..64");
    CS_REQUIRE(src && tgt && m && results && scratch, LR_EINVAL, "null pointer");
    f->mx = 0;
    for (int k = 0; k < npairs; ++k) {
        CS_REQUIRE(m[k] >= 0, LR_EINVAL, "negative correspondence count");
        CS_REQUIRE(m[k] <= CS_MAX_M, be.size_code, "more than 32768 correspondences");
        CS_REQUIRE(m[k] == 0 || (src[k] && tgt[k]), LR_EINVAL, "null point array");
        f->t.d[k] = cs_desc{ src[k], tgt[k], m_dev ? m_dev[k] : nullptr, out0 ? out0[k] : nullptr, out1 ? out1[k] : nullptr, m[k], 0 };
        f->mx = m[k] > f->mx ? m[k] : f->mx;
    }
    for (int k = npairs; k < LR_MAX_BATCH; ++k) f->t.d[k] = cs_desc{ nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0 };
    f->per = be.scratch_bytes(f->mx);
    if (scratch_bytes < f->per * (size_t)npairs) { lr_set_error("%s: scratch too small (npairs * %s(max m))", be.who, be.scratch_fn); return be.size_code; }
    CS_REQUIRE(((uintptr_t)scratch & 255) == 0, LR_EINVAL, "scratch must be 256-byte aligned");
    return lr_check_memory_device(scratch, (hipStream_t)stream, be.who, &f->n_cus);
}
