// What an entry point with a caller-owned scratch needs (not part of the ABI): the 256-byte rounding its layout is summed with, the pointer
// into a pair's arena, the refusal macro and the scratch check.  lr_corrset.h and lr_nn3.h include it.  lr_voxel_dedup stays outside:
// it returns LR_ESIZE, checks no alignment and takes no scratch at n = 0.
#pragma once
#include "lr_internal.h"

static inline size_t lr_al(size_t x) { return (x + 255) & ~size_t(255); }
#ifdef __HIPCC__
// byte `off` of pair `pair`'s arena; A = the kernel arguments { char *base; size_t stride; ... }
template <typename T, typename A> __device__ __forceinline__ T *lr_ptr(const A &g, int pair, size_t off) { return reinterpret_cast<T *>(g.base + (size_t)pair * g.stride + off); }
#endif

// refuses the call in the name of the `who` in scope
#define LR_REFUSE_UNLESS(cond, code, msg) do { if (!(cond)) { lr_set_error("%s: " msg, who); return code; } } while (0)

// The scratch checks, last of an entry point's checks and before any launch: `need` bytes (size_fn_text names the call that gives them;
// a short scratch returns size_code), 256-byte aligned, and the device rule of every entry point: the scratch is memory of the current
// device, a gfx950, and the stream belongs to it.  n_cus (nullable): its compute units.
static inline int lr_check_scratch(const char *who, void *scratch, size_t scratch_bytes, size_t need, const char *size_fn_text, int size_code,
                                   void *stream, int *n_cus)
{
    LR_REFUSE_UNLESS(scratch, LR_EINVAL, "null scratch");
    if (scratch_bytes < need) { lr_set_error("%s: scratch too small (%s)", who, size_fn_text); return size_code; }
    LR_REFUSE_UNLESS(((uintptr_t)scratch & 255) == 0, LR_EINVAL, "scratch must be 256-byte aligned");
    return lr_check_memory_device(scratch, (hipStream_t)stream, who, n_cus);
}
