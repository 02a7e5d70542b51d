// lr_dgr_inlier: Deep Global Registration's inlier network (ResUNetBN2C(1, 1, conv1_kernel_size 3, D = 6): a sparse 6-D ResUNet of 23
// convolutions with 3^6 = 729 offsets each) on integer 6-D cells, one logit per correspondence.
// Contract n3 (F1 .. F7, F9, F10, F12 in six dimensions with I1 .. I5) of include/lidarreg.h; DESIGN.md §20.
//
// Keys.  A cell is taken relative to the call's origin 8 floor(min_a / 8) per axis (an integer min-reduction on the device) and packed
// into six 10-bit fields, field_a = (c_a - origin_a) + 8, axis 0 most significant: ascending keys are ascending lexicographic cells and
// the +8 leaves room for the -8 neighbour of level 3.  Level 0 is kept in input order.
// The maps (dense gather tables [rows][729], one thread per entry), the gather convolution sp_conv_kernel (its streamed table form), the
// stage table, the scratch layout and the stage schedule are lr_sparse.h's.  Here: the origin and the key of a row, conv1 (Cin = 1, ones)
// and final (Cout = 1), which are vector kernels, and the entry point.  The batched entry (lr_dgr_inlier_batch, contract n4) is
// lr_dgr6_batch.h, included at the end.
#include "lr_scratch.h"
#include "lr_sparse.h"

#define D6_MAX_N 131072
#define D6_NK 729
#define D6_BIAS 8                    // field = (cell - origin) + 8
#define D6_REL_MAX 1007              // cell - origin above this on an axis: status 3 (field + 8 <= 1023)
#define D6_CTL_BYTES 256
typedef sp_codec<6, 10> d6_codec;

static_assert(sizeof(sp_ctl) <= D6_CTL_BYTES, "sp_ctl outgrew its place at the head of the scratch");

// widths = C1 C2 C3 C4 (down) T4 T3 T2 T1 (up); each a multiple of 32 in 32 .. 256 (I5)
static inline bool d6_widths_ok(const int32_t *w)
{
    if (!w) return false;
    for (int i = 0; i < 8; ++i) if (w[i] < 32 || w[i] > 256 || (w[i] & 31)) return false;
    return true;
}
static sp_layout d6_make_layout(size_t max_n, const int32_t *w) { return sp_make_layout(max_n, D6_NK, 0, w, D6_CTL_BYTES, false); }

// ---- maps -------------------------------------------------------------------------------------------------------------------------
// the key of input row i, LR_CELL_EMPTY when an axis lies past the extent limit
struct d6_row_key {
    const int32_t *coords;
    __device__ fc_u64 operator()(int i, const sp_ctl *ctl) const
    {
        fc_u64 key = 0;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const long long rel = (long long)coords[6 * (size_t)i + a] - (long long)sp_origin(ctl, a);      // >= 0: the origin is below the minimum
            ok = ok && rel <= D6_REL_MAX;
            key = (key << 10) | ((fc_u64)(rel + D6_BIAS) & d6_codec::FIELD);
        }
        return ok ? key : LR_CELL_EMPTY;
    }
};
__global__ void __launch_bounds__(256) d6_min_kernel(const int32_t *__restrict__ coords, int n, sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        int v = i < n ? coords[6 * (size_t)i + a] : INT_MAX;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d); v = o < v ? o : v; }
        if ((threadIdx.x & 63) == 0 && v != INT_MAX) atomicMin(&ctl->mn[a], v);
    }
}

// ---- convolutions -------------------------------------------------------------------------------------------------------------------
// conv1: Cin = 1 with the feature ones: a vector kernel over the row's 729 entries; BatchNorm folded, no ReLU
__global__ void __launch_bounds__(256) d6_conv1_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ W, const float *__restrict__ scale,
                                                       const float *__restrict__ offset, int cout, float *__restrict__ out, const sp_ctl *ctl)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(gid / cout), c = (int)(gid - (size_t)r * cout);
    if (ctl->status || r >= ctl->n[0]) return;
    const int32_t *row = nbr + (size_t)r * D6_NK;
    float acc = 0.0f;
    for (int k = 0; k < D6_NK; ++k)
        if (row[k] >= 0) acc = fmaf(1.0f, W[(size_t)k * cout + c], acc);
    out[gid] = fmaf(scale[c], acc, offset[c]);
}

// final (I4): Cout = 1: one fmaf chain over the row's channels from +0, then one add of the bias
__global__ void __launch_bounds__(256) d6_final_kernel(const float *__restrict__ x, int cin, const float *__restrict__ W, float *__restrict__ out, const sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || i >= ctl->n[0]) return;
    const float *row = x + (size_t)i * cin;
    float acc = 0.0f;
    for (int c = 0; c < cin; c += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c);
        acc = fmaf(v.x, W[c], acc); acc = fmaf(v.y, W[c + 1], acc); acc = fmaf(v.z, W[c + 2], acc); acc = fmaf(v.w, W[c + 3], acc);
    }
    out[i] = acc + W[cin + 1];                                         // { W[cin], scale = 1, offset = bias }
}
// the logits and the result block of a whole-network call; a refused input (status 2, 3) leaves zeros
__global__ void __launch_bounds__(256) d6_finish_kernel(const float *__restrict__ f, int n, float *__restrict__ out, const sp_ctl *ctl, lr_dgr_inlier_result *res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int status = ctl->status;
    if (i == 0) { res->status = status; res->n = n; res->n_tap = status ? 0 : n; res->reserved = 0; }
    if (i < n) out[i] = status ? 0.0f : f[i];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_dgr_inlier_params) == 40 && sizeof(lr_dgr_inlier_result) == 16, "ABI structs changed: update include/lidarreg.h and _ext.py together");

extern "C" size_t lr_dgr_inlier_weights_bytes(const int32_t *widths)
{
    if (!d6_widths_ok(widths)) return 0;
    return sp_weights_bytes(widths, D6_NK, D6_NK, 1);
}

extern "C" size_t lr_dgr_inlier_scratch_bytes(int max_n, const int32_t *widths)
{
    if (max_n < 0 || max_n > D6_MAX_N || !d6_widths_ok(widths)) return 0;
    return d6_make_layout((size_t)max_n, widths).total;
}

extern "C" int lr_dgr_inlier(const int32_t *coords, int n, const float *weights, size_t weights_bytes, const lr_dgr_inlier_params *p,
                             lr_dgr_inlier_result *result, float *logit_out, int32_t *tap_coords, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_dgr_inlier";
    LR_CHECK_STRUCT_SIZE(lr_dgr_inlier_params, p, who);
    LR_REFUSE_UNLESS(d6_widths_ok(p->widths), LR_EINVAL, "every width must be a multiple of 32 in 32 .. 256");
    LR_REFUSE_UNLESS(p->tap >= 0 && p->tap <= SP_STAGES, LR_EINVAL, "tap must lie in 0 .. 23");
    LR_REFUSE_UNLESS(n >= 0 && n <= D6_MAX_N, LR_EINVAL, "n must lie in 0 .. 131072");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_dgr_inlier_weights_bytes(p->widths), LR_EINVAL, "weights_bytes is below lr_dgr_inlier_weights_bytes(widths)");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    LR_REFUSE_UNLESS(n == 0 || (coords && logit_out), LR_EINVAL, "null coords or logit_out");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_dgr_inlier_scratch_bytes(n, p->widths), "lr_dgr_inlier_scratch_bytes(n, widths)", LR_EINVAL,
                                stream, nullptr));

    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(sp_empty_kernel<lr_dgr_inlier_result>, dim3(1), dim3(1), 0, st, result);
        LR_LAUNCH_CHECK();
        return LR_OK;
    }
    const int32_t *wd = p->widths;
    sp_run<SP_STREAMED> R;
    sp_stage_table(wd, D6_NK, D6_NK, 1, R.t);
    R.carve(scratch, d6_make_layout((size_t)n, wd), n, weights, st);
    const sp_layout &L = R.L;
    sp_ctl *ctl = R.ctl;
    const int gn = R.grid((size_t)n), C1 = wd[0];

    // maps (level 0 in input order)
    sp_init_launch(R.keys[0], R.val[0], 4 * L.cap_max, ctl, D6_CTL_BYTES, st);
    hipLaunchKernelGGL(d6_min_kernel, dim3(gn), dim3(256), 0, st, coords, n, ctl);
    hipLaunchKernelGGL(sp_l0_insert_kernel<d6_row_key>, dim3(gn), dim3(256), 0, st, d6_row_key{ coords }, n, R.keys[0], R.val[0], R.mask, R.rowkey[0], ctl);
    hipLaunchKernelGGL(sp_l0_check_kernel, dim3(gn), dim3(256), 0, st, R.rowkey[0], n, R.keys[0], R.val[0], R.mask, ctl);
    sp_maps<d6_codec, 0>(R);

    // a tap ends the call behind its stage
    const int tap = p->tap;
    const bool end = sp_stages(R, wd,
        [&](float *X) {
            hipLaunchKernelGGL(d6_conv1_kernel, dim3(R.grid((size_t)n * C1)), dim3(256), 0, st, R.nbr[0], R.w[1], R.w[1] + (size_t)D6_NK * C1,
                               R.w[1] + (size_t)D6_NK * C1 + C1, C1, X, ctl);
        },
        [&](const float *X, float *Y) { hipLaunchKernelGGL(d6_final_kernel, dim3(gn), dim3(256), 0, st, X, wd[7], R.w[23], Y, ctl); },
        [&](int s, const float *buf, int lvl) -> bool {
            if (tap != s) return false;
            const int cout = R.t[s].cout;
            const size_t items = (size_t)n * (cout > 6 ? cout : 6);
            hipLaunchKernelGGL((sp_tap_kernel<d6_codec, lr_dgr_inlier_result>), dim3(R.grid(items)), dim3(256), 0, st, buf, cout, lvl, R.rowkey[lvl], n, logit_out,
                               tap_coords, D6_BIAS, ctl, result);
            return true;
        });
    if (!end) hipLaunchKernelGGL(d6_finish_kernel, dim3(gn), dim3(256), 0, st, R.Y, n, logit_out, ctl, result);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

#include "lr_dgr6_batch.h"
