// lr_fcgf_extract: the FCGF feature extractor (ResUNetBN2C, a sparse 3-D ResUNet of 23 convolutions) on integer voxel cells.
// Contract n1 (F1 .. F12) of include/lidarreg.h; DESIGN.md §18.
//
// The maps, the gather convolution sp_conv_kernel (its LDS-cached table form: 27 offsets), the stage table, the scratch layout and the
// stage schedule are lr_sparse.h's, at the widths FC_WIDTHS with 27 offsets per table and, for conv1_kernel_size 5, an eleventh table
// [n][125] at level 0.  Here: the key of a cell (the layout of lr_cells_pack, bias 2^20; level 0 is kept in input order), conv1 (Cin = 1, a
// vector kernel), F8 and the entry point.
#include "lr_scratch.h"
#include "lr_sparse.h"

#define FC_MAX_N (1 << 20)
#define FC_BIAS (1 << 20)            // cell + bias is the 21-bit field of lr_cells_pack
#define FC_LIMIT ((1 << 20) - 2)     // |cell| >= this: status 3
static const int32_t FC_WIDTHS[8] = { 32, 64, 128, 256, 128, 64, 64, 64 };
typedef sp_codec<3, 21> fc_codec;
typedef sp_run<SP_CACHED> fc_run;

static sp_layout fc_make_layout(size_t max_n, size_t ctl_bytes = 256) { return sp_make_layout(max_n, 27, 125, FC_WIDTHS, ctl_bytes, true); }

// ---- maps -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool fc_in_range(int v) { return v > -FC_LIMIT && v < FC_LIMIT; }
struct fc_row_key {
    const int32_t *coords;
    __device__ fc_u64 operator()(int i, const sp_ctl *) const
    {
        const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
        if (!(fc_in_range(x) && fc_in_range(y) && fc_in_range(z))) return LR_CELL_EMPTY;
        return lr_cells_pack((fc_u64)(x + FC_BIAS), (fc_u64)(y + FC_BIAS), (fc_u64)(z + FC_BIAS));
    }
};

// ---- convolutions -------------------------------------------------------------------------------------------------------------------
// conv1: Cin = 1, 32 outputs, K^3 = 27 or 125 offsets; BatchNorm folded, no ReLU
__global__ void __launch_bounds__(256) fc_conv1_kernel(const float *__restrict__ feat_in, const int32_t *__restrict__ nbr, int nk, const float *__restrict__ W,
                                                       const float *__restrict__ scale, const float *__restrict__ offset, float *__restrict__ out, const sp_ctl *ctl)
{
    __shared__ float sW[125 * 32];
    for (int e = threadIdx.x; e < nk * 32; e += 256) sW[e] = W[e];
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(gid >> 5), c = (int)(gid & 31);
    if (ctl->status || r >= ctl->n[0]) return;
    float acc = 0.0f;
    for (int k = 0; k < nk; ++k) {
        const int idx = nbr[(size_t)r * nk + k];
        if (idx >= 0) acc = fmaf(feat_in ? feat_in[idx] : 1.0f, sW[k * 32 + c], acc);
    }
    out[(size_t)r * 32 + c] = fmaf(scale[c], acc, offset[c]);
}

// F8 and the result block of a whole-network call; a refused input (status 2, 3) leaves rows of zeros
__global__ void __launch_bounds__(256) fc_norm_kernel(const float *__restrict__ f, int n, float *__restrict__ out, const sp_ctl *ctl, lr_fcgf_result *res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int status = ctl->status;
    if (i == 0) { res->status = status; res->n = n; res->n_tap = status ? 0 : n; res->reserved = 0; }
    if (i >= n) return;
    float v[32], s = 0.0f;
#pragma unroll
    for (int c = 0; c < 32; ++c) { v[c] = status ? 0.0f : f[(size_t)i * 32 + c]; s = fmaf(v[c], v[c], s); }
    const float d = sqrtf(s) + 1e-8f;
#pragma unroll
    for (int c = 0; c < 32; ++c) out[(size_t)i * 32 + c] = status ? 0.0f : v[c] / d;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_fcgf_params) == 12 && sizeof(lr_fcgf_result) == 16, "ABI structs changed: update include/lidarreg.h and _ext.py together");

extern "C" size_t lr_fcgf_weights_bytes(int conv1_kernel_size)
{
    if (conv1_kernel_size != 3 && conv1_kernel_size != 5) return 0;
    return sp_weights_bytes(FC_WIDTHS, sp_ipow(conv1_kernel_size, 3), 27, 32);
}

extern "C" size_t lr_fcgf_scratch_bytes(int max_n)
{
    if (max_n < 0 || max_n > FC_MAX_N) return 0;
    return fc_make_layout((size_t)max_n).total;
}

// What the two entry points do alike: the stage table with the pointers into the scratch and the blob, the maps behind level 0,
// conv1's gather table, and the stages with F7's last one
static void fc_carve(fc_run &R, void *scratch, const sp_layout &L, int n, int K1, const float *weights, hipStream_t st)
{
    sp_stage_table(FC_WIDTHS, K1 * K1 * K1, 27, 32, R.t);
    R.carve(scratch, L, n, weights, st);
}
template <class C> static void fc_maps(const fc_run &R, int K1) { if (K1 == 5) sp_maps<C, 5>(R); else sp_maps<C, 0>(R); }
static const int32_t *fc_conv1_table(const fc_run &R, int K1) { return K1 == 5 ? R.extra : R.nbr[0]; }
template <typename Conv1, typename Done> static bool fc_stages(const fc_run &R, Conv1 conv1, Done done)
{
    return sp_stages(R, FC_WIDTHS, conv1, [&](const float *X, float *Y) { R.conv(23, X, 64, nullptr, 0, nullptr, nullptr, Y, 0, 0); }, done);
}

extern "C" int lr_fcgf_extract(const int32_t *coords, const float *feat_in, int n, const float *weights, size_t weights_bytes, const lr_fcgf_params *p,
                               lr_fcgf_result *result, float *feat_out, int32_t *tap_coords, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_fcgf_extract";
    LR_CHECK_STRUCT_SIZE(lr_fcgf_params, p, who);
    LR_REFUSE_UNLESS(p->conv1_kernel_size == 3 || p->conv1_kernel_size == 5, LR_EINVAL, "conv1_kernel_size must be 3 or 5");
    LR_REFUSE_UNLESS(p->tap >= 0 && p->tap <= SP_STAGES, LR_EINVAL, "tap must lie in 0 .. 23");
    LR_REFUSE_UNLESS(n >= 0 && n <= FC_MAX_N, LR_EINVAL, "n must lie in 0 .. 2^20");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_fcgf_weights_bytes(p->conv1_kernel_size), LR_EINVAL, "weights_bytes is below lr_fcgf_weights_bytes(conv1_kernel_size)");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    LR_REFUSE_UNLESS(n == 0 || (coords && feat_out), LR_EINVAL, "null coords or feat_out");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_fcgf_scratch_bytes(n), "lr_fcgf_scratch_bytes(n)", LR_EINVAL, stream, nullptr));

    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(sp_empty_kernel<lr_fcgf_result>, dim3(1), dim3(1), 0, st, result);
        LR_LAUNCH_CHECK();
        return LR_OK;
    }
    const int K1 = p->conv1_kernel_size;
    fc_run R;
    fc_carve(R, scratch, fc_make_layout((size_t)n), n, K1, weights, st);
    const sp_layout &L = R.L;
    sp_ctl *ctl = R.ctl;
    const int gn = R.grid((size_t)n);

    // maps (level 0 in input order; mn stays 0, so that a tap's cells are field - bias)
    LR_HIP(hipMemsetAsync(ctl, 0, 256, st));
    LR_HIP(hipMemsetAsync(R.keys[0], 0xff, 4 * L.cap_max * 8, st));
    LR_HIP(hipMemsetAsync(R.val[0], 0x7f, 4 * L.cap_max * 4, st));
    hipLaunchKernelGGL(sp_l0_insert_kernel<fc_row_key>, dim3(gn), dim3(256), 0, st, fc_row_key{ coords }, n, R.keys[0], R.val[0], R.mask, R.rowkey[0], ctl);
    hipLaunchKernelGGL(sp_l0_check_kernel, dim3(gn), dim3(256), 0, st, R.rowkey[0], n, R.keys[0], R.val[0], R.mask, ctl);
    fc_maps<fc_codec>(R, K1);

    // a tap ends the call behind its stage
    const int tap = p->tap;
    const bool end = fc_stages(R,
        [&](float *X) {
            hipLaunchKernelGGL(fc_conv1_kernel, dim3(R.grid((size_t)n * 32)), dim3(256), 0, st, feat_in, fc_conv1_table(R, K1), R.t[1].k3, R.w[1],
                               R.w[1] + (size_t)R.t[1].k3 * 32, R.w[1] + (size_t)R.t[1].k3 * 32 + 32, X, ctl);
        },
        [&](int s, const float *buf, int lvl) -> bool {
            if (tap != s) return false;
            const int cout = R.t[s].cout;
            const size_t items = (size_t)n * (cout > 3 ? cout : 3);
            hipLaunchKernelGGL((sp_tap_kernel<fc_codec, lr_fcgf_result>), dim3(R.grid(items)), dim3(256), 0, st, buf, cout, lvl, R.rowkey[lvl], n, feat_out, tap_coords,
                               FC_BIAS, ctl, result);
            return true;
        });
    if (!end) hipLaunchKernelGGL(fc_norm_kernel, dim3(gn), dim3(256), 0, st, R.Y, n, feat_out, ctl, result);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

#include "lr_fcgf_batch.h"
