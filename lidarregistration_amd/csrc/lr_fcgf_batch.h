// lr_fcgf_extract_batch: up to 64 clouds through ONE sequence of the launches of lr_fcgf.hip, which includes this file at its end.
// Contract n2 (B1 .. B5) of include/lidarreg.h; DESIGN.md §18.7.
//
// The clouds are concatenated: global row i = start[c] + the row inside cloud c.  A cell's key carries its cloud,
//   key = cloud << 57 | (x + 2^18) << 38 | (y + 2^18) << 19 | (z + 2^18)          (top bit clear: LR_CELL_EMPTY sorts behind every row),
// so one table per level serves every cloud and no cloud can find another cloud's cell.  Level 0 is sorted like the coarse levels: the rows
// of the accepted clouds (status 0) in ascending (cloud, x, y, z) order, perm[r] = the global input row of rank r; every cloud's rows are
// contiguous at every level and, inside a cloud, in the order F1 prescribes.  The codec carries the tag through the coarse levels and the
// gather tables, which are per row, so the maps and sp_conv_kernel of lr_sparse.h run unchanged over the total rows, a row tile across two
// clouds included; only level 0 and the two ends differ: conv1 reads feat_in, and the normalisation writes feat_out, of the row's cloud
// at perm[r] - start[cloud].  The status is per cloud (fb_ctl.status); the word that the shared kernels leave on stays 0.  The three
// level-0 kernels stay here: they find a row's cloud, and with it its status word, by a search in the cloud table.
#pragma once
#include <string.h>

#define FB_BIAS (1 << 18)            // cell + bias is a 19-bit field of the tagged key
#define FB_LIMIT ((1 << 18) - 2)     // |cell| >= this: status 3
#define FB_CTL_BYTES 512
typedef sp_codec<3, 19> fb_codec;      // the tag above bit 57: the cloud

// the clouds of a call: by value into the kernels that need them, like ov_desc_table (1800 bytes)
struct fb_table {
    const int32_t *coords[LR_MAX_BATCH];
    const float *feat_in[LR_MAX_BATCH];
    float *feat_out[LR_MAX_BATCH];
    int32_t start[LR_MAX_BATCH + 1];     // row offsets in concatenation order; start[c] = the total for c >= nclouds
    int32_t nclouds;
};
static_assert(sizeof(fb_table) + 512 <= 4096, "the cloud table no longer fits the kernel arguments");
// c.status stays 0, c.n[l] = rows of level l over the accepted clouds
struct fb_ctl { sp_ctl c; int32_t status[LR_MAX_BATCH]; };
static_assert(sizeof(fb_ctl) <= FB_CTL_BYTES, "fb_ctl outgrew its place at the head of the scratch");

// ---- maps -------------------------------------------------------------------------------------------------------------------------
// the cloud of global row i < start[nclouds]: the last c with start[c] <= i (an empty cloud shares its start with the next one)
__device__ __forceinline__ int fb_cloud_of(const fb_table &t, int i)
{
    int lo = 0, hi = t.nclouds;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.start[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ fc_u64 fb_key(int c, int x, int y, int z)
{
    return ((fc_u64)c << 57) | ((fc_u64)(x + FB_BIAS) << 38) | ((fc_u64)(y + FB_BIAS) << 19) | (fc_u64)(z + FB_BIAS);
}
__device__ __forceinline__ bool fb_in_range(int v) { return v > -FB_LIMIT && v < FB_LIMIT; }
// the cell of global row i and its cloud; false when the cell is past the range limit
__device__ __forceinline__ bool fb_row_key(const fb_table &t, int i, int &c, fc_u64 &key)
{
    c = fb_cloud_of(t, i);
    const int32_t *p = t.coords[c] + 3 * (size_t)(i - t.start[c]);
    const int x = p[0], y = p[1], z = p[2];
    key = 0;
    if (!(fb_in_range(x) && fb_in_range(y) && fb_in_range(z))) return false;
    key = fb_key(c, x, y, z);
    return true;
}

__global__ void __launch_bounds__(256) fb_l0_insert_kernel(fb_table t, int total, fc_u64 *keys, int32_t *val, unsigned mask, fb_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int c;
    fc_u64 key;
    if (!fb_row_key(t, i, c, key)) { atomicMax(&ctl->status[c], 3); return; }
    atomicMin(&val[lr_cells_claim(keys, mask, key)], i);
}
__global__ void __launch_bounds__(256) fb_l0_check_kernel(fb_table t, int total, const fc_u64 *__restrict__ keys, const int32_t *__restrict__ val, unsigned mask,
                                                          fb_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int c;
    fc_u64 key;
    if (!fb_row_key(t, i, c, key)) return;
    const int s = fc_find(keys, mask, key);
    if (s < 0 || val[s] != i) atomicMax(&ctl->status[c], 2);
}
// sortbuf[i] = the key of global row i when its cloud is accepted, no key otherwise and behind the rows; n[0] = the accepted rows
__global__ void __launch_bounds__(256) fb_l0_mark_kernel(fb_table t, int total, fc_u64 *__restrict__ sortbuf, int n_sort, fb_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    fc_u64 out = LR_CELL_EMPTY;
    if (i < total) {
        int c;
        fc_u64 key;
        if (fb_row_key(t, i, c, key) && ctl->status[c] == 0) out = key;
    }
    if (i < n_sort) sortbuf[i] = out;
    const unsigned long long live = __ballot(out != LR_CELL_EMPTY);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&ctl->c.n[0], __popcll(live));
}

// ---- the two ends of the network ----------------------------------------------------------------------------------------------------
// fc_conv1_kernel over the ranks: the neighbour of rank idx is row perm[idx] - start[c] of its cloud's feat_in
__global__ void __launch_bounds__(256) fb_conv1_kernel(fb_table t, const fc_u64 *__restrict__ rowkey, const int32_t *__restrict__ perm, const int32_t *__restrict__ nbr,
                                                       int nk, const float *__restrict__ W, const float *__restrict__ scale, const float *__restrict__ offset,
                                                       float *__restrict__ out, const fb_ctl *ctl)
{
    __shared__ float sW[125 * 32];
    for (int e = threadIdx.x; e < nk * 32; e += 256) sW[e] = W[e];
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(gid >> 5), c = (int)(gid & 31);
    if (r >= ctl->c.n[0]) return;
    const int cl = (int)(rowkey[r] >> 57);
    const float *f = t.feat_in[cl];
    const int base = t.start[cl];
    const unsigned rows = (unsigned)(t.start[cl + 1] - base);
    float acc = 0.0f;
    for (int k = 0; k < nk; ++k) {
        const int idx = nbr[(size_t)r * nk + k];
        if (idx < 0) continue;
        float v = 1.0f;
        if (f) {
            const unsigned j = (unsigned)(perm[idx] - base);      // (a rank of this cloud: j < rows)
            v = j < rows ? f[j] : 0.0f;
        }
        acc = fmaf(v, sW[k * 32 + c], acc);
    }
    out[(size_t)r * 32 + c] = fmaf(scale[c], acc, offset[c]);
}
// F8 of rank r into row perm[r] - start[c] of its cloud's feat_out
__global__ void __launch_bounds__(256) fb_norm_kernel(fb_table t, const float *__restrict__ f, const fc_u64 *__restrict__ rowkey, const int32_t *__restrict__ perm,
                                                      const fb_ctl *ctl)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= ctl->c.n[0]) return;
    const int cl = (int)(rowkey[r] >> 57), base = t.start[cl];
    const unsigned j = (unsigned)(perm[r] - base);
    if (j >= (unsigned)(t.start[cl + 1] - base)) return;          // (never: perm[r] is a row of cloud cl)
    float *out = t.feat_out[cl] + (size_t)j * 32;
    float v[32], s = 0.0f;
#pragma unroll
    for (int c = 0; c < 32; ++c) { v[c] = f[(size_t)r * 32 + c]; s = fmaf(v[c], v[c], s); }
    const float d = sqrtf(s) + 1e-8f;
#pragma unroll
    for (int c = 0; c < 32; ++c) out[c] = v[c] / d;
}
// the result blocks, and rows of zeros for the refused clouds
__global__ void __launch_bounds__(256) fb_finish_kernel(fb_table t, int total, const fb_ctl *ctl, lr_fcgf_result *res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < t.nclouds) {
        const int status = ctl->status[i], n = t.start[i + 1] - t.start[i];
        res[i].status = status; res[i].n = n; res[i].n_tap = status ? 0 : n; res[i].reserved = 0;
    }
    if (i >= total) return;
    const int c = fb_cloud_of(t, i);
    if (ctl->status[c] == 0) return;
    float *out = t.feat_out[c] + (size_t)(i - t.start[c]) * 32;
#pragma unroll
    for (int q = 0; q < 32; ++q) out[q] = 0.0f;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// bench hook (tools/fcgf_bench.py: the maps / convolutions split of a batch): a call ends behind this stage and stores no features; 0 = off
static int g_fb_stop_after = 0;
extern "C" int lr_debug_fcgf_batch_stop_after(int stage) { g_fb_stop_after = stage; return LR_OK; }

extern "C" size_t lr_fcgf_batch_scratch_bytes(int nclouds, int total_n)
{
    if (nclouds < 1 || nclouds > LR_MAX_BATCH || total_n < 0 || total_n > FC_MAX_N) return 0;
    return fc_make_layout((size_t)total_n, FB_CTL_BYTES).total;
}

extern "C" int lr_fcgf_extract_batch(int nclouds, const int32_t *const *coords, const float *const *feat_in, const int32_t *n, const float *weights,
                                     size_t weights_bytes, const lr_fcgf_params *p, lr_fcgf_result *results, float *const *feat_out, void *scratch,
                                     size_t scratch_bytes, void *stream)
{
    const char *who = "lr_fcgf_extract_batch";
    LR_CHECK_STRUCT_SIZE(lr_fcgf_params, p, who);
    LR_REFUSE_UNLESS(p->conv1_kernel_size == 3 || p->conv1_kernel_size == 5, LR_EINVAL, "conv1_kernel_size must be 3 or 5");
    LR_REFUSE_UNLESS(p->tap == 0, LR_EINVAL, "tap must be 0 (a batch has no tap)");
    LR_REFUSE_UNLESS(nclouds >= 1 && nclouds <= LR_MAX_BATCH, LR_EINVAL, "nclouds must lie in 1 .. 64");
    LR_REFUSE_UNLESS(coords, LR_EINVAL, "null coords");
    LR_REFUSE_UNLESS(n, LR_EINVAL, "null n");
    LR_REFUSE_UNLESS(feat_out, LR_EINVAL, "null feat_out");
    fb_table t;
    memset(&t, 0, sizeof t);
    t.nclouds = nclouds;
    long long sum = 0;
    for (int b = 0; b < nclouds; ++b) {
        if (n[b] < 0 || n[b] > FC_MAX_N) { lr_set_error("%s: n[%d] must lie in 0 .. 2^20", who, b); return LR_EINVAL; }
        if (n[b] > 0 && !coords[b]) { lr_set_error("%s: null coords[%d]", who, b); return LR_EINVAL; }
        if (n[b] > 0 && !feat_out[b]) { lr_set_error("%s: null feat_out[%d]", who, b); return LR_EINVAL; }
        t.coords[b] = coords[b]; t.feat_in[b] = feat_in ? feat_in[b] : nullptr; t.feat_out[b] = feat_out[b];
        t.start[b] = (int32_t)sum;
        sum += n[b];
        LR_REFUSE_UNLESS(sum <= FC_MAX_N, LR_EINVAL, "the sum of n must not exceed 2^20");
    }
    const int total = (int)sum;
    for (int b = nclouds; b <= LR_MAX_BATCH; ++b) t.start[b] = total;
    LR_REFUSE_UNLESS(results, LR_EINVAL, "null results");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_fcgf_weights_bytes(p->conv1_kernel_size), LR_EINVAL, "weights_bytes is below lr_fcgf_weights_bytes(conv1_kernel_size)");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_fcgf_batch_scratch_bytes(nclouds, total), "lr_fcgf_batch_scratch_bytes(nclouds, sum of n)", LR_EINVAL,
                                stream, nullptr));

    hipStream_t st = (hipStream_t)stream;
    const int K1 = p->conv1_kernel_size;
    fc_run R;
    fc_carve(R, scratch, fc_make_layout((size_t)total, FB_CTL_BYTES), total, K1, weights, st);
    const sp_layout &L = R.L;
    fb_ctl *ctl = R.at<fb_ctl>(0);
    sp_init_launch(R.keys[0], R.val[0], total > 0 ? 4 * L.cap_max : 0, R.ctl, FB_CTL_BYTES, st);
    if (total > 0) {
        const int gn = R.grid((size_t)total);

        // maps: level 0 sorted, with perm (in the room behind the levels' keys)
        hipLaunchKernelGGL(fb_l0_insert_kernel, dim3(gn), dim3(256), 0, st, t, total, R.keys[0], R.val[0], R.mask, ctl);
        hipLaunchKernelGGL(fb_l0_check_kernel, dim3(gn), dim3(256), 0, st, t, total, R.keys[0], R.val[0], R.mask, ctl);
        hipLaunchKernelGGL(fb_l0_mark_kernel, dim3(R.grid(R.n_sort)), dim3(256), 0, st, t, total, R.sortbuf, (int)R.n_sort, ctl);
        fc_sort_launch(R.sortbuf, R.n_sort, st);
        hipLaunchKernelGGL(sp_index_kernel, dim3(gn), dim3(256), 0, st, R.sortbuf, 0, R.keys[0], R.val[0], R.mask, R.rowkey[0], R.perm, R.ctl);
        fc_maps<fb_codec>(R, K1);

        const int stop = g_fb_stop_after;
        const bool cut = fc_stages(R,
            [&](float *X) {
                hipLaunchKernelGGL(fb_conv1_kernel, dim3(R.grid((size_t)total * 32)), dim3(256), 0, st, t, R.rowkey[0], R.perm, fc_conv1_table(R, K1), R.t[1].k3,
                                   R.w[1], R.w[1] + (size_t)R.t[1].k3 * 32, R.w[1] + (size_t)R.t[1].k3 * 32 + 32, X, ctl);
            },
            [&](int s, const float *, int) { return s == stop; });
        if (!cut) hipLaunchKernelGGL(fb_norm_kernel, dim3(gn), dim3(256), 0, st, t, R.Y, R.rowkey[0], R.perm, ctl);
    }
    hipLaunchKernelGGL(fb_finish_kernel, dim3(R.grid((size_t)(total > nclouds ? total : nclouds))), dim3(256), 0, st, t, total, ctl, results);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
