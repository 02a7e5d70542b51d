// lr_dgr_inlier_batch: up to 8 pairs' correspondence sets through ONE sequence of the launches of lr_dgr6.hip, which includes this file at
// its end.  Contract n4 (P1 .. P5) of include/lidarreg.h; DESIGN.md §20.7.
//
// The pairs are concatenated: global row i = start[k] + the row inside pair k.  A cell's key carries its pair above the six fields,
//   key = pair << 60 | six 10-bit fields (cell_a - origin_a(pair) + 8), axis 0 most significant      (top bit clear: LR_CELL_EMPTY sorts last),
// where every pair has its OWN origin 8 floor(min_a / 8), from six integer minima per pair (a segmented min-reduction over the rows).  So
// I2's extent limit and F10 hold per pair wherever each pair lies, one table per level serves every pair, and no pair finds another
// pair's cell.  Three tag bits, 60 .. 62, hence at most 8 pairs: a fourth would be bit 63, which must stay clear -- with tag 15 a neighbour
// query whose six fields are all 1023 would be the empty-slot word itself, and the sort would no longer put the empty word last.
// Level 0 is sorted like the coarse levels: the rows of the accepted pairs (status 0) in ascending (pair, cell) order, perm[r] = the global
// input row of rank r; every pair's rows are contiguous at every level.  The codec carries the tag through coarse(), neighbour(), the
// tables and the sort, so sp_maps, sp_stages, sp_conv_kernel, d6_conv1_kernel (the feature is ones: no permutation) and d6_final_kernel
// run unchanged over the total rows, a row tile across two pairs included.
// Why the bytes are those of the one-pair call (P2): I3 fixes the fmaf chain of an output element by idx(o) and the channel, not by the
// order of the rows; a pair's keys relative to its own origin are the one-pair call's keys but for the tag, and the tag makes every pair's
// maps its own: each row gathers the same neighbours' values in the same offset order.  (An offset a tile skips, or walks for another
// pair's rows, adds +0 products to a chain that began at +0: F5.)
// The status is per pair (db_ctl.status); the word the shared kernels leave on (sp_ctl.status) stays 0 and n[0] is the accepted rows.
#pragma once
#include <string.h>

#define DB_MAX_PAIRS 8               // the tag: bits 60 .. 62
#define DB_TAG_SHIFT 60
#define DB_CTL_BYTES 512

// the pairs of a call: by value into the kernels that need them, like fb_table
struct db_table {
    const int32_t *coords[DB_MAX_PAIRS];
    float *out[DB_MAX_PAIRS];
    int32_t start[DB_MAX_PAIRS + 1];     // row offsets in concatenation order; start[k] = the total for k >= npairs
    int32_t npairs;
};
static_assert(sizeof(db_table) + 512 <= 4096, "the pair table no longer fits the kernel arguments");
// c.status stays 0, c.n[l] = rows of level l over the accepted pairs, c.mn is unused; mn[k]: the per-axis minima of pair k
struct db_ctl { sp_ctl c; int32_t status[DB_MAX_PAIRS]; int32_t mn[DB_MAX_PAIRS][6]; };
static_assert(sizeof(db_ctl) <= DB_CTL_BYTES, "db_ctl outgrew its place at the head of the scratch");
static_assert(DB_TAG_SHIFT == 6 * 10 && DB_MAX_PAIRS <= (1 << (63 - DB_TAG_SHIFT)), "the tag lies above the six fields and below the top bit");

// ---- level 0 ------------------------------------------------------------------------------------------------------------------------
// the pair of global row i < start[npairs]: the last k with start[k] <= i (an empty pair shares its start with the next one)
__device__ __forceinline__ int db_pair_of(const db_table &t, int i)
{
    int lo = 0, hi = t.npairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.start[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// (sp_init_kernel has zeroed the block)
__global__ void db_init_kernel(db_ctl *ctl)
{
    if (threadIdx.x < DB_MAX_PAIRS * 6) ctl->mn[threadIdx.x / 6][threadIdx.x % 6] = INT_MAX;
}
// the six minima of every pair.  A wave inside one pair reduces by shuffles and one lane stores; a wave that spans a pair boundary (several,
// with pairs of one row) must not fold one pair's minimum into another's: its lanes store one by one
__global__ void __launch_bounds__(256) db_min_kernel(db_table t, int total, db_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < total;
    const int k = on ? db_pair_of(t, i) : -1;
    const int k0 = __shfl(k, 0);                                       // lane 0 is the wave's smallest row: off only when the whole wave is
    if (k0 < 0) return;
    const bool one_pair = __all(!on || k == k0);
    const int32_t *p = on ? t.coords[k] + 6 * (size_t)(i - t.start[k]) : nullptr;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        int v = on ? p[a] : INT_MAX;
        if (one_pair) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d); v = o < v ? o : v; }
            if ((threadIdx.x & 63) == 0) atomicMin(&ctl->mn[k0][a], v);
        } else if (on) {
            atomicMin(&ctl->mn[k][a], v);
        }
    }
}
// the tagged key of global row i and its pair; LR_CELL_EMPTY when an axis lies past the pair's extent limit
__device__ __forceinline__ fc_u64 db_row_key(const db_table &t, int i, const db_ctl *ctl, int &k)
{
    k = db_pair_of(t, i);
    const int32_t *p = t.coords[k] + 6 * (size_t)(i - t.start[k]);
    fc_u64 key = (fc_u64)k;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const long long origin = (long long)((ctl->mn[k][a] >> 3) << 3);                                       // 8 floor(min / 8)
        const long long rel = (long long)p[a] - origin;                                                        // >= 0
        ok = ok && rel <= D6_REL_MAX;
        key = (key << 10) | ((fc_u64)(rel + D6_BIAS) & d6_codec::FIELD);
    }
    return ok ? key : LR_CELL_EMPTY;
}
// rowkeys[i] = the key of global row i (kept for the two kernels behind this one: they find the pair in its tag)
__global__ void __launch_bounds__(256) db_l0_insert_kernel(db_table t, int total, fc_u64 *keys, int32_t *val, unsigned mask, fc_u64 *__restrict__ rowkeys, db_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int k;
    const fc_u64 key = db_row_key(t, i, ctl, k);
    rowkeys[i] = key;
    if (key == LR_CELL_EMPTY) { atomicMax(&ctl->status[k], 3); return; }
    atomicMin(&val[lr_cells_claim(keys, mask, key)], i);
}
__global__ void __launch_bounds__(256) db_l0_check_kernel(const fc_u64 *__restrict__ rowkeys, int total, const fc_u64 *__restrict__ keys,
                                                          const int32_t *__restrict__ val, unsigned mask, db_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const fc_u64 key = rowkeys[i];
    if (key == LR_CELL_EMPTY) return;
    const int s = fc_find(keys, mask, key);
    if (s < 0 || val[s] != i) atomicMax(&ctl->status[(int)(key >> DB_TAG_SHIFT)], 2);
}
// in place: sortbuf[i] keeps the key of global row i when its pair is accepted, no key otherwise and behind the rows; n[0] = the accepted rows
__global__ void __launch_bounds__(256) db_l0_mark_kernel(int total, fc_u64 *__restrict__ sortbuf, int n_sort, db_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    fc_u64 out = LR_CELL_EMPTY;
    if (i < total) {
        const fc_u64 key = sortbuf[i];
        if (key != LR_CELL_EMPTY && ctl->status[(int)(key >> DB_TAG_SHIFT)] == 0) out = key;
    }
    if (i < n_sort) sortbuf[i] = out;
    const unsigned long long live = __ballot(out != LR_CELL_EMPTY);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&ctl->c.n[0], __popcll(live));
}

// ---- the end ------------------------------------------------------------------------------------------------------------------------
// the logit of rank r into row perm[r] - start[pair] of its pair's logit_out, zeros into the rows of the refused pairs, the result blocks
__global__ void __launch_bounds__(256) db_finish_kernel(db_table t, int total, const float *__restrict__ f, const fc_u64 *__restrict__ rowkey,
                                                        const int32_t *__restrict__ perm, const db_ctl *ctl, lr_dgr_inlier_result *res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < t.npairs) {
        const int status = ctl->status[i], n = t.start[i + 1] - t.start[i];
        res[i].status = status; res[i].n = n; res[i].n_tap = status ? 0 : n; res[i].reserved = 0;
    }
    if (i >= total) return;
    if (i < ctl->c.n[0]) {
        const int k = (int)(rowkey[i] >> DB_TAG_SHIFT), base = t.start[k];
        const unsigned j = (unsigned)(perm[i] - base);
        if (j < (unsigned)(t.start[k + 1] - base)) t.out[k][j] = f[i];          // (always: perm[i] is a row of pair k)
    }
    const int k = db_pair_of(t, i);
    if (ctl->status[k] != 0) t.out[k][i - t.start[k]] = 0.0f;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static sp_layout db_make_layout(size_t total, const int32_t *w) { return sp_make_layout(total, D6_NK, 0, w, DB_CTL_BYTES, true); }

extern "C" size_t lr_dgr_inlier_batch_scratch_bytes(int npairs, int total_n, const int32_t *widths)
{
    if (npairs < 1 || npairs > DB_MAX_PAIRS || total_n < 0 || total_n > D6_MAX_N || !d6_widths_ok(widths)) return 0;
    return db_make_layout((size_t)total_n, widths).total;
}

extern "C" int lr_dgr_inlier_batch(int npairs, const int32_t *const *coords, const int32_t *n, const float *weights, size_t weights_bytes,
                                   const lr_dgr_inlier_params *p, lr_dgr_inlier_result *results, float *const *logit_out, void *scratch,
                                   size_t scratch_bytes, void *stream)
{
    const char *who = "lr_dgr_inlier_batch";
    LR_CHECK_STRUCT_SIZE(lr_dgr_inlier_params, p, who);
    LR_REFUSE_UNLESS(d6_widths_ok(p->widths), LR_EINVAL, "every width must be a multiple of 32 in 32 .. 256");
    LR_REFUSE_UNLESS(p->tap == 0, LR_EINVAL, "tap must be 0 (a batch has no tap)");
    LR_REFUSE_UNLESS(npairs >= 1 && npairs <= DB_MAX_PAIRS, LR_EINVAL, "npairs must lie in 1 .. 8");
    LR_REFUSE_UNLESS(coords, LR_EINVAL, "null coords");
    LR_REFUSE_UNLESS(n, LR_EINVAL, "null n");
    LR_REFUSE_UNLESS(logit_out, LR_EINVAL, "null logit_out");
    db_table t;
    memset(&t, 0, sizeof t);
    t.npairs = npairs;
    long long sum = 0;
    for (int k = 0; k < npairs; ++k) {
        if (n[k] < 0 || n[k] > D6_MAX_N) { lr_set_error("%s: n[%d] must lie in 0 .. 131072", who, k); return LR_EINVAL; }
        if (n[k] > 0 && !coords[k]) { lr_set_error("%s: null coords[%d]", who, k); return LR_EINVAL; }
        if (n[k] > 0 && !logit_out[k]) { lr_set_error("%s: null logit_out[%d]", who, k); return LR_EINVAL; }
        t.coords[k] = coords[k]; t.out[k] = logit_out[k];
        t.start[k] = (int32_t)sum;
        sum += n[k];
        LR_REFUSE_UNLESS(sum <= D6_MAX_N, LR_EINVAL, "the sum of n must not exceed 131072");
    }
    const int total = (int)sum;
    for (int k = npairs; k <= DB_MAX_PAIRS; ++k) t.start[k] = total;
    LR_REFUSE_UNLESS(results, LR_EINVAL, "null results");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_dgr_inlier_weights_bytes(p->widths), LR_EINVAL, "weights_bytes is below lr_dgr_inlier_weights_bytes(widths)");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_dgr_inlier_batch_scratch_bytes(npairs, total, p->widths),
                                "lr_dgr_inlier_batch_scratch_bytes(npairs, sum of n, widths)", LR_EINVAL, stream, nullptr));

    hipStream_t st = (hipStream_t)stream;
    const int32_t *wd = p->widths;
    sp_run<SP_STREAMED> R;
    sp_stage_table(wd, D6_NK, D6_NK, 1, R.t);
    R.carve(scratch, db_make_layout((size_t)total, wd), total, weights, st);
    const sp_layout &L = R.L;
    db_ctl *ctl = R.at<db_ctl>(0);
    sp_init_launch(R.keys[0], R.val[0], total > 0 ? 4 * L.cap_max : 0, R.ctl, DB_CTL_BYTES, st);
    if (total > 0) {
        const int gn = R.grid((size_t)total), C1 = wd[0];

        // maps: every pair's origin, then level 0 sorted, with perm (in the room behind the levels' keys)
        hipLaunchKernelGGL(db_init_kernel, dim3(1), dim3(64), 0, st, ctl);
        hipLaunchKernelGGL(db_min_kernel, dim3(gn), dim3(256), 0, st, t, total, ctl);
        hipLaunchKernelGGL(db_l0_insert_kernel, dim3(gn), dim3(256), 0, st, t, total, R.keys[0], R.val[0], R.mask, R.sortbuf, ctl);
        hipLaunchKernelGGL(db_l0_check_kernel, dim3(gn), dim3(256), 0, st, R.sortbuf, total, R.keys[0], R.val[0], R.mask, ctl);
        hipLaunchKernelGGL(db_l0_mark_kernel, dim3(R.grid(R.n_sort)), dim3(256), 0, st, total, R.sortbuf, (int)R.n_sort, ctl);
        fc_sort_launch(R.sortbuf, R.n_sort, st);
        hipLaunchKernelGGL(sp_index_kernel, dim3(gn), dim3(256), 0, st, R.sortbuf, 0, R.keys[0], R.val[0], R.mask, R.rowkey[0], R.perm, R.ctl);
        sp_maps<d6_codec, 0>(R);

        sp_stages(R, wd,
            [&](float *X) {
                hipLaunchKernelGGL(d6_conv1_kernel, dim3(R.grid((size_t)total * C1)), dim3(256), 0, st, R.nbr[0], R.w[1], R.w[1] + (size_t)D6_NK * C1,
                                   R.w[1] + (size_t)D6_NK * C1 + C1, C1, X, R.ctl);
            },
            [&](const float *X, float *Y) { hipLaunchKernelGGL(d6_final_kernel, dim3(gn), dim3(256), 0, st, X, wd[7], R.w[23], Y, R.ctl); },
            [&](int, const float *, int) { return false; });
    }
    hipLaunchKernelGGL(db_finish_kernel, dim3(R.grid((size_t)(total > npairs ? total : npairs))), dim3(256), 0, st, t, total, R.Y, R.rowkey[0], R.perm, ctl, results);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
