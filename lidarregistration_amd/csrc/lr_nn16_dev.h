// What more than one stage of the NN path compiles: lr_nn16.hip (prep, range, the forward direction), lr_nn16_pass.hip (the filter pass),
// lr_nn16_exact.hip (exact verification), lr_nn16_rev.hip (seeds, ordering and the reverse direction).  Device text is header-only: there
// is no relocatable device code, so every translation unit inlines its own copy.  What a single stage uses stays in that stage's file.
// The contract, why the candidate set is a superset and the error bound are at the top of lr_nn16.hip.
#pragma once
#include "lr_internal.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define LR_INF __builtin_huge_valf()
#define LR_IMAX 0x7fffffff

// order-preserving image of a float in an unsigned integer (smaller float <=> smaller integer; NaN never travels)
__device__ __forceinline__ uint32_t lr_ord_enc(float v) { const uint32_t b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float lr_ord_dec(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
#define LR_ORD_INF 0xff800000u      // lr_ord_enc(+inf)

// E_i of the thresholds, scale = n0_i + max_j n1_j (derivation: "Error bound" at the top of lr_nn16.hip)
__device__ __forceinline__ float lr_nn16_err(float scale) { return 1.05e-3f * scale + 4e-7f; }

#define LR_BLOCK_ROWS 256        // rows per filter-pass block: 4 waves x 64 rows (four 16-row MFMA blocks per wave)
#define LR_EX_ROWS 64            // rows per block of the exact stage: those of one filter-pass wave
// Entry of a hit list / of the candidate store (8 bytes): x = column (22 bits) | kb << 22 | LR_PB_HASG; y = 16-bit row mask | g16 << 16.
// kb = lane / 16 of the lane that saw the hit: bit b = 4 rbk + g of the mask <-> row 16 rbk + 4 kb + g of the wave (the lane's 16
// accumulator registers of one 16-column block).  The walk parks entries with an empty mask; derive() fills it in.
#define LR_PB_COLMASK 0x3fffffu
#define LR_PB_HASG 0x1000000u    // entry flag (in x): exactly one row, and y carries its filter value g rounded up to 16 bits
// row (0..63 of the wave) of mask bit b (0..15) of an entry of lane group kb
__device__ __forceinline__ int lr_pb_row(int kb, int b) { return 16 * (b >> 2) + 4 * kb + (b & 3); }
__device__ __forceinline__ int lr_pb_kb(unsigned x) { return (int)(x >> 22) & 3; }

#define LR_RS_BUCKETS 4096

// monotone map distance -> bucket: linear over the pair's range of forward NN distances [lo, hi] (well spread keys keep
// the sort's atomics apart); any monotone map is valid, a coarser one only prunes less
__device__ __forceinline__ int rs_bucket(float v, float lo, float scale)
{
    const int b = (int)((v - lo) * scale);
    return min(max(b, 0), LR_RS_BUCKETS - 1);
}
__device__ __forceinline__ float rs_scale(float lo, float hi) { return hi > lo ? (float)LR_RS_BUCKETS / (hi - lo) : 0.0f; }

// what the thresholds are made of: squared norms of the query rows (by data row), per-32-row maxima of the column cloud's squared
// norms, how many neighbours are wanted, and the sampling stride of phase 1 (forward direction)
struct lr_thr_in {
    const float *nQ;
    const float *range_c;          // { largest, smallest } squared norm of the column cloud (nn16_range_kernel), or nullptr
    int need, sstride;
};
// grid shape of a 1-D XCD-aware launch + direction (0: rows = cloud 0, columns = cloud 1; 1: the reverse pass)
struct lr_pb_grid { int gx, gy, total, dir, only; };      // only != 0: the other instantiation is not launched (single-pair calls, see lr_nn16_form_hint)
// Where the exact stage (nn16_exact_kernel) leaves its results: the two neighbours by data row, and (forward direction of a pair) the
// seeds of the reverse pass
struct lr_ex_out {
    int32_t *idx1, *idx2;
    float *s1o, *s2o;
    uint32_t *seed_out;              // [columns] smallest forward distance pointing at each column (bit pattern), or nullptr
    float *seed_s1;                  // [rows] column key of the reverse pass (2nd-NN distance, or the NN distance when need == 1)
    uint32_t *seed_range;            // { smallest, largest } of the seeds and keys
    unsigned long long *seed64;      // forward: [columns] (distance bits << 32) | smallest row at that distance; reverse: the seeds to start from
};

// ------------------------------------------------------------------ host side
// One filter pass: what nn16_passb_kernel takes between its clock words and its grid (the candidate store is the workspace's), and the
// shape of the pass.  dir 0: rows = cloud 0, columns = cloud 1; 1: the reverse pass.
struct lr_pb_args {
    const _Float16 *Hq; int na; const int32_t *rowmap, *na_dev;
    const _Float16 *Hc; const float *nC; int nb, tps;
    const float *tau;
    const int32_t *colmap; const float *tile_min; const uint32_t *row_bound; const int32_t *rev_offs; const uint32_t *rev_range;
    float *yfin; int yfin_stride; uint32_t *yshare;
    lr_thr_in thr;
    int row_blocks, strips, dir;
};
// lr_nn16_pass.hip: the launch site of the filter pass, bracketed by the direction's stage-timer events
int lr_nn16_passb(const lr_call &c, const lr_pb_args &a);
// lr_nn16_exact.hip: the launch site of the exact stage.  dir 0: rows = cloud 0 (Fq, na) against columns = cloud 1 (Fc, nb); 1: the reverse
// direction, rows = cloud 1.  strips: what the filter pass ran with.  yfin: its final thresholds [strip][max_n], or nullptr.  rowmap /
// na_dev: the compacted row list of the reverse direction, or nullptr.
int lr_nn16_exact(const lr_call &c, int dir, const float *Fq, int na, const float *Fc, int nb, int strips, int need,
                  const float *yfin, const int32_t *rowmap, const int32_t *na_dev, const lr_ex_out &out);

// The launch plan of a filter pass: row blocks of LR_BLOCK_ROWS rows, column strips per row block, column tiles (32 columns) per strip,
// and the sampling stride of phase 1 (forward direction only).
struct lr_nn16_plan { int row_blocks, strips, tps, sstride; };

// Forward direction, rows = na, columns = nb.  blocks_target / blocks_batch: LR_OPT_NN_BLOCKS / LR_OPT_NN_BLOCKS_BATCH (3 / 12 blocks per
// CU by default); sample_stride_option: LR_OPT_NN_SAMPLE_STRIDE (0: by the strip length).
constexpr lr_nn16_plan lr_nn16_plan_fwd(int na, int nb, int pairs, int blocks_target, int blocks_batch, int sample_stride_option)
{
    const int ntiles = lr_cdiv(nb, 32);
    const int row_blocks = lr_cdiv(na, LR_BLOCK_ROWS);
    // strips: enough blocks (over all pairs of a batched call) to fill 256 CUs a few times over, at least 64 tiles per strip
    // (a single pair: as many strips as keep ALL blocks resident at once -- the strips of a row block pool their thresholds, see the
    // kernel, so a shorter strip no longer means a looser one, and a second round of blocks would be a tail)
    int strips = pairs > 1 ? lr_cdiv(blocks_batch, row_blocks * pairs) : blocks_target / row_blocks;
    int smax = ntiles / 64;
    if (strips > smax) strips = smax;
    if (strips > LR_NN_MAX_STRIPS) strips = LR_NN_MAX_STRIPS;
    if (strips < 1) strips = 1;
    const int tps = lr_cdiv(ntiles, strips);
    // phase 1 of the filter pass samples every `sstride`-th tile of a strip (any subset gives a valid, if looser, start; the walk
    // tightens it).  Its cost is ~ tiles / stride per row, the extra hits of a looser start ~ 2 ln(stride) per row: about 32
    // sampled tiles per strip, a stride of at most 32.
    // With several strips per row block the start thresholds are pooled, so the budget is per ROW: about 64 sampled tiles over all strips.
    int sstride = sample_stride_option > 0 ? sample_stride_option : (strips > 1 ? ntiles / 64 : tps / 32);
    if (sample_stride_option <= 0) { const int cap = strips > 1 ? 16 : 32; if (sstride > cap) sstride = cap; }      // (pipeline, 30k points: 16 / 24 / 32 / 48 / 64 -> 11 750 / 11 820 / 11 910 / 11 880 / 11 920 pairs/s)
    if (sstride < 1) sstride = 1;
    if (sstride > tps) sstride = tps;          // (one sampled tile per strip at least; keeps phase 1's column index in range)
    return { row_blocks, strips, tps, sstride };
}

// Reverse direction, rows = na (cloud 1), columns = nb (cloud 0).  rev_strips_option: LR_OPT_REV_STRIPS (0: by the number of pairs; the
// option is clamped to LR_REV_MAX_STRIPS where it is set).
constexpr lr_nn16_plan lr_nn16_plan_rev(int na, int nb, int pairs, int rev_strips_option)
{
    const int ntiles = lr_cdiv(nb, 32);
    const int row_blocks = lr_cdiv(na, LR_BLOCK_ROWS);
    // the grid offers every row block the maximum number of strips; a block uses as many as its column prefix is worth
    // strips offered to every row block (no pass-A partial arrays on this path: not bound by LR_NN_MAX_STRIPS).  A block that is
    // not needed leaves after three loads, but tens of thousands of them still cost: 8 for one pair (parallelism for the row blocks
    // with long prefixes), fewer the more pairs a batched call brings (2 at 32 pairs: 7 990 against 7 740 pairs/s with 16)
    int strips = rev_strips_option > 0 ? rev_strips_option : 48 / pairs;
    if (rev_strips_option <= 0) { if (strips > 8) strips = 8; if (strips < 2) strips = 2; }
    int smax = ntiles / 8;
    if (strips > smax) strips = smax;
    if (strips < 1) strips = 1;
    return { row_blocks, strips, lr_cdiv(ntiles, strips), 0 };
}

// The plans at the sizes of the headline workload, of the tests' small pairs and of a degenerate pair, derived by hand from the text above
// (blocks_target 768, blocks_batch 3072: 256 CUs) ...
constexpr bool lr_nn16_plan_is(const lr_nn16_plan &p, int row_blocks, int strips, int tps, int sstride)
{
    return p.row_blocks == row_blocks && p.strips == strips && p.tps == tps && p.sstride == sstride;
}
static_assert(lr_nn16_plan_is(lr_nn16_plan_fwd(30000, 30000, 1, 768, 3072, 0), 118, 6, 157, 14), "forward plan, one 30k pair");
static_assert(lr_nn16_plan_is(lr_nn16_plan_fwd(30000, 30000, 32, 768, 3072, 0), 118, 1, 938, 29), "forward plan, 32 pairs of 30k");
static_assert(lr_nn16_plan_is(lr_nn16_plan_fwd(3000, 2500, 1, 768, 3072, 0), 12, 1, 79, 2), "forward plan, one small pair");
static_assert(lr_nn16_plan_is(lr_nn16_plan_fwd(5, 20, 1, 768, 3072, 0), 1, 1, 1, 1), "forward plan, less than one tile");
static_assert(lr_nn16_plan_is(lr_nn16_plan_rev(30000, 30000, 1, 0), 118, 8, 118, 0), "reverse plan, one 30k pair");
static_assert(lr_nn16_plan_is(lr_nn16_plan_rev(30000, 30000, 32, 0), 118, 2, 469, 0), "reverse plan, 32 pairs of 30k");
static_assert(lr_nn16_plan_is(lr_nn16_plan_rev(30000, 30000, 1, 64), 118, 64, 15, 0), "reverse plan, LR_OPT_REV_STRIPS 64");
static_assert(lr_nn16_plan_is(lr_nn16_plan_rev(50, 100, 1, 0), 1, 1, 4, 0), "reverse plan, four tiles");
// ... and what the kernels rely on, whatever the sizes and options: the strips cover every column tile, the forward strips fit yfin and
// the candidate counters (LR_NN_MAX_STRIPS), phase 1 samples at least one tile of a strip, the reverse strips fit the counters
constexpr bool lr_nn16_plans_hold()
{
    const int sizes[] = { 1, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 3000, 8192, 30000, 65537, 200000 };
    const int many[] = { 1, 2, 3, 16, 32, 64 }, blocks[] = { 1, 768, 912 }, strides[] = { 0, 1, 64, 4096 }, rev_opts[] = { 0, 1, 8, LR_REV_MAX_STRIPS };
    for (int na : sizes) for (int nb : sizes) for (int pairs : many) {
        for (int bt : blocks) for (int ss : strides) {
            const lr_nn16_plan p = lr_nn16_plan_fwd(na, nb, pairs, bt, 4 * bt, ss);
            if (p.strips < 1 || p.strips > LR_NN_MAX_STRIPS || p.strips * p.tps < lr_cdiv(nb, 32) || p.sstride < 1 || p.sstride > p.tps) return false;
        }
        for (int ro : rev_opts) {
            const lr_nn16_plan p = lr_nn16_plan_rev(na, nb, pairs, ro);
            if (p.strips < 1 || p.strips > LR_REV_MAX_STRIPS || p.strips * p.tps < lr_cdiv(nb, 32) || p.sstride != 0) return false;
        }
    }
    return true;
}
static_assert(lr_nn16_plans_hold(), "a launch plan leaves column tiles uncovered or exceeds a strip limit");
