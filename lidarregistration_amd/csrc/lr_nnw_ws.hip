// The NN stage of a wide workspace (lr_workspace_create_wide: descriptors of 33..128 numbers): what lr_nn16_prep / _run / _reverse are to
// the narrow one.  Exact f32 on the matrix cores, the hot path and the contract of lr_nnw_dev.h (lr_nn_wide's, which is orc_nn_top2's).
//
//   nnwb_prep_kernel     a thread per row of either cloud of every pair: the norm chain, ONCE per call for both directions; a cloud-1 row
//                        also starts as "nobody's target" (flag 0, reverse NN -1); block 0 clears the pair's counter block when asked
//   nnwb_kernel<NS, TOP2, GATHER>
//                        a block = nnw_block over 128 rows and one strip of column tiles of the pair blockIdx.z names.  The grid is sized
//                        on the host from the largest clouds of the call; a block past its pair's rows or tiles leaves before the first
//                        barrier.  GATHER: the rows are the entries of a device list of device length (the reverse direction)
//   nnwb_merge_kernel    more than one strip: a thread per row merges the strips' partials (in the arena) in ascending strip order under
//                        (s, j) -- a total order: the result does not depend on the strip count
//   reverse              top-1 of cloud-1 rows against cloud 0 over the unique forward targets only (matching.py:224-225): a flag per
//                        targeted column (plain stores), the list of flagged columns in ascending j (lr_block_count / lr_ordered_slot),
//                        the kernel's A rows gathered through it; rev[j] = -1 for every other column, as lr_nn16_reverse leaves it
// No atomics, no host synchronisation, no allocation: a call is graph-capturable like the narrow one.
#include "lr_nnw_dev.h"
#include "lr_prims.h"

struct nnwb_args {
    const float *A, *B;              // row / column cloud of a single-pair call (a batched call reads its descriptor table)
    int na, nb, dim;
    int rev;                         // 1: the rows are cloud 1 (A = F1 of the descriptor table, B = F0)
    const float *nrmA, *nrmB;        // arena pointers from here on (moved by pair * stride)
    const int32_t *list, *n_list;    // GATHER: the rows and their live number
    nnw_part *part; size_t prow;     // partials [strips][prow] (strips > 1 only)
    int rblocks, strips, tps;        // the call's plan: row blocks and strips of the grid, tiles per strip
    int32_t *idx1, *idx2; float *s1, *s2;      // outputs per row (GATHER: idx1[list[row]])
    lr_zargs z;
};

__global__ void __launch_bounds__(256)
nnwb_prep_kernel(const float *__restrict__ F0, int n0, const float *__restrict__ F1, int n1, int dim, float *__restrict__ nrm0, float *__restrict__ nrm1,
                 uint8_t *__restrict__ flag, int32_t *__restrict__ rev, int32_t *__restrict__ counters, int zero_counters, lr_zargs z)
{
    if (z.descs) { const lr_pair_desc d = z.descs[blockIdx.z]; F0 = d.F0; n0 = d.n0; F1 = d.F1; n1 = d.n1; }
    lr_z(nrm0, z, blockIdx.z); lr_z(nrm1, z, blockIdx.z); lr_z(flag, z, blockIdx.z); lr_z(rev, z, blockIdx.z); lr_z(counters, z, blockIdx.z);
    if (zero_counters && blockIdx.x == 0 && (int)threadIdx.x < LR_CNT_TOTAL) counters[threadIdx.x] = 0;
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)n0 + (size_t)n1) return;
    const bool second = r >= (size_t)n0;
    const size_t row = second ? r - (size_t)n0 : r;
    const float *x = (second ? F1 : F0) + row * (size_t)dim;
    float acc = 0.0f;
    for (int k = 0; k < dim; ++k) acc = fmaf(x[k], x[k], acc);
    (second ? nrm1 : nrm0)[row] = acc;
    if (second) { flag[row] = 0; rev[row] = -1; }
}

// live strips of a pair whose column cloud has `tiles` tiles under the call's plan
__device__ __forceinline__ int nnwb_live_strips(int tiles, int tps, int strips) { return min(strips, (tiles + tps - 1) / tps); }

template <int NS, bool TOP2, bool GATHER> __global__ void __launch_bounds__(256) nnwb_kernel(nnwb_args g)
{
    const int pair = blockIdx.z;
    const float *A = g.A, *B = g.B;
    int na = g.na, nb = g.nb;
    if (g.z.descs) {
        const lr_pair_desc d = g.z.descs[pair];
        A = g.rev ? d.F1 : d.F0; B = g.rev ? d.F0 : d.F1; na = g.rev ? d.n1 : d.n0; nb = g.rev ? d.n0 : d.n1;
    }
    const float *nrmA = g.nrmA, *nrmB = g.nrmB;
    const int32_t *list = g.list, *n_list = g.n_list;
    nnw_part *part = g.part;
    int32_t *idx1 = g.idx1, *idx2 = g.idx2;
    float *s1 = g.s1, *s2 = g.s2;
    lr_z(nrmA, g.z, pair); lr_z(nrmB, g.z, pair); lr_z(list, g.z, pair); lr_z(n_list, g.z, pair); lr_z(part, g.z, pair);
    lr_z(idx1, g.z, pair); lr_z(idx2, g.z, pair); lr_z(s1, g.z, pair); lr_z(s2, g.z, pair);
    if constexpr (GATHER) na = min(na, *n_list);
    const int rb = (int)blockIdx.x % g.rblocks, strip = (int)blockIdx.x / g.rblocks;
    const int tiles = (nb + 31) / 32, t0 = strip * g.tps;
    // (block-uniform, before the first barrier: the grid is sized for the largest pair of the call)
    if (rb * NNW_ROWS >= na || t0 >= tiles) return;
    const int t1 = min(t0 + g.tps, tiles);
    const bool partial = g.strips > 1;
    const size_t prow = g.prow;
    auto emit = [&](size_t row, float b1, int32_t j1, float b2, int32_t j2) {
        if (partial) { part[(size_t)strip * prow + row] = nnw_part{ b1, j1, b2, j2 }; return; }
        const size_t o = GATHER ? (size_t)list[row] : row;
        idx1[o] = j1;
        if (TOP2 && idx2) idx2[o] = j2;
        if (s1) s1[o] = b1;
        if (TOP2 && s2) s2[o] = b2;
    };
    if constexpr (GATHER) nnw_block<NS, TOP2>(A, nrmA, (size_t)na, [&](size_t i) { return (size_t)list[i]; }, B, nrmB, (size_t)nb, g.dim, rb, t0, t1, emit);
    else nnw_block<NS, TOP2>(A, nrmA, (size_t)na, [](size_t i) { return i; }, B, nrmB, (size_t)nb, g.dim, rb, t0, t1, emit);
}

__global__ void __launch_bounds__(256) nnwb_merge_kernel(nnwb_args g)
{
    const int pair = blockIdx.z;
    int na = g.na, nb = g.nb;
    if (g.z.descs) { const lr_pair_desc d = g.z.descs[pair]; na = g.rev ? d.n1 : d.n0; nb = g.rev ? d.n0 : d.n1; }
    const int32_t *list = g.list, *n_list = g.n_list;
    const nnw_part *part = g.part;
    int32_t *idx1 = g.idx1, *idx2 = g.idx2;
    float *s1 = g.s1, *s2 = g.s2;
    lr_z(list, g.z, pair); lr_z(n_list, g.z, pair); lr_z(part, g.z, pair);
    lr_z(idx1, g.z, pair); lr_z(idx2, g.z, pair); lr_z(s1, g.z, pair); lr_z(s2, g.z, pair);
    if (list) na = min(na, *n_list);
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= (size_t)na) return;
    const int live = nnwb_live_strips((nb + 31) / 32, g.tps, g.strips);      // (the strips past the pair's own tiles wrote nothing)
    const nnw_part a = part[row];
    float b1 = a.s1, b2 = a.s2;
    int32_t j1 = a.i1, j2 = a.i2;
    for (int s = 1; s < live; ++s) {
        const nnw_part c = part[(size_t)s * g.prow + row];
        nnw_merge2(b1, j1, b2, j2, c.s1, c.i1, c.s2, c.i2);
    }
    const size_t o = list ? (size_t)list[row] : row;
    idx1[o] = j1;
    if (idx2) idx2[o] = j2;
    if (s1) s1[o] = b1;
    if (s2) s2[o] = b2;
}

// ------------------------------------------------------------------ the reverse direction's row list
__global__ void __launch_bounds__(256)
nnwb_target_kernel(int n0, int n1, const int32_t *__restrict__ idx1, uint8_t *__restrict__ flag, lr_zargs z)
{
    if (z.descs) { n0 = z.descs[blockIdx.z].n0; n1 = z.descs[blockIdx.z].n1; }
    lr_z(idx1, z, blockIdx.z); lr_z(flag, z, blockIdx.z);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n0) return;
    const int j = idx1[i];
    if ((unsigned)j < (unsigned)n1) flag[j] = 1;      // (plain store: every writer of a byte writes the same value)
}

__global__ void __launch_bounds__(256)
nnwb_count_kernel(int n1, const uint8_t *__restrict__ flag, int32_t *__restrict__ blk_cnt, lr_zargs z)
{
    if (z.descs) n1 = z.descs[blockIdx.z].n1;
    lr_z(flag, z, blockIdx.z); lr_z(blk_cnt, z, blockIdx.z);
    const int j = blockIdx.x * 256 + threadIdx.x;
    lr_block_count(j < n1 && flag[j] != 0, blk_cnt);
}

// the flagged columns in ascending j; the last block leaves their number
__global__ void __launch_bounds__(256)
nnwb_list_kernel(int n1, const uint8_t *__restrict__ flag, const int32_t *__restrict__ blk_cnt, int32_t *__restrict__ list, int32_t *__restrict__ n_list, lr_zargs z)
{
    __shared__ int s_wave[4];
    __shared__ int s_part[4];
    if (z.descs) n1 = z.descs[blockIdx.z].n1;
    lr_z(flag, z, blockIdx.z); lr_z(blk_cnt, z, blockIdx.z); lr_z(list, z, blockIdx.z); lr_z(n_list, z, blockIdx.z);
    const int before = lr_blocks_before(blk_cnt), j = blockIdx.x * 256 + threadIdx.x;
    const bool k = j < n1 && flag[j] != 0;
    int prefix;
    const int slot = lr_ordered_slot(k, before, s_wave, s_part, prefix);
    if (k) list[slot] = j;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_list = prefix + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// ------------------------------------------------------------------ host side
// Partials a wide arena holds: strips <= ceil(NNW_BLOCKS / row blocks) and <= NNW_MAX_STRIPS, rows <= 128 row blocks, so
// strips x rows <= 128 NNW_BLOCKS + 128 row blocks whatever the sizes of a call are.
size_t lr_nnw_part_entries(int max_n) { return (size_t)NNW_ROWS * NNW_BLOCKS + (size_t)NNW_ROWS * (size_t)lr_cdiv(max_n, NNW_ROWS); }

// rows x cols of the largest pair of the call -> the grid: strips so that pairs x row blocks x strips is about NNW_BLOCKS
static void nnwb_plan(const lr_call &c, nnwb_args &g, int rows, int cols)
{
    const int tiles = lr_cdiv(cols, 32);
    g.rblocks = lr_cdiv(rows, NNW_ROWS);
    int strips = lr_cdiv(NNW_BLOCKS, g.rblocks * c.pairs);
    if (strips > NNW_MAX_STRIPS) strips = NNW_MAX_STRIPS;
    if (strips > tiles) strips = tiles;
    // (the arena's partials: lr_nnw_part_entries covers every plan; the loop is the bound the kernels rely on, stated where they are launched)
    while (strips > 1 && (size_t)strips * (size_t)rows > c.ws->nnw_part_cap) --strips;
    if (strips < 1) strips = 1;
    g.tps = lr_cdiv(tiles, strips);
    g.strips = lr_cdiv(tiles, g.tps);      // (no empty strip)
    g.prow = (size_t)rows;
    g.part = c.ws->nnw_parts;
}

template <bool TOP2, bool GATHER> static void nnwb_launch(const lr_call &c, const nnwb_args &g)
{
    const dim3 grid((unsigned)(g.rblocks * g.strips), 1, (unsigned)c.pairs);
    switch (nnw_steps(g.dim)) {
    case 18: nnwb_kernel<18, TOP2, GATHER><<<grid, dim3(256), 0, c.st>>>(g); break;
    case 24: nnwb_kernel<24, TOP2, GATHER><<<grid, dim3(256), 0, c.st>>>(g); break;
    case 32: nnwb_kernel<32, TOP2, GATHER><<<grid, dim3(256), 0, c.st>>>(g); break;
    case 48: nnwb_kernel<48, TOP2, GATHER><<<grid, dim3(256), 0, c.st>>>(g); break;
    default: nnwb_kernel<64, TOP2, GATHER><<<grid, dim3(256), 0, c.st>>>(g); break;
    }
    if (g.strips > 1) nnwb_merge_kernel<<<dim3((unsigned)lr_cdiv((int)g.prow, 256), 1, (unsigned)c.pairs), dim3(256), 0, c.st>>>(g);
}

int lr_nnw_prep(const lr_call &c, const float *F0, int n0, const float *F1, int n1, int dim, bool zero_counters)
{
    lr_workspace *ws = c.ws;
    const size_t rows = (size_t)n0 + (size_t)n1;
    nnwb_prep_kernel<<<dim3((unsigned)((rows + 255) / 256), 1, (unsigned)c.pairs), dim3(256), 0, c.st>>>(F0, n0, F1, n1, dim, ws->nrm0, ws->nrm1, ws->nnw_flag,
                                                                                                        ws->rev_idx1, ws->counters, zero_counters ? 1 : 0, c.z);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

int lr_nnw_run(const lr_call &c, const float *F0, int n0, const float *F1, int n1, int dim, int32_t *idx1, int32_t *idx2, float *s1, float *s2)
{
    lr_workspace *ws = c.ws;
    nnwb_args g = {};
    g.A = F0; g.B = F1; g.na = n0; g.nb = n1; g.dim = dim; g.rev = 0;
    g.nrmA = ws->nrm0; g.nrmB = ws->nrm1;
    g.idx1 = idx1; g.idx2 = idx2; g.s1 = s1; g.s2 = idx2 ? s2 : nullptr;
    g.z = c.z;
    nnwb_plan(c, g, n0, n1);
    LR_TRY_HIP(lr_timer_mark(c, LR_EV_FWD_FILTER_BEGIN));
    if (idx2) nnwb_launch<true, false>(c, g); else nnwb_launch<false, false>(c, g);
    LR_TRY_HIP(lr_timer_mark(c, LR_EV_FWD_FILTER_END));
    LR_LAUNCH_CHECK();
    return LR_OK;
}

int lr_nnw_reverse(const lr_call &c, const float *F0, int n0, const float *F1, int n1, int dim, const int32_t *fwd_idx1, int32_t *rev)
{
    lr_workspace *ws = c.ws;
    int32_t *n_rows = ws->counters + LR_CNT_NREV;
    const dim3 g0((unsigned)lr_cdiv(n0, 256), 1, (unsigned)c.pairs), g1((unsigned)lr_cdiv(n1, 256), 1, (unsigned)c.pairs);
    nnwb_target_kernel<<<g0, dim3(256), 0, c.st>>>(n0, n1, fwd_idx1, ws->nnw_flag, c.z);
    nnwb_count_kernel<<<g1, dim3(256), 0, c.st>>>(n1, ws->nnw_flag, ws->nnw_blk, c.z);
    nnwb_list_kernel<<<g1, dim3(256), 0, c.st>>>(n1, ws->nnw_flag, ws->nnw_blk, ws->nnw_list, n_rows, c.z);
    nnwb_args g = {};
    g.A = F1; g.B = F0; g.na = n1; g.nb = n0; g.dim = dim; g.rev = 1;
    g.nrmA = ws->nrm1; g.nrmB = ws->nrm0;
    g.list = ws->nnw_list; g.n_list = n_rows;
    g.idx1 = rev;
    g.z = c.z;
    nnwb_plan(c, g, n1, n0);      // (the live length of the list is a device value: the grid is for all n1 rows, surplus blocks leave)
    LR_TRY_HIP(lr_timer_mark(c, LR_EV_REV_FILTER_BEGIN));
    nnwb_launch<false, true>(c, g);
    LR_TRY_HIP(lr_timer_mark(c, LR_EV_REV_FILTER_END));
    LR_LAUNCH_CHECK();
    return LR_OK;
}
