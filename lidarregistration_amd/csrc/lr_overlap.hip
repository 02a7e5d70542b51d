// Voxel-grid down-sampling (one centroid per voxel) and the pair overlap measure on gfx950.
//
// Replaces Open3D's PointCloud.voxel_down_sample as the reference calls it (BalancedDatasetGenerator/GenerateBalancedSet.py:143-147,
// FCGF_FAST/net/refinement_tester.py:69-73) and the overlap measure its balanced sets are stratified by (GenerateBalancedSet.py:155-205:
// both clouds down-sampled, share of source voxels with a target voxel centre closer than sqrt(2) voxel).  Open3D is third-party and not
// vendored: its part of the contract is recalled (include/lidarreg.h), restated in tests/overlap_cpu.py.
//
// Structure.  A call serves npairs pairs x 1 or 2 clouds in one sequence of launches: the pair is the grid's z index, the cloud its y
// index; each pair owns an arena of the caller's scratch, `stride` bytes apart, headed by the control blocks of its clouds.  Per cloud:
//   1. transform (fp64, the expression of icp_iter_kernel), finite test, per-axis min / max (integer atomics on an order-preserving
//      image of the doubles: exact under any order);
//   2. cell key 3 x 21 bits into the open-addressing table of lr_cells.h; the slot keeps the smallest point index (atomicMin) and the
//      count (integer atomicAdd): neither depends on the order the threads run in;
//   3. flag + ordered compaction: output row of every cell = rank of its first point; first, count;
//   4. a STABLE cell-major ordering of the point indices: LSD radix sort on the row, 8-bit digits, per-block digit histograms, in-block
//      ranks from ordered ballots;
//   5. every cell's segment is summed left to right -- by one lane, or, for a long segment, by the wave with the loads in parallel and
//      the additions in order -- and divided by the count.
// The overlap: the target's centroids are bucketed into a hashed grid of cell ~ r (counting sort; order inside a bucket is irrelevant:
// only existence within r is asked), every source centroid tests the 27 surrounding buckets, counts through integer atomics.
// No floating-point atomic anywhere; every word a kernel reads has been written by a kernel of the same call (scratch contents are irrelevant).
// The table, the hash, the compaction steps and the block scan are the shared ones (lr_cells.h, lr_prims.h); this file owns the cell rule
// -- the floor of (p - vmb) / voxel -- and its kernels over the pairs' arenas (lr_ptr).
#include "lr_scratch.h"
#include "lr_cells.h"
#include <math.h>
#include <string.h>

#define OV_MAX_N 4194304             // points per cloud (2^22)
#define OV_CELLS 2097152.0           // 2^21 cells per axis
#define OV_NOKEY 0x00ffffff          // sort key of a dropped point: behind every row (rows <= n < 2^(8 passes))
#define OV_LIGHT 32                  // segments up to this long are summed by their own lane
#define OV_QCLAMP 1099511627776.0    // 2^40: grid coordinates of the search are clamped here (far outside the target's grid)

// one pair of a call: by value into the setup kernel, like cs_desc_table (64 * 40 bytes)
struct ov_desc { const double *xyz0, *xyz1, *T; int32_t n0, n1; lr_overlap_result *res; };
struct ov_desc_table { ov_desc d[LR_MAX_BATCH]; };
// lr_voxel_mean's caller outputs (single cloud)
struct ov_outs { double *cent; float *cent_f32; int32_t *counts, *first, *info; };
static_assert(sizeof(ov_desc_table) + sizeof(ov_outs) + 512 <= 4096, "the descriptor table no longer fits the kernel arguments");

// control block of one cloud
struct ov_cloud {
    const double *xyz;
    double T[12];
    double vmb[3];
    unsigned long long lo[3], hi[3];     // order-preserving images of the min / max
    int32_t has_T, n, n_live;            // n_live: n, or 0 once the cloud is empty or refused
    int32_t dropped, status, rows;
    uint32_t cap_mask;
    int32_t n_overlap;                   // (cloud 0)
};
struct ov_pair { ov_cloud c[2]; lr_overlap_result *res; };

struct ov_layout { size_t P, slot_of, ordA, ordB, hist, keys, first, cnt, rowof, blk, seg, cent, counts, firstrow, end; };
struct ov_args {
    char *base;
    size_t stride;
    ov_layout L[2];
    size_t bk_cnt, bk_fill, bk_pts;      // hashed grid of the target's centroids
    uint32_t bk_mask;
    int32_t clouds;
    double voxel, r, g;                  // g: edge of the search grid's cells
};

static size_t ov_buckets(size_t n)
{
    size_t c = 1024;
    while (c < n) c <<= 1;
    return c;
}
// arena of one cloud of up to n points, from byte `o`
static ov_layout ov_make_layout(size_t o, size_t n)
{
    const size_t nn = n > 0 ? n : 1, cap = lr_cells_capacity(n), nb = (nn + 255) / 256;
    ov_layout L;
    L.P = o;        o += lr_al(nn * 24);
    L.slot_of = o;  o += lr_al(nn * 4);
    L.ordA = o;     o += lr_al(nn * 4);
    L.ordB = o;     o += lr_al(nn * 4);
    L.hist = o;     o += lr_al(nb * 256 * 4);
    L.keys = o;     o += lr_al(cap * 8);
    L.first = o;    o += lr_al(cap * 4);
    L.cnt = o;      o += lr_al(cap * 4);
    L.rowof = o;    o += lr_al(cap * 4);
    L.blk = o;      o += lr_al((nb + 2) * 4);
    L.seg = o;      o += lr_al(nn * 4);
    L.cent = o;     o += lr_al(nn * 24);
    L.counts = o;   o += lr_al(nn * 4);
    L.firstrow = o; o += lr_al(nn * 4);
    L.end = o;
    return L;
}
// arena of one pair: control blocks | cloud 0 | cloud 1 | hashed grid (clouds == 2)
static size_t ov_make_args(ov_args *g, size_t n0, size_t n1, int clouds)
{
    size_t o = lr_al(sizeof(ov_pair));
    g->L[0] = ov_make_layout(o, n0); o = g->L[0].end;
    g->L[1] = g->L[0];
    g->bk_cnt = g->bk_fill = g->bk_pts = 0; g->bk_mask = 0;
    if (clouds == 2) {
        g->L[1] = ov_make_layout(o, n1); o = g->L[1].end;
        const size_t nb = ov_buckets(n1);
        g->bk_mask = (uint32_t)(nb - 1);
        g->bk_cnt = o;  o += lr_al(nb * 4);
        g->bk_fill = o; o += lr_al(nb * 4);
        g->bk_pts = o;  o += lr_al((n1 > 0 ? n1 : 1) * 24);
    }
    g->clouds = clouds;
    return o;
}

__device__ __forceinline__ ov_cloud *ov_ctl(const ov_args &g, int pair, int cl) { return &lr_ptr<ov_pair>(g, pair, 0)->c[cl]; }

// ---- setup: descriptors by value -> control blocks (no host copy, graph-capturable) ------------------------------------------
__global__ void ov_setup_kernel(ov_desc_table t, ov_args g, int npairs)
{
    const int k = threadIdx.x >> 1, cl = threadIdx.x & 1;
    if (k >= npairs || cl >= g.clouds) return;
    const ov_desc d = t.d[k];
    ov_pair *pp = lr_ptr<ov_pair>(g, k, 0);
    ov_cloud *c = &pp->c[cl];
    if (cl == 0) pp->res = d.res;
    c->xyz = cl ? d.xyz1 : d.xyz0;
    c->n = cl ? d.n1 : d.n0;
    c->n_live = c->n;
    c->has_T = cl == 0 && d.T != nullptr;
    for (int q = 0; q < 12; ++q) c->T[q] = c->has_T ? d.T[q] : (q % 5 == 0 ? 1.0 : 0.0);
    for (int a = 0; a < 3; ++a) { c->lo[a] = ~0ull; c->hi[a] = 0ull; c->vmb[a] = 0.0; }
    c->dropped = 0; c->status = 0; c->rows = 0; c->n_overlap = 0;
    c->cap_mask = (uint32_t)(lr_cells_capacity((size_t)c->n) - 1);
}

// table and bucket words the later kernels accumulate into
__global__ void __launch_bounds__(256) ov_init_kernel(ov_args g)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const ov_cloud *c = ov_ctl(g, pair, cl);
    const size_t cap = c->n > 0 ? (size_t)c->cap_mask + 1 : 0;
    unsigned long long *keys = lr_ptr<unsigned long long>(g, pair, g.L[cl].keys);
    int32_t *first = lr_ptr<int32_t>(g, pair, g.L[cl].first), *cnt = lr_ptr<int32_t>(g, pair, g.L[cl].cnt);
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += (size_t)gridDim.x * 256) { keys[s] = LR_CELL_EMPTY; first[s] = 0x7fffffff; cnt[s] = 0; }
    if (cl == 1) {
        int32_t *bc = lr_ptr<int32_t>(g, pair, g.bk_cnt), *bf = lr_ptr<int32_t>(g, pair, g.bk_fill);
        for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s <= g.bk_mask; s += (size_t)gridDim.x * 256) { bc[s] = 0; bf[s] = 0; }
    }
}

// ---- 1. transform, finite test, bounds ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ov_xform_kernel(ov_args g)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    ov_cloud *c = ov_ctl(g, pair, cl);
    const int n = c->n;
    if ((int)blockIdx.x * 256 >= n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double *P = lr_ptr<double>(g, pair, g.L[cl].P);
    int32_t *slot_of = lr_ptr<int32_t>(g, pair, g.L[cl].slot_of);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    bool bad = false;
    if (i < n) {
        const double x = c->xyz[3 * (size_t)i], y = c->xyz[3 * (size_t)i + 1], z = c->xyz[3 * (size_t)i + 2];
        double p[3] = { x, y, z };
        if (c->has_T) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = ((c->T[4 * a] * x + c->T[4 * a + 1] * y) + c->T[4 * a + 2] * z) + c->T[4 * a + 3];
        }
        bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
#pragma unroll
        for (int a = 0; a < 3; ++a) { P[3 * (size_t)i + a] = p[a]; if (!bad) { lo[a] = p[a]; hi[a] = p[a]; } }
        slot_of[i] = bad ? -1 : 0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], m)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], m)); }
    const unsigned long long nbad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (lo[a] <= hi[a]) { atomicMin(&c->lo[a], lr_ord_enc(lo[a])); atomicMax(&c->hi[a], lr_ord_enc(hi[a])); }
        if (nbad) atomicAdd(&c->dropped, __popcll(nbad));
    }
}

__global__ void ov_bounds_kernel(ov_args g)
{
    if (threadIdx.x != 0) return;
    ov_cloud *c = ov_ctl(g, blockIdx.z, blockIdx.y);
    const int kept = c->n - c->dropped;
    int status = 0;
    if (kept <= 0) status = 1;
    else {
        for (int a = 0; a < 3; ++a) {
            const double lo = lr_ord_dec(c->lo[a]), hi = lr_ord_dec(c->hi[a]);
            const double vmb = lo - g.voxel * 0.5;
            c->vmb[a] = vmb;
            if (!((hi - vmb) / g.voxel < OV_CELLS)) status = 2;
        }
    }
    c->status = status;
    if (status) c->n_live = 0;
}

// ---- 2. cells ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ov_insert_kernel(ov_args g)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const ov_cloud *c = ov_ctl(g, pair, cl);
    const int n = c->n_live;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t *slot_of = lr_ptr<int32_t>(g, pair, g.L[cl].slot_of);
    if (slot_of[i] < 0) return;                      // dropped
    const double *P = lr_ptr<double>(g, pair, g.L[cl].P);
    unsigned long long ca[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)                      // 0 <= cell < 2^21 (ov_bounds_kernel)
        ca[a] = (unsigned long long)((int)floor((P[3 * (size_t)i + a] - c->vmb[a]) / g.voxel) & 0x1fffff);
    const unsigned s = lr_cells_claim(lr_ptr<unsigned long long>(g, pair, g.L[cl].keys), c->cap_mask, lr_cells_pack(ca[0], ca[1], ca[2]));
    atomicMin(&lr_ptr<int32_t>(g, pair, g.L[cl].first)[s], i);
    atomicAdd(&lr_ptr<int32_t>(g, pair, g.L[cl].cnt)[s], 1);
    slot_of[i] = (int32_t)s;
}

// ---- 3. flag + ordered compaction ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ov_is_first(const ov_args &g, int pair, int cl, int i, int n, int &slot)
{
    slot = -1;
    return i < n && lr_cells_is_first(lr_ptr<int32_t>(g, pair, g.L[cl].first), lr_ptr<int32_t>(g, pair, g.L[cl].slot_of), i, slot);
}

__global__ void __launch_bounds__(256) ov_flag_kernel(ov_args g)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const int n = ov_ctl(g, pair, cl)->n_live;
    if ((int)blockIdx.x * 256 >= n) return;
    int slot;
    lr_block_count(ov_is_first(g, pair, cl, blockIdx.x * 256 + threadIdx.x, n, slot), lr_ptr<int32_t>(g, pair, g.L[cl].blk));
}

__global__ void __launch_bounds__(256) ov_compact_kernel(ov_args g)
{
    __shared__ int s_w[4], s_p[4];
    const int pair = blockIdx.z, cl = blockIdx.y;
    ov_cloud *c = ov_ctl(g, pair, cl);
    const int n = c->n_live;
    if ((int)blockIdx.x * 256 >= n) return;
    const int before = lr_blocks_before(lr_ptr<int32_t>(g, pair, g.L[cl].blk)), i = blockIdx.x * 256 + threadIdx.x;
    int slot, prefix;
    const bool k = ov_is_first(g, pair, cl, i, n, slot);
    const int row = lr_ordered_slot(k, before, s_w, s_p, prefix);
    if (k) {
        lr_ptr<int32_t>(g, pair, g.L[cl].rowof)[slot] = row;
        lr_ptr<int32_t>(g, pair, g.L[cl].firstrow)[row] = i;
        lr_ptr<int32_t>(g, pair, g.L[cl].counts)[row] = lr_ptr<int32_t>(g, pair, g.L[cl].cnt)[slot];
    }
    if ((int)blockIdx.x == (n - 1) / 256 && threadIdx.x == 0) c->rows = prefix + s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// ---- 4. stable LSD radix sort of the point indices on their row ----------------------------------------------------------------
__device__ __forceinline__ int ov_key(const ov_args &g, int pair, int cl, int i)
{
    const int s = lr_ptr<int32_t>(g, pair, g.L[cl].slot_of)[i];
    return s < 0 ? OV_NOKEY : lr_ptr<int32_t>(g, pair, g.L[cl].rowof)[s];
}
// rank of this thread's element among the block's elements of the same digit, in thread order; s_cnt[w * 256 + d] = elements of
// digit d in wave w
__device__ __forceinline__ int ov_block_rank(int digit, bool valid, int *s_cnt)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 1024; k += 256) s_cnt[k] = 0;
    __syncthreads();
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool b = (digit >> bit) & 1;
        const unsigned long long bal = __ballot(valid && b);
        same &= b ? bal : ~bal;
    }
    const int rank_w = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank_w == 0) s_cnt[wave * 256 + digit] = __popcll(same);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += s_cnt[w * 256 + digit];
    return off + rank_w;
}
// element t of the pass's input sequence (pass 0: the identity) and its digit
__device__ __forceinline__ bool ov_sort_item(const ov_args &g, int pair, int cl, int n, int pass, int &idx, int &digit)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    idx = 0; digit = 0;
    if (t >= n) return false;
    idx = pass == 0 ? t : lr_ptr<int32_t>(g, pair, (pass & 1) ? g.L[cl].ordA : g.L[cl].ordB)[t];
    digit = (ov_key(g, pair, cl, idx) >> (8 * pass)) & 255;
    return true;
}

__global__ void __launch_bounds__(256) ov_sort_hist_kernel(ov_args g, int pass)
{
    __shared__ int s_cnt[1024];
    const int pair = blockIdx.z, cl = blockIdx.y;
    const int n = ov_ctl(g, pair, cl)->n_live;
    if ((int)blockIdx.x * 256 >= n) return;
    int idx, digit;
    const bool valid = ov_sort_item(g, pair, cl, n, pass, idx, digit);
    ov_block_rank(digit, valid, s_cnt);
    const int nb = (n + 255) / 256, d = threadIdx.x;
    lr_ptr<int32_t>(g, pair, g.L[cl].hist)[(size_t)d * nb + blockIdx.x] = (s_cnt[d] + s_cnt[256 + d]) + (s_cnt[512 + d] + s_cnt[768 + d]);
}

__global__ void __launch_bounds__(1024) ov_sort_scan_kernel(ov_args g)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const int n = ov_ctl(g, pair, cl)->n_live;
    lr_block_exscan(lr_ptr<int32_t>(g, pair, g.L[cl].hist), (size_t)256 * ((n + 255) / 256));
}

__global__ void __launch_bounds__(256) ov_sort_scatter_kernel(ov_args g, int pass)
{
    __shared__ int s_cnt[1024];
    const int pair = blockIdx.z, cl = blockIdx.y;
    const int n = ov_ctl(g, pair, cl)->n_live;
    if ((int)blockIdx.x * 256 >= n) return;
    int idx, digit;
    const bool valid = ov_sort_item(g, pair, cl, n, pass, idx, digit);
    const int rank = ov_block_rank(digit, valid, s_cnt);
    const int nb = (n + 255) / 256;
    // digit-major offsets: every position is below n (the histogram sums to n)
    if (valid) lr_ptr<int32_t>(g, pair, (pass & 1) ? g.L[cl].ordB : g.L[cl].ordA)[lr_ptr<int32_t>(g, pair, g.L[cl].hist)[(size_t)digit * nb + blockIdx.x] + rank] = idx;
}

// segment start of every row in the sorted sequence
__global__ void __launch_bounds__(256) ov_heads_kernel(ov_args g, int passes)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const ov_cloud *c = ov_ctl(g, pair, cl);
    const int kept = c->n_live - c->dropped;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= kept) return;
    const int32_t *ord = lr_ptr<int32_t>(g, pair, (passes & 1) ? g.L[cl].ordA : g.L[cl].ordB);
    const int key = ov_key(g, pair, cl, ord[t]);
    if (t == 0 || ov_key(g, pair, cl, ord[t - 1]) != key) lr_ptr<int32_t>(g, pair, g.L[cl].seg)[key] = t;
}

// ---- 5. centroids ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ov_centroid_kernel(ov_args g, int passes, ov_outs outs)
{
    const int pair = blockIdx.z, cl = blockIdx.y;
    const ov_cloud *c = ov_ctl(g, pair, cl);
    const int rows = c->rows;
    if ((int)blockIdx.x * 256 >= rows) return;
    const int row = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool active = row < rows;
    const int32_t *ord = lr_ptr<int32_t>(g, pair, (passes & 1) ? g.L[cl].ordA : g.L[cl].ordB);
    const double *P = lr_ptr<double>(g, pair, g.L[cl].P);
    const int32_t *counts = lr_ptr<int32_t>(g, pair, g.L[cl].counts);
    const int start = active ? lr_ptr<int32_t>(g, pair, g.L[cl].seg)[row] : 0, cnt = active ? counts[row] : 0;
    double s[3] = { 0.0, 0.0, 0.0 };
    const bool heavy = cnt > OV_LIGHT;
    if (!heavy)
        for (int k = 0; k < cnt; ++k) {
            const size_t i = (size_t)ord[start + k];
            s[0] += P[3 * i]; s[1] += P[3 * i + 1]; s[2] += P[3 * i + 2];
        }
    // long segments: one at a time by the whole wave -- 64 loads in flight, the additions in segment order on every lane
    unsigned long long hm = __ballot(heavy);
    while (hm) {
        const int l = __ffsll((long long)hm) - 1;
        hm &= hm - 1;
        const int hs = __shfl(start, l), hc = __shfl(cnt, l);
        double a[3] = { 0.0, 0.0, 0.0 };
        for (int base = 0; base < hc; base += 64) {
            const int m = hc - base < 64 ? hc - base : 64;
            double p[3] = { 0.0, 0.0, 0.0 };
            if (lane < m) {
                const size_t i = (size_t)ord[hs + base + lane];
                p[0] = P[3 * i]; p[1] = P[3 * i + 1]; p[2] = P[3 * i + 2];
            }
            for (int j = 0; j < m; ++j) { a[0] += __shfl(p[0], j); a[1] += __shfl(p[1], j); a[2] += __shfl(p[2], j); }
        }
        if (lane == l) { s[0] = a[0]; s[1] = a[1]; s[2] = a[2]; }
    }
    if (!active) return;
    double *cent = lr_ptr<double>(g, pair, g.L[cl].cent);
    const int first = lr_ptr<int32_t>(g, pair, g.L[cl].firstrow)[row];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double v = s[a] / (double)cnt;
        cent[3 * (size_t)row + a] = v;
        if (outs.cent) outs.cent[3 * (size_t)row + a] = v;
        if (outs.cent_f32) outs.cent_f32[3 * (size_t)row + a] = (float)v;
    }
    if (outs.counts) outs.counts[row] = cnt;
    if (outs.first) outs.first[row] = first;
}

__global__ void ov_info_kernel(ov_args g, ov_outs outs)
{
    if (threadIdx.x != 0) return;
    const ov_cloud *c = ov_ctl(g, 0, 0);
    outs.info[0] = c->rows; outs.info[1] = c->dropped; outs.info[2] = c->status; outs.info[3] = 0;
}

// ---- 6. the search ---------------------------------------------------------------------------------------------------------------
// grid cell of a centroid, relative to the target's origin; clamped (NaN included) far outside the target's own cells
__device__ __forceinline__ void ov_qcell(const double *p, const double *o, double gcell, long long q[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double v = floor((p[a] - o[a]) / gcell);
        if (!(v > -OV_QCLAMP)) v = -OV_QCLAMP;
        if (!(v < OV_QCLAMP)) v = OV_QCLAMP;
        q[a] = (long long)v;
    }
}
__device__ __forceinline__ uint32_t ov_bucket(long long x, long long y, long long z, uint32_t mask)
{
    return (uint32_t)lr_mix64((unsigned long long)x * 73856093ull ^ (unsigned long long)y * 19349663ull ^ (unsigned long long)z * 83492791ull) & mask;
}

__global__ void __launch_bounds__(256) ov_bhist_kernel(ov_args g)
{
    const int pair = blockIdx.z;
    const ov_cloud *c1 = ov_ctl(g, pair, 1);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= c1->rows) return;
    long long q[3];
    ov_qcell(lr_ptr<double>(g, pair, g.L[1].cent) + 3 * (size_t)t, c1->vmb, g.g, q);
    atomicAdd(&lr_ptr<int32_t>(g, pair, g.bk_cnt)[ov_bucket(q[0], q[1], q[2], g.bk_mask)], 1);
}

__global__ void __launch_bounds__(1024) ov_bscan_kernel(ov_args g)
{
    if (ov_ctl(g, blockIdx.z, 1)->rows == 0) return;
    lr_block_exscan(lr_ptr<int32_t>(g, blockIdx.z, g.bk_cnt), (size_t)g.bk_mask + 1);
}

__global__ void __launch_bounds__(256) ov_bscatter_kernel(ov_args g)
{
    const int pair = blockIdx.z;
    const ov_cloud *c1 = ov_ctl(g, pair, 1);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= c1->rows) return;
    const double *p = lr_ptr<double>(g, pair, g.L[1].cent) + 3 * (size_t)t;
    long long q[3];
    ov_qcell(p, c1->vmb, g.g, q);
    const uint32_t b = ov_bucket(q[0], q[1], q[2], g.bk_mask);
    // bucket starts + fills stay below rows (the counts sum to it)
    const int at = lr_ptr<int32_t>(g, pair, g.bk_cnt)[b] + atomicAdd(&lr_ptr<int32_t>(g, pair, g.bk_fill)[b], 1);
    double *out = lr_ptr<double>(g, pair, g.bk_pts) + 3 * (size_t)at;
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
}

__global__ void __launch_bounds__(256) ov_search_kernel(ov_args g)
{
    const int pair = blockIdx.z;
    ov_cloud *c0 = ov_ctl(g, pair, 0);
    const ov_cloud *c1 = ov_ctl(g, pair, 1);
    const int rows0 = c0->rows;
    if ((int)blockIdx.x * 256 >= rows0 || c1->rows == 0) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (t < rows0) {
        const double *a = lr_ptr<double>(g, pair, g.L[0].cent) + 3 * (size_t)t;
        const double ax = a[0], ay = a[1], az = a[2];
        long long q[3];
        ov_qcell(a, c1->vmb, g.g, q);
        const int32_t *bs = lr_ptr<int32_t>(g, pair, g.bk_cnt), *bf = lr_ptr<int32_t>(g, pair, g.bk_fill);
        const double *pts = lr_ptr<double>(g, pair, g.bk_pts);
        for (int cc = 0; cc < 27 && !hit; ++cc) {
            const uint32_t b = ov_bucket(q[0] + (cc % 3) - 1, q[1] + ((cc / 3) % 3) - 1, q[2] + (cc / 9) - 1, g.bk_mask);
            const int s = bs[b], e = s + bf[b];
            for (int u = s; u < e; ++u) {
                const double dx = ax - pts[3 * (size_t)u], dy = ay - pts[3 * (size_t)u + 1], dz = az - pts[3 * (size_t)u + 2];
                if (__dsqrt_rn((dx * dx + dy * dy) + dz * dz) < g.r) { hit = true; break; }
            }
        }
    }
    const unsigned long long bal = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&c0->n_overlap, __popcll(bal));
}

// ---- 7. result blocks ------------------------------------------------------------------------------------------------------------
__global__ void ov_result_kernel(ov_args g, int npairs)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const ov_pair *pp = lr_ptr<ov_pair>(g, k, 0);
    const ov_cloud &a = pp->c[0], &b = pp->c[1];
    lr_overlap_result r;
    r.status = (a.status == 2 || b.status == 2) ? 2 : ((a.status || b.status) ? 1 : 0);
    r.n0_ds = a.rows; r.n1_ds = b.rows; r.n0_dropped = a.dropped; r.n1_dropped = b.dropped;
    r.n_overlap = 0; r.frac = 0.0; r.frac_sym = 0.0;
    if (r.status == 0) {
        r.n_overlap = a.n_overlap;
        r.frac = (double)r.n_overlap / (double)a.rows;
        const double back = (double)r.n_overlap / (double)b.rows;
        r.frac_sym = back < r.frac ? back : r.frac;
    }
    *pp->res = r;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_overlap_params) == 24 && sizeof(lr_overlap_result) == 40, "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_voxel_mean_scratch_bytes(int n)
{
    if (n < 0 || n > OV_MAX_N) return 0;
    ov_args g;
    return ov_make_args(&g, (size_t)n, 0, 1);
}

extern "C" size_t lr_overlap_scratch_bytes(int max_n0, int max_n1)
{
    if (max_n0 < 0 || max_n0 > OV_MAX_N || max_n1 < 0 || max_n1 > OV_MAX_N) return 0;
    ov_args g;
    return ov_make_args(&g, (size_t)max_n0, (size_t)max_n1, 2);
}

// every cloud of the call through stages 1..5
static void ov_launch_clouds(const ov_desc_table &t, const ov_outs &outs, const ov_args &g, int npairs, int mx, hipStream_t st)
{
    const int nb = lr_cdiv(mx > 0 ? mx : 1, 256), passes = mx < 256 ? 1 : (mx < 65536 ? 2 : 3);
    const dim3 grid(nb, g.clouds, npairs), one(1, g.clouds, npairs);
    const int ib = nb < 64 ? 4 * nb : 256;           // init blocks: the table has up to 4 slots per point, the grid strides
    hipLaunchKernelGGL(ov_setup_kernel, dim3(1), dim3(128), 0, st, t, g, npairs);
    hipLaunchKernelGGL(ov_init_kernel, dim3(ib, g.clouds, npairs), dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_xform_kernel, grid, dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_bounds_kernel, one, dim3(64), 0, st, g);
    hipLaunchKernelGGL(ov_insert_kernel, grid, dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_flag_kernel, grid, dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_compact_kernel, grid, dim3(256), 0, st, g);
    for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(ov_sort_hist_kernel, grid, dim3(256), 0, st, g, pass);
        hipLaunchKernelGGL(ov_sort_scan_kernel, one, dim3(1024), 0, st, g);
        hipLaunchKernelGGL(ov_sort_scatter_kernel, grid, dim3(256), 0, st, g, pass);
    }
    hipLaunchKernelGGL(ov_heads_kernel, grid, dim3(256), 0, st, g, passes);
    hipLaunchKernelGGL(ov_centroid_kernel, grid, dim3(256), 0, st, g, passes, outs);
}

extern "C" int lr_voxel_mean(const double *xyz, int n, const double *T, double voxel_size, double *cent, float *cent_f32, int32_t *counts,
                             int32_t *first, int32_t *info, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_voxel_mean";
    LR_REFUSE_UNLESS(voxel_size > 0.0 && isfinite(voxel_size), LR_EINVAL, "voxel_size must be positive and finite");
    LR_REFUSE_UNLESS(n >= 0 && n <= OV_MAX_N, LR_EINVAL, "n must lie in 0..4194304");
    LR_REFUSE_UNLESS(info, LR_EINVAL, "null info");
    LR_REFUSE_UNLESS(n == 0 || xyz, LR_EINVAL, "null xyz");
    ov_args g;
    const size_t need = ov_make_args(&g, (size_t)n, 0, 1);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, need, "lr_voxel_mean_scratch_bytes(n)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch); g.stride = need;
    g.voxel = voxel_size; g.r = 0.0; g.g = 1.0;
    ov_desc_table t;
    memset(&t, 0, sizeof t);
    t.d[0].xyz0 = xyz; t.d[0].T = T; t.d[0].n0 = n;
    const ov_outs outs = { cent, cent_f32, counts, first, info };
    hipStream_t st = (hipStream_t)stream;
    ov_launch_clouds(t, outs, g, 1, n, st);
    hipLaunchKernelGGL(ov_info_kernel, dim3(1), dim3(64), 0, st, g, outs);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

static int ov_run(const char *who, int npairs, const double *const *xyz0, const int32_t *n0, const double *const *xyz1, const int32_t *n1,
                  const double *const *T, const lr_overlap_params *p, lr_overlap_result *results, void *scratch, size_t scratch_bytes, void *stream)
{
    LR_CHECK_STRUCT_SIZE(lr_overlap_params, p, who);
    LR_REFUSE_UNLESS(p->voxel_size > 0.0 && isfinite(p->voxel_size), LR_EINVAL, "voxel_size must be positive and finite");
    LR_REFUSE_UNLESS(p->radius >= 0.0 && isfinite(p->radius), LR_EINVAL, "radius must be finite and not negative");
    // one centroid per voxel bounds what a search cell of edge r can hold; a radius far from the voxel size would unbound the search
    LR_REFUSE_UNLESS(p->radius == 0.0 || (p->radius >= p->voxel_size * 0.0625 && p->radius <= p->voxel_size * 4.0), LR_EINVAL, "radius must be 0 or lie in voxel_size / 16 .. 4 voxel_size");
    LR_REFUSE_UNLESS(npairs >= 1 && npairs <= LR_MAX_BATCH, LR_EINVAL, "npairs must lie in 1..64");
    LR_REFUSE_UNLESS(xyz0 && n0 && xyz1 && n1 && results, LR_EINVAL, "null pointer");
    ov_desc_table t;
    memset(&t, 0, sizeof t);
    int mx0 = 0, mx1 = 0;
    for (int k = 0; k < npairs; ++k) {
        LR_REFUSE_UNLESS(n0[k] >= 0 && n0[k] <= OV_MAX_N && n1[k] >= 0 && n1[k] <= OV_MAX_N, LR_EINVAL, "n0 / n1 must lie in 0..4194304");
        LR_REFUSE_UNLESS((n0[k] == 0 || xyz0[k]) && (n1[k] == 0 || xyz1[k]), LR_EINVAL, "null xyz0 / xyz1");
        t.d[k] = ov_desc{ xyz0[k], xyz1[k], T ? T[k] : nullptr, n0[k], n1[k], results + k };
        mx0 = n0[k] > mx0 ? n0[k] : mx0; mx1 = n1[k] > mx1 ? n1[k] : mx1;
    }
    ov_args g;
    const size_t per = ov_make_args(&g, (size_t)mx0, (size_t)mx1, 2);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, per * (size_t)npairs, "npairs * lr_overlap_scratch_bytes(max n0, max n1)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch); g.stride = per;
    g.voxel = p->voxel_size;
    g.r = p->radius == 0.0 ? sqrt(2.0) * p->voxel_size : p->radius;
    g.g = g.r * (1.0 + 1.0 / 65536.0);               // a little wider than r: partners within r lie in adjacent cells whatever the quotients' rounding
    const ov_outs none = { nullptr, nullptr, nullptr, nullptr, nullptr };
    hipStream_t st = (hipStream_t)stream;
    ov_launch_clouds(t, none, g, npairs, mx0 > mx1 ? mx0 : mx1, st);
    hipLaunchKernelGGL(ov_bhist_kernel, dim3(lr_cdiv(mx1 > 0 ? mx1 : 1, 256), 1, npairs), dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_bscan_kernel, dim3(1, 1, npairs), dim3(1024), 0, st, g);
    hipLaunchKernelGGL(ov_bscatter_kernel, dim3(lr_cdiv(mx1 > 0 ? mx1 : 1, 256), 1, npairs), dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_search_kernel, dim3(lr_cdiv(mx0 > 0 ? mx0 : 1, 256), 1, npairs), dim3(256), 0, st, g);
    hipLaunchKernelGGL(ov_result_kernel, dim3(1), dim3(64), 0, st, g, npairs);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_overlap_batch(int npairs, const double *const *xyz0, const int32_t *n0, const double *const *xyz1, const int32_t *n1,
                                const double *const *T, const lr_overlap_params *p, lr_overlap_result *results, void *scratch,
                                size_t scratch_bytes, void *stream)
{
    return ov_run("lr_overlap_batch", npairs, xyz0, n0, xyz1, n1, T, p, results, scratch, scratch_bytes, stream);
}

extern "C" int lr_overlap(const double *xyz0, int n0, const double *xyz1, int n1, const double *T, const lr_overlap_params *p,
                          lr_overlap_result *result, void *scratch, size_t scratch_bytes, void *stream)
{
    return ov_run("lr_overlap", 1, &xyz0, &n0, &xyz1, &n1, &T, p, result, scratch, scratch_bytes, stream);
}
