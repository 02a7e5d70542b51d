// lr_dgr_inlier: Deep Global Registration's inlier network (ResUNetBN2C(1, 1, conv1_kernel_size 3, D = 6): a sparse 6-D ResUNet of 23
// convolutions with 3^6 = 729 offsets each) on integer 6-D cells, one logit per correspondence.
// Contract n3 (F1 .. F7, F9, F10, F12 in six dimensions with I1 .. I5) of include/lidarreg.h; DESIGN.md §20.
//
// Keys.  A cell is taken relative to the call's origin 8 floor(min_a / 8) per axis (an integer min-reduction on the device) and packed
// into six 10-bit fields, field_a = (c_a - origin_a) + 8, axis 0 most significant: ascending keys are ascending lexicographic cells, the
// +8 leaves room for the -8 neighbour of level 3, and a coarse cell is the key with the low bits of its fields cleared.  A level's rows are
// kept as their keys.  Levels, tables and the sort are those of lr_fcgf.hip (lr_sparse.h, lr_cells.h).
// Maps (once per call): dense gather tables [rows][729] int32, -1 = absent, one thread per entry: nbr[l] (F2), dn[l] (F3), up[l] (F4).
// Convolutions.  d6_conv_kernel is fc_conv_kernel's 729-offset sibling: the same tile, v_mfma_f32_32x32x2_f32 chain, register-staged
// double buffering and fused epilogue; the tile's table slice (64 x 729 entries) does not fit in LDS, so the block passes over it once
// to flag the offsets at which some row has a neighbour, lists them in ascending order, and reads each step's 64 / 128 entries from the
// table, one step ahead of the row gather that needs them.  conv1 (Cin = 1, ones) and final (Cout = 1) are vector kernels.
#include "lr_scratch.h"
#include "lr_sparse.h"
#include <limits.h>

#define D6_MAX_N 131072
#define D6_NK 729
#define D6_STAGES 23
#define D6_BIAS 8                    // field = (cell - origin) + 8
#define D6_REL_MAX 1007              // cell - origin above this on an axis: status 3 (field + 8 <= 1023)
#define D6_FIELD 0x3ffull
#define D6_CTL_BYTES 256
#define D6_AS 36                     // floats per row of the gathered tile in LDS (32 + 4: rows stay 16-byte aligned)

struct d6_ctl { int32_t status, n[4], mn[6], pad[5]; };      // mn: the per-axis minimum of the input
static_assert(sizeof(d6_ctl) <= D6_CTL_BYTES, "d6_ctl outgrew its place at the head of the scratch");
struct d6_stage { int k3, cin, cout; };

// widths = C1 C2 C3 C4 (down) T4 T3 T2 T1 (up); each a multiple of 32 in 32 .. 256 (I5)
static inline bool d6_widths_ok(const int32_t *w)
{
    if (!w) return false;
    for (int i = 0; i < 8; ++i) if (w[i] < 32 || w[i] > 256 || (w[i] & 31)) return false;
    return true;
}
static inline void d6_stage_table(const int32_t *w, d6_stage *t)      // t[1 .. 23] (I4)
{
    const int C1 = w[0], C2 = w[1], C3 = w[2], C4 = w[3], T4 = w[4], T3 = w[5], T2 = w[6], T1 = w[7];
    const int io[D6_STAGES + 1][2] = { { 0, 0 }, { 1, C1 }, { C1, C1 }, { C1, C1 }, { C1, C2 }, { C2, C2 }, { C2, C2 }, { C2, C3 }, { C3, C3 }, { C3, C3 },
        { C3, C4 }, { C4, C4 }, { C4, C4 }, { C4, T4 }, { T4, T4 }, { T4, T4 }, { T4 + C3, T3 }, { T3, T3 }, { T3, T3 }, { T3 + C2, T2 }, { T2, T2 },
        { T2, T2 }, { T2 + C1, T1 }, { T1, 1 } };
    for (int s = 1; s <= D6_STAGES; ++s) t[s] = d6_stage{ s >= 22 ? 1 : D6_NK, io[s][0], io[s][1] };
}
static inline size_t d6_stage_floats(const d6_stage &s) { return (size_t)s.k3 * s.cin * s.cout + 2 * (size_t)s.cout; }
static inline int d6_max_width(const int32_t *w) { int m = 0; for (int i = 0; i < 8; ++i) m = w[i] > m ? w[i] : m; return m; }

struct d6_layout { size_t keys, val, rowkey, sort, tbl, X, Y, Z, S1, S2, S4, total, m, cap_max; };
static d6_layout d6_make_layout(size_t max_n, const int32_t *w)
{
    d6_layout L;
    const size_t m = (max_n + 63) & ~size_t(63);      // rows every array is sized for: all sizes below are multiples of 256 bytes
    const size_t mw = (size_t)d6_max_width(w);
    L.m = m;
    L.cap_max = 4 * m + 1024;                         // lr_cells_capacity(n) < 4 n, or 1024
    size_t o = D6_CTL_BYTES;
    L.keys = o;   o += 4 * L.cap_max * 8;
    L.val = o;    o += 4 * L.cap_max * 4;
    L.rowkey = o; o += 4 * m * 8;
    L.sort = o;   o += (2 * m + FC_SORT_CHUNK) * 8;
    L.tbl = o;    o += 10 * m * D6_NK * 4;            // nbr[0..3], dn[0..2], up[0..2]
    L.X = o;      o += m * mw * 4;
    L.Y = o;      o += m * mw * 4;
    L.Z = o;      o += m * mw * 4;
    L.S1 = o;     o += m * (size_t)w[0] * 4;
    L.S2 = o;     o += m * (size_t)w[1] * 4;
    L.S4 = o;     o += m * (size_t)w[2] * 4;
    L.total = o;
    return L;
}

// ---- maps -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int d6_origin(const d6_ctl *ctl, int a) { return (ctl->mn[a] >> 3) << 3; }      // 8 floor(min / 8)
// the key of input row i, LR_CELL_EMPTY when an axis lies past the extent limit
__device__ __forceinline__ fc_u64 d6_row_key(const int32_t *__restrict__ coords, int i, const d6_ctl *ctl)
{
    fc_u64 key = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const long long rel = (long long)coords[6 * (size_t)i + a] - (long long)d6_origin(ctl, a);      // >= 0: the origin is below the minimum
        ok = ok && rel <= D6_REL_MAX;
        key = (key << 10) | ((fc_u64)(rel + D6_BIAS) & D6_FIELD);
    }
    return ok ? key : LR_CELL_EMPTY;
}
// the level-(lvl+1) cell of a level-lvl key: floor(v / 2^sh) 2^sh on every axis (the bias is a multiple of 8)
__device__ __forceinline__ fc_u64 d6_coarse_of(fc_u64 key, int sh)
{
    const fc_u64 low = (1ull << sh) - 1;
    return key & ~(low * ((1ull << 50) | (1ull << 40) | (1ull << 30) | (1ull << 20) | (1ull << 10) | 1ull));
}

// the control block and the four tables' words the later kernels accumulate into: a call is kernel launches only
__global__ void __launch_bounds__(256) d6_init_kernel(fc_u64 *__restrict__ keys, int32_t *__restrict__ val, size_t slots, d6_ctl *ctl)
{
    if (blockIdx.x == 0) {
        for (int w = threadIdx.x; w < D6_CTL_BYTES / 4; w += 256) reinterpret_cast<int32_t *>(ctl)[w] = 0;
        __syncthreads();
        if (threadIdx.x < 6) ctl->mn[threadIdx.x] = INT_MAX;
    }
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (size_t)gridDim.x * 256) { keys[s] = LR_CELL_EMPTY; val[s] = 0x7f7f7f7f; }
}
__global__ void __launch_bounds__(256) d6_min_kernel(const int32_t *__restrict__ coords, int n, d6_ctl *ctl)
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
__global__ void __launch_bounds__(256) d6_l0_insert_kernel(const int32_t *__restrict__ coords, int n, fc_u64 *keys, int32_t *val, unsigned mask,
                                                           fc_u64 *__restrict__ rowkey, d6_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const fc_u64 key = d6_row_key(coords, i, ctl);
    rowkey[i] = key;
    if (key == LR_CELL_EMPTY) { atomicMax(&ctl->status, 3); return; }
    atomicMin(&val[lr_cells_claim(keys, mask, key)], i);
}
__global__ void __launch_bounds__(256) d6_l0_check_kernel(const fc_u64 *__restrict__ rowkey, int n, const fc_u64 *__restrict__ keys, const int32_t *__restrict__ val,
                                                          unsigned mask, d6_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) ctl->n[0] = n;
    if (i >= n) return;
    const fc_u64 key = rowkey[i];
    if (key == LR_CELL_EMPTY) return;
    const int s = fc_find(keys, mask, key);
    if (s < 0 || val[s] != i) atomicMax(&ctl->status, 2);
}
__global__ void __launch_bounds__(256) d6_coarse_insert_kernel(const fc_u64 *__restrict__ rowkey, int lvl, fc_u64 *keys, int32_t *val, unsigned mask, const d6_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || i >= ctl->n[lvl]) return;
    atomicMin(&val[lr_cells_claim(keys, mask, d6_coarse_of(rowkey[i], lvl + 1))], i);
}
// sortbuf[i] = the coarse key of fine row i when it stands for its cell (smallest row of the cell), no key otherwise and behind the rows
__global__ void __launch_bounds__(256) d6_coarse_mark_kernel(const fc_u64 *__restrict__ rowkey, int lvl, const fc_u64 *__restrict__ keys, const int32_t *__restrict__ val,
                                                             unsigned mask, fc_u64 *__restrict__ sortbuf, int n_sort, d6_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status) return;
    fc_u64 out = LR_CELL_EMPTY;
    if (i < ctl->n[lvl]) {
        const fc_u64 key = d6_coarse_of(rowkey[i], lvl + 1);
        const int s = fc_find(keys, mask, key);
        if (s >= 0 && val[s] == i) out = key;
    }
    if (i < n_sort) sortbuf[i] = out;
    const unsigned long long live = __ballot(out != LR_CELL_EMPTY);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&ctl->n[lvl + 1], __popcll(live));
}
// the sorted keys are the level's rows: row r of level lvl = the cell of rank r (I2)
__global__ void __launch_bounds__(256) d6_index_kernel(const fc_u64 *__restrict__ sorted, int lvl, const fc_u64 *__restrict__ keys, int32_t *__restrict__ val,
                                                       unsigned mask, fc_u64 *__restrict__ rowkey, const d6_ctl *ctl)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || r >= ctl->n[lvl]) return;
    const fc_u64 key = sorted[r];
    const int s = fc_find(keys, mask, key);
    if (s >= 0) val[s] = r;
    rowkey[r] = key;
}
// tbl[r][k] = the row of (cell of rowkey[r]) + o(k) step in the table, -1 when absent; r < n[lvl_out];
// I1: idx(o) = sum_a (o_a + 1) 3^a, axis 0 fastest -- the one place the offset order lives on the device
__global__ void __launch_bounds__(256) d6_nbr_kernel(const fc_u64 *__restrict__ rowkey, int lvl_out, const fc_u64 *__restrict__ keys, const int32_t *__restrict__ val,
                                                     unsigned mask, int step, int32_t *__restrict__ tbl, const d6_ctl *ctl)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || gid >= (size_t)ctl->n[lvl_out] * D6_NK) return;
    const int r = (int)(gid / D6_NK);
    int k = (int)(gid - (size_t)r * D6_NK);
    const fc_u64 key = rowkey[r];
    fc_u64 q = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const int f = (int)((key >> (10 * (5 - a))) & D6_FIELD) + (k % 3 - 1) * step;
        k /= 3;
        ok = ok && f >= 0 && f <= (int)D6_FIELD;
        q |= ((fc_u64)f & D6_FIELD) << (10 * (5 - a));
    }
    int idx = -1;
    if (ok) {
        const int s = fc_find(keys, mask, q);
        if (s >= 0) idx = val[s];
    }
    tbl[gid] = idx;
}

// ---- convolutions -------------------------------------------------------------------------------------------------------------------
// conv1: Cin = 1 with the feature ones: a vector kernel over the row's 729 entries; BatchNorm folded, no ReLU
__global__ void __launch_bounds__(256) d6_conv1_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ W, const float *__restrict__ scale,
                                                       const float *__restrict__ offset, int cout, float *__restrict__ out, const d6_ctl *ctl)
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

struct d6_conv {
    const float *in0, *in1;          // the input's rows: [.][c0] and, behind them in channel order, [.][c1] (in1 unused at c1 = 0)
    int c0, c1;
    const int32_t *nbr;              // [rows][729] input rows, -1 = absent; null: one offset and the row itself (1x1)
    const float *W, *scale, *offset; // W[nk][c0 + c1][Cout]
    const float *res;                // nullable residual [rows][Cout]
    float *out;                      // [rows][Cout]
    int relu, lvl, cout;             // rows = ctl->n[lvl]
};

// block tile: 32 WR rows x 32 WC columns (grid y: the column tiles of Cout); wave (wr, wc) owns one 32 x 32 accumulator.  The rows and the
// weight slab of the next (offset, 32 channels) step are fetched into registers while the matrix cores work on the current one.
template <int WR, int WC> __global__ void __launch_bounds__(256) d6_conv_kernel(d6_conv a, const d6_ctl *ctl)
{
    constexpr int TM = 32 * WR, TN = 32 * WC;
    static_assert(WR * WC == 4, "four waves");
    __shared__ float As[TM * D6_AS];
    __shared__ float Bs[32 * TN];
    __shared__ int s_any[D6_NK], s_live[D6_NK], s_nlive;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ctl->status) return;
    const int rows = ctl->n[a.lvl], row0 = blockIdx.x * TM, nk = a.nbr ? D6_NK : 1, col0 = blockIdx.y * TN, cout = a.cout;
    if (row0 >= rows) return;
    for (int k = tid; k < nk; k += 256) s_any[k] = a.nbr ? 0 : 1;
    __syncthreads();
    if (a.nbr) {                                                       // one coalesced pass over the tile's slice of the table: the live rows'
        const int live_rows = rows - row0 < TM ? rows - row0 : TM;     // entries are contiguous, and 16-byte aligned (row0 is a multiple of 64)
        const int total = live_rows * D6_NK, total4 = total >> 2;
        const int32_t *slice = a.nbr + (size_t)row0 * D6_NK;
        int k = (4 * tid) % D6_NK;                                     // the offset of entry 4 e; 1024 = 729 + 295
        for (int e = tid; e < total4; e += 256) {
            const int4 v = reinterpret_cast<const int4 *>(slice)[e];
            const int k1 = k + 1 < D6_NK ? k + 1 : k + 1 - D6_NK, k2 = k + 2 < D6_NK ? k + 2 : k + 2 - D6_NK, k3 = k + 3 < D6_NK ? k + 3 : k + 3 - D6_NK;
            if (v.x >= 0) s_any[k] = 1;
            if (v.y >= 0) s_any[k1] = 1;
            if (v.z >= 0) s_any[k2] = 1;
            if (v.w >= 0) s_any[k3] = 1;
            k += 295; if (k >= D6_NK) k -= D6_NK;
        }
        for (int e = 4 * total4 + tid; e < total; e += 256) if (slice[e] >= 0) s_any[e % D6_NK] = 1;
    }
    __syncthreads();
    if (wave == 0) {                                                   // the offsets some row of the tile has a neighbour at, ascending: the
        int base = 0;                                                  // others are skipped, block-uniformly (F5: the same bits)
        for (int k0 = 0; k0 < nk; k0 += 64) {
            const int k = k0 + lane;
            const bool on = k < nk && s_any[k] != 0;
            const unsigned long long m = __ballot(on);
            if (on) s_live[base + __popcll(m & ((1ull << lane) - 1ull))] = k;
            base += __popcll(m);
        }
        if (lane == 0) s_nlive = base;
    }
    __syncthreads();
    fc_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const int wr = wave / WC, wc = wave % WC, cin = a.c0 + a.c1, nch = cin >> 5, steps = s_nlive * nch;
    const int a_at = (wr * 32 + (lane & 31)) * D6_AS + (lane >> 5), b_at = (lane >> 5) * TN + wc * 32 + (lane & 31);
    float4 ra[WR], rb0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb1 = rb0;
    // this thread's rows' entries of step s's offset, straight from the table (-1: absent, or a row past the level's count)
    auto entries = [&](int s, int (&idx)[WR]) {
        const int k = s_live[s / nch];
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const int row = row0 + ((tid + 256 * i) >> 3);
            idx[i] = row < rows ? (a.nbr ? a.nbr[(size_t)row * D6_NK + k] : row) : -1;
        }
    };
    int nidx[WR];                                                      // the entries of the step the next round fetches: read one round
    if (steps > 0) entries(0, nidx);                                   // ahead, so that a round's row gather does not wait for them
    // step s = (live offset s / nch, channels 32 (s % nch) ..).  Round `it` puts step it (fetched in the round before) into LDS, fetches
    // the rows and the slab of W of step it + 1 into ra / rb, and multiplies step it; round -1 only fetches.
    for (int it = -1; it < steps; ++it) {
        if (it >= 0) {
            __syncthreads();                                           // the previous step's reads of As / Bs are done
#pragma unroll
            for (int i = 0; i < WR; ++i) { const int e = tid + 256 * i; *reinterpret_cast<float4 *>(&As[(e >> 3) * D6_AS + 4 * (e & 7)]) = ra[i]; }
            *reinterpret_cast<float4 *>(&Bs[(tid / (TN / 4)) * TN + 4 * (tid % (TN / 4))]) = rb0;
            if constexpr (WC == 2) *reinterpret_cast<float4 *>(&Bs[((tid + 256) / (TN / 4)) * TN + 4 * (tid % (TN / 4))]) = rb1;
            __syncthreads();
        }
        if (it + 1 < steps) {
            const int k = s_live[(it + 1) / nch], ch = ((it + 1) % nch) << 5;
            const bool first = ch < a.c0;
            const float *src = first ? a.in0 : a.in1;
            const int cs = first ? a.c0 : a.c1, co = first ? ch : ch - a.c0;
            int idx[WR];
#pragma unroll
            for (int i = 0; i < WR; ++i) idx[i] = nidx[i];
            if (it + 2 < steps) entries(it + 2, nidx);
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const int e = tid + 256 * i;
                ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (idx[i] >= 0) ra[i] = *reinterpret_cast<const float4 *>(src + (size_t)idx[i] * cs + co + 4 * (e & 7));
            }
            const float *w = a.W + ((size_t)k * cin + ch + tid / (TN / 4)) * cout + col0 + 4 * (tid % (TN / 4));
            rb0 = *reinterpret_cast<const float4 *>(w);
            if constexpr (WC == 2) rb1 = *reinterpret_cast<const float4 *>(w + (size_t)(256 / (TN / 4)) * cout);
        }
        if (it >= 0) {
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[a_at + 2 * kk], Bs[b_at + 2 * kk * TN], acc, 0, 0, 0);
        }
    }
    const int col = col0 + wc * 32 + (lane & 31);
    const float sc = a.scale[col], of = a.offset[col];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = row0 + wr * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (row < rows) {
            float y = fmaf(sc, acc[q], of);
            if (a.res) y = y + a.res[(size_t)row * cout + col];
            a.out[(size_t)row * cout + col] = a.relu ? fc_relu(y) : y;
        }
    }
}

// final (I4): Cout = 1: one fmaf chain over the row's channels from +0, then one add of the bias
__global__ void __launch_bounds__(256) d6_final_kernel(const float *__restrict__ x, int cin, const float *__restrict__ W, float *__restrict__ out, const d6_ctl *ctl)
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
__global__ void __launch_bounds__(256) d6_finish_kernel(const float *__restrict__ f, int n, float *__restrict__ out, const d6_ctl *ctl, lr_dgr_inlier_result *res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int status = ctl->status;
    if (i == 0) { res->status = status; res->n = n; res->n_tap = status ? 0 : n; res->reserved = 0; }
    if (i < n) out[i] = status ? 0.0f : f[i];
}
// tap: the activations [n_level][cout] of the stage, the level's cells [n_level][6], the result block
__global__ void __launch_bounds__(256) d6_tap_kernel(const float *__restrict__ f, int cout, int lvl, const fc_u64 *__restrict__ rowkey, int n, float *__restrict__ out,
                                                     int32_t *__restrict__ tap_coords, const d6_ctl *ctl, lr_dgr_inlier_result *res)
{
    const int status = ctl->status, rows = status ? 0 : ctl->n[lvl];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid == 0) { res->status = status; res->n = n; res->n_tap = rows; res->reserved = 0; }
    if (gid < (size_t)rows * cout) out[gid] = f[gid];
    if (tap_coords && gid < (size_t)rows * 6) {
        const int r = (int)(gid / 6), a = (int)(gid - (size_t)r * 6);
        tap_coords[gid] = (int)((rowkey[r] >> (10 * (5 - a))) & D6_FIELD) - D6_BIAS + d6_origin(ctl, a);
    }
}
__global__ void d6_empty_kernel(lr_dgr_inlier_result *res) { res->status = 0; res->n = 0; res->n_tap = 0; res->reserved = 0; }

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_dgr_inlier_params) == 40 && sizeof(lr_dgr_inlier_result) == 16, "ABI structs changed: update include/lidarreg.h and _ext.py together");

extern "C" size_t lr_dgr_inlier_weights_bytes(const int32_t *widths)
{
    if (!d6_widths_ok(widths)) return 0;
    d6_stage t[D6_STAGES + 1];
    d6_stage_table(widths, t);
    size_t f = 0;
    for (int s = 1; s <= D6_STAGES; ++s) f += d6_stage_floats(t[s]);
    return f * sizeof(float);
}

extern "C" size_t lr_dgr_inlier_scratch_bytes(int max_n, const int32_t *widths)
{
    if (max_n < 0 || max_n > D6_MAX_N || !d6_widths_ok(widths)) return 0;
    return d6_make_layout((size_t)max_n, widths).total;
}

namespace {
struct d6_run {
    hipStream_t st;
    char *base;
    d6_layout L;
    d6_ctl *ctl;
    int n;
    d6_stage t[D6_STAGES + 1];
    const float *w[D6_STAGES + 1];      // the stages' blocks in the blob
    fc_u64 *keys[4], *rowkey[4];
    int32_t *val[4], *nbr[4], *dn[3], *up[3];
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    int grid(size_t items) const { return (int)((items + 255) / 256); }

    void conv(int s, const float *in0, int c0, const float *in1, int c1, const int32_t *tbl, const float *res, float *out, int relu, int lvl) const
    {
        const d6_stage &g = t[s];
        const float *W = w[s];
        const size_t nw = (size_t)g.k3 * g.cin * g.cout;
        const d6_conv a = { in0, in1, c0, c1, tbl, W, W + nw, W + nw + g.cout, res, out, relu, lvl, g.cout };
        const d6_ctl *c = ctl;
        // (the grid covers n rows, the most a level can have: the blocks past the level's live count leave at once)
        if (g.cout % 64) hipLaunchKernelGGL((d6_conv_kernel<4, 1>), dim3(lr_cdiv(n, 128), g.cout / 32), dim3(256), 0, st, a, c);
        else             hipLaunchKernelGGL((d6_conv_kernel<2, 2>), dim3(lr_cdiv(n, 64), g.cout / 64), dim3(256), 0, st, a, c);
    }
};
}

// The 23 stages (I4); done(s, buf, lvl) is told that `buf` holds stage s of level lvl and ends the sequence by returning true.
template <typename Done> static bool d6_stages(const d6_run &R, const int32_t *wd, Done done)
{
    const d6_layout &L = R.L;
    float *X = R.at<float>(L.X), *Y = R.at<float>(L.Y), *Z = R.at<float>(L.Z), *S1 = R.at<float>(L.S1), *S2 = R.at<float>(L.S2), *S4 = R.at<float>(L.S4);
    const int C1 = wd[0], C2 = wd[1], C3 = wd[2], C4 = wd[3], T4 = wd[4], T3 = wd[5], T2 = wd[6], T1 = wd[7];
    int s = 0;
    // a residual block: its two stages
    auto block = [&](const float *in, float *tmp, float *out, int C, int lvl) -> bool {
        R.conv(s + 1, in, C, nullptr, 0, R.nbr[lvl], nullptr, tmp, 1, lvl);
        if (done(++s, tmp, lvl)) return true;
        R.conv(s + 1, tmp, C, nullptr, 0, R.nbr[lvl], in, out, 1, lvl);
        return done(++s, out, lvl);
    };
    hipLaunchKernelGGL(d6_conv1_kernel, dim3(R.grid((size_t)R.n * C1)), dim3(256), 0, R.st, R.nbr[0], R.w[1], R.w[1] + (size_t)D6_NK * C1,
                       R.w[1] + (size_t)D6_NK * C1 + C1, C1, X, R.ctl);
    if (done(++s, X, 0)) return true;
    if (block(X, Y, S1, C1, 0)) return true;
    R.conv(4, S1, C1, nullptr, 0, R.dn[0], nullptr, X, 0, 1);              if (done(++s, X, 1)) return true;
    if (block(X, Y, S2, C2, 1)) return true;
    R.conv(7, S2, C2, nullptr, 0, R.dn[1], nullptr, X, 0, 2);              if (done(++s, X, 2)) return true;
    if (block(X, Y, S4, C3, 2)) return true;
    R.conv(10, S4, C3, nullptr, 0, R.dn[2], nullptr, X, 0, 3);             if (done(++s, X, 3)) return true;
    if (block(X, Y, Z, C4, 3)) return true;
    R.conv(13, Z, C4, nullptr, 0, R.up[2], nullptr, X, 0, 2);              if (done(++s, X, 2)) return true;
    if (block(X, Y, Z, T4, 2)) return true;
    R.conv(16, Z, T4, S4, C3, R.up[1], nullptr, X, 0, 1);                  if (done(++s, X, 1)) return true;
    if (block(X, Y, Z, T3, 1)) return true;
    R.conv(19, Z, T3, S2, C2, R.up[0], nullptr, X, 0, 0);                  if (done(++s, X, 0)) return true;
    if (block(X, Y, Z, T2, 0)) return true;
    R.conv(22, Z, T2, S1, C1, nullptr, nullptr, X, 1, 0);                  if (done(++s, X, 0)) return true;
    hipLaunchKernelGGL(d6_final_kernel, dim3(R.grid((size_t)R.n)), dim3(256), 0, R.st, X, T1, R.w[23], Y, R.ctl);
    return done(++s, Y, 0);
}

extern "C" int lr_dgr_inlier(const int32_t *coords, int n, const float *weights, size_t weights_bytes, const lr_dgr_inlier_params *p,
                             lr_dgr_inlier_result *result, float *logit_out, int32_t *tap_coords, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_dgr_inlier";
    LR_CHECK_STRUCT_SIZE(lr_dgr_inlier_params, p, who);
    LR_REFUSE_UNLESS(d6_widths_ok(p->widths), LR_EINVAL, "every width must be a multiple of 32 in 32 .. 256");
    LR_REFUSE_UNLESS(p->tap >= 0 && p->tap <= D6_STAGES, LR_EINVAL, "tap must lie in 0 .. 23");
    LR_REFUSE_UNLESS(n >= 0 && n <= D6_MAX_N, LR_EINVAL, "n must lie in 0 .. 131072");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_dgr_inlier_weights_bytes(p->widths), LR_EINVAL, "weights_bytes is below lr_dgr_inlier_weights_bytes(widths)");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    LR_REFUSE_UNLESS(n == 0 || (coords && logit_out), LR_EINVAL, "null coords or logit_out");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_dgr_inlier_scratch_bytes(n, p->widths), "lr_dgr_inlier_scratch_bytes(n, widths)", LR_EINVAL,
                                stream, nullptr));

    d6_run R;
    R.st = (hipStream_t)stream;
    hipStream_t st = R.st;
    if (n == 0) {
        hipLaunchKernelGGL(d6_empty_kernel, dim3(1), dim3(1), 0, st, result);
        LR_LAUNCH_CHECK();
        return LR_OK;
    }
    R.base = reinterpret_cast<char *>(scratch);
    R.L = d6_make_layout((size_t)n, p->widths);
    const d6_layout &L = R.L;
    R.ctl = R.at<d6_ctl>(0);
    R.n = n;
    d6_stage_table(p->widths, R.t);
    { const float *W = weights; for (int s = 1; s <= D6_STAGES; ++s) { R.w[s] = W; W += d6_stage_floats(R.t[s]); } }
    const size_t cap = lr_cells_capacity((size_t)n), m = L.m;
    const unsigned mask = (unsigned)(cap - 1);
    for (int l = 0; l < 4; ++l) {
        R.keys[l] = R.at<fc_u64>(L.keys) + (size_t)l * L.cap_max;
        R.val[l] = R.at<int32_t>(L.val) + (size_t)l * L.cap_max;
        R.rowkey[l] = R.at<fc_u64>(L.rowkey) + (size_t)l * m;
        R.nbr[l] = R.at<int32_t>(L.tbl) + (size_t)l * m * D6_NK;
        if (l < 3) { R.dn[l] = R.at<int32_t>(L.tbl) + (size_t)(4 + l) * m * D6_NK; R.up[l] = R.at<int32_t>(L.tbl) + (size_t)(7 + l) * m * D6_NK; }
    }
    fc_u64 *sortbuf = R.at<fc_u64>(L.sort);
    d6_ctl *ctl = R.ctl;
    const int gn = R.grid((size_t)n), gt = R.grid((size_t)n * D6_NK);

    // maps
    {
        const size_t slots = 4 * L.cap_max, blocks = (slots + 255) / 256;
        hipLaunchKernelGGL(d6_init_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, R.keys[0], R.val[0], slots, ctl);
    }
    hipLaunchKernelGGL(d6_min_kernel, dim3(gn), dim3(256), 0, st, coords, n, ctl);
    hipLaunchKernelGGL(d6_l0_insert_kernel, dim3(gn), dim3(256), 0, st, coords, n, R.keys[0], R.val[0], mask, R.rowkey[0], ctl);
    hipLaunchKernelGGL(d6_l0_check_kernel, dim3(gn), dim3(256), 0, st, R.rowkey[0], n, R.keys[0], R.val[0], mask, ctl);
    unsigned n_sort = FC_SORT_CHUNK;
    while (n_sort < (unsigned)n) n_sort <<= 1;
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL(d6_coarse_insert_kernel, dim3(gn), dim3(256), 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, ctl);
        hipLaunchKernelGGL(d6_coarse_mark_kernel, dim3(R.grid(n_sort)), dim3(256), 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, sortbuf, (int)n_sort, ctl);
        fc_sort_launch(sortbuf, n_sort, st);
        hipLaunchKernelGGL(d6_index_kernel, dim3(gn), dim3(256), 0, st, sortbuf, l + 1, R.keys[l + 1], R.val[l + 1], mask, R.rowkey[l + 1], ctl);
    }
    for (int l = 0; l < 4; ++l)
        hipLaunchKernelGGL(d6_nbr_kernel, dim3(gt), dim3(256), 0, st, R.rowkey[l], l, R.keys[l], R.val[l], mask, 1 << l, R.nbr[l], ctl);
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL(d6_nbr_kernel, dim3(gt), dim3(256), 0, st, R.rowkey[l + 1], l + 1, R.keys[l], R.val[l], mask, 1 << l, R.dn[l], ctl);
        hipLaunchKernelGGL(d6_nbr_kernel, dim3(gt), dim3(256), 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, -(1 << l), R.up[l], ctl);
    }

    // a tap ends the call behind its stage
    const int tap = p->tap;
    const bool end = d6_stages(R, p->widths, [&](int s, const float *buf, int lvl) -> bool {
        if (tap != s) return false;
        const int cout = R.t[s].cout;
        const size_t items = (size_t)n * (cout > 6 ? cout : 6);
        hipLaunchKernelGGL(d6_tap_kernel, dim3(R.grid(items)), dim3(256), 0, st, buf, cout, lvl, R.rowkey[lvl], n, logit_out, tap_coords, ctl, result);
        return true;
    });
    if (!end) hipLaunchKernelGGL(d6_finish_kernel, dim3(gn), dim3(256), 0, st, R.at<float>(L.Y), n, logit_out, ctl, result);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
