// The sparse ResUNet the two networks share (lr_fcgf.hip with lr_fcgf_batch.h: three dimensions, 27 / 125 offsets; lr_dgr6.hip: six
// dimensions, 729 offsets), not part of the ABI: the key codec, the map kernels on a level's rows kept as their keys, the gather
// convolution, the stage table, the scratch layout and the 23-stage schedule.  An entry point keeps its argument checks, its level-0
// step (how a row's key and its status word are found) and its two ends (conv1, the last stage, what leaves the call).
// The kernels are static or templates on a codec / table form that one translation unit alone instantiates.
#pragma once
#include "lr_cells.h"
#include <limits.h>

#define FC_SORT_CHUNK 2048
#define SP_STAGES 23
#define SP_AS 36                     // floats per row of the gathered tile in LDS (32 + 4: rows stay 16-byte aligned)

typedef unsigned long long fc_u64;
typedef float fc_f32x16 __attribute__((ext_vector_type(16)));
constexpr int sp_ipow(int b, int e) { return e ? b * sp_ipow(b, e - 1) : 1; }

// the head of every call's control block.  mn: the per-axis minimum of the input (lr_dgr6.hip; the FCGF calls leave it 0: no origin)
struct sp_ctl { int32_t status, n[4], mn[6], pad[5]; };
__device__ __forceinline__ int sp_origin(const sp_ctl *ctl, int a) { return (ctl->mn[a] >> 3) << 3; }      // 8 floor(min / 8)

// A key is D fields of B bits, axis 0 most significant; whatever lies above bit D B is a tag that every operation carries unchanged.
// A field is a cell coordinate plus a bias that is a multiple of 8, so a coarse cell is the key with the low bits of its fields cleared.
template <int D, int B> struct sp_codec {
    static_assert(D * B <= 63, "the top bit stays clear: LR_CELL_EMPTY sorts behind every key");
    static constexpr int dims = D;
    static constexpr fc_u64 FIELD = (1ull << B) - 1;
    static constexpr fc_u64 ones() { fc_u64 o = 0; for (int a = 0; a < D; ++a) o |= 1ull << (B * a); return o; }
    __device__ static __forceinline__ int field(fc_u64 key, int a) { return (int)((key >> (B * (D - 1 - a))) & FIELD); }
    // the level-(lvl+1) cell of a level-lvl key: floor(v / 2^sh) 2^sh on every axis
    __device__ static __forceinline__ fc_u64 coarse(fc_u64 key, int sh) { return key & ~(((1ull << sh) - 1) * ones()); }
    // q = the key of (cell + o(k) step), idx(o) = sum_a (o_a + K/2) K^a: axis 0 fastest (F2, I1 -- the one place the offset order lives on
    // the device); false when a field leaves [0, 2^B): such a neighbour is absent
    __device__ static __forceinline__ bool neighbour(fc_u64 key, int k, int K, int step, fc_u64 &q)
    {
        bool ok = true;
        q = key & ~(FIELD * ones());
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const int f = field(key, a) + (k % K - (K >> 1)) * step;
            k /= K;
            ok = ok && f >= 0 && f <= (int)FIELD;
            q |= ((fc_u64)f & FIELD) << (B * (D - 1 - a));
        }
        return ok;
    }
};

// the slot of `key`, -1 when the table does not hold it (at most half of the slots are taken: an empty one is met)
__device__ __forceinline__ int fc_find(const fc_u64 *__restrict__ keys, unsigned mask, fc_u64 key)
{
    unsigned s = (unsigned)lr_mix64(key) & mask;
    for (;;) {
        const fc_u64 k = keys[s];
        if (k == key) return (int)s;
        if (k == LR_CELL_EMPTY) return -1;
        s = (s + 1) & mask;
    }
}

// bitonic sort, ascending, of n_sort = 2^p >= 2048 keys: the steps with a distance below 2048 run in LDS, 2048 keys per block
static __global__ void __launch_bounds__(1024) fc_sort_local_kernel(fc_u64 *__restrict__ keys, unsigned k_lo, unsigned k_hi)
{
    __shared__ fc_u64 s[FC_SORT_CHUNK];
    const unsigned tid = threadIdx.x, base = blockIdx.x * FC_SORT_CHUNK;
    s[tid] = keys[base + tid]; s[tid + 1024] = keys[base + tid + 1024];
    __syncthreads();
    for (unsigned k = k_lo; k <= k_hi; k <<= 1)
        for (unsigned j = (k >> 1) < 1024u ? (k >> 1) : 1024u; j >= 1; j >>= 1) {
            const unsigned i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1));
            const bool up = ((base + i) & k) == 0;
            const fc_u64 a = s[i], b = s[i + j];
            if ((a > b) == up) { s[i] = b; s[i + j] = a; }
            __syncthreads();
        }
    keys[base + tid] = s[tid]; keys[base + tid + 1024] = s[tid + 1024];
}
static __global__ void __launch_bounds__(256) fc_sort_global_kernel(fc_u64 *__restrict__ keys, unsigned j, unsigned k, unsigned half)
{
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const bool up = (i & k) == 0;
    const fc_u64 a = keys[i], b = keys[i + j];
    if ((a > b) == up) { keys[i] = b; keys[i + j] = a; }
}

// the whole sort of buf[0 .. n_sort), n_sort a power of two >= FC_SORT_CHUNK, on stream st
static inline void fc_sort_launch(fc_u64 *buf, unsigned n_sort, hipStream_t st)
{
    const unsigned half_blocks = (n_sort / 2 + 255) / 256;
    hipLaunchKernelGGL(fc_sort_local_kernel, dim3(n_sort / FC_SORT_CHUNK), dim3(1024), 0, st, buf, 2u, (unsigned)FC_SORT_CHUNK);
    for (unsigned k = 2 * FC_SORT_CHUNK; k <= n_sort; k <<= 1) {
        for (unsigned j = k >> 1; j >= FC_SORT_CHUNK; j >>= 1)
            hipLaunchKernelGGL(fc_sort_global_kernel, dim3(half_blocks), dim3(256), 0, st, buf, j, k, n_sort / 2);
        hipLaunchKernelGGL(fc_sort_local_kernel, dim3(n_sort / FC_SORT_CHUNK), dim3(1024), 0, st, buf, k, k);
    }
}

__device__ __forceinline__ float fc_relu(float y) { return y > 0.0f ? y : (y != y ? y : 0.0f); }

// ---- maps -------------------------------------------------------------------------------------------------------------------------
// Every level's cells live in a table of lr_cells.h (key -> row).  Level l+1 is made from level l: every fine row claims its coarse cell,
// the smallest fine row of a cell stands for it, the representatives' keys are sorted and a cell's row is its rank (F1, I2).

// the control block (ctl_words 32-bit words) and the four tables' words the later kernels accumulate into: a call is kernel launches only
static __global__ void __launch_bounds__(256) sp_init_kernel(fc_u64 *__restrict__ keys, int32_t *__restrict__ val, size_t slots, sp_ctl *ctl, int ctl_words)
{
    if (blockIdx.x == 0) {
        for (int w = threadIdx.x; w < ctl_words; w += 256) reinterpret_cast<int32_t *>(ctl)[w] = 0;
        __syncthreads();
        if (threadIdx.x < 6) ctl->mn[threadIdx.x] = INT_MAX;
    }
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (size_t)gridDim.x * 256) { keys[s] = LR_CELL_EMPTY; val[s] = 0x7f7f7f7f; }
}
static inline void sp_init_launch(fc_u64 *keys, int32_t *val, size_t slots, sp_ctl *ctl, size_t ctl_bytes, hipStream_t st)
{
    const size_t blocks = (slots + 255) / 256;
    hipLaunchKernelGGL(sp_init_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, keys, val, slots, ctl, (int)(ctl_bytes / 4));
}
// level 0 of a call with one status word: row_key(i, ctl) is the key of input row i, LR_CELL_EMPTY when the cell is past the call's limit
template <class RowKey> __global__ void __launch_bounds__(256) sp_l0_insert_kernel(RowKey row_key, int n, fc_u64 *keys, int32_t *val, unsigned mask,
                                                                                   fc_u64 *__restrict__ rowkey, sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const fc_u64 key = row_key(i, ctl);
    rowkey[i] = key;
    if (key == LR_CELL_EMPTY) { atomicMax(&ctl->status, 3); return; }
    atomicMin(&val[lr_cells_claim(keys, mask, key)], i);
}
static __global__ void __launch_bounds__(256) sp_l0_check_kernel(const fc_u64 *__restrict__ rowkey, int n, const fc_u64 *__restrict__ keys,
                                                                 const int32_t *__restrict__ val, unsigned mask, sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) ctl->n[0] = n;
    if (i >= n) return;
    const fc_u64 key = rowkey[i];
    if (key == LR_CELL_EMPTY) return;
    const int s = fc_find(keys, mask, key);
    if (s < 0 || val[s] != i) atomicMax(&ctl->status, 2);
}
template <class C> __global__ void __launch_bounds__(256) sp_coarse_insert_kernel(const fc_u64 *__restrict__ rowkey, int lvl, fc_u64 *keys, int32_t *val, unsigned mask,
                                                                                  const sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || i >= ctl->n[lvl]) return;
    atomicMin(&val[lr_cells_claim(keys, mask, C::coarse(rowkey[i], lvl + 1))], i);
}
// sortbuf[i] = the coarse key of fine row i when it stands for its cell (smallest row of the cell), no key otherwise and behind the rows
template <class C> __global__ void __launch_bounds__(256) sp_coarse_mark_kernel(const fc_u64 *__restrict__ rowkey, int lvl, const fc_u64 *__restrict__ keys,
                                                                                const int32_t *__restrict__ val, unsigned mask, fc_u64 *__restrict__ sortbuf, int n_sort,
                                                                                sp_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status) return;
    fc_u64 out = LR_CELL_EMPTY;
    if (i < ctl->n[lvl]) {
        const fc_u64 key = C::coarse(rowkey[i], lvl + 1);
        const int s = fc_find(keys, mask, key);
        if (s >= 0 && val[s] == i) out = key;
    }
    if (i < n_sort) sortbuf[i] = out;
    const unsigned long long live = __ballot(out != LR_CELL_EMPTY);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&ctl->n[lvl + 1], __popcll(live));
}
// the sorted keys are the level's rows: row r of level lvl = the cell of rank r.  perm (nullable; a sorted level 0): the table held the
// cell's input row, which goes to perm[r]
static __global__ void __launch_bounds__(256) sp_index_kernel(const fc_u64 *__restrict__ sorted, int lvl, const fc_u64 *__restrict__ keys, int32_t *__restrict__ val,
                                                              unsigned mask, fc_u64 *__restrict__ rowkey, int32_t *__restrict__ perm, const sp_ctl *ctl)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || r >= ctl->n[lvl]) return;
    const fc_u64 key = sorted[r];
    const int s = fc_find(keys, mask, key);
    int row = -1;
    if (s >= 0) { row = val[s]; val[s] = r; }
    if (perm) perm[r] = row;
    rowkey[r] = key;
}
// tbl[r][k] = the row of (cell of rowkey[r]) + o(k) step in the table, -1 when absent; r < n[lvl_out], K^D offsets, one thread per entry
template <class C, int K> __global__ void __launch_bounds__(256) sp_nbr_kernel(const fc_u64 *__restrict__ rowkey, int lvl_out, const fc_u64 *__restrict__ keys,
                                                                               const int32_t *__restrict__ val, unsigned mask, int step, int32_t *__restrict__ tbl,
                                                                               const sp_ctl *ctl)
{
    constexpr int nk = sp_ipow(K, C::dims);
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || gid >= (size_t)ctl->n[lvl_out] * nk) return;
    const int r = (int)(gid / nk);
    fc_u64 q;
    int idx = -1;
    if (C::neighbour(rowkey[r], (int)(gid - (size_t)r * nk), K, step, q)) {
        const int s = fc_find(keys, mask, q);
        if (s >= 0) idx = val[s];
    }
    tbl[gid] = idx;
}

// ---- the gather convolution ---------------------------------------------------------------------------------------------------------
struct sp_conv {
    const float *in0, *in1;          // the input's rows: [.][c0] and, behind them in channel order, [.][c1] (in1 unused at c1 = 0)
    int c0, c1;
    const int32_t *nbr;              // [rows][nk] input rows, -1 = absent; null: one offset and the row itself (1x1)
    int nk;                          // SP_CACHED: at most 27 (SP_STREAMED: the table is [rows][729])
    const float *W, *scale, *offset; // W[nk][c0 + c1][Cout]
    const float *res;                // nullable residual [rows][Cout]
    float *out;                      // [rows][Cout]
    int relu, lvl, cout;             // rows = ctl->n[lvl]
};
// where a step's row indices come from: the tile's slice of a table of at most 27 offsets, cached in LDS; or a table of 729 offsets, whose
// slice (64 x 729 entries) does not fit, read from memory one step ahead of the row gather that needs the entries
enum sp_table { SP_CACHED, SP_STREAMED };
#define SP_NK_STREAMED 729

// The one hot kernel.  A block owns 32 WR rows x 32 WC columns of Cout (grid y: the column tiles); wave (wr, wc) owns one 32 x 32
// accumulator.  Per offset in ascending order (skipped when no row of the tile has that neighbour) and per 32 input channels it gathers the
// neighbours' rows into LDS (zeros for absent ones), stages the offset's weight slab and accumulates on v_mfma_f32_32x32x2_f32, which is
// bit for bit the fmaf chain of F5.  The rows and the weight slab of the next (offset, 32 channels) step are fetched into registers while
// the matrix cores work on the current one.  The epilogue F6 is fused; a two-source input (the cat) is read in place.
template <int WR, int WC, sp_table TABLE> __global__ void __launch_bounds__(256) sp_conv_kernel(sp_conv a, const sp_ctl *ctl)
{
    constexpr int TM = 32 * WR, TN = 32 * WC, NK = TABLE == SP_CACHED ? 27 : SP_NK_STREAMED;
    static_assert(WR * WC == 4, "four waves");
    __shared__ float As[TM * SP_AS];
    __shared__ float Bs[32 * TN];
    __shared__ int s_any[NK], s_live[NK], s_nlive;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ctl->status) return;
    const int rows = ctl->n[a.lvl], row0 = blockIdx.x * TM, nk = TABLE == SP_CACHED ? a.nk : a.nbr ? NK : 1, col0 = blockIdx.y * TN, cout = a.cout;
    if (row0 >= rows) return;
    // the offsets some row of the tile has a neighbour at, ascending: the others are skipped, block-uniformly (F5: the same bits)
    const int *tile = nullptr;                                        // SP_CACHED: the tile's slice of the table, [TM][nk]
    if constexpr (TABLE == SP_CACHED) {
        __shared__ int s_nbr[TM * 27];
        tile = s_nbr;
        if (tid < 27) s_any[tid] = 0;
        __syncthreads();
        for (int e = tid; e < TM * nk; e += 256) {
            const int r = e / nk, k = e - r * nk, row = row0 + r;
            int idx = -1;
            if (row < rows) idx = a.nbr ? a.nbr[(size_t)row * nk + k] : row;
            s_nbr[e] = idx;
            if (idx >= 0) s_any[k] = 1;
        }
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int k = 0; k < nk; ++k) if (s_any[k]) s_live[c++] = k;
            s_nlive = c;
        }
    } else {
        for (int k = tid; k < nk; k += 256) s_any[k] = a.nbr ? 0 : 1;
        __syncthreads();
        if (a.nbr) {                                                       // one coalesced pass over the tile's slice of the table: the live rows'
            const int live_rows = rows - row0 < TM ? rows - row0 : TM;     // entries are contiguous, and 16-byte aligned (row0 is a multiple of 64)
            const int total = live_rows * NK, total4 = total >> 2;
            const int32_t *slice = a.nbr + (size_t)row0 * NK;
            int k = (4 * tid) % NK;                                        // the offset of entry 4 e; 1024 = 729 + 295
            for (int e = tid; e < total4; e += 256) {
                const int4 v = reinterpret_cast<const int4 *>(slice)[e];
                const int k1 = k + 1 < NK ? k + 1 : k + 1 - NK, k2 = k + 2 < NK ? k + 2 : k + 2 - NK, k3 = k + 3 < NK ? k + 3 : k + 3 - NK;
                if (v.x >= 0) s_any[k] = 1;
                if (v.y >= 0) s_any[k1] = 1;
                if (v.z >= 0) s_any[k2] = 1;
                if (v.w >= 0) s_any[k3] = 1;
                k += 295; if (k >= NK) k -= NK;
            }
            for (int e = 4 * total4 + tid; e < total; e += 256) if (slice[e] >= 0) s_any[e % NK] = 1;
        }
        __syncthreads();
        if (wave == 0) {
            int base = 0;
            for (int k0 = 0; k0 < nk; k0 += 64) {
                const int k = k0 + lane;
                const bool on = k < nk && s_any[k] != 0;
                const unsigned long long m = __ballot(on);
                if (on) s_live[base + __popcll(m & ((1ull << lane) - 1ull))] = k;
                base += __popcll(m);
            }
            if (lane == 0) s_nlive = base;
        }
    }
    __syncthreads();
    fc_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const int wr = wave / WC, wc = wave % WC, cin = a.c0 + a.c1, nch = cin >> 5, steps = s_nlive * nch;
    const int a_at = (wr * 32 + (lane & 31)) * SP_AS + (lane >> 5), b_at = (lane >> 5) * TN + wc * 32 + (lane & 31);
    float4 ra[WR], rb0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb1 = rb0;      // (rb as an array of two went to scratch memory)
    // SP_STREAMED: this thread's rows' entries of step s's offset, straight from the table (-1: absent, or a row past the level's count)
    auto entries = [&](int s, int (&idx)[WR]) {
        const int k = s_live[s / nch];
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const int row = row0 + ((tid + 256 * i) >> 3);
            idx[i] = row < rows ? (a.nbr ? a.nbr[(size_t)row * NK + k] : row) : -1;
        }
    };
    int nidx[WR];                                                      // the entries of the step the next round fetches: read one round
    if constexpr (TABLE == SP_STREAMED) {                              // ahead, so that a round's row gather does not wait for them
        if (steps > 0) entries(0, nidx);
    }
    // step s = (live offset s / nch, channels 32 (s % nch) ..).  Round `it` puts step it (fetched in the round before) into LDS, fetches
    // the rows and the slab of W of step it + 1 into ra / rb, and multiplies step it; round -1 only fetches.
    for (int it = -1; it < steps; ++it) {
        if (it >= 0) {
            __syncthreads();                                           // the previous step's reads of As / Bs are done
#pragma unroll
            for (int i = 0; i < WR; ++i) { const int e = tid + 256 * i; *reinterpret_cast<float4 *>(&As[(e >> 3) * SP_AS + 4 * (e & 7)]) = ra[i]; }
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
            if constexpr (TABLE == SP_STREAMED) {
#pragma unroll
                for (int i = 0; i < WR; ++i) idx[i] = nidx[i];
                if (it + 2 < steps) entries(it + 2, nidx);
            }
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const int e = tid + 256 * i;
                if constexpr (TABLE == SP_CACHED) idx[i] = tile[(e >> 3) * nk + k];
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

// tap: the activations [n_level][cout] of the stage, the level's cells [n_level][D] decoded from their keys, the result block
template <class C, class Result> __global__ void __launch_bounds__(256) sp_tap_kernel(const float *__restrict__ f, int cout, int lvl, const fc_u64 *__restrict__ rowkey,
                                                                                      int n, float *__restrict__ out, int32_t *__restrict__ tap_coords, int bias,
                                                                                      const sp_ctl *ctl, Result *res)
{
    const int status = ctl->status, rows = status ? 0 : ctl->n[lvl];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid == 0) { res->status = status; res->n = n; res->n_tap = rows; res->reserved = 0; }
    if (gid < (size_t)rows * cout) out[gid] = f[gid];
    if (tap_coords && gid < (size_t)rows * C::dims) {
        const int r = (int)(gid / C::dims), a = (int)(gid - (size_t)r * C::dims);
        tap_coords[gid] = C::field(rowkey[r], a) - bias + sp_origin(ctl, a);
    }
}
template <class Result> __global__ void sp_empty_kernel(Result *res) { res->status = 0; res->n = 0; res->n_tap = 0; res->reserved = 0; }

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct sp_stage { int k3, cin, cout; };
// t[1 .. 23] (F7, I4) of widths w = C1 C2 C3 C4 (down) T4 T3 T2 T1 (up): nk_conv1 offsets in stage 1, nk in stages 2 .. 21, one in the last two
static inline void sp_stage_table(const int32_t *w, int nk_conv1, int nk, int cout_final, sp_stage *t)
{
    const int C1 = w[0], C2 = w[1], C3 = w[2], C4 = w[3], T4 = w[4], T3 = w[5], T2 = w[6], T1 = w[7];
    const int io[SP_STAGES + 1][2] = { { 0, 0 }, { 1, C1 }, { C1, C1 }, { C1, C1 }, { C1, C2 }, { C2, C2 }, { C2, C2 }, { C2, C3 }, { C3, C3 }, { C3, C3 },
        { C3, C4 }, { C4, C4 }, { C4, C4 }, { C4, T4 }, { T4, T4 }, { T4, T4 }, { T4 + C3, T3 }, { T3, T3 }, { T3, T3 }, { T3 + C2, T2 }, { T2, T2 },
        { T2, T2 }, { T2 + C1, T1 }, { T1, cout_final } };
    for (int s = 1; s <= SP_STAGES; ++s) t[s] = sp_stage{ s == 1 ? nk_conv1 : s >= 22 ? 1 : nk, io[s][0], io[s][1] };
}
static inline size_t sp_stage_floats(const sp_stage &s) { return (size_t)s.k3 * s.cin * s.cout + 2 * (size_t)s.cout; }
static inline size_t sp_weights_bytes(const int32_t *w, int nk_conv1, int nk, int cout_final)
{
    sp_stage t[SP_STAGES + 1];
    sp_stage_table(w, nk_conv1, nk, cout_final, t);
    size_t f = 0;
    for (int s = 1; s <= SP_STAGES; ++s) f += sp_stage_floats(t[s]);
    return f * sizeof(float);
}

// Gather tables, -1 = absent, [rows][nk] each, in this order:
//   nbr[l]  row of c + o t_l at level l                                       (F2)
//   extra   the same at level 0 for a wider conv1 (nk_extra offsets; 0: none)
//   dn[l]   row of v + o t_l at level l, v a cell of level l+1                (F3)
//   up[l]   row of u - o t_l at level l+1, u a cell of level l                (F4: the transpose of dn, stored output-stationary as well)
struct sp_layout { size_t keys, val, rowkey, sort, tbl, extra, dn, X, Y, Z, S1, S2, S4, total, m, cap_max, ctl_bytes; int nk; };
// perm: room for the int32 permutation of a sorted level 0 behind the four levels' keys
static sp_layout sp_make_layout(size_t max_n, int nk, int nk_extra, const int32_t *w, size_t ctl_bytes, bool perm)
{
    sp_layout L;
    const size_t m = (max_n + 63) & ~size_t(63);      // rows every array is sized for: all sizes below are multiples of 256 bytes
    size_t mw = 0;
    for (int i = 0; i < 8; ++i) mw = (size_t)w[i] > mw ? (size_t)w[i] : mw;
    L.m = m;
    L.nk = nk;
    L.ctl_bytes = ctl_bytes;
    L.cap_max = 4 * m + 1024;                         // lr_cells_capacity(n) < 4 n, or 1024
    size_t o = ctl_bytes;
    L.keys = o;   o += 4 * L.cap_max * 8;
    L.val = o;    o += 4 * L.cap_max * 4;
    L.rowkey = o; o += 4 * m * 8 + (perm ? m * 4 : 0);
    L.sort = o;   o += (2 * m + FC_SORT_CHUNK) * 8;
    L.tbl = o;    o += 4 * m * nk * 4;
    L.extra = o;  o += m * nk_extra * 4;
    L.dn = o;     o += 6 * m * nk * 4;                // dn[0..2], up[0..2]
    L.X = o;      o += m * mw * 4;
    L.Y = o;      o += m * mw * 4;
    L.Z = o;      o += m * mw * 4;
    L.S1 = o;     o += m * (size_t)w[0] * 4;
    L.S2 = o;     o += m * (size_t)w[1] * 4;
    L.S4 = o;     o += m * (size_t)w[2] * 4;
    L.total = o;
    return L;
}

namespace {
template <sp_table TABLE> struct sp_run {
    hipStream_t st;
    char *base;
    sp_layout L;
    sp_ctl *ctl;
    int n;
    unsigned mask, n_sort;
    sp_stage t[SP_STAGES + 1];
    const float *w[SP_STAGES + 1];      // the stages' blocks in the blob
    fc_u64 *keys[4], *rowkey[4], *sortbuf;
    int32_t *val[4], *perm, *nbr[4], *extra, *dn[3], *up[3];
    float *X, *Y, *Z, *S1, *S2, *S4;    // activations: three of the widest level, the three skips
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    int grid(size_t items) const { return (int)((items + 255) / 256); }

    // the pointers into a scratch of layout L_ for n_ rows, and into the blob of the stages t (filled by the caller)
    void carve(void *scratch, const sp_layout &L_, int n_, const float *weights, hipStream_t stream)
    {
        st = stream; base = reinterpret_cast<char *>(scratch); L = L_; n = n_;
        ctl = at<sp_ctl>(0);
        for (int s = 1; s <= SP_STAGES; ++s) { w[s] = weights; weights += sp_stage_floats(t[s]); }
        mask = (unsigned)(lr_cells_capacity((size_t)n) - 1);
        n_sort = FC_SORT_CHUNK;
        while (n_sort < (unsigned)n) n_sort <<= 1;
        const size_t m = L.m, tb = m * L.nk;
        for (int l = 0; l < 4; ++l) {
            keys[l] = at<fc_u64>(L.keys) + (size_t)l * L.cap_max;
            val[l] = at<int32_t>(L.val) + (size_t)l * L.cap_max;
            rowkey[l] = at<fc_u64>(L.rowkey) + (size_t)l * m;
            nbr[l] = at<int32_t>(L.tbl) + (size_t)l * tb;
            if (l < 3) { dn[l] = at<int32_t>(L.dn) + (size_t)l * tb; up[l] = at<int32_t>(L.dn) + (size_t)(3 + l) * tb; }
        }
        perm = at<int32_t>(L.rowkey + 4 * m * 8);
        extra = at<int32_t>(L.extra);
        sortbuf = at<fc_u64>(L.sort);
        X = at<float>(L.X); Y = at<float>(L.Y); Z = at<float>(L.Z); S1 = at<float>(L.S1); S2 = at<float>(L.S2); S4 = at<float>(L.S4);
    }
    // stage s (a 1x1 stage: tbl null)
    void conv(int s, const float *in0, int c0, const float *in1, int c1, const int32_t *tbl, const float *res, float *out, int relu, int lvl) const
    {
        const sp_stage &g = t[s];
        const float *W = w[s];
        const size_t nw = (size_t)g.k3 * g.cin * g.cout;
        const sp_conv a = { in0, in1, c0, c1, tbl, g.k3, W, W + nw, W + nw + g.cout, res, out, relu, lvl, g.cout };
        const sp_ctl *c = ctl;
        // (the grid covers n rows, the most a level can have: the blocks past the level's live count leave at once)
        if (g.cout % 64) hipLaunchKernelGGL((sp_conv_kernel<4, 1, TABLE>), dim3(lr_cdiv(n, 128), g.cout / 32), dim3(256), 0, st, a, c);
        else             hipLaunchKernelGGL((sp_conv_kernel<2, 2, TABLE>), dim3(lr_cdiv(n, 64), g.cout / 64), dim3(256), 0, st, a, c);
    }
};
}

// The coarse levels from level 0's keys (R.rowkey[0], R.ctl->n[0]) and the ten gather tables (eleven with KX: conv1's wider level-0 table)
template <class C, int KX, class Run> static void sp_maps(const Run &R)
{
    hipStream_t st = R.st;
    sp_ctl *ctl = R.ctl;
    const unsigned mask = R.mask;
    constexpr int nk = sp_ipow(3, C::dims);
    const dim3 gn(R.grid((size_t)R.n)), gt(R.grid((size_t)R.n * nk)), b(256);
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL(sp_coarse_insert_kernel<C>, gn, b, 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, ctl);
        hipLaunchKernelGGL(sp_coarse_mark_kernel<C>, dim3(R.grid(R.n_sort)), b, 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, R.sortbuf, (int)R.n_sort, ctl);
        fc_sort_launch(R.sortbuf, R.n_sort, st);
        hipLaunchKernelGGL(sp_index_kernel, gn, b, 0, st, R.sortbuf, l + 1, R.keys[l + 1], R.val[l + 1], mask, R.rowkey[l + 1], (int32_t *)nullptr, ctl);
    }
    for (int l = 0; l < 4; ++l)
        hipLaunchKernelGGL((sp_nbr_kernel<C, 3>), gt, b, 0, st, R.rowkey[l], l, R.keys[l], R.val[l], mask, 1 << l, R.nbr[l], ctl);
    if constexpr (KX != 0)
        hipLaunchKernelGGL((sp_nbr_kernel<C, KX>), dim3(R.grid((size_t)R.n * sp_ipow(KX, C::dims))), b, 0, st, R.rowkey[0], 0, R.keys[0], R.val[0], mask, 1, R.extra, ctl);
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL((sp_nbr_kernel<C, 3>), gt, b, 0, st, R.rowkey[l + 1], l + 1, R.keys[l], R.val[l], mask, 1 << l, R.dn[l], ctl);
        hipLaunchKernelGGL((sp_nbr_kernel<C, 3>), gt, b, 0, st, R.rowkey[l], l, R.keys[l + 1], R.val[l + 1], mask, -(1 << l), R.up[l], ctl);
    }
}

// The 23 stages (F7, I4) on the maps and buffers of R: conv1(X) launches stage 1 into X and last(X, Y) stage 23 from X into Y;
// done(s, buf, lvl) is told that `buf` holds stage s of level lvl and ends the sequence by returning true.  The output is left in Y.
template <typename Run, typename Conv1, typename Last, typename Done> static bool sp_stages(const Run &R, const int32_t *wd, Conv1 conv1, Last last, Done done)
{
    float *X = R.X, *Y = R.Y, *Z = R.Z, *S1 = R.S1, *S2 = R.S2, *S4 = R.S4;
    const int C1 = wd[0], C2 = wd[1], C3 = wd[2], C4 = wd[3], T4 = wd[4], T3 = wd[5], T2 = wd[6];
    int s = 0;
    // a residual block: its two stages
    auto block = [&](const float *in, float *tmp, float *out, int C, int lvl) -> bool {
        R.conv(s + 1, in, C, nullptr, 0, R.nbr[lvl], nullptr, tmp, 1, lvl);
        if (done(++s, tmp, lvl)) return true;
        R.conv(s + 1, tmp, C, nullptr, 0, R.nbr[lvl], in, out, 1, lvl);
        return done(++s, out, lvl);
    };
    conv1(X);
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
    last(X, Y);
    return done(++s, Y, 0);
}
