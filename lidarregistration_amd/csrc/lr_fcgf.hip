// lr_fcgf_extract: the FCGF feature extractor (ResUNetBN2C, a sparse 3-D ResUNet of 23 convolutions) on integer voxel cells.
// Contract n1 (F1 .. F12) of include/lidarreg.h; DESIGN.md §18.
//
// Maps (once per call).  Every level's cells live in a table of lr_cells.h (packed biased key -> row).  Level l+1 is made from level l:
// every fine row claims its coarse cell, the smallest fine row of a cell stands for it, the representatives' keys are sorted (bitonic, keys
// only) and a cell's row is its rank (F1: ascending (x, y, z), whatever the input order and the hash did).  Gather tables, -1 = absent:
//   nbr27[l]  [n_l][27]      row of c + o t_l at level l                 (F2, K = 3)
//   nbr125    [n][125]       the same at level 0 for K = 5               (conv1)
//   dn[l]     [n_{l+1}][27]  row of v + o t_l at level l, v coarse       (F3)
//   up[l]     [n_l][27]      row of u - o t_l at level l+1, u fine       (F4: the transpose of dn, stored output-stationary as well)
// Convolutions.  fc_conv_kernel is the one hot kernel: a block owns 64 output rows x 64 columns of Cout (128 x 32 at Cout = 32); per offset
// in ascending order (skipped when no row of the tile has that neighbour) and per 32 input channels it gathers the neighbours' rows into
// LDS (zeros for absent ones), stages the offset's weight slab and accumulates on v_mfma_f32_32x32x2_f32, which is bit for bit the fmaf
// chain of F5.  The epilogue F6 is fused; a two-source input (the cat) is read in place.  conv1 (Cin = 1) is a vector kernel.
#include "lr_scratch.h"
#include "lr_sparse.h"

#define FC_MAX_N (1 << 20)
#define FC_BIAS (1 << 20)            // cell + bias is the 21-bit field of lr_cells_pack
#define FC_LIMIT ((1 << 20) - 2)     // |cell| >= this: status 3
#define FC_STAGES 23

struct fc_ctl { int32_t status, n[4], pad[3]; };
struct fc_stage { int k3, cin, cout; };

static inline int fc_stage_table(int k1, fc_stage *t)      // t[1 .. 23]
{
    static const int io[FC_STAGES + 1][2] = { { 0, 0 }, { 1, 32 }, { 32, 32 }, { 32, 32 }, { 32, 64 }, { 64, 64 }, { 64, 64 }, { 64, 128 }, { 128, 128 },
        { 128, 128 }, { 128, 256 }, { 256, 256 }, { 256, 256 }, { 256, 128 }, { 128, 128 }, { 128, 128 }, { 256, 64 }, { 64, 64 }, { 64, 64 },
        { 128, 64 }, { 64, 64 }, { 64, 64 }, { 96, 64 }, { 64, 32 } };
    for (int s = 1; s <= FC_STAGES; ++s) t[s] = fc_stage{ s == 1 ? k1 * k1 * k1 : s >= 22 ? 1 : 27, io[s][0], io[s][1] };
    return FC_STAGES;
}
static inline size_t fc_stage_floats(const fc_stage &s) { return (size_t)s.k3 * s.cin * s.cout + 2 * (size_t)s.cout; }

struct fc_layout { size_t keys, val, coords, sort, nbr27, nbr125, dn, up, X, Y, Z, S1, S2, S4, total, m, cap_max; };
static fc_layout fc_make_layout(size_t max_n, size_t ctl_bytes = 256)
{
    fc_layout L;
    const size_t m = (max_n + 63) & ~size_t(63);      // rows every array is sized for: all sizes below are multiples of 256 bytes
    L.m = m;
    L.cap_max = 4 * m + 1024;                         // lr_cells_capacity(n) < 4 n, or 1024
    size_t o = ctl_bytes;                             // fc_ctl (the batch entry: fb_ctl)
    L.keys = o;   o += 4 * L.cap_max * 8;
    L.val = o;    o += 4 * L.cap_max * 4;
    L.coords = o; o += 3 * m * 12;                    // levels 1 .. 3
    L.sort = o;   o += (2 * m + FC_SORT_CHUNK) * 8;
    L.nbr27 = o;  o += 4 * m * 27 * 4;
    L.nbr125 = o; o += m * 125 * 4;
    L.dn = o;     o += 3 * m * 27 * 4;
    L.up = o;     o += 3 * m * 27 * 4;
    L.X = o;      o += m * 256 * 4;
    L.Y = o;      o += m * 256 * 4;
    L.Z = o;      o += m * 256 * 4;
    L.S1 = o;     o += m * 32 * 4;
    L.S2 = o;     o += m * 64 * 4;
    L.S4 = o;     o += m * 128 * 4;
    L.total = o;
    return L;
}

// ---- maps -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ fc_u64 fc_key(int x, int y, int z) { return lr_cells_pack((fc_u64)(x + FC_BIAS), (fc_u64)(y + FC_BIAS), (fc_u64)(z + FC_BIAS)); }
__device__ __forceinline__ bool fc_in_range(int v) { return v > -FC_LIMIT && v < FC_LIMIT; }

__global__ void __launch_bounds__(256) fc_l0_insert_kernel(const int32_t *__restrict__ coords, int n, fc_u64 *keys, int32_t *val, unsigned mask, fc_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
    if (!(fc_in_range(x) && fc_in_range(y) && fc_in_range(z))) { atomicMax(&ctl->status, 3); return; }
    atomicMin(&val[lr_cells_claim(keys, mask, fc_key(x, y, z))], i);
}
__global__ void __launch_bounds__(256) fc_l0_check_kernel(const int32_t *__restrict__ coords, int n, const fc_u64 *__restrict__ keys,
                                                          const int32_t *__restrict__ val, unsigned mask, fc_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) ctl->n[0] = n;
    if (i >= n) return;
    const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
    if (!(fc_in_range(x) && fc_in_range(y) && fc_in_range(z))) return;
    const int s = fc_find(keys, mask, fc_key(x, y, z));
    if (s < 0 || val[s] != i) atomicMax(&ctl->status, 2);
}
// coords of row i of level `lvl` (level 0: the caller's)
__device__ __forceinline__ void fc_coarse_of(const int32_t *__restrict__ coords, int i, int sh, int &x, int &y, int &z)
{
    x = (coords[3 * (size_t)i] >> sh) << sh; y = (coords[3 * (size_t)i + 1] >> sh) << sh; z = (coords[3 * (size_t)i + 2] >> sh) << sh;      // floor: -1 -> -2
}
__global__ void __launch_bounds__(256) fc_coarse_insert_kernel(const int32_t *__restrict__ coords, int lvl, fc_u64 *keys, int32_t *val, unsigned mask, const fc_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || i >= ctl->n[lvl]) return;
    int x, y, z;
    fc_coarse_of(coords, i, lvl + 1, x, y, z);
    atomicMin(&val[lr_cells_claim(keys, mask, fc_key(x, y, z))], i);
}
// sortbuf[i] = the coarse key of fine row i when it stands for its cell (smallest row of the cell), no key otherwise and behind the rows
__global__ void __launch_bounds__(256) fc_coarse_mark_kernel(const int32_t *__restrict__ coords, int lvl, const fc_u64 *__restrict__ keys,
                                                             const int32_t *__restrict__ val, unsigned mask, fc_u64 *__restrict__ sortbuf, int n_sort, fc_ctl *ctl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || i >= n_sort) return;
    fc_u64 out = LR_CELL_EMPTY;
    if (i < ctl->n[lvl]) {
        int x, y, z;
        fc_coarse_of(coords, i, lvl + 1, x, y, z);
        const fc_u64 key = fc_key(x, y, z);
        const int s = fc_find(keys, mask, key);
        if (s >= 0 && val[s] == i) { out = key; atomicAdd(&ctl->n[lvl + 1], 1); }
    }
    sortbuf[i] = out;
}
// the sorted keys are the level's rows: row r of level lvl = the cell of rank r
__global__ void __launch_bounds__(256) fc_coarse_index_kernel(const fc_u64 *__restrict__ sorted, int lvl, const fc_u64 *__restrict__ keys, int32_t *__restrict__ val,
                                                              unsigned mask, int32_t *__restrict__ coords, const fc_ctl *ctl)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || r >= ctl->n[lvl]) return;
    const fc_u64 key = sorted[r];
    const int s = fc_find(keys, mask, key);
    if (s >= 0) val[s] = r;
    coords[3 * (size_t)r] = (int)(key >> 42) - FC_BIAS; coords[3 * (size_t)r + 1] = (int)((key >> 21) & 0x1fffff) - FC_BIAS; coords[3 * (size_t)r + 2] = (int)(key & 0x1fffff) - FC_BIAS;
}
// tbl[r][k] = the row of (coords[r] + o(k) step) in the table, -1 when absent; r < n[lvl_out], K^3 offsets, x fastest (F2)
__global__ void __launch_bounds__(256) fc_nbr_kernel(const int32_t *__restrict__ coords, int lvl_out, const fc_u64 *__restrict__ keys, const int32_t *__restrict__ val,
                                                     unsigned mask, int K, int step, int32_t *__restrict__ tbl, const fc_ctl *ctl)
{
    const int k3 = K * K * K, h = K >> 1;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ctl->status || gid >= (size_t)ctl->n[lvl_out] * k3) return;
    const int r = (int)(gid / k3), k = (int)(gid % k3);
    const int x = coords[3 * (size_t)r] + (k % K - h) * step + FC_BIAS, y = coords[3 * (size_t)r + 1] + (k / K % K - h) * step + FC_BIAS,
              z = coords[3 * (size_t)r + 2] + (k / (K * K) - h) * step + FC_BIAS;
    int idx = -1;
    if (x >= 0 && x < 2 * FC_BIAS && y >= 0 && y < 2 * FC_BIAS && z >= 0 && z < 2 * FC_BIAS) {
        const int s = fc_find(keys, mask, lr_cells_pack((fc_u64)x, (fc_u64)y, (fc_u64)z));
        if (s >= 0) idx = val[s];
    }
    tbl[gid] = idx;
}

// ---- convolutions -------------------------------------------------------------------------------------------------------------------
// conv1: Cin = 1, 32 outputs, K^3 = 27 or 125 offsets; BatchNorm folded, no ReLU
__global__ void __launch_bounds__(256) fc_conv1_kernel(const float *__restrict__ feat_in, const int32_t *__restrict__ nbr, int nk, const float *__restrict__ W,
                                                       const float *__restrict__ scale, const float *__restrict__ offset, float *__restrict__ out, const fc_ctl *ctl)
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

struct fc_conv {
    const float *in0, *in1;          // the input's rows: [.][c0] and, behind them in channel order, [.][c1] (in1 unused at c1 = 0)
    int c0, c1;
    const int32_t *nbr;              // [rows][nk] input rows, -1 = absent; null: nk = 1 and the row itself (1x1)
    int nk;
    const float *W, *scale, *offset; // W[nk][c0 + c1][Cout]
    const float *res;                // nullable residual [rows][Cout]
    float *out;                      // [rows][Cout]
    int relu, lvl, cout;             // rows = ctl->n[lvl]
};
#define FC_AS 36                     // floats per row of the gathered tile in LDS (32 + 4: rows stay 16-byte aligned)

// block tile: 32 WR rows x 32 WC columns (grid y: the column tiles of Cout); wave (wr, wc) owns one 32 x 32 accumulator.  The rows and the
// weight slab of the next (offset, 32 channels) step are fetched into registers while the matrix cores work on the current one.
template <int WR, int WC> __global__ void __launch_bounds__(256) fc_conv_kernel(fc_conv a, const fc_ctl *ctl)
{
    constexpr int TM = 32 * WR, TN = 32 * WC;
    static_assert(WR * WC == 4, "four waves");
    __shared__ float As[TM * FC_AS];
    __shared__ float Bs[32 * TN];
    __shared__ int s_nbr[TM * 27];
    __shared__ int s_any[27], s_live[27], s_nlive;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ctl->status) return;
    const int rows = ctl->n[a.lvl], row0 = blockIdx.x * TM, nk = a.nk, col0 = blockIdx.y * TN, cout = a.cout;
    if (row0 >= rows) return;
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
    if (tid == 0) {                                                    // the offsets some row of the tile has a neighbour at, ascending: the
        int c = 0;                                                     // others are skipped, block-uniformly (F5: the same bits)
        for (int k = 0; k < nk; ++k) if (s_any[k]) s_live[c++] = k;
        s_nlive = c;
    }
    __syncthreads();
    fc_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const int wr = wave / WC, wc = wave % WC, cin = a.c0 + a.c1, nch = cin >> 5, steps = s_nlive * nch;
    const int a_at = (wr * 32 + (lane & 31)) * FC_AS + (lane >> 5), b_at = (lane >> 5) * TN + wc * 32 + (lane & 31);
    float4 ra[WR], rb0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb1 = rb0;      // (rb as an array of two went to scratch memory)
    // step s = (live offset s / nch, channels 32 (s % nch) ..).  Round `it` puts step it (fetched in the round before) into LDS, fetches
    // the rows and the slab of W of step it + 1 into ra / rb, and multiplies step it; round -1 only fetches.
    for (int it = -1; it < steps; ++it) {
        if (it >= 0) {
            __syncthreads();                                           // the previous step's reads of As / Bs are done
#pragma unroll
            for (int i = 0; i < WR; ++i) { const int e = tid + 256 * i; *reinterpret_cast<float4 *>(&As[(e >> 3) * FC_AS + 4 * (e & 7)]) = ra[i]; }
            *reinterpret_cast<float4 *>(&Bs[(tid / (TN / 4)) * TN + 4 * (tid % (TN / 4))]) = rb0;
            if constexpr (WC == 2) *reinterpret_cast<float4 *>(&Bs[((tid + 256) / (TN / 4)) * TN + 4 * (tid % (TN / 4))]) = rb1;
            __syncthreads();
        }
        if (it + 1 < steps) {
            const int k = s_live[(it + 1) / nch], ch = ((it + 1) % nch) << 5;
            const bool first = ch < a.c0;
            const float *src = first ? a.in0 : a.in1;
            const int cs = first ? a.c0 : a.c1, co = first ? ch : ch - a.c0;
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const int e = tid + 256 * i, idx = s_nbr[(e >> 3) * nk + k];
                ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (idx >= 0) ra[i] = *reinterpret_cast<const float4 *>(src + (size_t)idx * cs + co + 4 * (e & 7));
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

// F8 and the result block of a whole-network call; a refused input (status 2, 3) leaves rows of zeros
__global__ void __launch_bounds__(256) fc_norm_kernel(const float *__restrict__ f, int n, float *__restrict__ out, const fc_ctl *ctl, lr_fcgf_result *res)
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
// tap: the activations [n_level][cout] of the stage, the level's cells, the result block
__global__ void __launch_bounds__(256) fc_tap_kernel(const float *__restrict__ f, int cout, int lvl, const int32_t *__restrict__ coords, int n, float *__restrict__ out,
                                                     int32_t *__restrict__ tap_coords, const fc_ctl *ctl, lr_fcgf_result *res)
{
    const int status = ctl->status, rows = status ? 0 : ctl->n[lvl];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid == 0) { res->status = status; res->n = n; res->n_tap = rows; res->reserved = 0; }
    if (gid < (size_t)rows * cout) out[gid] = f[gid];
    if (tap_coords && gid < (size_t)rows * 3) tap_coords[gid] = coords[gid];
}
__global__ void fc_empty_kernel(lr_fcgf_result *res) { res->status = 0; res->n = 0; res->n_tap = 0; res->reserved = 0; }

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_fcgf_params) == 12 && sizeof(lr_fcgf_result) == 16, "ABI structs changed: update include/lidarreg.h and _ext.py together");

extern "C" size_t lr_fcgf_weights_bytes(int conv1_kernel_size)
{
    if (conv1_kernel_size != 3 && conv1_kernel_size != 5) return 0;
    fc_stage t[FC_STAGES + 1];
    fc_stage_table(conv1_kernel_size, t);
    size_t f = 0;
    for (int s = 1; s <= FC_STAGES; ++s) f += fc_stage_floats(t[s]);
    return f * sizeof(float);
}

extern "C" size_t lr_fcgf_scratch_bytes(int max_n)
{
    if (max_n < 0 || max_n > FC_MAX_N) return 0;
    return fc_make_layout((size_t)max_n).total;
}

namespace {
struct fc_run {
    hipStream_t st;
    char *base;
    fc_layout L;
    fc_ctl *ctl;
    int n;
    fc_stage t[FC_STAGES + 1];
    const float *w[FC_STAGES + 1];      // the stages' blocks in the blob
    const int32_t *coords[4];
    fc_u64 *keys[4];
    int32_t *val[4], *nbr27[4], *dn[3], *up[3];
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    int grid(size_t items) const { return (int)((items + 255) / 256); }

    void conv(int s, const float *in0, int c0, const float *in1, int c1, const int32_t *nbr, const float *res, float *out, int relu, int lvl) const
    {
        const fc_stage &g = t[s];
        const float *W = w[s];
        const fc_conv a = { in0, in1, c0, c1, nbr, g.k3, W, W + (size_t)g.k3 * g.cin * g.cout, W + (size_t)g.k3 * g.cin * g.cout + g.cout, res, out, relu, lvl, g.cout };
        const fc_ctl *c = ctl;
        // (the grid covers n rows, the most a level can have: the blocks past the level's live count leave at once)
        if (g.cout == 32) hipLaunchKernelGGL((fc_conv_kernel<4, 1>), dim3(lr_cdiv(n, 128), 1), dim3(256), 0, st, a, c);
        else              hipLaunchKernelGGL((fc_conv_kernel<2, 2>), dim3(lr_cdiv(n, 64), g.cout / 64), dim3(256), 0, st, a, c);
    }
};
}

// The 23 stages (F7) on the maps and buffers of R, shared by the two entry points: conv1(X) launches stage 1 into X; done(s, buf, lvl) is
// told that `buf` holds stage s of level lvl and ends the sequence by returning true.  The network's output is left in Y.
template <typename Conv1, typename Done> static bool fc_stages(const fc_run &R, Conv1 conv1, Done done)
{
    const fc_layout &L = R.L;
    float *X = R.at<float>(L.X), *Y = R.at<float>(L.Y), *Z = R.at<float>(L.Z), *S1 = R.at<float>(L.S1), *S2 = R.at<float>(L.S2), *S4 = R.at<float>(L.S4);
    int s = 0;
    // a residual block: its two stages
    auto block = [&](const float *in, float *tmp, float *out, int C, int lvl) -> bool {
        R.conv(s + 1, in, C, nullptr, 0, R.nbr27[lvl], nullptr, tmp, 1, lvl);
        if (done(++s, tmp, lvl)) return true;
        R.conv(s + 1, tmp, C, nullptr, 0, R.nbr27[lvl], in, out, 1, lvl);
        return done(++s, out, lvl);
    };
    conv1(X);
    if (done(++s, X, 0)) return true;
    if (block(X, Y, S1, 32, 0)) return true;
    R.conv(4, S1, 32, nullptr, 0, R.dn[0], nullptr, X, 0, 1);              if (done(++s, X, 1)) return true;
    if (block(X, Y, S2, 64, 1)) return true;
    R.conv(7, S2, 64, nullptr, 0, R.dn[1], nullptr, X, 0, 2);              if (done(++s, X, 2)) return true;
    if (block(X, Y, S4, 128, 2)) return true;
    R.conv(10, S4, 128, nullptr, 0, R.dn[2], nullptr, X, 0, 3);            if (done(++s, X, 3)) return true;
    if (block(X, Y, Z, 256, 3)) return true;
    R.conv(13, Z, 256, nullptr, 0, R.up[2], nullptr, X, 0, 2);             if (done(++s, X, 2)) return true;
    if (block(X, Y, Z, 128, 2)) return true;
    R.conv(16, Z, 128, S4, 128, R.up[1], nullptr, X, 0, 1);                if (done(++s, X, 1)) return true;
    if (block(X, Y, Z, 64, 1)) return true;
    R.conv(19, Z, 64, S2, 64, R.up[0], nullptr, X, 0, 0);                  if (done(++s, X, 0)) return true;
    if (block(X, Y, Z, 64, 0)) return true;
    R.conv(22, Z, 64, S1, 32, nullptr, nullptr, X, 1, 0);                  if (done(++s, X, 0)) return true;
    R.conv(23, X, 64, nullptr, 0, nullptr, nullptr, Y, 0, 0);              return done(++s, Y, 0);
}

extern "C" int lr_fcgf_extract(const int32_t *coords, const float *feat_in, int n, const float *weights, size_t weights_bytes, const lr_fcgf_params *p,
                               lr_fcgf_result *result, float *feat_out, int32_t *tap_coords, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_fcgf_extract";
    LR_CHECK_STRUCT_SIZE(lr_fcgf_params, p, who);
    LR_REFUSE_UNLESS(p->conv1_kernel_size == 3 || p->conv1_kernel_size == 5, LR_EINVAL, "conv1_kernel_size must be 3 or 5");
    LR_REFUSE_UNLESS(p->tap >= 0 && p->tap <= FC_STAGES, LR_EINVAL, "tap must lie in 0 .. 23");
    LR_REFUSE_UNLESS(n >= 0 && n <= FC_MAX_N, LR_EINVAL, "n must lie in 0 .. 2^20");
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    LR_REFUSE_UNLESS(weights_bytes >= lr_fcgf_weights_bytes(p->conv1_kernel_size), LR_EINVAL, "weights_bytes is below lr_fcgf_weights_bytes(conv1_kernel_size)");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    LR_REFUSE_UNLESS(n == 0 || (coords && feat_out), LR_EINVAL, "null coords or feat_out");
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, lr_fcgf_scratch_bytes(n), "lr_fcgf_scratch_bytes(n)", LR_EINVAL, stream, nullptr));

    fc_run R;
    R.st = (hipStream_t)stream;
    hipStream_t st = R.st;
    if (n == 0) {
        hipLaunchKernelGGL(fc_empty_kernel, dim3(1), dim3(1), 0, st, result);
        LR_LAUNCH_CHECK();
        return LR_OK;
    }
    R.base = reinterpret_cast<char *>(scratch);
    R.L = fc_make_layout((size_t)n);
    const fc_layout &L = R.L;
    R.ctl = R.at<fc_ctl>(0);
    R.n = n;
    fc_stage_table(p->conv1_kernel_size, R.t);
    { const float *W = weights; for (int s = 1; s <= FC_STAGES; ++s) { R.w[s] = W; W += fc_stage_floats(R.t[s]); } }
    const size_t cap = lr_cells_capacity((size_t)n), m = L.m;
    const unsigned mask = (unsigned)(cap - 1);
    R.coords[0] = coords;
    for (int l = 0; l < 4; ++l) {
        R.keys[l] = R.at<fc_u64>(L.keys) + (size_t)l * L.cap_max;
        R.val[l] = R.at<int32_t>(L.val) + (size_t)l * L.cap_max;
        R.nbr27[l] = R.at<int32_t>(L.nbr27) + (size_t)l * m * 27;
        if (l) R.coords[l] = R.at<int32_t>(L.coords) + (size_t)(l - 1) * m * 3;
        if (l < 3) { R.dn[l] = R.at<int32_t>(L.dn) + (size_t)l * m * 27; R.up[l] = R.at<int32_t>(L.up) + (size_t)l * m * 27; }
    }
    int32_t *nbr125 = R.at<int32_t>(L.nbr125);
    fc_u64 *sortbuf = R.at<fc_u64>(L.sort);
    fc_ctl *ctl = R.ctl;
    const int gn = R.grid((size_t)n);

    // maps
    LR_HIP(hipMemsetAsync(ctl, 0, 256, st));
    LR_HIP(hipMemsetAsync(R.keys[0], 0xff, 4 * L.cap_max * 8, st));
    LR_HIP(hipMemsetAsync(R.val[0], 0x7f, 4 * L.cap_max * 4, st));
    hipLaunchKernelGGL(fc_l0_insert_kernel, dim3(gn), dim3(256), 0, st, coords, n, R.keys[0], R.val[0], mask, ctl);
    hipLaunchKernelGGL(fc_l0_check_kernel, dim3(gn), dim3(256), 0, st, coords, n, R.keys[0], R.val[0], mask, ctl);
    unsigned n_sort = FC_SORT_CHUNK;
    while (n_sort < (unsigned)n) n_sort <<= 1;
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL(fc_coarse_insert_kernel, dim3(gn), dim3(256), 0, st, R.coords[l], l, R.keys[l + 1], R.val[l + 1], mask, ctl);
        hipLaunchKernelGGL(fc_coarse_mark_kernel, dim3(R.grid(n_sort)), dim3(256), 0, st, R.coords[l], l, R.keys[l + 1], R.val[l + 1], mask, sortbuf, (int)n_sort, ctl);
        fc_sort_launch(sortbuf, n_sort, st);
        hipLaunchKernelGGL(fc_coarse_index_kernel, dim3(gn), dim3(256), 0, st, sortbuf, l + 1, R.keys[l + 1], R.val[l + 1], mask, const_cast<int32_t *>(R.coords[l + 1]), ctl);
    }
    const int K1 = p->conv1_kernel_size;
    for (int l = 0; l < 4; ++l)
        hipLaunchKernelGGL(fc_nbr_kernel, dim3(R.grid((size_t)n * 27)), dim3(256), 0, st, R.coords[l], l, R.keys[l], R.val[l], mask, 3, 1 << l, R.nbr27[l], ctl);
    if (K1 == 5)
        hipLaunchKernelGGL(fc_nbr_kernel, dim3(R.grid((size_t)n * 125)), dim3(256), 0, st, R.coords[0], 0, R.keys[0], R.val[0], mask, 5, 1, nbr125, ctl);
    for (int l = 0; l < 3; ++l) {
        hipLaunchKernelGGL(fc_nbr_kernel, dim3(R.grid((size_t)n * 27)), dim3(256), 0, st, R.coords[l + 1], l + 1, R.keys[l], R.val[l], mask, 3, 1 << l, R.dn[l], ctl);
        hipLaunchKernelGGL(fc_nbr_kernel, dim3(R.grid((size_t)n * 27)), dim3(256), 0, st, R.coords[l], l, R.keys[l + 1], R.val[l + 1], mask, 3, -(1 << l), R.up[l], ctl);
    }

    // a tap ends the call behind its stage
    const int tap = p->tap;
    const bool end = fc_stages(R,
        [&](float *X) {
            hipLaunchKernelGGL(fc_conv1_kernel, dim3(R.grid((size_t)n * 32)), dim3(256), 0, st, feat_in, K1 == 5 ? nbr125 : R.nbr27[0], K1 * K1 * K1, R.w[1],
                               R.w[1] + (size_t)K1 * K1 * K1 * 32, R.w[1] + (size_t)K1 * K1 * K1 * 32 + 32, X, ctl);
        },
        [&](int s, const float *buf, int lvl) -> bool {
            if (tap != s) return false;
            const int cout = R.t[s].cout;
            const size_t items = (size_t)n * (cout > 3 ? cout : 3);
            hipLaunchKernelGGL(fc_tap_kernel, dim3(R.grid(items)), dim3(256), 0, st, buf, cout, lvl, R.coords[lvl], n, feat_out, tap_coords, ctl, result);
            return true;
        });
    const float *Y = R.at<float>(L.Y);
    if (!end) hipLaunchKernelGGL(fc_norm_kernel, dim3(gn), dim3(256), 0, st, Y, n, feat_out, ctl, result);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

#include "lr_fcgf_batch.h"
