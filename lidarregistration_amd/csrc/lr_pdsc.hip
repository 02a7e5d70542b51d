// PointDSC's SC-NonLocal correspondence encoder and confidence head on gfx950 (Experiments/models/PointDSC.py:9-77, :107-113, :150-153,
// :171), inference mode.  The contract (E1-E6) and the weight blob are stated in include/lidarreg.h and DESIGN.md §16 and restated in
// numpy in tests/pdsc_cpu.py.
//
// The reference materialises three M x M fp32 matrices per layer (compatibility, logits, softmax weights); here none is stored: the
// attention kernel is a flash-style pass that re-evaluates compat(i,j) from the six coordinates where it is used.
//
// Kernels (each launched ONCE for a batch, the pair is grid z or the block index; a single-pair call is a batch of one):
//   pd_setup_kernel    descriptors by value -> control blocks: live M and the attention's work plan
//   pd_prep_kernel     one block per pair: dead rows (E1), the fp64 column means in a fixed tree (E2), 32-byte records
//                      { s.xyz, t.xyz, live, 0 } (a dead row: all zero), the centred input rows [m][8], the result struct
//   pd_rowtile_kernel  every small layer: 64 rows x up to 128 outputs per block, y = act(scale * (W x) + offset) (+ residual); the weight
//                      chunk and the transposed row tile sit in LDS, a thread owns 8 rows x 4 outputs, fp32 fmaf over ascending input
//   pd_attn_kernel     the hot path: block = 128 queries (32 per wave) x one chunk of keys, tiles of 32 keys double-buffered in LDS.
//                      S^T = K Q^T on v_mfma_f32_32x32x2_f32 (keys on rows, queries on columns, 64 steps): lane l then owns query l & 31 and
//                      holds 16 keys of the tile, lane l ^ 32 the other 16; compat, scale, running maximum / sum and the rescale factor are
//                      lane-local, one exchange of the tile maximum with the partner lane; the probabilities go from those registers into
//                      the B operand of O^T = V^T P^T (4 x 16 accumulator registers for 128 channels).  Unnormalised O, m and l of the chunk go
//                      to part[chunk][row] by plain stores
//   pd_combine_kernel  merges a row's chunks in ascending order and normalises -> message
//   pd_final_kernel    features and confidence to the caller's arrays: 0 / -inf on dead rows, 0 past the live count
// No floating-point atomics anywhere: every sum has one order, which depends on the pair's own live M only -- never on the batch the
// pair is in, on the device, on scheduling or on what the scratch held.
#include "lr_corrset.h"
#include "lr_prims.h"
#include <math.h>
#include <float.h>

#define PD_C 128                     // channels
#define PD_MAX_LAYERS 16
#define PD_IN 8                      // input row: the 6 centred coordinates and two zeros
#define PD_RT_ROWS 64                // rows per block of the row-tile kernel
#define PD_RT_OUTS 128               // outputs per block of the row-tile kernel
#define PD_QB 128                    // queries per attention block: 4 waves x 32
#define PD_KT 32                     // keys per tile
#define PD_MAX_CHUNKS 8              // key chunks per row
#define PD_TARGET_BLOCKS 512         // attention blocks a pair's plan aims at (a constant: the plan must not depend on the device)
#define PD_NB 1024
#define PD_VS 136                    // floats between the V rows in LDS: 4 rows apart = 32 banks apart (the two half-waves read keys 4 apart)
#define PD_KS (PD_C * PD_KT + 32)    // floats of a K tile in LDS: channel-major, the upper 64 channels shifted by 32 banks

typedef float pd_f32x16 __attribute__((ext_vector_type(16)));
typedef float pd_f32x4 __attribute__((ext_vector_type(4)));

// per-pair control block at the head of the pair's scratch arena
struct pd_ctl {
    const float *a, *b;
    float *feat_out, *conf_out;
    int32_t m_host, m;               // what the caller passed as m; the live count (m_dev clamped to 0..m_host)
    int32_t dead, nlive;             // rows with a non-finite coordinate among the m; m - dead
    int32_t nb, chunks, per, pad;    // attention plan: query blocks of 128, key chunks, keys per chunk (a multiple of 32)
};

// Work plan of one pair's attention pass: nb * chunks blocks of 128 queries x `per` keys.  A function of the pair's live M alone
// (the order of a row's sums follows from it).
struct pd_plan { int nb, chunks, per; };
__host__ __device__ static inline pd_plan pd_make_plan(int m)
{
    pd_plan p;
    p.nb = m > 0 ? (m + PD_QB - 1) / PD_QB : 1;
    int ch = PD_TARGET_BLOCKS / p.nb;
    if (ch > PD_MAX_CHUNKS) ch = PD_MAX_CHUNKS;
    if (ch < 1) ch = 1;
    const int tiles = m > 0 ? (m + PD_KT - 1) / PD_KT : 1;
    if (ch > tiles) ch = tiles;
    const int tpc = (tiles + ch - 1) / ch;
    p.per = tpc * PD_KT;
    p.chunks = (tiles + tpc - 1) / tpc;
    return p;
}
// blocks the attention launch needs for ANY live count up to mx: nb(m) * chunks(m) <= min(8 nb(mx), max(512, nb(mx)))
static inline int pd_max_blocks(int mx)
{
    const int nb = mx > 0 ? (mx + PD_QB - 1) / PD_QB : 1;
    int a = PD_MAX_CHUNKS * nb;
    const int b = nb > PD_TARGET_BLOCKS ? nb : PD_TARGET_BLOCKS;
    if (a > b) a = b;
    return a;
}

struct pd_layout { size_t ctl, rec, x0, A, B, qkv, msg, f1, f2, conf, part_o, part_ml, total; };
static pd_layout pd_make_layout(int max_m)
{
    const size_t Mp = ((size_t)(max_m < 1 ? 1 : max_m) + PD_QB - 1) / PD_QB * PD_QB;
    const size_t prow = (size_t)pd_max_blocks(max_m) * PD_QB;      // rows of part[chunk][row]: at most 8 Mp, at most 65536
    pd_layout L;
    size_t o = 0;
    L.ctl = o;     o += lr_al(sizeof(pd_ctl));
    L.rec = o;     o += lr_al(Mp * 32);
    L.x0 = o;      o += lr_al(Mp * PD_IN * 4);
    L.A = o;       o += lr_al(Mp * PD_C * 4);
    L.B = o;       o += lr_al(Mp * PD_C * 4);
    L.qkv = o;     o += lr_al(Mp * 3 * PD_C * 4);
    L.msg = o;     o += lr_al(Mp * PD_C * 4);
    L.f1 = o;      o += lr_al(Mp * 64 * 4);
    L.f2 = o;      o += lr_al(Mp * 64 * 4);
    L.conf = o;    o += lr_al(Mp * 4);
    L.part_o = o;  o += lr_al(prow * PD_C * 4);
    L.part_ml = o; o += lr_al(prow * 8);
    L.total = o;
    return L;
}

struct pd_args {
    char *base;                      // scratch arena of pair 0
    size_t stride;                   // bytes between consecutive pairs' arenas
    pd_layout L;
};

// the weight blob: floats of a block { Wt[in][out], scale[out], offset[out] }
static constexpr size_t pd_blk(size_t n_in, size_t n_out) { return n_in * n_out + 2 * n_out; }
static constexpr size_t PD_W_L0 = pd_blk(PD_IN, PD_C);
static constexpr size_t PD_W_PCN = pd_blk(PD_C, PD_C), PD_W_QKV = pd_blk(PD_C, 3 * PD_C);
static constexpr size_t PD_W_F1 = pd_blk(PD_C, 64), PD_W_F2 = pd_blk(64, 64), PD_W_F3 = pd_blk(64, PD_C);
static constexpr size_t PD_W_LAYER = PD_W_PCN + PD_W_QKV + PD_W_F1 + PD_W_F2 + PD_W_F3;
static constexpr size_t PD_W_HEAD = pd_blk(PD_C, 32) + pd_blk(32, 32) + pd_blk(32, 1);

// ---- setup: descriptors by value -> control blocks (no host copy, graph-capturable) ------------------------------------------
__global__ void pd_setup_kernel(cs_desc_table t, pd_args g, int npairs)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const cs_desc d = t.d[k];
    pd_ctl *c = lr_ptr<pd_ctl>(g, k, g.L.ctl);
    const int m = cs_live_m(d);
    const pd_plan p = pd_make_plan(m);
    c->a = d.a; c->b = d.b; c->feat_out = (float *)d.out0; c->conf_out = (float *)d.out1;
    c->m_host = d.m; c->m = m;
    c->dead = 0; c->nlive = 0;
    c->nb = p.nb; c->chunks = p.chunks; c->per = p.per; c->pad = 0;
}

// ---- E1, E2: dead rows, the column means, records and the centred input ---------------------------------------------------------
__global__ void __launch_bounds__(PD_NB) pd_prep_kernel(pd_args g, lr_pdsc_result *results)
{
    __shared__ double s_red[PD_NB];
    const int pair = blockIdx.x, tid = threadIdx.x;
    pd_ctl *c = lr_ptr<pd_ctl>(g, pair, g.L.ctl);
    const int m = c->m;
    double sum[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, cnt = 0.0;
    for (int i = tid; i < m; i += PD_NB) {
        float r[6];
        if (cs_load_row(c->a, c->b, i, r)) {
            for (int k = 0; k < 6; ++k) sum[k] += (double)r[k];
            cnt += 1.0;
        }
    }
    double mean[6];
    const double n = lr_block_tree_sum<PD_NB>(cnt, s_red);
    for (int k = 0; k < 6; ++k) { const double s = lr_block_tree_sum<PD_NB>(sum[k], s_red); mean[k] = n > 0.0 ? s / n : 0.0; }
    float *rec = lr_ptr<float>(g, pair, g.L.rec), *x0 = lr_ptr<float>(g, pair, g.L.x0);
    for (int i = tid; i < m; i += PD_NB) {
        float r[6];
        const bool ok = cs_load_row(c->a, c->b, i, r);
        for (int k = 0; k < 6; ++k) {
            rec[(size_t)i * 8 + k] = ok ? r[k] : 0.0f;
            x0[(size_t)i * PD_IN + k] = ok ? (float)((double)r[k] - mean[k]) : 0.0f;
        }
        rec[(size_t)i * 8 + 6] = ok ? 1.0f : 0.0f; rec[(size_t)i * 8 + 7] = 0.0f;
        x0[(size_t)i * PD_IN + 6] = 0.0f; x0[(size_t)i * PD_IN + 7] = 0.0f;
    }
    if (tid == 0) {
        const int nlive = (int)n;
        c->nlive = nlive; c->dead = m - nlive;
        lr_pdsc_result *res = results + pair;
        res->status = nlive > 0 ? 0 : 1; res->m = m; res->dead = m - nlive; res->reserved = 0;
    }
}

// ---- the small layers -------------------------------------------------------------------------------------------------------------
// out[row][o] = act(scale[o] * sum_i W[o][i] in[row][i] + offset[o]) (+ res[row][o]), rows below the pair's live count.  W points at the
// layer's block { Wt[n_in][n_out], scale, offset }; n_in a multiple of 4, at most 128.  Block = 64 rows x outputs [128 y, 128 y + 128).
struct pd_layer {
    size_t in_off, out_off, res_off;     // arena offsets; res_off = ~0: no residual
    int ld_in, ld_out, ld_res, n_in, n_out, relu;
};

__global__ void __launch_bounds__(256) pd_rowtile_kernel(pd_args g, pd_layer y, const float *__restrict__ W)
{
    __shared__ float s_w[PD_C * PD_RT_OUTS];
    __shared__ float s_x[PD_C * PD_RT_ROWS];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int m = lr_ptr<pd_ctl>(g, pair, g.L.ctl)->m;
    const int row0 = blockIdx.x * PD_RT_ROWS, o0 = blockIdx.y * PD_RT_OUTS;
    if (row0 >= m) return;
    const int no = min(PD_RT_OUTS, y.n_out - o0);
    if ((y.n_out & 3) == 0) {                        // (the blob's blocks start at multiples of 4 floats: 16-byte loads, several in flight)
#pragma unroll 4
        for (int idx = tid; idx < y.n_in * (PD_RT_OUTS / 4); idx += 256) {
            const int i = idx >> 5, o = 4 * (idx & 31);
            pd_f32x4 v = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (o < no) v = *reinterpret_cast<const pd_f32x4 *>(W + (size_t)i * y.n_out + o0 + o);
            *reinterpret_cast<pd_f32x4 *>(&s_w[4 * idx]) = v;
        }
    } else {
        for (int idx = tid; idx < y.n_in * PD_RT_OUTS; idx += 256) {
            const int i = idx >> 7, o = idx & 127;
            s_w[idx] = o < no ? W[(size_t)i * y.n_out + o0 + o] : 0.0f;
        }
    }
    const float *in = lr_ptr<float>(g, pair, y.in_off);
    {
        const int row = tid & 63;
        for (int c4 = tid >> 6; c4 < y.n_in / 4; c4 += 4) {
            pd_f32x4 v = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (row0 + row < m) v = *reinterpret_cast<const pd_f32x4 *>(in + (size_t)(row0 + row) * y.ld_in + 4 * c4);
            for (int k = 0; k < 4; ++k) s_x[(4 * c4 + k) * PD_RT_ROWS + row] = v[k];
        }
    }
    __syncthreads();
    const int to = tid & 31, tr = tid >> 5;          // outputs 4 to .. 4 to + 3, rows 8 tr .. 8 tr + 7
    float acc[8][4];
    for (int r = 0; r < 8; ++r)
        for (int k = 0; k < 4; ++k) acc[r][k] = 0.0f;
#pragma unroll 4
    for (int i = 0; i < y.n_in; ++i) {
        const pd_f32x4 w = *reinterpret_cast<const pd_f32x4 *>(&s_w[i * PD_RT_OUTS + 4 * to]);
        const pd_f32x4 xa = *reinterpret_cast<const pd_f32x4 *>(&s_x[i * PD_RT_ROWS + 8 * tr]);
        const pd_f32x4 xb = *reinterpret_cast<const pd_f32x4 *>(&s_x[i * PD_RT_ROWS + 8 * tr + 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc[r][k] = fmaf(xa[r], w[k], acc[r][k]); acc[4 + r][k] = fmaf(xb[r], w[k], acc[4 + r][k]); }
    }
    const float *scale = W + (size_t)y.n_in * y.n_out, *offset = scale + y.n_out;
    float *out = lr_ptr<float>(g, pair, y.out_off);
    const float *res = y.res_off != ~size_t(0) ? lr_ptr<const float>(g, pair, y.res_off) : nullptr;
    const int ob = o0 + 4 * to;
    if (4 * to >= no) return;
    float sc[4], of[4];
    for (int k = 0; k < 4; ++k) { const bool in_range = ob + k < y.n_out; sc[k] = in_range ? scale[ob + k] : 0.0f; of[k] = in_range ? offset[ob + k] : 0.0f; }
    for (int r = 0; r < 8; ++r) {
        const int row = row0 + 8 * tr + r;
        if (row >= m) break;
        for (int k = 0; k < 4; ++k) {
            if (ob + k >= y.n_out) break;
            float v = fmaf(sc[k], acc[r][k], of[k]);
            if (y.relu) v = fmaxf(v, 0.0f);
            if (res) v = v + res[(size_t)row * y.ld_res + ob + k];
            out[(size_t)row * y.ld_out + ob + k] = v;
        }
    }
}

// ---- the hot path -----------------------------------------------------------------------------------------------------------------
struct pd_tile_regs { pd_f32x4 k[4], v[4], r; };

// tile t of the chunk [k0, k1) -> registers (keys at and past k1: zeros, i.e. records that are not live)
__device__ __forceinline__ void pd_tile_fetch(pd_tile_regs &T, const float *__restrict__ qkv, const float *__restrict__ rec, int kbase, int k1, int tid)
{
    const pd_f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + 256 * j;
        const int kk = kbase + (idx & 31), c4 = idx >> 5;           // K: the key is the fast index (conflict-free LDS writes, channel-major)
        T.k[j] = kk < k1 ? *reinterpret_cast<const pd_f32x4 *>(qkv + (size_t)kk * (3 * PD_C) + PD_C + 4 * c4) : zero;
        const int kv = kbase + (idx >> 5), v4 = idx & 31;           // V: the channel is the fast index (coalesced, row-major in LDS)
        T.v[j] = kv < k1 ? *reinterpret_cast<const pd_f32x4 *>(qkv + (size_t)kv * (3 * PD_C) + 2 * PD_C + 4 * v4) : zero;
    }
    T.r = zero;
    if (tid < 64) {
        const int kk = kbase + (tid >> 1);
        if (kk < k1) T.r = *reinterpret_cast<const pd_f32x4 *>(rec + (size_t)kk * 8 + 4 * (tid & 1));
    }
}
__device__ __forceinline__ void pd_tile_store(const pd_tile_regs &T, float *s_k, float *s_v, float *s_r, int tid)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + 256 * j;
        const int key = idx & 31, c4 = idx >> 5;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const int ch = 4 * c4 + e; s_k[ch * PD_KT + key + (ch >= 64 ? 32 : 0)] = T.k[j][e]; }
        *reinterpret_cast<pd_f32x4 *>(&s_v[(idx >> 5) * PD_VS + 4 * (idx & 31)]) = T.v[j];
    }
    if (tid < 64) *reinterpret_cast<pd_f32x4 *>(&s_r[(tid >> 1) * 8 + 4 * (tid & 1)]) = T.r;
}

__global__ void __launch_bounds__(256) pd_attn_kernel(pd_args g, float nk, float qscale)
{
    __shared__ float s_k[2][PD_KS];
    __shared__ float s_v[2][PD_KT * PD_VS];
    __shared__ float s_r[2][PD_KT * 8];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const pd_ctl *c = lr_ptr<pd_ctl>(g, pair, g.L.ctl);
    const int m = c->m, nb = c->nb;
    if (m <= 0 || (int)blockIdx.x >= nb * c->chunks) return;
    const int rb = (int)blockIdx.x % nb, ch = (int)blockIdx.x / nb;
    const int lane = tid & 63, h = lane >> 5, ql = lane & 31;
    const int q = rb * PD_QB + (tid >> 6) * 32 + ql, qc = q < m ? q : m - 1;
    const int k0 = ch * c->per, k1 = min(m, k0 + c->per);
    const float *__restrict__ qkv = lr_ptr<const float>(g, pair, g.L.qkv);
    const float *__restrict__ rec = lr_ptr<const float>(g, pair, g.L.rec);

    // the query's row: lane half h holds channels 64 h .. 64 h + 63 (MFMA step s contracts channels s and 64 + s)
    float qr[64];
    {
        const pd_f32x4 *src = reinterpret_cast<const pd_f32x4 *>(qkv + (size_t)qc * (3 * PD_C) + 64 * h);
#pragma unroll
        for (int j = 0; j < 16; ++j) { const pd_f32x4 v = src[j]; qr[4 * j] = v[0]; qr[4 * j + 1] = v[1]; qr[4 * j + 2] = v[2]; qr[4 * j + 3] = v[3]; }
    }
    float own[6];
    {
        const pd_f32x4 r0 = *reinterpret_cast<const pd_f32x4 *>(rec + (size_t)qc * 8), r1 = *reinterpret_cast<const pd_f32x4 *>(rec + (size_t)qc * 8 + 4);
        own[0] = r0[0]; own[1] = r0[1]; own[2] = r0[2]; own[3] = r0[3]; own[4] = r1[0]; own[5] = r1[1];
    }

    pd_f32x16 o[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.0f;
    float m_run = -FLT_MAX, l_run = 0.0f;

    const int ntiles = (k1 - k0 + PD_KT - 1) / PD_KT;
    pd_tile_regs T;
    pd_tile_fetch(T, qkv, rec, k0, k1, tid);
    pd_tile_store(T, s_k[0], s_v[0], s_r[0], tid);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        const bool more = t + 1 < ntiles;            // (block-uniform)
        if (more) pd_tile_fetch(T, qkv, rec, k0 + (t + 1) * PD_KT, k1, tid);
        // S^T = K Q^T: keys on rows, queries on columns
        pd_f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
        const float *kb = &s_k[buf][h * (64 * PD_KT + 32) + ql];
#pragma unroll
        for (int s = 0; s < 64; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[s * PD_KT], qr[s], S, 0, 0, 0);
        // logits of this lane's 16 keys: key (r & 3) + 8 (r >> 2) + 4 h of the tile
        float x[16], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = (r & 3) + 8 * (r >> 2) + 4 * h;
            const pd_f32x4 r0 = *reinterpret_cast<const pd_f32x4 *>(&s_r[buf][key * 8]), r1 = *reinterpret_cast<const pd_f32x4 *>(&s_r[buf][key * 8 + 4]);
            const float cij = cs_compat(own, r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], nk);
            x[r] = r1[2] > 0.0f ? cij * (S[r] * qscale) : -INFINITY;
            tmax = fmaxf(tmax, x[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));    // the one exchange with the partner half
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __expf(m_run - m_new);
        float lsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { x[r] = __expf(x[r] - m_new); lsum += x[r]; }
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {                  // (a factor of exactly 1 changes no bit)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
        }
        // O^T += V^T P^T: channels on rows, queries on columns; step r contracts the keys the two lane halves hold in register r
        const float *vb = &s_v[buf][4 * h * PD_VS + ql];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) o[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[key * PD_VS + 32 * cb], x[r], o[cb], 0, 0, 0);
        }
        if (more) pd_tile_store(T, s_k[buf ^ 1], s_v[buf ^ 1], s_r[buf ^ 1], tid);
        __syncthreads();
    }
    // the chunk's partial: unnormalised O, running maximum, sum (the two halves' sums added once, lower half first)
    const float l_lo = __shfl(l_run, ql), l_hi = __shfl(l_run, ql + 32);
    if (q >= m) return;
    const size_t prow = (size_t)ch * ((size_t)nb * PD_QB) + q;
    float *po = lr_ptr<float>(g, pair, g.L.part_o) + prow * PD_C;
    if (h == 0) {
        float *pml = lr_ptr<float>(g, pair, g.L.part_ml) + prow * 2;
        pml[0] = m_run; pml[1] = l_lo + l_hi;
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const pd_f32x4 v = { o[cb][4 * g4], o[cb][4 * g4 + 1], o[cb][4 * g4 + 2], o[cb][4 * g4 + 3] };
            *reinterpret_cast<pd_f32x4 *>(po + 32 * cb + 8 * g4 + 4 * h) = v;
        }
}

// message[row][c] = sum over the chunks (ascending) of O_chunk[row][c] exp(m_chunk - max) / sum of l_chunk exp(m_chunk - max)
__global__ void __launch_bounds__(256) pd_combine_kernel(pd_args g)
{
    const int pair = blockIdx.z, tid = threadIdx.x;
    const pd_ctl *c = lr_ptr<pd_ctl>(g, pair, g.L.ctl);
    const int m = c->m, row = blockIdx.x * 2 + (tid >> 7), chn = tid & 127;
    if (row >= m) return;
    const int chunks = c->chunks;
    const size_t cstride = (size_t)c->nb * PD_QB;
    const float *po = lr_ptr<const float>(g, pair, g.L.part_o), *pml = lr_ptr<const float>(g, pair, g.L.part_ml);
    float mx = -FLT_MAX;
    for (int k = 0; k < chunks; ++k) mx = fmaxf(mx, pml[((size_t)k * cstride + row) * 2]);
    float l = 0.0f, acc = 0.0f;
    for (int k = 0; k < chunks; ++k) {
        const size_t pr = (size_t)k * cstride + row;
        const float w = __expf(pml[pr * 2] - mx);
        l = fmaf(pml[pr * 2 + 1], w, l);
        acc = fmaf(po[pr * PD_C + chn], w, acc);
    }
    lr_ptr<float>(g, pair, g.L.msg)[(size_t)row * PD_C + chn] = l > 0.0f ? acc / l : 0.0f;
}

// features and confidence to the caller's arrays
__global__ void __launch_bounds__(256) pd_final_kernel(pd_args g)
{
    const int pair = blockIdx.z, tid = threadIdx.x;
    const pd_ctl *c = lr_ptr<pd_ctl>(g, pair, g.L.ctl);
    const int row = blockIdx.x * 2 + (tid >> 7), chn = tid & 127;
    if (row >= c->m_host) return;
    const bool in = row < c->m;
    const bool live = in && lr_ptr<const float>(g, pair, g.L.rec)[(size_t)row * 8 + 6] > 0.0f;
    if (c->feat_out) c->feat_out[(size_t)row * PD_C + chn] = live ? lr_ptr<const float>(g, pair, g.L.A)[(size_t)row * PD_C + chn] : 0.0f;
    if (c->conf_out && chn == 0) c->conf_out[row] = live ? lr_ptr<const float>(g, pair, g.L.conf)[row] : (in ? -INFINITY : 0.0f);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_pdsc_params) == 16 && sizeof(lr_pdsc_result) == 16, "ABI structs changed: update include/lidarreg.h and _ext.py together");

extern "C" size_t lr_pdsc_weights_bytes(int num_layers)
{
    if (num_layers < 1 || num_layers > PD_MAX_LAYERS) return 0;
    return (PD_W_L0 + (size_t)num_layers * PD_W_LAYER + PD_W_HEAD) * sizeof(float);
}

extern "C" size_t lr_pdsc_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > CS_MAX_M) return 0;
    return pd_make_layout(max_m).total;
}

static int check_pdsc_params(const lr_pdsc_params *p, const char *who)
{
    LR_CHECK_STRUCT_SIZE(lr_pdsc_params, p, who);
    if (p->num_layers < 1 || p->num_layers > PD_MAX_LAYERS) { lr_set_error("%s: num_layers must lie in 1..%d", who, PD_MAX_LAYERS); return LR_EINVAL; }
    if (!(p->sigma_d > 0.0 && isfinite(p->sigma_d))) { lr_set_error("%s: sigma_d must be positive and finite", who); return LR_EINVAL; }
    return LR_OK;
}

static void pd_layer_launch(const pd_args &g, int mx, int npairs, hipStream_t st, const float *W, size_t in_off, int ld_in, int n_in,
                            size_t out_off, int ld_out, int n_out, int relu, size_t res_off = ~size_t(0), int ld_res = 0)
{
    const pd_layer y = { in_off, out_off, res_off, ld_in, ld_out, ld_res, n_in, n_out, relu };
    hipLaunchKernelGGL(pd_rowtile_kernel, dim3(lr_cdiv(mx, PD_RT_ROWS), lr_cdiv(n_out, PD_RT_OUTS), npairs), dim3(256), 0, st, g, y, W);
}

// `who`: the entry point the params and weights messages name; the checks of the shared front report as lr_pdsc_encode_batch
static int pd_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                  const float *weights, size_t weights_bytes, const lr_pdsc_params *p, lr_pdsc_result *results, float *const *feat_out,
                  float *const *conf_out, void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_pdsc_encode_batch", "npairs * lr_pdsc_scratch_bytes(max m)", lr_pdsc_scratch_bytes, LR_EINVAL };
    LR_TRY_HIP(check_pdsc_params(p, who));
    LR_REFUSE_UNLESS(weights, LR_EINVAL, "null weights");
    LR_REFUSE_UNLESS(((uintptr_t)weights & 15) == 0, LR_EINVAL, "weights must be 16-byte aligned");
    if (weights_bytes < lr_pdsc_weights_bytes(p->num_layers)) { lr_set_error("%s: weights_bytes is below lr_pdsc_weights_bytes(num_layers)", who); return LR_EINVAL; }
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, (void *const *)feat_out, (void *const *)conf_out, results, scratch, scratch_bytes, stream, &f));
    const int mx = f.mx;

    pd_args g;
    g.base = reinterpret_cast<char *>(scratch);
    g.stride = f.per;
    g.L = pd_make_layout(mx);
    const pd_layout &L = g.L;
    const float nk = (float)(-1.0 / (p->sigma_d * p->sigma_d));
    const float qscale = (float)(1.0 / sqrt((double)PD_C));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pd_setup_kernel, dim3(1), dim3(64), 0, st, f.t, g, npairs);
    hipLaunchKernelGGL(pd_prep_kernel, dim3(npairs), dim3(PD_NB), 0, st, g, results);
    if (mx > 0) {
        const float *W = weights;
        pd_layer_launch(g, mx, npairs, st, W, L.x0, PD_IN, PD_IN, L.A, PD_C, PD_C, 0);                      W += PD_W_L0;
        for (int layer = 0; layer < p->num_layers; ++layer) {
            pd_layer_launch(g, mx, npairs, st, W, L.A, PD_C, PD_C, L.B, PD_C, PD_C, 1);                     W += PD_W_PCN;
            pd_layer_launch(g, mx, npairs, st, W, L.B, PD_C, PD_C, L.qkv, 3 * PD_C, 3 * PD_C, 0);           W += PD_W_QKV;
            hipLaunchKernelGGL(pd_attn_kernel, dim3(pd_max_blocks(mx), 1, npairs), dim3(256), 0, st, g, nk, qscale);
            hipLaunchKernelGGL(pd_combine_kernel, dim3(lr_cdiv(mx, 2), 1, npairs), dim3(256), 0, st, g);
            pd_layer_launch(g, mx, npairs, st, W, L.msg, PD_C, PD_C, L.f1, 64, 64, 1);                      W += PD_W_F1;
            pd_layer_launch(g, mx, npairs, st, W, L.f1, 64, 64, L.f2, 64, 64, 1);                           W += PD_W_F2;
            pd_layer_launch(g, mx, npairs, st, W, L.f2, 64, 64, L.A, PD_C, PD_C, 0, L.B, PD_C);             W += PD_W_F3;
        }
        pd_layer_launch(g, mx, npairs, st, W, L.A, PD_C, PD_C, L.f1, 64, 32, 1);                            W += pd_blk(PD_C, 32);
        pd_layer_launch(g, mx, npairs, st, W, L.f1, 64, 32, L.f2, 64, 32, 1);                               W += pd_blk(32, 32);
        pd_layer_launch(g, mx, npairs, st, W, L.f2, 64, 32, L.conf, 1, 1, 0);
        hipLaunchKernelGGL(pd_final_kernel, dim3(lr_cdiv(mx, 2), 1, npairs), dim3(256), 0, st, g);
    }
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_pdsc_encode_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                    const float *weights, size_t weights_bytes, const lr_pdsc_params *p, lr_pdsc_result *results,
                                    float *const *feat_out, float *const *conf_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return pd_run("lr_pdsc_encode_batch", npairs, src, tgt, m, m_dev, weights, weights_bytes, p, results, feat_out, conf_out, scratch, scratch_bytes, stream);
}

extern "C" int lr_pdsc_encode(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, size_t weights_bytes,
                              const lr_pdsc_params *p, lr_pdsc_result *result, float *feat_out, float *conf_out, void *scratch,
                              size_t scratch_bytes, void *stream)
{
    return pd_run("lr_pdsc_encode", 1, &src, &tgt, &m, &m_dev, weights, weights_bytes, p, result, &feat_out, &conf_out, scratch, scratch_bytes, stream);
}
