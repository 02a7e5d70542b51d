// PointDSC's tail on gfx950: seed picking, the per-seed neural spectral matching, the per-seed fits, hypothesis selection and the post
// refinement (Experiments/models/PointDSC.py:199-217, :234-358, :403-438; models/common.py:7-69), inference mode, on the features and the
// confidence of lr_pdsc.hip.  The contract (S1-S10) is stated in include/lidarreg.h and DESIGN.md §17 and restated in numpy in
// tests/pdsc_solve_cpu.py.
//
// The reference forms the M x M feature distance matrix to take every row's k nearest neighbours and then keeps the seeds' rows; here only
// the seeds' rows are ever formed, tile by tile, behind a running top-k' -- no M x M and no n_seeds x M matrix is stored.
//
// Kernels (each launched ONCE for a batch; a single-pair call is a batch of one):
//   ps_setup_kernel    descriptors by value -> control blocks (src, tgt, m_dev, labels, seeds travel in cs_desc_table)
//   ps_setup2_kernel   the second by-value table: features and confidence per pair; the single call's trace outputs
//   ps_prep_kernel     a wave per row: S1 (dead rows), S3 (normalised features), 32-byte records { s.xyz, t.xyz, live, conf }
//   ps_plan_kernel     a thread per pair: live count, n_seeds, k', the kNN's plan
//   ps_nms_kernel      S2: the M x M test streamed through LDS in tiles of 256 rows; stores a key per row, nothing per pair of rows
//   ps_rank_kernel     S2's order without a sort: rank_i = #{ live j : (key_j, j) before (key_i, i) }, streamed the same way; rank_i < n_seeds
//                      puts row i at seeds[rank_i]
//   ps_knn_kernel      the hot path (S4): block = 128 seeds (32 per wave) x one chunk of keys, key tiles of 32 double-buffered in LDS,
//                      S^T = K Q^T on v_mfma_f32_32x32x2_f32 as in pd_attn_kernel; both lanes of a seed put their 16 similarities of the tile
//                      into LDS, the lane of the lower half-wave owns the seed's top-k' list there (unordered, its last entry under S4's
//                      order tracked): a key enters only if it sorts before that entry, which it replaces; the list is ordered once, when
//                      the chunk ends
//   ps_merge_kernel    a thread per seed merges its chunks' sorted lists under S4's total order
//   ps_seedfit_kernel  a wave per seed: S5 (k' x k' in LDS), S6, S7
//   ps_score_kernel    a block per seed: S8's integer count over all rows
//   ps_final_kernel    a block per pair: the best seed, labels, S9's loop, the result block
// No floating-point atomics; the one integer atomic counts dead rows.
#include "lr_corrset.h"
#include "lr_prims.h"
#include "lr_contract.h"
#include <math.h>
#include <float.h>

#define PS_C 128                     // channels
#define PS_KMAX 64                   // largest k
#define PS_QB 128                    // seeds per kNN block: 4 waves x 32
#define PS_KT 32                     // keys per tile
#define PS_MAX_CHUNKS 8
#define PS_TARGET_BLOCKS 512         // kNN blocks a pair's plan aims at (a constant: the plan must not depend on the device)
#define PS_KS (PS_C * PS_KT + 32)    // floats of a key tile in LDS: channel-major, the upper 64 channels shifted by 32 banks
#define PS_NB 1024                   // threads of the per-pair final kernel
#define PS_FS 129                    // floats between the neighbours' feature rows in LDS (lane a reads bank (a + c) % 64)

typedef float ps_f32x16 __attribute__((ext_vector_type(16)));
typedef float ps_f32x4 __attribute__((ext_vector_type(4)));
typedef float ps_f32x2 __attribute__((ext_vector_type(2)));

// per-pair control block at the head of the pair's scratch arena
struct ps_ctl {
    const float *a, *b, *feat, *conf;
    uint8_t *labels_out;
    int32_t *seeds_out;
    int32_t *knn_out; float *weight_out; double *seedT_out; int32_t *count_out;      // the single call's trace outputs
    int32_t m_host, m;               // what the caller passed as m; m_dev clamped to 0..m_host
    int32_t dead, nlive;
    int32_t n_seeds, kp;             // kp = k' = min(k, nlive - 1)
    int32_t nsb, chunks, per, seed_cap;      // kNN plan: seed blocks of 128, key chunks, keys per chunk; entries of seeds_out
};

// Work plan of one pair's kNN pass: nsb * chunks blocks of 128 seeds x `per` keys: a function of n_seeds and m alone.
struct ps_plan { int nsb, chunks, per; };
__host__ __device__ static inline ps_plan ps_make_plan(int n_seeds, int m)
{
    ps_plan p;
    p.nsb = n_seeds > 0 ? (n_seeds + PS_QB - 1) / PS_QB : 1;
    int ch = PS_TARGET_BLOCKS / p.nsb;
    if (ch > PS_MAX_CHUNKS) ch = PS_MAX_CHUNKS;
    if (ch < 1) ch = 1;
    const int tiles = m > 0 ? (m + PS_KT - 1) / PS_KT : 1;
    if (ch > tiles) ch = tiles;
    const int tpc = (tiles + ch - 1) / ch;
    p.per = tpc * PS_KT;
    p.chunks = (tiles + tpc - 1) / tpc;
    return p;
}
// blocks the kNN launch needs for ANY seed count up to smax: nsb * chunks <= min(8 nsb(smax), max(512, nsb(smax)))
static inline int ps_max_blocks(int smax)
{
    const int nsb = smax > 0 ? (smax + PS_QB - 1) / PS_QB : 1;
    int a = PS_MAX_CHUNKS * nsb;
    const int b = nsb > PS_TARGET_BLOCKS ? nsb : PS_TARGET_BLOCKS;
    if (a > b) a = b;
    return a;
}

struct ps_layout { size_t ctl, rec, fn, key, seeds, part_v, part_i, part_n, knn, wgt, seedT, count, total; };
static ps_layout ps_make_layout(int max_m)
{
    // (ratio <= 1: as many seed slots as rows)
    const size_t Mp = ((size_t)(max_m < 1 ? 1 : max_m) + PS_QB - 1) / PS_QB * PS_QB;
    const size_t prow = (size_t)ps_max_blocks(max_m) * PS_QB;      // rows of part[chunk][seed]
    ps_layout L;
    size_t o = 0;
    L.ctl = o;    o += lr_al(sizeof(ps_ctl));
    L.rec = o;    o += lr_al(Mp * 32);
    L.fn = o;     o += lr_al(Mp * PS_C * 4);
    L.key = o;    o += lr_al(Mp * 4);
    L.seeds = o;  o += lr_al(Mp * 4);
    L.part_v = o; o += lr_al(prow * PS_KMAX * 4);
    L.part_i = o; o += lr_al(prow * PS_KMAX * 4);
    L.part_n = o; o += lr_al(prow * 4);
    L.knn = o;    o += lr_al(Mp * PS_KMAX * 4);
    L.wgt = o;    o += lr_al(Mp * PS_KMAX * 4);
    L.seedT = o;  o += lr_al(Mp * 16 * 8);
    L.count = o;  o += lr_al(Mp * 4);
    L.total = o;
    return L;
}

struct ps_args {
    char *base;                      // scratch arena of pair 0
    size_t stride;                   // bytes between consecutive pairs' arenas
    ps_layout L;
};

// the pointers cs_desc has no room for
struct ps_ext { const float *feat, *conf; };
struct ps_ext_table { ps_ext d[LR_MAX_BATCH]; };
struct ps_trace { int32_t *knn; float *weight; double *seedT; int32_t *count; };
static_assert(sizeof(ps_ext_table) + sizeof(ps_args) + sizeof(ps_trace) + 64 <= 4096, "the second table no longer fits the kernel arguments");

// what the kernels read of lr_pdsc_solve_params
struct ps_consts {
    int k, num_iterations, refine_iters;
    float R, nk_d, nk_f;             // (float)nms_radius, (float)(-1 / sigma_d^2), (float)(-1 / sigma^2)
    double ratio, thr, rthr;
};

// ---- setup ------------------------------------------------------------------------------------------------------------------------
__global__ void ps_setup_kernel(cs_desc_table t, ps_args g, int npairs, double ratio)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const cs_desc d = t.d[k];
    ps_ctl *c = lr_ptr<ps_ctl>(g, k, g.L.ctl);
    c->a = d.a; c->b = d.b; c->labels_out = (uint8_t *)d.out0; c->seeds_out = (int32_t *)d.out1;
    c->m_host = d.m; c->m = cs_live_m(d);
    c->dead = 0; c->nlive = 0; c->n_seeds = 0; c->kp = 0;
    c->nsb = 1; c->chunks = 1; c->per = PS_KT;
    c->seed_cap = (int)((double)d.m * ratio);
}

__global__ void ps_setup2_kernel(ps_ext_table t, ps_args g, int npairs, ps_trace tr)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    ps_ctl *c = lr_ptr<ps_ctl>(g, k, g.L.ctl);
    c->feat = t.d[k].feat; c->conf = t.d[k].conf;
    c->knn_out = tr.knn; c->weight_out = tr.weight; c->seedT_out = tr.seedT; c->count_out = tr.count;
}

// the butterfly of S3 / S6: every lane ends with the same value
__device__ __forceinline__ float ps_wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

// ---- S1, S3: a wave per row ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ps_prep_kernel(ps_args g)
{
    const int pair = blockIdx.z, lane = threadIdx.x & 63;
    ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= c->m) return;
    float r[6];
    const bool finite = cs_load_row(c->a, c->b, i, r);
    const float cf = c->conf[i];
    const ps_f32x2 f = *reinterpret_cast<const ps_f32x2 *>(c->feat + (size_t)i * PS_C + 2 * lane);
    const bool ok = fabsf(cf) <= FLT_MAX && fabsf(f[0]) <= FLT_MAX && fabsf(f[1]) <= FLT_MAX && finite;      // (false for NaN and inf)
    const bool live = __all(ok);
    const float nrm = sqrtf(ps_wave_sum(f[0] * f[0] + f[1] * f[1]));
    const float den = fmaxf(nrm, 1e-12f);
    ps_f32x2 fn = { 0.0f, 0.0f };
    if (live) { fn[0] = f[0] / den; fn[1] = f[1] / den; }
    *reinterpret_cast<ps_f32x2 *>(lr_ptr<float>(g, pair, g.L.fn) + (size_t)i * PS_C + 2 * lane) = fn;
    if (lane < 8) {
        float v = 0.0f;
        if (live) v = lane < 6 ? r[lane] : (lane == 6 ? 1.0f : cf);      // (slot 7: conf)
        lr_ptr<float>(g, pair, g.L.rec)[(size_t)i * 8 + lane] = v;
    }
    if (lane == 0 && !live) atomicAdd(&c->dead, 1);
}

__global__ void ps_plan_kernel(ps_args g, int npairs, ps_consts P)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    ps_ctl *c = lr_ptr<ps_ctl>(g, k, g.L.ctl);
    const int nlive = c->m - c->dead;
    int kp = nlive - 1 < P.k ? nlive - 1 : P.k;
    if (kp < 0) kp = 0;
    int ns = (int)((double)nlive * P.ratio);         // Python's int(num_corr * ratio): the product in double, truncated
    if (kp < 1) ns = 0;
    const ps_plan p = ps_make_plan(ns, c->m);
    c->nlive = nlive; c->n_seeds = ns; c->kp = kp;
    c->nsb = p.nsb; c->chunks = p.chunks; c->per = p.per;
}

// ---- S2 -----------------------------------------------------------------------------------------------------------------------------
// key_i = conf_i if no live j within R has a larger conf, else 0.  Rows past m and dead rows enter a tile with conf -inf.
__global__ void __launch_bounds__(256) ps_nms_kernel(ps_args g, float R)
{
    __shared__ ps_f32x4 s_t[256];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int m = c->m;
    if ((int)blockIdx.x * 256 >= m) return;
    float *rec = lr_ptr<float>(g, pair, g.L.rec);
    const int i = blockIdx.x * 256 + tid, ic = i < m ? i : m - 1;
    const float px = rec[(size_t)ic * 8], py = rec[(size_t)ic * 8 + 1], pz = rec[(size_t)ic * 8 + 2], cf = rec[(size_t)ic * 8 + 7];
    const bool live = i < m && rec[(size_t)ic * 8 + 6] > 0.0f;
    bool lm = true;
    for (int base = 0; base < m; base += 256) {
        const int j = base + tid;
        ps_f32x4 e = { 0.0f, 0.0f, 0.0f, -INFINITY };
        if (j < m && rec[(size_t)j * 8 + 6] > 0.0f) { e[0] = rec[(size_t)j * 8]; e[1] = rec[(size_t)j * 8 + 1]; e[2] = rec[(size_t)j * 8 + 2]; e[3] = rec[(size_t)j * 8 + 7]; }
        __syncthreads();
        s_t[tid] = e;
        __syncthreads();
        const int n = min(256, m - base);
        for (int t = 0; t < n; ++t) {
            const ps_f32x4 q = s_t[t];
            const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
            const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
            lm = lm && (cf >= q[3] || dist >= R);
        }
    }
    // (other blocks still read conf from slot 7 of this row: the key has an array of its own)
    if (i < m) lr_ptr<float>(g, pair, g.L.key)[i] = live ? (lm ? cf : 0.0f) : 0.0f;
}

// (v, i) sorts before (w, j): descending value, ascending index
__device__ __forceinline__ bool ps_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ void __launch_bounds__(256) ps_rank_kernel(ps_args g)
{
    __shared__ ps_f32x2 s_t[256];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int m = c->m, ns = c->n_seeds, i = blockIdx.x * 256 + tid;
    // seeds_out's tail
    if (c->seeds_out && i >= ns && i < c->seed_cap) c->seeds_out[i] = -1;
    if ((int)blockIdx.x * 256 >= m || ns <= 0) return;
    const float *rec = lr_ptr<const float>(g, pair, g.L.rec);
    const float *key = lr_ptr<const float>(g, pair, g.L.key);
    const int ic = i < m ? i : m - 1;
    const float ki = key[ic];
    const bool live = i < m && rec[(size_t)ic * 8 + 6] > 0.0f;
    int rank = 0;
    for (int base = 0; base < m; base += 256) {
        const int j = base + tid;
        ps_f32x2 e = { 0.0f, 0.0f };
        if (j < m) { e[0] = key[j]; e[1] = rec[(size_t)j * 8 + 6]; }
        __syncthreads();
        s_t[tid] = e;
        __syncthreads();
        const int n = min(256, m - base);
        for (int t = 0; t < n; ++t) {
            const ps_f32x2 q = s_t[t];
            rank += (q[1] > 0.0f && ps_before(q[0], base + t, ki, i)) ? 1 : 0;
        }
    }
    if (live && rank < ns) {
        lr_ptr<int32_t>(g, pair, g.L.seeds)[rank] = i;
        if (c->seeds_out) c->seeds_out[rank] = i;
    }
}

// ---- the hot path: S4 -----------------------------------------------------------------------------------------------------------------
struct ps_tile_regs { ps_f32x4 k[4]; float live; };

// tile at kbase of the chunk [k0, k1) -> registers (keys at and past k1: zeros, not live)
__device__ __forceinline__ void ps_tile_fetch(ps_tile_regs &T, const float *__restrict__ fn, const float *__restrict__ rec, int kbase, int k1, int tid)
{
    const ps_f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + 256 * j;
        const int kk = kbase + (idx & 31), c4 = idx >> 5;           // the key is the fast index (conflict-free LDS writes, channel-major)
        T.k[j] = kk < k1 ? *reinterpret_cast<const ps_f32x4 *>(fn + (size_t)kk * PS_C + 4 * c4) : zero;
    }
    T.live = 0.0f;
    if (tid < PS_KT && kbase + tid < k1) T.live = rec[(size_t)(kbase + tid) * 8 + 6];
}
__device__ __forceinline__ void ps_tile_store(const ps_tile_regs &T, float *s_k, float *s_l, int tid)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = tid + 256 * j;
        const int key = idx & 31, c4 = idx >> 5;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const int ch = 4 * c4 + e; s_k[ch * PS_KT + key + (ch >= 64 ? 32 : 0)] = T.k[j][e]; }
    }
    if (tid < PS_KT) s_l[tid] = T.live;
}

__global__ void __launch_bounds__(256) ps_knn_kernel(ps_args g)
{
    __shared__ float s_k[2][PS_KS];
    __shared__ float s_l[2][PS_KT];
    __shared__ float s_lv[PS_KMAX][PS_QB];           // the seeds' lists, unordered until the chunk ends: [slot][seed of the block]
    __shared__ int s_li[PS_KMAX][PS_QB];
    __shared__ float s_c[PS_KT][PS_QB];              // the tile's similarities: [key of the tile][seed of the block]
    const int pair = blockIdx.z, tid = threadIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int m = c->m, ns = c->n_seeds, nsb = c->nsb, kp = c->kp;
    if (ns <= 0 || (int)blockIdx.x >= nsb * c->chunks) return;
    const int sb = (int)blockIdx.x % nsb, ch = (int)blockIdx.x / nsb;
    const int lane = tid & 63, h = lane >> 5, ql = lane & 31;
    const int sl = (tid >> 6) * 32 + ql;             // seed of the block
    const int q = sb * PS_QB + sl;
    const int32_t *seeds = lr_ptr<const int32_t>(g, pair, g.L.seeds);
    const int self = seeds[q < ns ? q : ns - 1];
    const int k0 = ch * c->per, k1 = min(m, k0 + c->per);
    const float *__restrict__ fn = lr_ptr<const float>(g, pair, g.L.fn);
    const float *__restrict__ rec = lr_ptr<const float>(g, pair, g.L.rec);

    // the seed's row: lane half h holds channels 64 h .. 64 h + 63 (MFMA step s contracts channels s and 64 + s)
    float qr[64];
    {
        const ps_f32x4 *src = reinterpret_cast<const ps_f32x4 *>(fn + (size_t)self * PS_C + 64 * h);
#pragma unroll
        for (int j = 0; j < 16; ++j) { const ps_f32x4 v = src[j]; qr[4 * j] = v[0]; qr[4 * j + 1] = v[1]; qr[4 * j + 2] = v[2]; qr[4 * j + 3] = v[3]; }
    }
    const bool owner = h == 0 && q < ns;
    int cnt = 0, thr_i = 0, thr_p = 0;               // entries of the list; its LAST entry under S4's order (value, row, slot) once it is full
    float thr_v = 0.0f;

    const int ntiles = (k1 - k0 + PS_KT - 1) / PS_KT;
    ps_tile_regs T;
    ps_tile_fetch(T, fn, rec, k0, k1, tid);
    ps_tile_store(T, s_k[0], s_l[0], tid);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1, kbase = k0 + t * PS_KT;
        const bool more = t + 1 < ntiles;            // (block-uniform)
        if (more) ps_tile_fetch(T, fn, rec, kbase + PS_KT, k1, tid);
        ps_f32x16 S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
        const float *kb = &s_k[buf][h * (64 * PS_KT + 32) + ql];
#pragma unroll
        for (int s = 0; s < 64; ++s) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[s * PS_KT], qr[s], S, 0, 0, 0);
        // this lane holds key (r & 3) + 8 (r >> 2) + 4 h of the tile in register r: both halves put theirs where the owner reads them
        // (the two lanes of a seed are lanes of one wave, whose LDS operations complete in order)
#pragma unroll
        for (int r = 0; r < 16; ++r) s_c[(r & 3) + 8 * (r >> 2) + 4 * h][sl] = S[r];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (owner) {
            for (int kt = 0; kt < PS_KT; ++kt) {
                const int key = kbase + kt;
                const float v = s_c[kt][sl];
                if (!(s_l[buf][kt] > 0.0f) || key == self) continue;
                bool rescan = false;
                if (cnt < kp) {
                    s_lv[cnt][sl] = v; s_li[cnt][sl] = key;
                    rescan = ++cnt == kp;
                } else if (ps_before(v, key, thr_v, thr_i)) {      // it replaces the last entry
                    s_lv[thr_p][sl] = v; s_li[thr_p][sl] = key;
                    rescan = true;
                }
                if (rescan) {                        // the new last entry: the one every other entry sorts before (independent loads)
                    thr_p = 0; thr_v = s_lv[0][sl]; thr_i = s_li[0][sl];
#pragma unroll 8
                    for (int p = 1; p < kp; ++p) {
                        const float w = s_lv[p][sl];
                        const int j = s_li[p][sl];
                        if (ps_before(thr_v, thr_i, w, j)) { thr_v = w; thr_i = j; thr_p = p; }
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (more) ps_tile_store(T, s_k[buf ^ 1], s_l[buf ^ 1], tid);
        __syncthreads();
    }
    if (!owner) return;
    const size_t prow = (size_t)ch * ((size_t)nsb * PS_QB) + q;
    float *pv = lr_ptr<float>(g, pair, g.L.part_v) + prow * PS_KMAX;
    int32_t *pi = lr_ptr<int32_t>(g, pair, g.L.part_i) + prow * PS_KMAX;
    // the chunk's list in S4's order, by selection
    for (int o = 0; o < cnt; ++o) {
        int bp = o, bi = s_li[o][sl];
        float bv = s_lv[o][sl];
        const float ov = bv;
        const int oi = bi;
        for (int p = o + 1; p < cnt; ++p) {
            const float w = s_lv[p][sl];
            const int j = s_li[p][sl];
            if (ps_before(w, j, bv, bi)) { bv = w; bi = j; bp = p; }
        }
        s_lv[bp][sl] = ov; s_li[bp][sl] = oi;
        pv[o] = bv; pi[o] = bi;
    }
    lr_ptr<int32_t>(g, pair, g.L.part_n)[prow] = cnt;
}

__global__ void __launch_bounds__(256) ps_merge_kernel(ps_args g, int k)
{
    const int pair = blockIdx.z;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int ns = c->n_seeds, kp = c->kp, q = blockIdx.x * 256 + threadIdx.x;
    if (q >= ns) return;
    const int chunks = c->chunks;
    const size_t cstride = (size_t)c->nsb * PS_QB;
    const float *pv = lr_ptr<const float>(g, pair, g.L.part_v);
    const int32_t *pi = lr_ptr<const int32_t>(g, pair, g.L.part_i), *pn = lr_ptr<const int32_t>(g, pair, g.L.part_n);
    int32_t *knn = lr_ptr<int32_t>(g, pair, g.L.knn) + (size_t)q * PS_KMAX;
    int head[PS_MAX_CHUNKS];
#pragma unroll
    for (int x = 0; x < PS_MAX_CHUNKS; ++x) head[x] = 0;
    for (int o = 0; o < kp; ++o) {
        int best = -1, bi = 0;
        float bv = 0.0f;
#pragma unroll
        for (int x = 0; x < PS_MAX_CHUNKS; ++x) {
            if (x < chunks) {
                const size_t pr = (size_t)x * cstride + q;
                if (head[x] < pn[pr]) {
                    const float v = pv[pr * PS_KMAX + head[x]];
                    const int j = pi[pr * PS_KMAX + head[x]];
                    if (best < 0 || ps_before(v, j, bv, bi)) { best = x; bv = v; bi = j; }
                }
            }
        }
        // (live - 1 >= k' candidates exist over the chunks: best >= 0)
#pragma unroll
        for (int x = 0; x < PS_MAX_CHUNKS; ++x) head[x] += x == best ? 1 : 0;
        knn[o] = bi;
        if (c->knn_out) c->knn_out[(size_t)q * k + o] = bi;
    }
    if (c->knn_out) for (int o = kp; o < k; ++o) c->knn_out[(size_t)q * k + o] = -1;
}

// ---- S5, S6, S7: a wave per seed --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) ps_seedfit_kernel(ps_args g, ps_consts P)
{
    __shared__ float s_f[PS_KMAX * PS_FS];
    __shared__ float s_M[PS_KMAX][PS_KMAX + 1];
    __shared__ float s_p[PS_KMAX][8];
    __shared__ float s_v[PS_KMAX];
    __shared__ double s_w[PS_KMAX];
    __shared__ double s_c[8];
    __shared__ double s_H[9];
    const int pair = blockIdx.z, a = threadIdx.x, q = blockIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    if (q >= c->n_seeds) return;
    const int kp = c->kp;
    const float *fn = lr_ptr<const float>(g, pair, g.L.fn), *rec = lr_ptr<const float>(g, pair, g.L.rec);
    const int32_t *knn = lr_ptr<const int32_t>(g, pair, g.L.knn) + (size_t)q * PS_KMAX;
    const bool in = a < kp;
    const int j = in ? knn[a] : 0;
    float fa[PS_C], own[6];
    {
        const ps_f32x4 *src = reinterpret_cast<const ps_f32x4 *>(fn + (size_t)j * PS_C);
#pragma unroll
        for (int x = 0; x < PS_C / 4; ++x) {
            const ps_f32x4 v = src[x];
#pragma unroll
            for (int e = 0; e < 4; ++e) { fa[4 * x + e] = v[e]; s_f[a * PS_FS + 4 * x + e] = v[e]; }
        }
        for (int x = 0; x < 6; ++x) { own[x] = rec[(size_t)j * 8 + x]; s_p[a][x] = own[x]; }
    }
    __syncthreads();
    // S5
    for (int b = 0; b < kp; ++b) {
        float dot = 0.0f;
#pragma unroll
        for (int x = 0; x < PS_C; ++x) dot = fmaf(fa[x], s_f[b * PS_FS + x], dot);
        const float fs = fmaxf(0.0f, fmaf(1.0f - dot, P.nk_f, 1.0f));
        s_M[a][b] = (in && a != b) ? fs * cs_compat(own, s_p[b][0], s_p[b][1], s_p[b][2], s_p[b][3], s_p[b][4], s_p[b][5], P.nk_d) : 0.0f;
    }
    // S6
    float v = in ? 1.0f : 0.0f;
    for (int it = 0; it < P.num_iterations; ++it) {
        __syncthreads();
        s_v[a] = v;
        __syncthreads();
        float u = 0.0f;
        for (int b = 0; b < kp; ++b) u = fmaf(s_M[a][b], s_v[b], u);
        if (!in) u = 0.0f;
        const float nrm = sqrtf(ps_wave_sum(u * u));
        v = u / (nrm + 1e-6f);
    }
    const float w = v / (ps_wave_sum(v) + 1e-6f);
    if (c->weight_out) for (int o = a; o < P.k; o += 64) c->weight_out[(size_t)q * P.k + o] = o < kp ? w : 0.0f;
    // S7: fp64, every sum from 0 in ascending order of the neighbour
    __syncthreads();
    s_w[a] = in ? (double)w : 0.0;
    __syncthreads();
    if (a < 7) {
        double s = 0.0;
        for (int b = 0; b < kp; ++b) s += a == 0 ? s_w[b] : s_w[b] * (double)s_p[b][a - 1];
        s_c[a] = s;
    }
    __syncthreads();
    const double den = s_c[0] + 1e-6;                // models/common.py:24-25
    if (a < 9) {
        const int x = a / 3, y = a % 3;
        const double cx = s_c[1 + x] / den, cy = s_c[4 + y] / den;
        double s = 0.0;
        for (int b = 0; b < kp; ++b) s += (s_w[b] * ((double)s_p[b][x] - cx)) * ((double)s_p[b][3 + y] - cy);
        s_H[a] = s;
    }
    __syncthreads();
    if (a == 0) {
        double H[3][3], cen[6], T[16];
        for (int x = 0; x < 9; ++x) H[x / 3][x % 3] = s_H[x];
        for (int x = 0; x < 6; ++x) cen[x] = s_c[1 + x] / den;
        lr_rt_from_cov(H, cen, cen + 3, T);
        double *out = lr_ptr<double>(g, pair, g.L.seedT) + (size_t)q * 16;
        for (int x = 0; x < 16; ++x) out[x] = T[x];
        if (c->seedT_out) for (int x = 0; x < 16; ++x) c->seedT_out[(size_t)q * 16 + x] = T[x];
    }
}

// ---- S8 -----------------------------------------------------------------------------------------------------------------------------
// the residual of row r = { s.xyz, t.xyz, .. } under T, fp64, no fused multiply-add
__device__ __forceinline__ double ps_resid(const double *T, const float *r)
{
    const double sx = (double)r[0], sy = (double)r[1], sz = (double)r[2];
    const double dx = (((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3]) - (double)r[3];
    const double dy = (((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7]) - (double)r[4];
    const double dz = (((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11]) - (double)r[5];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// the block's sum of one int per thread (NT threads)
template <int NT> __device__ __forceinline__ int ps_block_isum(int v, int *s)
{
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if (lane == 0) s[tid >> 6] = v;
    __syncthreads();
    int tot = 0;
    for (int w = 0; w < NT / 64; ++w) tot += s[w];
    return tot;
}

__global__ void __launch_bounds__(256) ps_score_kernel(ps_args g, double thr)
{
    __shared__ int s_cnt[4];
    const int pair = blockIdx.z, tid = threadIdx.x, q = blockIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    if (q >= c->n_seeds) return;
    const int m = c->m;
    const float *rec = lr_ptr<const float>(g, pair, g.L.rec);
    const double *Tg = lr_ptr<const double>(g, pair, g.L.seedT) + (size_t)q * 16;
    double T[12];
    for (int x = 0; x < 12; ++x) T[x] = Tg[x];
    int n = 0;
    for (int i = tid; i < m; i += 256) {
        const ps_f32x4 r0 = *reinterpret_cast<const ps_f32x4 *>(rec + (size_t)i * 8), r1 = *reinterpret_cast<const ps_f32x4 *>(rec + (size_t)i * 8 + 4);
        const float r[6] = { r0[0], r0[1], r0[2], r0[3], r1[0], r1[1] };
        n += (r1[2] > 0.0f && ps_resid(T, r) < thr) ? 1 : 0;
    }
    const int tot = ps_block_isum<256>(n, s_cnt);
    if (tid == 0) {
        lr_ptr<int32_t>(g, pair, g.L.count)[q] = tot;
        if (c->count_out) c->count_out[q] = tot;
    }
}

// ---- the best seed, labels, S9, the result ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PS_NB) ps_final_kernel(ps_args g, ps_consts P, lr_pdsc_solve_result *results)
{
    __shared__ double s_red[PS_NB];
    __shared__ int s_cnt[PS_NB / 64];
    __shared__ int s_bc[PS_NB], s_br[PS_NB];
    __shared__ double s_T[16];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const ps_ctl *c = lr_ptr<ps_ctl>(g, pair, g.L.ctl);
    const int m = c->m, mh = c->m_host, ns = c->n_seeds;
    const float *rec = lr_ptr<const float>(g, pair, g.L.rec);
    const int32_t *count = lr_ptr<const int32_t>(g, pair, g.L.count);
    uint8_t *labels = c->labels_out;
    lr_pdsc_solve_result *res = results + pair;

    // the first seed of largest count
    int bc = -1, br = 0x7fffffff;
    for (int q = tid; q < ns; q += PS_NB) { const int n = count[q]; if (n > bc) { bc = n; br = q; } }
    s_bc[tid] = bc; s_br[tid] = br;
    __syncthreads();
    for (int h = PS_NB / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const int oc = s_bc[tid + h], orr = s_br[tid + h];
            if (oc > s_bc[tid] || (oc == s_bc[tid] && orr < s_br[tid])) { s_bc[tid] = oc; s_br[tid] = orr; }
        }
        __syncthreads();
    }
    const int best = ns > 0 ? s_br[0] : -1;
    if (tid < 16) s_T[tid] = best >= 0 ? lr_ptr<const double>(g, pair, g.L.seedT)[(size_t)best * 16 + tid] : (tid % 5 == 0 ? 1.0 : 0.0);
    __syncthreads();
    double T[12];
    for (int x = 0; x < 12; ++x) T[x] = s_T[x];

    // labels: the best seed's inliers, 0 on dead rows and at and past the live count
    int nl = 0;
    for (int i = tid; i < mh; i += PS_NB) {
        bool on = false;
        if (best >= 0 && i < m && rec[(size_t)i * 8 + 6] > 0.0f) on = ps_resid(T, rec + (size_t)i * 8) < P.thr;
        if (labels) labels[i] = on ? 1 : 0;
        nl += on ? 1 : 0;
    }
    nl = ps_block_isum<PS_NB>(nl, s_cnt);
    if (tid == 0) {
        for (int x = 0; x < 16; ++x) res->T_best[x] = s_T[x];
        res->status = c->nlive <= 0 ? 1 : (ns <= 0 ? 2 : 0);
        res->m = m; res->dead = c->dead; res->n_seeds = ns;
        res->best_rank = best; res->best_index = best >= 0 ? lr_ptr<const int32_t>(g, pair, g.L.seeds)[best] : -1;
        res->best_count = best >= 0 ? s_bc[0] : 0;
        res->n_labels = nl;
        res->reserved[0] = 0; res->reserved[1] = 0; res->reserved[2] = 0;
    }

    // S9
    int prev = 0, rounds = 0;
    for (int it = 0; best >= 0 && it < P.refine_iters; ++it) {
        int n = 0;
        for (int i = tid; i < m; i += PS_NB)
            n += (rec[(size_t)i * 8 + 6] > 0.0f && ps_resid(T, rec + (size_t)i * 8) < P.rthr) ? 1 : 0;
        n = ps_block_isum<PS_NB>(n, s_cnt);
        if (n == prev) break;                        // (block-uniform)
        prev = n;
        double v[9];
        for (int x = 0; x < 7; ++x) v[x] = 0.0;
        for (int i = tid; i < m; i += PS_NB) {
            const float *r = rec + (size_t)i * 8;
            if (!(r[6] > 0.0f)) continue;
            const double d = ps_resid(T, r);
            if (!(d < P.rthr)) continue;
            const double e = d / P.rthr, w = 1.0 / (1.0 + e * e);
            v[0] += w;
            for (int x = 0; x < 6; ++x) v[1 + x] += w * (double)r[x];
        }
        const double den = lr_block_tree_sum<PS_NB>(v[0], s_red) + 1e-6;
        double cen[6];
        for (int x = 0; x < 6; ++x) cen[x] = lr_block_tree_sum<PS_NB>(v[1 + x], s_red) / den;
        for (int x = 0; x < 9; ++x) v[x] = 0.0;
        for (int i = tid; i < m; i += PS_NB) {
            const float *r = rec + (size_t)i * 8;
            if (!(r[6] > 0.0f)) continue;
            const double d = ps_resid(T, r);
            if (!(d < P.rthr)) continue;
            const double e = d / P.rthr, w = 1.0 / (1.0 + e * e);
            for (int x = 0; x < 3; ++x)
                for (int y = 0; y < 3; ++y) v[3 * x + y] += (w * ((double)r[x] - cen[x])) * ((double)r[3 + y] - cen[3 + y]);
        }
        double H[3][3];
        for (int x = 0; x < 9; ++x) H[x / 3][x % 3] = lr_block_tree_sum<PS_NB>(v[x], s_red);
        if (tid == 0) { double Tn[16]; lr_rt_from_cov(H, cen, cen + 3, Tn); for (int x = 0; x < 16; ++x) s_T[x] = Tn[x]; }
        __syncthreads();
        for (int x = 0; x < 12; ++x) T[x] = s_T[x];
        ++rounds;
    }
    __syncthreads();
    if (tid == 0) {
        for (int x = 0; x < 16; ++x) res->T[x] = s_T[x];
        res->refine_rounds = rounds;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_pdsc_solve_params) == 64 && sizeof(lr_pdsc_solve_result) == 304, "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_pdsc_solve_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > CS_MAX_M) return 0;
    return ps_make_layout(max_m).total;
}

// a pair's share of a register call: the encoder's arena, its features and confidence, the solver's arena
struct pr_layout { size_t enc, feat, conf, solve; };
static pr_layout pr_make_layout(int max_m)
{
    const size_t Mp = ((size_t)(max_m < 1 ? 1 : max_m) + PS_QB - 1) / PS_QB * PS_QB;
    pr_layout L;
    L.enc = lr_pdsc_scratch_bytes(max_m);
    L.feat = lr_al(Mp * PS_C * 4);
    L.conf = lr_al(Mp * 4);
    L.solve = ps_make_layout(max_m).total;
    return L;
}

extern "C" size_t lr_pdsc_register_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > CS_MAX_M) return 0;
    const pr_layout L = pr_make_layout(max_m);
    return L.enc + L.feat + L.conf + L.solve;
}

static int check_solve_params(const lr_pdsc_solve_params *p, const char *who)
{
    LR_CHECK_STRUCT_SIZE(lr_pdsc_solve_params, p, who);
    if (p->num_iterations < 1 || p->num_iterations > 1000) { lr_set_error("%s: num_iterations must lie in 1..1000", who); return LR_EINVAL; }
    if (p->k < 1 || p->k > PS_KMAX) { lr_set_error("%s: k must lie in 1..%d", who, PS_KMAX); return LR_EINVAL; }
    if (p->refine_iters < 0 || p->refine_iters > 1000) { lr_set_error("%s: refine_iters must lie in 0..1000", who); return LR_EINVAL; }
    if (!(p->ratio > 0.0 && p->ratio <= 1.0)) { lr_set_error("%s: ratio must lie in (0, 1]", who); return LR_EINVAL; }
    if (!(p->nms_radius >= 0.0 && isfinite(p->nms_radius))) { lr_set_error("%s: nms_radius must be non-negative and finite", who); return LR_EINVAL; }
    if (!(p->inlier_threshold > 0.0 && isfinite(p->inlier_threshold))) { lr_set_error("%s: inlier_threshold must be positive and finite", who); return LR_EINVAL; }
    if (!(p->refine_threshold > 0.0 && isfinite(p->refine_threshold))) { lr_set_error("%s: refine_threshold must be positive and finite", who); return LR_EINVAL; }
    if (!(p->sigma_d > 0.0 && isfinite(p->sigma_d))) { lr_set_error("%s: sigma_d must be positive and finite", who); return LR_EINVAL; }
    if (!(p->sigma > 0.0 && isfinite(p->sigma))) { lr_set_error("%s: sigma must be positive and finite", who); return LR_EINVAL; }
    return LR_OK;
}

// the launches of a checked call; `scratch`: arena of pair 0, `stride` bytes between the pairs' arenas
static int ps_launch(const cs_front &f, const ps_ext_table &ext, const ps_trace &tr, int npairs, const lr_pdsc_solve_params *p,
                     lr_pdsc_solve_result *results, void *scratch, size_t stride, void *stream)
{
    const int mx = f.mx;
    ps_args g;
    g.base = reinterpret_cast<char *>(scratch);
    g.stride = stride;
    g.L = ps_make_layout(mx);
    ps_consts P;
    P.k = p->k; P.num_iterations = p->num_iterations; P.refine_iters = p->refine_iters;
    P.R = (float)p->nms_radius;
    P.nk_d = (float)(-1.0 / (p->sigma_d * p->sigma_d));
    P.nk_f = (float)(-1.0 / (p->sigma * p->sigma));
    P.ratio = p->ratio; P.thr = p->inlier_threshold; P.rthr = p->refine_threshold;
    const int smax = (int)((double)mx * p->ratio);   // no pair has more seeds: n_seeds = (int)(live * ratio), live <= mx
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ps_setup_kernel, dim3(1), dim3(64), 0, st, f.t, g, npairs, p->ratio);
    hipLaunchKernelGGL(ps_setup2_kernel, dim3(1), dim3(64), 0, st, ext, g, npairs, tr);
    if (mx > 0) {
        hipLaunchKernelGGL(ps_prep_kernel, dim3(lr_cdiv(mx, 4), 1, npairs), dim3(256), 0, st, g);
        hipLaunchKernelGGL(ps_plan_kernel, dim3(1), dim3(64), 0, st, g, npairs, P);
        hipLaunchKernelGGL(ps_nms_kernel, dim3(lr_cdiv(mx, 256), 1, npairs), dim3(256), 0, st, g, P.R);
        hipLaunchKernelGGL(ps_rank_kernel, dim3(lr_cdiv(mx, 256), 1, npairs), dim3(256), 0, st, g);
        if (smax > 0) {
            hipLaunchKernelGGL(ps_knn_kernel, dim3(ps_max_blocks(smax), 1, npairs), dim3(256), 0, st, g);
            hipLaunchKernelGGL(ps_merge_kernel, dim3(lr_cdiv(smax, 256), 1, npairs), dim3(256), 0, st, g, P.k);
            hipLaunchKernelGGL(ps_seedfit_kernel, dim3(smax, 1, npairs), dim3(64), 0, st, g, P);
            hipLaunchKernelGGL(ps_score_kernel, dim3(smax, 1, npairs), dim3(256), 0, st, g, P.thr);
        }
    }
    hipLaunchKernelGGL(ps_final_kernel, dim3(npairs), dim3(PS_NB), 0, st, g, P, results);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

static int ps_fill_ext(const char *who, int npairs, const int32_t *m, const float *const *feat, const float *const *conf, ps_ext_table *ext)
{
    LR_REFUSE_UNLESS(feat && conf, LR_EINVAL, "null pointer");
    for (int k = 0; k < LR_MAX_BATCH; ++k) ext->d[k] = ps_ext{ nullptr, nullptr };
    for (int k = 0; k < npairs; ++k) {
        LR_REFUSE_UNLESS(m[k] == 0 || feat[k], LR_EINVAL, "null feat");
        LR_REFUSE_UNLESS(m[k] == 0 || conf[k], LR_EINVAL, "null conf");
        LR_REFUSE_UNLESS(((uintptr_t)feat[k] & 7) == 0, LR_EINVAL, "feat must be 8-byte aligned");
        ext->d[k] = ps_ext{ feat[k], conf[k] };
    }
    return LR_OK;
}

// `who`: the entry point the params messages name; the checks of the shared front report as lr_pdsc_solve_batch
static int ps_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                  const float *const *feat, const float *const *conf, const lr_pdsc_solve_params *p, lr_pdsc_solve_result *results,
                  uint8_t *const *labels_out, int32_t *const *seeds_out, const ps_trace &tr, void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_pdsc_solve_batch", "npairs * lr_pdsc_solve_scratch_bytes(max m)", lr_pdsc_solve_scratch_bytes, LR_EINVAL };
    LR_TRY_HIP(check_solve_params(p, who));
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, (void *const *)labels_out, (void *const *)seeds_out, results, scratch, scratch_bytes, stream, &f));
    ps_ext_table ext;
    LR_TRY_HIP(ps_fill_ext(who, npairs, m, feat, conf, &ext));
    return ps_launch(f, ext, tr, npairs, p, results, scratch, f.per, stream);
}

extern "C" int lr_pdsc_solve_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                   const float *const *feat, const float *const *conf, const lr_pdsc_solve_params *p,
                                   lr_pdsc_solve_result *results, uint8_t *const *labels_out, int32_t *const *seeds_out, void *scratch,
                                   size_t scratch_bytes, void *stream)
{
    const ps_trace none = { nullptr, nullptr, nullptr, nullptr };
    return ps_run("lr_pdsc_solve_batch", npairs, src, tgt, m, m_dev, feat, conf, p, results, labels_out, seeds_out, none, scratch, scratch_bytes, stream);
}

extern "C" int lr_pdsc_solve(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *feat, const float *conf,
                             const lr_pdsc_solve_params *p, lr_pdsc_solve_result *result, uint8_t *labels_out, int32_t *seeds_out,
                             int32_t *knn_out, float *weight_out, double *seedT_out, int32_t *count_out, void *scratch, size_t scratch_bytes,
                             void *stream)
{
    const ps_trace tr = { knn_out, weight_out, seedT_out, count_out };
    return ps_run("lr_pdsc_solve", 1, &src, &tgt, &m, &m_dev, &feat, &conf, p, result, &labels_out, &seeds_out, tr, scratch, scratch_bytes, stream);
}

// encode, then solve: the scratch is [npairs encoder arenas][npairs feature blocks][npairs confidence blocks][npairs solver arenas]
static int pr_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                  const float *weights, size_t weights_bytes, const lr_pdsc_params *ep, const lr_pdsc_solve_params *sp,
                  lr_pdsc_solve_result *results, float *const *feat_out, float *const *conf_out, uint8_t *const *labels_out,
                  int32_t *const *seeds_out, void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_pdsc_register_batch", "npairs * lr_pdsc_register_scratch_bytes(max m)", lr_pdsc_register_scratch_bytes, LR_EINVAL };
    LR_TRY_HIP(check_solve_params(sp, who));
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, (void *const *)labels_out, (void *const *)seeds_out, results, scratch, scratch_bytes, stream, &f));
    const pr_layout L = pr_make_layout(f.mx);
    char *base = reinterpret_cast<char *>(scratch);
    char *feat0 = base + L.enc * npairs, *conf0 = feat0 + L.feat * npairs, *solve0 = conf0 + L.conf * npairs;
    float *fo[LR_MAX_BATCH], *co[LR_MAX_BATCH];
    for (int k = 0; k < npairs; ++k) {
        fo[k] = feat_out && feat_out[k] ? feat_out[k] : reinterpret_cast<float *>(feat0 + L.feat * k);
        co[k] = conf_out && conf_out[k] ? conf_out[k] : reinterpret_cast<float *>(conf0 + L.conf * k);
    }
    // the encoder's result blocks are not the caller's: they land in the head of the solver's arenas, in the records ps_prep_kernel then overwrites
    static_assert(sizeof(lr_pdsc_result) * LR_MAX_BATCH <= 256 * 8, "the encoder's result blocks fit the first solver arena's records");
    LR_TRY_HIP(lr_pdsc_encode_batch(npairs, src, tgt, m, m_dev, weights, weights_bytes, ep, reinterpret_cast<lr_pdsc_result *>(solve0 + ps_make_layout(f.mx).rec),
                                    fo, co, base, L.enc * npairs, stream));
    ps_ext_table ext;
    LR_TRY_HIP(ps_fill_ext(who, npairs, m, fo, co, &ext));
    const ps_trace none = { nullptr, nullptr, nullptr, nullptr };
    return ps_launch(f, ext, none, npairs, sp, results, solve0, L.solve, stream);
}

extern "C" int lr_pdsc_register_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                      const float *weights, size_t weights_bytes, const lr_pdsc_params *ep, const lr_pdsc_solve_params *sp,
                                      lr_pdsc_solve_result *results, float *const *feat_out, float *const *conf_out, uint8_t *const *labels_out,
                                      int32_t *const *seeds_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return pr_run("lr_pdsc_register_batch", npairs, src, tgt, m, m_dev, weights, weights_bytes, ep, sp, results, feat_out, conf_out, labels_out,
                  seeds_out, scratch, scratch_bytes, stream);
}

extern "C" int lr_pdsc_register(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, size_t weights_bytes,
                                const lr_pdsc_params *ep, const lr_pdsc_solve_params *sp, lr_pdsc_solve_result *result, float *feat_out,
                                float *conf_out, uint8_t *labels_out, int32_t *seeds_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return pr_run("lr_pdsc_register", 1, &src, &tgt, &m, &m_dev, weights, weights_bytes, ep, sp, result, &feat_out, &conf_out, &labels_out,
                  &seeds_out, scratch, scratch_bytes, stream);
}
