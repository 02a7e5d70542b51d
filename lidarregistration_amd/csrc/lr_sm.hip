// Spectral matching (Leordeanu & Hebert) on gfx950 -- the reference survey's SM() baseline
// (Experiments/baseline_scripts/baseline_3DMatch.py:19-53, run by baseline_KITTI.py:51-52 with inlier_threshold 0.6 and top_ratio
// 0.05; the weighted fit is models/common.py:7-45).  The contract is stated in include/lidarreg.h and DESIGN.md §11 and restated in
// numpy in tests/sm_cpu.py.
//
// The reference materialises the M x M compatibility matrix (M x M x 6 floats of differences first); here it is never stored: every
// power iteration re-evaluates c(i,j) on the fly, 10 M^2 evaluations of a short fp32 chain.
//
// Kernels (each launched ONCE for a batch, the pair is grid z or the block index; a single-pair call is a batch of one):
//   sm_setup_kernel    descriptors by value -> control blocks: live M, K, the work plan of the matvec
//   sm_pack_kernel     32-byte records { a.xyz, b.xyz, v, 0 }, v = 1; a correspondence with a non-finite coordinate becomes six NaNs
//                      (fmaxf(0, NaN) = 0: compatibility 0 with everything); the list is padded to a multiple of 4 with such records
//   sm_matvec_kernel   the hot path: work item = 64 rows (one per lane, the row's six coordinates in registers) x one chunk of columns;
//                      the column records are wave-uniform and arrive by scalar loads, four per wait, ping-pong as in the scoring loop
//                      of lr_score.hip; partial sums go to part[chunk][row] by plain stores
//   sm_norm_kernel     one block per pair: row sums over the chunks (ascending, fp64), the norm by a fixed-order tree, v back into the
//                      records
//   sm_select_kernel   one block per pair: the K-th largest v by four radix passes over the float bits (v >= 0: integer order is float
//                      order), ties at the cut by ascending index; labels and the ascending index list (in-block ranks: lr_block_rank
//                      of lr_prims.h, the header of the integer steps the cloud-level kernels share)
//   sm_fit_kernel      one block per pair: weighted fp64 centroids and covariance in a fixed order, Horn's solver of lr_contract.h
// No floating-point atomics anywhere: every sum has one order, which depends on the pair's own M (and the device's compute-unit count)
// only -- never on the batch the pair is in, on scheduling or on what the scratch held.
#include "lr_corrset.h"
#include "lr_prims.h"
#include "lr_contract.h"
#include <math.h>

#define SM_MAX_CHUNKS 64
#define SM_MAX_TARGET 4096           // upper bound of the matvec's work items per pair (it sizes part[][] without knowing the device)
#define SM_MAX_ITERS 1000

typedef float sm_f32x8 __attribute__((ext_vector_type(8)));

// per-pair control block at the head of the pair's scratch arena
struct sm_ctl {
    const float *a, *b;
    float *eig_out;
    uint8_t *labels_out;
    int32_t m_host, m;               // what the caller passed as m; the live count (m_dev clamped to 0..m_host)
    int32_t K;
    int32_t rb, chunks, per;         // matvec plan: row blocks of 64, column chunks, columns per chunk (a multiple of 4)
    int32_t nsel, pad;
};

// Work plan of one pair's matvec: rb * chunks work items of 64 rows x `per` columns, about `target` of them.  A function of the
// pair's live M and the device constant `target` alone (the sums' order follows from it).
struct sm_plan { int rb, chunks, per; };
__host__ __device__ static inline sm_plan sm_make_plan(int m, int target)
{
    sm_plan p;
    p.rb = m > 0 ? (m + 63) >> 6 : 1;
    int ch = target / p.rb;
    if (ch > p.rb) ch = p.rb;        // at least 64 columns per chunk
    if (ch > SM_MAX_CHUNKS) ch = SM_MAX_CHUNKS;
    if (ch < 1) ch = 1;
    const int m4 = m > 0 ? (m + 3) & ~3 : 4;
    p.per = (((m4 + ch - 1) / ch) + 3) & ~3;
    p.chunks = (m4 + p.per - 1) / p.per;
    return p;
}

struct sm_layout { size_t ctl, rec, part, rowsum, sel, total; };
static sm_layout sm_make_layout(int max_m)
{
    const size_t Mp = ((size_t)(max_m < 1 ? 1 : max_m) + 63) & ~size_t(63);
    // part[chunk][row] of a live M uses chunks * rb * 64 floats with its OWN row stride rb * 64, and sm_make_plan keeps
    // chunks <= min(target / rb, rb, 64): at most min(SM_MAX_TARGET, rb^2, 64 rb) * 64 floats (or one row of rb * 64 when target < rb),
    // which grows with rb -- so the bound at the largest M covers every smaller live count
    const size_t rb = Mp / 64;
    size_t items = SM_MAX_TARGET;
    if (items > rb * rb) items = rb * rb;
    if (items > SM_MAX_CHUNKS * rb) items = SM_MAX_CHUNKS * rb;
    if (items < rb) items = rb;
    sm_layout L;
    size_t o = 0;
    L.ctl = o;    o += lr_al(sizeof(sm_ctl));
    L.rec = o;    o += lr_al(Mp * 32);
    L.part = o;   o += lr_al(items * 64 * 4);
    L.rowsum = o; o += lr_al(Mp * 8);
    L.sel = o;    o += lr_al(Mp * 4);
    L.total = o;
    return L;
}

struct sm_args {
    char *base;                      // scratch arena of pair 0
    size_t stride;                   // bytes between consecutive pairs' arenas
    int target;                      // work items per pair the matvec plans for (from the compute-unit count)
    sm_layout L;
};

// ---- setup: descriptors by value -> control blocks (no host copy, graph-capturable) ------------------------------------------
__global__ void sm_setup_kernel(cs_desc_table t, sm_args g, int npairs, double top_ratio)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const cs_desc d = t.d[k];
    sm_ctl *c = lr_ptr<sm_ctl>(g, k, g.L.ctl);
    const int m = cs_live_m(d);
    const sm_plan p = sm_make_plan(m, g.target);
    c->a = d.a; c->b = d.b; c->eig_out = (float *)d.out0; c->labels_out = (uint8_t *)d.out1;
    c->m_host = d.m; c->m = m;
    c->K = (int)((double)m * top_ratio);             // Python's int(M * top_ratio): the product in double, truncated
    c->rb = p.rb; c->chunks = p.chunks; c->per = p.per;
    c->nsel = 0; c->pad = 0;
}

// ---- records -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sm_pack_kernel(sm_args g)
{
    const int pair = blockIdx.z;
    const sm_ctl *c = lr_ptr<sm_ctl>(g, pair, g.L.ctl);
    const int m = c->m, m4 = (m + 3) & ~3, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m4) return;
    float *rec = lr_ptr<float>(g, pair, g.L.rec) + (size_t)i * 8;
    float r[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    bool ok = i < m;
    if (ok) {
        const float *a = c->a + (size_t)3 * i, *b = c->b + (size_t)3 * i;
        r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = b[0]; r[4] = b[1]; r[5] = b[2];
        for (int k = 0; k < 6; ++k) ok = ok && fabsf(r[k]) <= 3.4028234e38f;      // (false for NaN and inf)
    }
    const float bad = __builtin_nanf("");
    for (int k = 0; k < 6; ++k) rec[k] = ok ? r[k] : bad;
    rec[6] = i < m ? 1.0f : 0.0f;                    // v0 = 1; padding records carry v = 0
    rec[7] = 0.0f;
}

// ---- the hot path ----------------------------------------------------------------------------------------------------------------
// c(i,j) v_j added to acc.  fp32 on direct differences, (dx dx + dy dy) + dz dz, two correctly rounded square roots, then
// subtract, multiply, fma, max, fma (-ffp-contract=off: nothing else is fused).  nk = -1 / (2 sigma^2).
template <bool DIAG>
__device__ __forceinline__ float sm_elem(const float (&p)[6], const sm_f32x8 r, float nk, float acc, int i, int j)
{
    const float d = cs_len_diff(p, r[0], r[1], r[2], r[3], r[4], r[5]);
    float cij = fmaxf(0.0f, fmaf(d * d, nk, 4.5f));
    if (DIAG) cij = (i == j) ? 0.0f : cij;           // the diagonal is decided by index: a duplicated correspondence keeps its 4.5
    return fmaf(cij, r[6], acc);
}

// one lane's row over the records [begin, end) (both multiples of 4), ascending.  Scalar loads return out of order, so every wait for
// one drains all of them: four records per wait, the next four requested before the arithmetic of these four, ping-pong between two
// register sets (no copies); the last request of a stream re-reads its own records: nothing is read past the end.
template <bool DIAG>
__device__ __forceinline__ float sm_stream(const sm_f32x8 *__restrict__ rec, int begin, int end, const float (&p)[6], float nk, float acc, int i)
{
    if (begin >= end) return acc;
    sm_f32x8 c0[4], c1[4];
    auto load4 = [&](int at, sm_f32x8 (&r)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = rec[at + k];
        __builtin_amdgcn_sched_barrier(0);           // (the loads stay ahead of the arithmetic that follows)
    };
    auto four = [&](const sm_f32x8 (&r)[4], int j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = sm_elem<DIAG>(p, r[k], nk, acc, i, j + k);
    };
    int j = begin;
    load4(j, c0);
    for (;;) {
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): the records in hand, BEFORE the next request is issued
        load4(j + 8 <= end ? j + 4 : j, c1);
        four(c0, j);
        j += 4;
        if (j >= end) break;
        __builtin_amdgcn_s_waitcnt(0xC07F);
        load4(j + 8 <= end ? j + 4 : j, c0);
        four(c1, j);
        j += 4;
        if (j >= end) break;
    }
    return acc;
}

__global__ void __launch_bounds__(256)
sm_matvec_kernel(const float *__restrict__ rec_, float *__restrict__ part_, const sm_ctl *__restrict__ ctl_, size_t stride, float nk)
{
    // (the arena offset is pointer arithmetic on the __restrict__ parameters: the compiler then knows that the record stream is global
    // memory, uniform and not clobbered by the kernel's own stores -- what keeps it on scalar loads)
    const int pair = blockIdx.z;
    const sm_ctl *__restrict__ c = reinterpret_cast<const sm_ctl *>(reinterpret_cast<const char *>(ctl_) + (size_t)pair * stride);
    const sm_f32x8 *__restrict__ rec = reinterpret_cast<const sm_f32x8 *>(reinterpret_cast<const char *>(rec_) + (size_t)pair * stride);
    float *__restrict__ part = reinterpret_cast<float *>(reinterpret_cast<char *>(part_) + (size_t)pair * stride);
    const int m = c->m;
    if (m <= 0) return;
    const int rb = c->rb, chunks = c->chunks, per = c->per, m4 = (m + 3) & ~3;
    const int lane = threadIdx.x & 63;
    // a block is four independent waves; wave w of the pair's blocks takes the work items w, w + W, ...  (the wave index is
    // wave-uniform, which the compiler cannot see through threadIdx: without the readfirstlane the record loads become per-lane loads)
    const int W = (int)gridDim.x * 4, w0 = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    for (int w = w0; w < rb * chunks; w += W) {
        const int r = w % rb, ch = w / rb;
        const int i0 = r * 64, i = i0 + lane, ii = i < m ? i : m - 1;
        const sm_f32x8 own = rec[ii];
        const float p[6] = { own[0], own[1], own[2], own[3], own[4], own[5] };
        const int j0 = ch * per, j1 = min(m4, j0 + per);
        const int lo = max(j0, min(j1, i0)), hi = max(j0, min(j1, i0 + 64));      // the columns that can meet the diagonal: [lo, hi)
        float acc = 0.0f;
        acc = sm_stream<false>(rec, j0, lo, p, nk, acc, i);
        acc = sm_stream<true>(rec, lo, hi, p, nk, acc, i);
        acc = sm_stream<false>(rec, hi, j1, p, nk, acc, i);
        if (i < m) part[(size_t)ch * (rb * 64) + i] = acc;      // row stride of THIS live M: rb * 64
    }
}

// ---- normalisation ----------------------------------------------------------------------------------------------------------------
#define SM_NB 1024
__global__ void __launch_bounds__(SM_NB) sm_norm_kernel(sm_args g, int last)
{
    __shared__ double s_red[SM_NB];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const sm_ctl *c = lr_ptr<sm_ctl>(g, pair, g.L.ctl);
    const int m = c->m, chunks = c->chunks, Mp = c->rb * 64;
    if (m <= 0) return;
    const float *part = lr_ptr<float>(g, pair, g.L.part);
    double *rowsum = lr_ptr<double>(g, pair, g.L.rowsum);
    float *rec = lr_ptr<float>(g, pair, g.L.rec);
    double q = 0.0;
    for (int i = tid; i < m; i += SM_NB) {
        double s = 0.0;
        for (int ch = 0; ch < chunks; ++ch) s += (double)part[(size_t)ch * Mp + i];
        rowsum[i] = s;
        q += s * s;
    }
    const double den = sqrt(lr_block_tree_sum<SM_NB>(q, s_red)) + 1e-6;
    float *eig = last ? c->eig_out : nullptr;
    for (int i = tid; i < m; i += SM_NB) {
        const float v = (float)(rowsum[i] / den);
        rec[(size_t)i * 8 + 6] = v;
        if (eig) eig[i] = v;
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SM_NB) sm_select_kernel(sm_args g)
{
    __shared__ int s_hist[256];
    __shared__ int s_cnt[SM_NB / 64];
    __shared__ unsigned s_pick[2];
    const int pair = blockIdx.x, tid = threadIdx.x;
    sm_ctl *c = lr_ptr<sm_ctl>(g, pair, g.L.ctl);
    const int m = c->m, mh = c->m_host, K = c->K;
    const uint32_t *rec = lr_ptr<uint32_t>(g, pair, g.L.rec);
    int32_t *sel = lr_ptr<int32_t>(g, pair, g.L.sel);
    uint8_t *labels = c->labels_out;
    float *eig = c->eig_out;
    // the K-th largest value: its bits (v >= 0), most significant byte first
    uint32_t prefix = 0, mask = 0;
    int need = K;
    if (K > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < m; i += SM_NB) {
                const uint32_t bits = rec[(size_t)i * 8 + 6];
                if ((bits & mask) == prefix) atomicAdd(&s_hist[(bits >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int b = 255, left = need;
                for (; b > 0; --b) { const int h = s_hist[b]; if (left <= h) break; left -= h; }
                s_pick[0] = (unsigned)b; s_pick[1] = (unsigned)left;
            }
            __syncthreads();
            prefix |= s_pick[0] << shift; mask |= 255u << shift;
            need = (int)s_pick[1];
            __syncthreads();
        }
    }
    // `need` of the entries equal to the cut value are taken, by ascending index; everything above it is
    int n_eq = 0, n_sel = 0;
    for (int base = 0; base < mh; base += SM_NB) {
        const int i = base + tid;
        const bool live = i < m && K > 0;
        const uint32_t bits = live ? rec[(size_t)i * 8 + 6] : 0u;
        const bool eq = live && bits == prefix, gt = live && bits > prefix;
        int tot_eq, tot_sel;
        const int rank = n_eq + lr_block_rank<SM_NB>(eq, s_cnt, tot_eq);
        const bool take = gt || (eq && rank < need);
        const int pos = n_sel + lr_block_rank<SM_NB>(take, s_cnt, tot_sel);
        if (take) sel[pos] = i;
        if (i < mh) {
            if (labels) labels[i] = take ? 1 : 0;
            if (eig && i >= m) eig[i] = 0.0f;        // (past the live count: nothing was computed)
        }
        n_eq += tot_eq; n_sel += tot_sel;
    }
    if (tid == 0) c->nsel = n_sel;
}

// ---- weighted fit -----------------------------------------------------------------------------------------------------------------
#define SM_FB 256
__global__ void __launch_bounds__(SM_FB) sm_fit_kernel(sm_args g, lr_sm_result *results)
{
    __shared__ double s_red[SM_FB];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const sm_ctl *c = lr_ptr<sm_ctl>(g, pair, g.L.ctl);
    const int K = c->K, n = c->nsel;
    const float *rec = lr_ptr<float>(g, pair, g.L.rec);
    const int32_t *sel = lr_ptr<int32_t>(g, pair, g.L.sel);
    const float *a = c->a, *b = c->b;
    lr_sm_result *res = results + pair;
    // weights w = v of the selected entries; an entry of weight 0 adds nothing and is not read (its coordinates may be non-finite)
    double v[9];
    double sw = 0.0;
    for (int k = tid; k < n; k += SM_FB) sw += (double)rec[(size_t)sel[k] * 8 + 6];
    sw = lr_block_tree_sum(sw, s_red, blockDim.x);
    const int status = (K < 3 || !(sw > 0.0)) ? 1 : 0;
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!status) {
        const double den = sw + 1e-6;                // models/common.py:24-25
        double cen[6];
        for (int x = 0; x < 6; ++x) v[x] = 0.0;
        for (int k = tid; k < n; k += SM_FB) {
            const int i = sel[k];
            const double w = (double)rec[(size_t)i * 8 + 6];
            if (w > 0.0) {
                for (int x = 0; x < 3; ++x) { v[x] += w * (double)a[(size_t)3 * i + x]; v[3 + x] += w * (double)b[(size_t)3 * i + x]; }
            }
        }
        for (int x = 0; x < 6; ++x) cen[x] = lr_block_tree_sum(v[x], s_red, blockDim.x) / den;
        for (int x = 0; x < 9; ++x) v[x] = 0.0;
        for (int k = tid; k < n; k += SM_FB) {
            const int i = sel[k];
            const double w = (double)rec[(size_t)i * 8 + 6];
            if (w > 0.0) {
                double da[3], db[3];
                for (int x = 0; x < 3; ++x) { da[x] = (double)a[(size_t)3 * i + x] - cen[x]; db[x] = (double)b[(size_t)3 * i + x] - cen[3 + x]; }
                for (int x = 0; x < 3; ++x)
                    for (int y = 0; y < 3; ++y) v[3 * x + y] += (w * da[x]) * db[y];
            }
        }
        double H[3][3];
        for (int x = 0; x < 9; ++x) H[x / 3][x % 3] = lr_block_tree_sum(v[x], s_red, blockDim.x);
        if (tid == 0) lr_rt_from_cov(H, cen, cen + 3, T);
    }
    if (tid == 0) {
        for (int i = 0; i < 16; ++i) res->T[i] = T[i];
        res->status = status; res->K = K; res->m = c->m; res->reserved = 0;
        res->weight_sum = sw;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_sm_params) == 24 && sizeof(lr_sm_result) == 152, "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_sm_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > CS_MAX_M) return 0;
    return sm_make_layout(max_m).total;
}

static int check_sm_params(const lr_sm_params *p, const char *who)
{
    LR_CHECK_STRUCT_SIZE(lr_sm_params, p, who);
    if (p->iterations < 1 || p->iterations > SM_MAX_ITERS) { lr_set_error("%s: iterations must lie in 1..%d", who, SM_MAX_ITERS); return LR_EINVAL; }
    if (!(p->inlier_threshold > 0.0 && isfinite(p->inlier_threshold))) { lr_set_error("%s: inlier_threshold must be positive and finite", who); return LR_EINVAL; }
    if (!(p->top_ratio > 0.0 && p->top_ratio <= 1.0)) { lr_set_error("%s: top_ratio must lie in (0, 1]", who); return LR_EINVAL; }
    return LR_OK;
}

// `who`: the entry point the params messages name; the checks of the shared front have always reported as lr_sm_batch
static int sm_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                  const lr_sm_params *p, lr_sm_result *results, float *const *eig_out, uint8_t *const *labels_out,
                  void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_sm_batch", "npairs * lr_sm_scratch_bytes(max m)", lr_sm_scratch_bytes, LR_EINVAL };
    LR_TRY_HIP(check_sm_params(p, who));
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, (void *const *)eig_out, (void *const *)labels_out, results, scratch, scratch_bytes, stream, &f));
    const int mx = f.mx;

    sm_args g;
    g.base = reinterpret_cast<char *>(scratch);
    g.stride = f.per;
    g.L = sm_make_layout(mx);
    g.target = 8 * f.n_cus;                          // two waves per SIMD
    if (g.target > SM_MAX_TARGET) g.target = SM_MAX_TARGET;
    if (g.target < 64) g.target = 64;
    const double sigma = p->inlier_threshold / 3.0;
    const float nk = (float)(-1.0 / (2.0 * sigma * sigma));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sm_setup_kernel, dim3(1), dim3(64), 0, st, f.t, g, npairs, p->top_ratio);
    if (mx > 0) {
        const sm_plan plan = sm_make_plan(mx, g.target);
        int items = plan.rb * plan.chunks;           // (a smaller live M plans at most max(target, its row blocks) items; the waves stride over them)
        if (items < g.target && mx >= 64) items = g.target;
        hipLaunchKernelGGL(sm_pack_kernel, dim3(lr_cdiv(mx + 3, 256), 1, npairs), dim3(256), 0, st, g);
        for (int it = 0; it < p->iterations; ++it) {
            hipLaunchKernelGGL(sm_matvec_kernel, dim3(lr_cdiv(items, 4), 1, npairs), dim3(256), 0, st,
                               (const float *)(g.base + g.L.rec), (float *)(g.base + g.L.part), (const sm_ctl *)(g.base + g.L.ctl), g.stride, nk);
            hipLaunchKernelGGL(sm_norm_kernel, dim3(npairs), dim3(SM_NB), 0, st, g, it + 1 == p->iterations ? 1 : 0);
        }
    }
    hipLaunchKernelGGL(sm_select_kernel, dim3(npairs), dim3(SM_NB), 0, st, g);
    hipLaunchKernelGGL(sm_fit_kernel, dim3(npairs), dim3(SM_FB), 0, st, g, results);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_sm_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                           const lr_sm_params *p, lr_sm_result *results, float *const *eig_out, uint8_t *const *labels_out,
                           void *scratch, size_t scratch_bytes, void *stream)
{
    return sm_run("lr_sm_batch", npairs, src, tgt, m, m_dev, p, results, eig_out, labels_out, scratch, scratch_bytes, stream);
}

extern "C" int lr_sm(const float *src, const float *tgt, int m, const int32_t *m_dev, const lr_sm_params *p, lr_sm_result *result,
                     float *eig_out, uint8_t *labels_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return sm_run("lr_sm", 1, &src, &tgt, &m, &m_dev, p, result, &eig_out, &labels_out, scratch, scratch_bytes, stream);
}
