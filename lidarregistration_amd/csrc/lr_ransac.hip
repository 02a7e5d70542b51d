// RANSAC on gfx950: hypothesis generation, the merge of a batch into the running best model, and the call that strings the stages together.
//
// Replaces the third-party loops behind Experiments/algorithms/FR.py:122-139 (Open3D
// registration_ransac_based_on_correspondence) and GC_RANSAC.py:46-49 (pygcransac.findRigidTransform,
// native driver GC-RANSAC/src/pygcransac/src/gcransac_python.cpp:404-624 with the authors' edge-length
// pre-check preemption_edge_length.h:71-128), plus the LS refit FR.py:99-111.
//
// Structure (all counts stay on device, no host round trip):
//   gen     one thread per hypothesis id h: Philox sample -> ELC (fp64) -> minimal-sample Kabsch (fp64, Horn
//           quaternion + Jacobi) -> fp32 model appended to a dense list                                      (this file)
//   score   one LANE per surviving hypothesis over a wave-uniform correspondence stream                      (lr_score.hip)
//   select  more inliers, then lower error, then lower hypothesis id (ties on the count are the norm when
//           the inlier noise is far below the threshold, so the error is accumulated for everyone)           (this file)
//   lo      local optimisation of a new best model, final iterated least squares                             (lr_lo.hip)
//   refit   fp64 moments of the inliers over the ORIGINAL NN pairs -> Kabsch                                 (lr_refit.hip)
// What more than one of them compiles is lr_ransac_dev.h.
#include "lr_ransac_dev.h"
#include <type_traits>

// unweighted Kabsch on NS (3 or 4) sample points held in registers
template <int NS>
__device__ __forceinline__ void kabsch_sample(const double P[NS][3], const double Q[NS][3], double T[16])
{
    double cp[3] = { 0, 0, 0 }, cq[3] = { 0, 0, 0 }, W = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        W = W + 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { cp[a] = cp[a] + 1.0 * P[i][a]; cq[a] = cq[a] + 1.0 * Q[i][a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { cp[a] = cp[a] / W; cq[a] = cq[a] / W; }
    double H[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double pc[3], qc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { pc[a] = P[i][a] - cp[a]; qc[a] = Q[i][a] - cq[a]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) H[a][b] = H[a][b] + (1.0 * pc[a]) * qc[b];
    }
    lr_rt_from_cov(H, cp, cq, T);
}

// PROSAC growth function (Chum & Matas 2005, as tabulated by USAC / GC-RANSAC's prosac_sampler.h):
//   T_n = T_N prod_{i<ns} (n-i)/(M-i),  G[ns] = 1,  G[n+1] = G[n] + ceil(T_{n+1} - T_n)
// Draw k uses the first n_k = min(M, ns + #{n in [ns, M) : G[n] <= k}) correspondences.  T_n is evaluated in closed
// form (same operation order as oracle/oracle.c) so that the table is a parallel prefix sum: one block.
__device__ __forceinline__ double prosac_Tn(int n, int M, int ns, double TN)
{
    double t = TN;
    for (int i = 0; i < ns; ++i) t = t * (double)(n - i) / (double)(M - i);
    return t;
}

__global__ void __launch_bounds__(1024)
prosac_growth_kernel(int m_max, const int32_t *__restrict__ m_dev, int ns, int TN, int32_t *__restrict__ G, lr_zargs z)
{
    lr_z(m_dev, z, blockIdx.z); lr_z(G, z, blockIdx.z);
    __shared__ long long s_w[16];
    __shared__ long long s_carry;
    const int M = m_dev ? min(*m_dev, m_max) : m_max;
    if (threadIdx.x == 0) s_carry = 1;       // G[ns] = 1
    __syncthreads();
    // elements n = ns .. M-1 carry d_n = ceil(T_{n+1} - T_n) >= 1; G[n] = 1 + sum_{j<n} d_j, written for n = ns .. M.
    // Four consecutive elements per thread (five evaluations of T instead of eight, a quarter of the block-wide scans: the kernel is one
    // block per pair and sits in a single pair's critical path -- 30 us with one element per thread)
    constexpr int E = 4;
    for (int base = ns; base < M; base += E * 1024) {
        const int n0 = base + E * (int)threadIdx.x;
        long long d[E], tot = 0;
        double t_prev = n0 < M ? prosac_Tn(n0, M, ns, (double)TN) : 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            d[e] = 0;
            if (n0 + e < M) {
                const double t_next = prosac_Tn(n0 + e + 1, M, ns, (double)TN);
                d[e] = (long long)ceil(t_next - t_prev);
                if (d[e] < 1) d[e] = 1;
                t_prev = t_next;
            }
            tot += d[e];
        }
        long long inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(inc, o); if ((int)(threadIdx.x & 63) >= o) inc += v; }
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        long long pre = s_carry;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += s_w[w];
        long long g = pre + inc - tot;                            // G[n0]
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (n0 + e < M) {
                G[n0 + e] = (int32_t)(g < 0x3fffffffLL ? g : 0x3fffffffLL);
                g += d[e];
                if (n0 + e == M - 1) G[M] = (int32_t)(g < 0x3fffffffLL ? g : 0x3fffffffLL);
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = pre + inc;
        __syncthreads();
    }
}

// sample of hypothesis h and its edge-length pre-check; false when the pre-check rejects it
template <int NS>
__device__ __forceinline__ bool hypothesis_sample(const float *__restrict__ corr8, int m, uint64_t seed, uint64_t h,
                                                  int use_elc, double P[NS][3], double Q[NS][3],
                                                  const int32_t *__restrict__ G, int TN, int unique = 0)
{
    uint32_t c[4] = { (uint32_t)h, (uint32_t)(h >> 32), 0u, 0u };
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    // PROSAC: draw k = h + 1 takes NS-1 indices from the first n-1 correspondences and the n-th one
    int n_top = 0;
    if (G && h < (uint64_t)TN && m > NS) {
        const int k = (int)h + 1;
        int lo = NS, hi = m;                       // first n in [NS, m) with G[n] > k
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (G[mid] <= k) lo = mid + 1; else hi = mid; }
        n_top = min(m, lo);                        // = NS + #{n : G[n] <= k}
    }
    uint32_t sidx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        uint32_t s = __umulhi(c[k], (uint32_t)m);
        if (n_top) s = k < NS - 1 ? __umulhi(c[k], (uint32_t)(n_top - 1)) : (uint32_t)(n_top - 1);
        sidx[k] = s;
        // the correspondence's six floats sit at every second place of the first 48 bytes of its pair's record (lr_corr_at): three 16-byte
        // gathers and a selection by parity instead of six 4-byte gathers -- a gather costs the memory pipe a cache line per lane whatever
        // its width, and the gathers are what this kernel waits for
        const f32x4 *rec = reinterpret_cast<const f32x4 *>(corr8 + (size_t)(s >> 1) * 16);
        const f32x4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        const bool odd = (s & 1u) != 0u;
        P[k][0] = (double)(odd ? r0.y : r0.x); P[k][1] = (double)(odd ? r0.w : r0.z); P[k][2] = (double)(odd ? r1.y : r1.x);
        Q[k][0] = (double)(odd ? r1.w : r1.z); Q[k][1] = (double)(odd ? r2.y : r2.x); Q[k][2] = (double)(odd ? r2.w : r2.z);
    }
    bool ok = true;
    if (unique) {       // GC-RANSAC's samplers draw distinct indices: a repeated index rejects the draw
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = i + 1; j < NS; ++j) if (sidx[i] == sidx[j]) ok = false;
    }
    if (!use_elc) return ok;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = i + 1; j < NS; ++j) {
            double sx = P[j][0] - P[i][0], sy = P[j][1] - P[i][1], sz = P[j][2] - P[i][2];
            double tx = Q[j][0] - Q[i][0], ty = Q[j][1] - Q[i][1], tz = Q[j][2] - Q[i][2];
            // the contract compares the LENGTHS (oracle.c: ds < dt * 0.9 || dt < ds * 0.9, sqrt and products rounded in fp64).  The
            // roundings move either side by < 4 ulp, so away from equality the squares decide the same way, and the six fp64 square
            // roots per draw -- a third of this kernel -- are only taken inside a relative band of 1e-13 around it (or when a square is
            // zero or not finite: every comparison below is then false)
            const double a2 = (sx * sx + sy * sy) + sz * sz, b2 = (tx * tx + ty * ty) + tz * tz;
            const double band = 1e-13 * (a2 + b2);
            if (fabs(a2 - 0.81 * b2) > band && fabs(b2 - 0.81 * a2) > band) {
                if (a2 < 0.81 * b2 || b2 < 0.81 * a2) ok = false;
            } else {
                const double ds = sqrt(a2), dt = sqrt(b2);
                if (ds < dt * 0.9 || dt < ds * 0.9) ok = false;
            }
        }
    return ok;
}

// ------------------------------------------------------------------ gen
// 256 hypothesis ids per block.  Phase 1: every thread draws its sample and runs the pre-check (cheap, ~93 % fail on
// 3-point samples at a 40 % inlier ratio).  Phase 2: the survivors are compacted through LDS so that the expensive fp64
// Kabsch runs on densely packed lanes of one wave instead of a few stragglers in every wave.
template <int NS>
__global__ void __launch_bounds__(256)
ransac_gen_kernel(const float *__restrict__ corr8, int m_max, const int32_t *__restrict__ m_dev, lr_ransac_params p,
                  int h_begin, int h_end, int32_t *__restrict__ model_h,
                  uint32_t *__restrict__ score_cnt, unsigned long long *__restrict__ score_ssq,
                  int32_t *__restrict__ counters, const int32_t *__restrict__ G, int TN,
                  lr_score_info *__restrict__ info, lr_zargs z)
{
    // ids that passed the pre-check -> dense list model_h[0 .. NVALID) (appended by whole groups: one device atomic per block and
    // FIT_AT ids); ransac_fit_kernel estimates their models.  The fit (fp64 Kabsch, a dependent chain of ~14 us for a wave) used to
    // run here, on the 18 of 256 ids of a group that pass the edge-length check: a quarter of ONE wave per block for the full length
    // of the fit, 1.25 such waves per SIMD -- 61 of the kernel's 111 us per 32-pair launch were that wait.
    constexpr int FIT_AT = 192;
    __shared__ int s_pass[FIT_AT + 256];
    __shared__ int s_np, s_base;
    lr_z(info, z, blockIdx.z);
    if (blockIdx.x == 0) lr_score_info_reset(info);       // the scoring passes of this batch elect their pilot model afresh
    lr_z(corr8, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(model_h, z, blockIdx.z); lr_z(score_cnt, z, blockIdx.z); lr_z(score_ssq, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(G, z, blockIdx.z);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    if (m <= 0 || reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT)->done) return;
    if (threadIdx.x == 0) s_np = 0;
    __syncthreads();
    // (a capped grid strides over the 256-id groups: the launches of the batches behind an early exit then cost a few hundred
    // idle blocks instead of tens of thousands)
    for (int blk = blockIdx.x; blk * 256 < h_end - h_begin; blk += gridDim.x) {
        const int h = h_begin + blk * 256 + threadIdx.x;
        {
            double P[NS][3], Q[NS][3];
            if (h < h_end && hypothesis_sample<NS>(corr8, m, p.seed, (uint64_t)h, p.use_elc == 1, P, Q, G, TN, p.sampler != 0)) s_pass[atomicAdd(&s_np, 1)] = h;
        }
        __syncthreads();
        const int np = s_np;
        const bool last = (blk + (int)gridDim.x) * 256 >= h_end - h_begin;
        if (threadIdx.x == 0 && np > 0 && (np >= FIT_AT || last)) s_base = atomicAdd(&counters[LR_CNT_NVALID], np);
        __syncthreads();                             // (every thread has read np before the next group's ids are appended)
        if (np < FIT_AT && !last) continue;          // (block-uniform: np and last are the same for every thread)
        for (int e = threadIdx.x; e < np; e += 256) {
            const int slot = s_base + e;
            model_h[slot] = s_pass[e];
            score_cnt[slot] = 0u;
            score_ssq[slot] = 0ull;
        }
        if (!last) {
            __syncthreads();
            if (threadIdx.x == 0) s_np = 0;
            __syncthreads();
        }
    }
}

// the models of the ids ransac_gen_kernel listed: a thread per list slot re-draws its sample (same Philox counter) and fits it
template <int NS>
__global__ void __launch_bounds__(64)
ransac_fit_kernel(const float *__restrict__ corr8, int m_max, const int32_t *__restrict__ m_dev, lr_ransac_params p,
                  float *__restrict__ models, double *__restrict__ models64, const int32_t *__restrict__ model_h,
                  const int32_t *__restrict__ counters, const int32_t *__restrict__ G, int TN, int model_stride, lr_zargs z)
{
    lr_z(corr8, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(models, z, blockIdx.z); lr_z(models64, z, blockIdx.z); lr_z(model_h, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(G, z, blockIdx.z);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    if (m <= 0 || reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT)->done) return;
    const int V = counters[LR_CNT_NVALID];
    // (a capped grid strides over the list: with the pre-check the list is a fraction of the batch, and tens of thousands of blocks
    // that only find that out cost more than the fits)
    for (int slot = blockIdx.x * 64 + threadIdx.x; slot < V; slot += gridDim.x * 64) {
        const int hh = model_h[slot];
        double P[NS][3], Q[NS][3], T[16];
        hypothesis_sample<NS>(corr8, m, p.seed, (uint64_t)hh, 0, P, Q, G, TN);
        kabsch_sample<NS>(P, Q, T);
        // fp32 models component-major ([12][model_stride]: the scoring kernel's 64 lanes read 64 consecutive floats per
        // component), fp64 models row-major (only the winner is ever read back)
#pragma unroll
        for (int k = 0; k < 12; ++k) { models[(size_t)k * model_stride + slot] = (float)T[k]; models64[(size_t)slot * 12 + k] = T[k]; }
    }
}

// ------------------------------------------------------------------ SPRT pre-verification (--fast_rejection SPRT)
// See oracle/oracle.c (sprt_test) for the test and its sources.  One LANE per model, the first LR_SPRT_HORIZON
// correspondences in list order as a wave-uniform stream (scalar loads); a wave leaves as soon as all its models are
// decided.  Survivors are appended to a second dense model list (their order does not matter: the winner is chosen by
// score and hypothesis id); the consistent / verified point counts of the rejected models feed the next batch's design.
__global__ void __launch_bounds__(256)
ransac_sprt_kernel(const float *__restrict__ corr8, int m_max, const int32_t *__restrict__ m_dev, float thr2,
                   const float *__restrict__ models, const double *__restrict__ models64, const int32_t *__restrict__ model_h,
                   float *__restrict__ models2, double *__restrict__ models64_2, int32_t *__restrict__ model_h2,
                   uint32_t *__restrict__ score_cnt, unsigned long long *__restrict__ score_ssq, int32_t *__restrict__ counters,
                   int model_stride, lr_zargs z)
{
    lr_z(corr8, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(models, z, blockIdx.z); lr_z(models64, z, blockIdx.z); lr_z(model_h, z, blockIdx.z);
    lr_z(models2, z, blockIdx.z); lr_z(models64_2, z, blockIdx.z); lr_z(model_h2, z, blockIdx.z); lr_z(score_cnt, z, blockIdx.z);
    lr_z(score_ssq, z, blockIdx.z); lr_z(counters, z, blockIdx.z);
    lr_ransac_state *state = reinterpret_cast<lr_ransac_state *>(counters + LR_CNT_COUNT);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int V = counters[LR_CNT_NVALID];
    if (V <= 0 || m <= 0 || state->done) return;
    const int lane = threadIdx.x & 63;
    const int group = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (group * 64 >= V) return;
    const double eps = state->sprt_eps > 0.0 ? state->sprt_eps : LR_SPRT_EPS0, delta = state->sprt_delta > 0.0 ? state->sprt_delta : LR_SPRT_DELTA0;
    const double A = lr_sprt_threshold(eps, delta), fin = delta / eps, fout = (1.0 - delta) / (1.0 - eps);
    const int slot = group * 64 + lane;
    const bool active = slot < V;
    const size_t ms = (size_t)model_stride;
    const lr_model12 M = lr_load_model(models + (active ? slot : 0), ms);
    const int n = min(m, LR_SPRT_HORIZON);
    double lambda = 1.0;
    int inl = 0, k_rej = 0;
    bool rejected = !active;
    for (int i = 0; i < n; ++i) {
        if (__builtin_amdgcn_ballot_w64(!rejected) == 0ull) break;
        const float d2 = lr_corr_d2(M.Rt, corr8, i);
        if (!rejected) {
            if (d2 < thr2) { inl += 1; lambda = lambda * fin; } else lambda = lambda * fout;
            if (lambda > A) { rejected = true; k_rej = i + 1; }
        }
    }
    const bool keep = active && !rejected;
    // survivors -> the second list
    const unsigned long long kb = __builtin_amdgcn_ballot_w64(keep);
    int base = 0;
    if (lane == 0 && kb) base = atomicAdd(&counters[LR_CNT_NVALID2], (int)__builtin_popcountll(kb));
    base = __shfl(base, 0);
    if (keep) {
        const int dst = base + (int)__builtin_popcountll(kb & ((1ull << lane) - 1ull));
        lr_store_model(models2 + dst, ms, M);
#pragma unroll
        for (int k = 0; k < 12; ++k) models64_2[(size_t)dst * 12 + k] = models64[(size_t)slot * 12 + k];
        model_h2[dst] = model_h[slot];
        score_cnt[dst] = 0u; score_ssq[dst] = 0ull;
    }
    // rejected models: consistent / verified points (integer sums: order independent)
    unsigned long long ri = (active && rejected) ? (unsigned long long)inl : 0ull, rp = (active && rejected) ? (unsigned long long)k_rej : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { ri += __shfl_xor(ri, o); rp += __shfl_xor(rp, o); }
    if (lane == 0 && rp) { atomicAdd(&state->rej_inl, ri); atomicAdd(&state->rej_pts, rp); }
}

// ------------------------------------------------------------------ select
// best = more inliers, then lower fixed-point error, then lower hypothesis id (lr_score_better); its fp64 model was kept by gen

// best of this batch -> merged into the running state; confidence test; outputs rewritten from the state every batch
__global__ void __launch_bounds__(1024)
ransac_final_kernel(const uint32_t *__restrict__ score_cnt, const unsigned long long *__restrict__ score_ssq,
                    const int32_t *__restrict__ model_h, const double *__restrict__ models64,
                    int32_t *__restrict__ counters, int m_max, const int32_t *__restrict__ m_dev, lr_ransac_params p, int h_end,
                    double *__restrict__ T_out, lr_ransac_result *__restrict__ res, int vslot, int32_t *__restrict__ lo_ctl_words, lr_zargs z)
{
    __shared__ unsigned long long s_q[16];
    // the control block of the local optimisation's helper blocks starts from zero at every launch that may use it (before any way out
    // of this kernel: the launch that follows runs whatever happens here)
    if (lo_ctl_words) {
        lr_z(lo_ctl_words, z, blockIdx.z);
        for (int k = threadIdx.x; k < LR_LO_CTL_BYTES / 4; k += 1024) lo_ctl_words[k] = 0;
    }
    lr_z(score_cnt, z, blockIdx.z); lr_z(score_ssq, z, blockIdx.z); lr_z(model_h, z, blockIdx.z); lr_z(models64, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(T_out, z, blockIdx.z); lr_z(res, z, blockIdx.z);
    __shared__ uint32_t s_c[16];
    __shared__ int s_h[16], s_s[16];
    lr_ransac_state *state = reinterpret_cast<lr_ransac_state *>(counters + LR_CNT_COUNT);
    if (state->done) return;
    const uint32_t msac_T = lr_msac_T(p.scoring, p.thr2);
    const int V = counters[vslot];
    uint32_t bc = 0; unsigned long long bq = ~0ull; int bh = 0x7fffffff, bs = -1;
    for (int s = threadIdx.x; s < V; s += 1024) {
        uint32_t c = score_cnt[s];
        if (c == 0) continue;
        unsigned long long q = score_ssq[s];
        int h = model_h[s];
        if (lr_score_better(c, q, h, bc, bq, bh, msac_T)) { bc = c; bq = q; bh = h; bs = s; }
    }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        uint32_t oc = (uint32_t)__shfl_xor((int)bc, mk);
        unsigned long long oq = __shfl_xor(bq, mk);
        int oh = __shfl_xor(bh, mk), os = __shfl_xor(bs, mk);
        if (lr_score_better(oc, oq, oh, bc, bq, bh, msac_T)) { bc = oc; bq = oq; bh = oh; bs = os; }
    }
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = bc; s_q[threadIdx.x >> 6] = bq; s_h[threadIdx.x >> 6] = bh; s_s[threadIdx.x >> 6] = bs; }
    __syncthreads();
    if (threadIdx.x >= 16) return;
    for (int w = 1; w < 16; ++w)
        if (lr_score_better(s_c[w], s_q[w], s_h[w], bc, bq, bh, msac_T)) { bc = s_c[w]; bq = s_q[w]; bh = s_h[w]; bs = s_s[w]; }
    // all 16 lanes hold the batch winner; merge it into the state (lane k moves T[k])
    const int k = threadIdx.x;
    const uint32_t oc = state->cnt; const unsigned long long oq = state->ssq; const int oh = state->h;
    const bool take = bc > 0 && bs >= 0 && (oc == 0 || lr_score_better(bc, bq, bh, oc, oq, oh, msac_T));
    double v = (k % 5 == 0) ? 1.0 : 0.0;
    if (k < 12) {
        if (take) { v = models64[(size_t)bs * 12 + k]; state->T[k] = v; }
        else if (oc > 0) v = state->T[k];
    }
    T_out[k] = v;
    if (k == 0) {
        const uint32_t nc = take ? bc : oc; const unsigned long long nq = take ? bq : oq; const int nh = take ? bh : oh;
        state->cnt = nc; state->ssq = nq; state->h = nh;
        state->n_valid += V; state->n_ids = h_end;
        counters[LR_CNT_NVALID] = 0;                       // the next batch appends from slot 0
        counters[LR_CNT_NVALID2] = 0;
        // with local optimisation a new best model is optimised first (ransac_lo_kernel, next on the stream); the exit test and the
        // re-design of the SPRT run there, on the optimised model
        const bool to_lo = take && p.local_opt == 1 && state->lo_calls < p.lo_max_calls;
        if (to_lo) state->lo_pending = 1;
        if (p.use_elc == 2 && !to_lo) lr_sprt_redesign(state, nc, m_dev ? min(*m_dev, m_max) : m_max);
        if (!to_lo && p.confidence > 0.0f && p.confidence < 1.0f && nc > 0) {
            // exit rule of Open3D's RANSAC / GC-RANSAC at batch granularity: stop once h_end >= log(1-conf)/log(1-(inl/M)^n)
            const int m = m_dev ? min(*m_dev, m_max) : m_max;
            const double f = (double)nc / (double)m;
            double fn = f;
            for (int q = 1; q < p.sample_size; ++q) fn = fn * f;
            const double kk = lr_det_log(1.0 - (double)p.confidence) / lr_det_log(1.0 - fn);
            if ((double)h_end >= kk && h_end >= p.min_iters) state->done = 1;
        }
        lr_ransac_result r;
        r.best_h = nc > 0 ? nh : -1; r.best_count = nc; r.pad0 = (uint32_t)state->lo_timeouts; r.best_ssq = nc > 0 ? nq : 0;
        r.n_valid = state->n_valid; r.n_ids = h_end;
        *res = r;
    }
}

// ------------------------------------------------------------------ the call
// Every refusal and every default, before anything is derived or launched.  *pe: the parameters as the kernels use them, defaults
// resolved and the truncated threshold applied (same rule as oracle.c eff_params).
static int ransac_resolve(const lr_ransac_params *p_in, int max_iters, int max_n0, int m_max, lr_ransac_params *pe)
{
    LR_REQUIRE(p_in->scoring >= 0 && p_in->scoring <= 2, LR_EINVAL, "lr_ransac: scoring must be 0 (count, then error), 1 (MSAC) or 2 (MSAC at GC-RANSAC's truncated threshold)");
    LR_REQUIRE(p_in->lo_rounds >= 0 && p_in->lo_trials >= 0 && p_in->lo_trials <= 20 && p_in->lo_max_calls >= 0 && p_in->min_iters >= 0, LR_EINVAL,
               "lr_ransac: lo_rounds, lo_trials (<= 20), lo_max_calls and min_iters must be >= 0 (0 = default)");
    *pe = *p_in;
    if (pe->scoring == 2) { pe->thr2 = pe->thr2 * 2.25f; pe->scoring = 1; }
    if (pe->lo_rounds <= 0) pe->lo_rounds = LR_LO_ROUNDS;
    if (pe->lo_trials <= 0) pe->lo_trials = LR_LO_TRIALS;
    if (pe->lo_max_calls <= 0) pe->lo_max_calls = pe->use_elc ? 20 : 50;
    if (pe->min_iters <= 0) pe->min_iters = pe->use_elc ? 20 : 50;
    LR_REQUIRE(pe->sample_size == 3 || pe->sample_size == 4, LR_EINVAL, "lr_ransac: sample_size must be 3 or 4");
    LR_REQUIRE(pe->iters >= 0 && pe->iters <= max_iters, LR_ESIZE, "lr_ransac: iters exceeds the workspace");
    LR_REQUIRE(m_max >= 0 && m_max <= max_n0, LR_ESIZE, "lr_ransac: m exceeds the workspace");
    LR_REQUIRE(pe->thr2 > 0.0f && pe->thr2 < 2048.0f, LR_EINVAL, "lr_ransac: thr2 must be in (0, 2048)");
    LR_REQUIRE(pe->use_elc >= 0 && pe->use_elc <= 2, LR_EINVAL, "lr_ransac: use_elc must be 0 (no pre-verification), 1 (edge-length check) or 2 (SPRT)");
    LR_REQUIRE(pe->sampler >= 0 && pe->sampler <= 2, LR_EINVAL, "lr_ransac: sampler must be 0 (uniform), 1 (PROSAC) or 2 (uniform, unique indices)");
    LR_REQUIRE(pe->local_opt >= 0 && pe->local_opt <= 2, LR_EINVAL, "lr_ransac: local_opt must be 0, 1 or 2");
    LR_REQUIRE(pe->prosac_growth >= 0, LR_EINVAL, "lr_ransac: prosac_growth must be >= 0");
    return LR_OK;
}

// batch lengths: the given one, constant; by default 1024, 8192, 65536, ... -- growing eightfold, so that the exit test is fine-grained
// where an easy pair stops (the reference tests after every iteration) while a long run still takes few batches (the launches
// of the batches after the exit cost ~5 us per kernel, ~40 us per batch: measured on the full-list run): 3 batches for 50k ids, 4 for the CLI's default 500k, 5 for 1M; an easy pair scores 1024 ids instead of the 8192 of round 2.
// Without an exit rule there is nothing to test between batches: a single one of all ids.  `prev`: the batch before (0: this is the first).
static long long ransac_batch_len(const lr_ransac_params &p, long long prev)
{
    const bool use_exit = p.confidence > 0.0f && p.confidence < 1.0f;
    if (!use_exit) return p.iters > 0 ? p.iters : 1;
    if (p.batch > 0) return p.batch;
    return prev > 0 ? 8 * prev : 1024;
}

int lr_ransac_run(const lr_call &c, const float *corr8, int m_max, const int32_t *m_dev, const lr_ransac_params *p_in,
                  double *T_out, lr_ransac_result *res)
{
    lr_workspace *ws = c.ws; hipStream_t st = c.st;
    lr_ransac_params p;
    LR_TRY_HIP(ransac_resolve(p_in, ws->max_iters, ws->max_n0, m_max, &p));
    const int TN = p.prosac_growth > 0 ? p.prosac_growth : 100000;
    const int32_t *G = nullptr;
    lr_score_info *info = reinterpret_cast<lr_score_info *>(ws->sc_info);
    // SPRT: every estimated model is pre-verified; the survivors form a second dense list, and that one is scored, merged and counted
    const bool sprt = p.use_elc == 2;
    const int vslot = sprt ? LR_CNT_NVALID2 : LR_CNT_NVALID;
    const float *models = sprt ? ws->models2 : ws->models;
    const double *models64 = sprt ? ws->models64_2 : ws->models64;
    const int32_t *model_h = sprt ? ws->model_h2 : ws->model_h;
    // (ransac_final_kernel zeroes the job slots of the local optimisation's helper blocks when the launch behind it has any)
    int32_t *lo_ctl_words = lr_lo_groups(c, p, m_max) > 1 ? reinterpret_cast<int32_t *>(ws->lo_ctl) : nullptr;
    LR_TRY_HIP(lr_timer_mark(c, LR_EV_RANSAC_BEGIN));
    if (p.sampler == 1) {
        hipLaunchKernelGGL(prosac_growth_kernel, dim3(1, 1, c.pairs), dim3(1024), 0, st, m_max, m_dev, p.sample_size, TN, ws->prosac_G, c.z);
        G = ws->prosac_G;
    }
    const long long n_ids = p.iters > 0 ? p.iters : 1;
    for (long long h0l = 0, B = ransac_batch_len(p, 0); h0l < n_ids; h0l += B, B = ransac_batch_len(p, B)) {
        const int h0 = (int)h0l;
        const int h1 = h0l + B < p.iters ? (int)(h0l + B) : p.iters;
        const int ids = h1 - h0 > 0 ? h1 - h0 : 1;
        const int gb_all = lr_cdiv(ids, 256);                               // 256-id groups of the batch
        const int gb = gb_all < 1024 ? gb_all : 1024;                       // blocks per pair (they stride over the groups)
        // fit: a wave per 64 list slots, at most 4096 waves in the launch (four per SIMD; they stride over longer lists)
        const int fb_all = lr_cdiv(ids, 64), fb_cap = 4096 / c.pairs > 16 ? 4096 / c.pairs : 16;
        const int fb = fb_all < fb_cap ? fb_all : fb_cap;
        auto draw_and_fit = [&](auto ns) {
            constexpr int NS = decltype(ns)::value;
            hipLaunchKernelGGL(ransac_gen_kernel<NS>, dim3(gb, 1, c.pairs), dim3(256), 0, st, corr8, m_max, m_dev, p, h0, h1, ws->model_h, ws->score_cnt, ws->score_ssq,
                               ws->counters, G, TN, info, c.z);
            hipLaunchKernelGGL(ransac_fit_kernel<NS>, dim3(fb, 1, c.pairs), dim3(64), 0, st, corr8, m_max, m_dev, p, ws->models, ws->models64, (const int32_t *)ws->model_h,
                               (const int32_t *)ws->counters, G, TN, ws->max_iters, c.z);
        };
        if (p.sample_size == 3) draw_and_fit(std::integral_constant<int, 3>{}); else draw_and_fit(std::integral_constant<int, 4>{});
        if (sprt)
            hipLaunchKernelGGL(ransac_sprt_kernel, dim3(gb_all, 1, c.pairs), dim3(256), 0, st, corr8, m_max, m_dev, p.thr2,
                               (const float *)ws->models, (const double *)ws->models64, (const int32_t *)ws->model_h, ws->models2, ws->models64_2, ws->model_h2,
                               ws->score_cnt, ws->score_ssq, ws->counters, ws->max_iters, c.z);
        lr_score_run(c, corr8, m_max, m_dev, p.thr2, models, h1 - h0, vslot);
        if (h0 == 0) LR_TRY_HIP(lr_timer_mark(c, LR_EV_RANSAC_END));      // (generation + scoring of the first batch)
        hipLaunchKernelGGL(ransac_final_kernel, dim3(1, 1, c.pairs), dim3(1024), 0, st, ws->score_cnt, ws->score_ssq, model_h, models64,
                           ws->counters, m_max, m_dev, p, h1, T_out, res, vslot, lo_ctl_words, c.z);
        if (p.local_opt == 1) lr_lo_run(c, corr8, m_max, m_dev, p, h1, 0, T_out, res);
    }
    if (p.local_opt) lr_lo_run(c, corr8, m_max, m_dev, p, p.iters, 1, T_out, res);      // final iterated least squares over the inliers
    LR_LAUNCH_CHECK();
    return LR_OK;
}
