// What follows a RANSAC call on gfx950: the inlier mask of its model, the least-squares refit (FR.py:99-111), and Kabsch on explicit point pairs.
//
//   refit   fp64 moments of the inliers over the ORIGINAL NN pairs -> Kabsch
//
// Arithmetic is spelled out op by op and is the oracle's (build: -ffp-contract=off): what both sides compute is one text, lr_contract.h.
#include "lr_internal.h"
#include <math.h>
#include "lr_contract.h"

// ------------------------------------------------------------------ inlier mask (what findRigidTransform returns next to the pose)
__global__ void __launch_bounds__(256)
inlier_mask_kernel(const float *__restrict__ src, const float *__restrict__ tgt, const int32_t *__restrict__ i0, const int32_t *__restrict__ i1,
                   int m_max, const int32_t *__restrict__ m_dev, const double *__restrict__ T, float thr2, uint8_t *__restrict__ mask,
                   int32_t *__restrict__ n_inliers)
{
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int c = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (c < m) {
        float Rt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = (float)T[k];
        const int a = i0 ? i0[c] : c, b = i1 ? i1[c] : c;
        in = lr_score_d2(Rt, src[3 * a], src[3 * a + 1], src[3 * a + 2], tgt[3 * b], tgt[3 * b + 1], tgt[3 * b + 2]) < thr2;
        mask[c] = in ? 1 : 0;
    }
    if (n_inliers) {
        const unsigned long long bal = __ballot(in);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_inliers, (int)__popcll(bal));
    }
}

int lr_inlier_mask_run(const float *src, const float *tgt, const int32_t *i0, const int32_t *i1, int m_max, const int32_t *m_dev,
                       const double *T, float thr2, uint8_t *mask, int32_t *n_inliers, hipStream_t st)
{
    if (n_inliers) LR_HIP(hipMemsetAsync(n_inliers, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(inlier_mask_kernel, dim3(lr_cdiv(m_max > 0 ? m_max : 1, 256)), dim3(256), 0, st, src, tgt, i0, i1, m_max, m_dev, T, thr2, mask, n_inliers);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

// sum of the block partials (fixed order) + Kabsch + result block; run by the block that finishes last
__device__ void refit_solve_body(const double *__restrict__ partial, int nblocks, const double *__restrict__ T_in,
                   const lr_ransac_result *__restrict__ gate, double *__restrict__ T_out, int32_t *__restrict__ n_inl,
                   lr_pair_result *__restrict__ pair_out, const int32_t *__restrict__ counters, int weighted)
{
    __shared__ double mom[16];
    __shared__ double stage[64 * 16];
    // partials are summed in block order (reproducible); they are staged through LDS 64 blocks at a time so the
    // 16 summing lanes do not walk a chain of dependent global loads
    double acc = 0.0;
    for (int b0 = 0; b0 < nblocks; b0 += 64) {
        const int nb = min(64, nblocks - b0);
        for (int t = threadIdx.x; t < nb * 16; t += blockDim.x) stage[t] = partial[(size_t)b0 * 16 + t];
        __syncthreads();
        if (threadIdx.x < 16)
            for (int b = 0; b < nb; ++b) acc += stage[b * 16 + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < 16) mom[threadIdx.x] = acc;
    // n_refit counts the inlier pairs (lidarreg.h); mom[0] is their weight sum, which is that count only when every weight is 1
    __shared__ int cnt_w[4];
    int cnt = 0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) cnt += (int)partial[(size_t)nblocks * 16 + b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if ((threadIdx.x & 63) == 0) cnt_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int count = cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3];
    const bool have_model = gate ? gate->best_h >= 0 : true;
    const double n = mom[0];
    double T[16];
    if (!have_model || !(n > 0.0) || (!weighted && n < 3.0))
        for (int k = 0; k < 16; ++k) T[k] = T_in[k];
    else
        lr_rt_from_moments(mom, T);
    const int n_used = have_model ? count : 0;
    for (int k = 0; k < 16; ++k) T_out[k] = T[k];
    if (n_inl) *n_inl = n_used;
    if (pair_out) {          // result block of lr_register_pair (fused: saves a launch)
        for (int k = 0; k < 16; ++k) { pair_out->T[k] = T[k]; pair_out->T_ransac[k] = T_in[k]; }
        pair_out->ransac = *gate;
        pair_out->n_corr = counters[LR_CNT_NCORR];
        pair_out->n_refit = n_used;
        pair_out->n_nn_fixed = counters[LR_CNT_FIX_TOTAL];
        pair_out->status = gate->best_h < 0 ? 1 : 0;
        for (int q = 0; q < 8; ++q) pair_out->reserved[q] = 0;
        {   // reserved[0]: (model, correspondence) evaluations of the scoring passes, in ppm of scanning every list in full (0: not recorded)
            const lr_ransac_state *state = reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT);
            if (state->evals_full > 0) pair_out->reserved[0] = (int32_t)((double)state->evals / (double)state->evals_full * 1e6);
            pair_out->reserved[1] = state->lo_timeouts;       // hand-off waits of the local optimisation that hit their bound (lr_ransac_state)
            // single-pair calls: the one form of the filter pass that was launched was the wrong one (forward: 1, reverse: 2) -- every row went through the exact scan
            pair_out->reserved[2] = (counters[LR_CNT_FORM_MISS_F] ? 1 : 0) | (counters[LR_CNT_FORM_MISS_R] ? 2 : 0);
        }
        for (int k = 0; k < 16; ++k) pair_out->T_icp[k] = T[k];      // overwritten by pair_icp_kernel when the ICP stage runs
        pair_out->icp.fitness = 0.0; pair_out->icp.inlier_rmse = 0.0; pair_out->icp.n_corr = 0; pair_out->icp.iterations = 0;
    }
}

// ------------------------------------------------------------------ refit (FR.py:99-111)
#define LR_REFIT_PER 4
// partial[b][0] = n, [1..3] = sum p, [4..6] = sum q, [7..15] = sum p q^T over the inliers of block b (n: their weight sum);
// behind the gridDim.x moment rows, partial[16 gridDim.x + b] = the number of inliers of block b
__global__ void __launch_bounds__(256)
refit_moments_kernel(const float *__restrict__ xyz0, int n0, const float *__restrict__ xyz1, const int32_t *__restrict__ idx1,
                     const double *__restrict__ T_in, double thr2, double *__restrict__ partial,
                     const int32_t *__restrict__ idx0, const int32_t *__restrict__ m_dev,
                     const float *__restrict__ F0, const float *__restrict__ F1,
                     int32_t *__restrict__ ticket, const lr_ransac_result *__restrict__ gate, double *__restrict__ T_out,
                     int32_t *__restrict__ n_inl, lr_pair_result *__restrict__ pair_out, const int32_t *__restrict__ counters, lr_zargs z)
{
    __shared__ double sm[4][16];
    __shared__ int s_cnt[4];
    __shared__ int s_last;
    if (z.descs) {
        const lr_pair_desc d = z.descs[blockIdx.z];
        xyz0 = d.xyz0; xyz1 = d.xyz1; n0 = d.n0;
        if (F0) { F0 = d.F0; F1 = d.F1; }
    }
    lr_z(idx1, z, blockIdx.z); lr_z(T_in, z, blockIdx.z); lr_z(partial, z, blockIdx.z); lr_z(idx0, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(ticket, z, blockIdx.z); lr_z(gate, z, blockIdx.z); lr_z(T_out, z, blockIdx.z); lr_z(n_inl, z, blockIdx.z); lr_z(counters, z, blockIdx.z);
    if (pair_out) pair_out += blockIdx.z;                  // the caller's result array, one block per pair
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = T_in[k];
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    int cnt = 0;
    // pairs (i, idx1[i]) over all n0 rows, or -- with idx0 -- the listed pairs (idx0[c], idx1[c]), c < *m_dev
    if (m_dev) n0 = min(n0, *m_dev);
    // LR_REFIT_PER pairs per thread (the 16 fp64 wave reductions below cost far more than a pair's moments: one pair per thread spent
    // most of the kernel in shuffles); the loads of all of them are issued before the first use
    int jj[LR_REFIT_PER], pp[LR_REFIT_PER];
#pragma unroll
    for (int u = 0; u < LR_REFIT_PER; ++u) {
        const int i = (blockIdx.x * LR_REFIT_PER + u) * 256 + threadIdx.x;
        jj[u] = i < n0 ? idx1[i] : -1;
        pp[u] = i < n0 ? (idx0 ? idx0[i] : i) : 0;
    }
#pragma unroll
    for (int u = 0; u < LR_REFIT_PER; ++u) {
        if (jj[u] < 0) continue;
        const int j = jj[u], pi = pp[u];
        double p[3] = { (double)xyz0[3 * pi], (double)xyz0[3 * pi + 1], (double)xyz0[3 * pi + 2] };
        double q[3] = { (double)xyz1[3 * j], (double)xyz1[3 * j + 1], (double)xyz1[3 * j + 2] };
        double r[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            r[a] = (((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3]) - q[a];
        double d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        if (d2 < thr2) {
            // weight 1 (Umeyama, FR.py:110-111) or the inverse feature distance of the pair (DGR's weighted
            // Procrustes refit, DGR/core/deep_global_registration.py:531-537)
            double w = 1.0;
            if (F0) {
                const float *fa = F0 + (size_t)pi * 32, *fb = F1 + (size_t)j * 32;
                float acc = 0.0f;
                for (int k = 0; k < 32; ++k) { const float e = fa[k] - fb[k]; const float q2 = e * e; acc = acc + q2; }
                w = 1.0 / (double)fmaxf(__builtin_sqrtf(acc), 1e-12f);
            }
            v[0] += w; cnt += 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) { v[1 + a] += w * p[a]; v[4 + a] += w * q[a]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] += (w * p[a]) * q[b];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        double s = v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) sm[wave][k] = s;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x < 16)
        partial[(size_t)blockIdx.x * 16 + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    if (threadIdx.x == 16)
        partial[(size_t)gridDim.x * 16 + blockIdx.x] = (double)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
    // ---- last block done: agent-scope release of the partials, ticket, acquire, then the solve (saves a launch)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == (int)gridDim.x - 1);
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next call
        }
    }
    __syncthreads();
    if (!s_last) return;
    refit_solve_body(partial, (int)gridDim.x, T_in, gate, T_out, n_inl, pair_out, counters, F0 ? 1 : 0);
}

int lr_refit_run(const lr_call &c, const float *xyz0, int n0, const float *xyz1, const int32_t *idx1,
                 const double *T_in, double thr2, double *T_out, int32_t *n_inl, const lr_ransac_result *gate,
                 lr_pair_result *pair_out, const int32_t *idx0, const int32_t *m_dev,
                 const float *F0, const float *F1)
{
    lr_workspace *ws = c.ws; hipStream_t st = c.st;
    const int nb = lr_cdiv(n0, 256 * LR_REFIT_PER);
    int32_t *ticket = ws->counters + LR_CNT_REFIT_TICKET;
    if (!pair_out) LR_HIP(hipMemsetAsync(ticket, 0, sizeof(int32_t), st));      // lr_register_pair starts from cleared counters
    hipLaunchKernelGGL(refit_moments_kernel, dim3(nb, 1, c.pairs), dim3(256), 0, st, xyz0, n0, xyz1, idx1, T_in, thr2, ws->refit_part, idx0, m_dev,
                       F0, F1, ticket, gate, T_out, n_inl, pair_out, (const int32_t *)ws->counters, c.z);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

// ------------------------------------------------------------------ a13: explicit point pairs
__global__ void kabsch_points_kernel(const double *__restrict__ P, const double *__restrict__ Q, const double *__restrict__ w,
                                     int n, double *__restrict__ T_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double cp[3] = { 0, 0, 0 }, cq[3] = { 0, 0, 0 }, W = 0.0;
    for (int i = 0; i < n; ++i) {
        double wi = w ? w[i] : 1.0;
        W = W + wi;
        for (int a = 0; a < 3; ++a) { cp[a] = cp[a] + wi * P[3 * i + a]; cq[a] = cq[a] + wi * Q[3 * i + a]; }
    }
    for (int a = 0; a < 3; ++a) { cp[a] = cp[a] / W; cq[a] = cq[a] / W; }
    double H[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
    for (int i = 0; i < n; ++i) {
        double wi = w ? w[i] : 1.0;
        double pc[3], qc[3];
        for (int a = 0; a < 3; ++a) { pc[a] = P[3 * i + a] - cp[a]; qc[a] = Q[3 * i + a] - cq[a]; }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) H[a][b] = H[a][b] + (wi * pc[a]) * qc[b];
    }
    double T[16];
    lr_rt_from_cov(H, cp, cq, T);
    for (int k = 0; k < 16; ++k) T_out[k] = T[k];
}

extern "C" int lr_kabsch(const double *P, const double *Q, const double *w, int n, double *T_out, void *stream)
{
    LR_REQUIRE(P && Q && T_out && n >= 1, LR_EINVAL, "lr_kabsch: bad argument");
    hipLaunchKernelGGL(kabsch_points_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, P, Q, w, n, T_out);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
