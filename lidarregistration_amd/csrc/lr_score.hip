// RANSAC inlier scoring on gfx950: every model of a batch (lr_ransac.hip) over the correspondences.
//
//   score   one LANE per surviving hypothesis; the correspondence stream is wave-uniform, so it arrives
//           through scalar loads (s_load_dwordx8) and every VALU op is useful work: ~21 ops per
//           (hypothesis, correspondence), no cross-lane reduction, no LDS traffic.  Inlier count and the
//           fixed-point squared error are both integers, so chunk partials combine with integer atomics
//           and the result does not depend on scheduling
// The arithmetic is lr_contract.h's fp32 scoring in its packed form (lr_ransac_dev.h).
#include "lr_ransac_dev.h"
#define LR_INF_F __builtin_huge_valf()

// Work items = (group of 64 hypotheses) x (chunk of correspondences); blocks stride over them.
//
// Pilot-ordered scoring (exact; the oracle scores everything and gets the same integers).  Most of the models that pass the
// pre-check are GOOD models -- all-inlier samples: 83 % of the survivors on the benchmark pair -- and they agree with each other
// to within the sensor noise, so they share their inlier set: scoring each of them over all M correspondences re-discovers the
// same 60 % of outliers thousands of times.  For two models v, * and a correspondence (p, q):
//     |T_v p - q| >= |T_* p - q| - |T_v p - T_* p|  >=  r_*(p, q) - eps_v,     eps_v = |R_v - R_*|_F rho + |(R_v - R_*) c0 + t_v - t_*|
// (c0, rho: centre and radius of a ball around the source points), so (p, q) can only be an inlier of v when r_* < thr + eps_v.
//   head    every model over the first LR_SC_HEAD correspondences in list order; the model with the most inliers there is the
//           pilot * (ransac_score_kernel<1>)
//   order   residuals r_* of the other correspondences -> LR_SC_NB buckets of LR_SC_W metres -> a copy of the records sorted
//           by bucket; per model the last bucket it has to look at, and the models sorted by that bucket, longest first
//           (ransac_order_kernel: one block per pair)
//   main    a group of 64 models of similar reach scans its prefix of the sorted records (ransac_score_kernel<0>)
// Counts and error sums are integer sums over the inliers, so neither the order of the records nor the skipped outliers change
// them.  A pilot that is a bad model only costs the saving (eps is large for everyone), never the result.  Rounding: r_*, eps
// and the scoring arithmetic are fp32 evaluations of quantities of the size of the coordinates; `slack` (1 cm + 4e-6 of that
// size) is two orders of magnitude above their rounding errors.  Not worth its set-up below LR_SC_MIN_M correspondences or
// LR_SC_MIN_V models: then the head is empty and the main pass scans the list as it lies.
#ifndef LR_SCORE_CHUNK
#define LR_SCORE_CHUNK 256
#endif

// one lane's model over the records [begin, end) of a stream (begin even; a trailing odd correspondence is taken alone)
__device__ __forceinline__ void lr_score_stream(const float *__restrict__ corr8, int begin, int end, int sub, float thr2,
                                                const lr_model12 &M, uint32_t &cnt, unsigned long long &ssq)
{
    // two correspondences per packed instruction: the record of a pair is wave-uniform (scalar load) and its halves feed
    // packed fp32 instructions directly; every component keeps the fma order of the arithmetic contract.
    // The error sum runs in 32 bits over sub-blocks short enough not to overflow (sub * thr2 * 2^20 < 2^32).
    // Scalar loads return out of order, so every wait for one drains all of them: the stream is read TWO records (four
    // correspondences) per wait, the loads of the next two issued before the arithmetic of these two -- one wait per ~50 vector
    // instructions with a full iteration of lookahead (a record per wait had the next record's loads and their wait ~25 instructions apart).
    const lr_model12x2 S(M.Rt);
    uint32_t q32 = 0;
    auto pair_of = [&](const f32x2 px, const f32x2 py, const f32x2 pz, const f32x2 qx, const f32x2 qy, const f32x2 qz) {
        const f32x2 d2 = lr_d2x2(S, px, py, pz, qx, qy, qz);
        // (lr_add_pair's statements, kept in place: through the helper the four integer terms of a record are summed in another order
        // and this kernel's assembly changes -- profiles/score_contract_isa.txt)
        const f32x2 fx = d2 * f32x2{ LR_SCORE_SCALE, LR_SCORE_SCALE };
        const bool in0 = d2.x < thr2, in1 = d2.y < thr2;
        cnt += (in0 ? 1u : 0u) + (in1 ? 1u : 0u);
        q32 += (in0 ? (uint32_t)fx.x : 0u) + (in1 ? (uint32_t)fx.y : 0u);
    };
    const int pend = end & ~1;
    for (int b0 = begin; b0 < pend; b0 += sub) {
        const int b1 = min(pend, b0 + sub);
        q32 = 0;
        int i = b0;
        const f32x2 *rec = reinterpret_cast<const f32x2 *>(corr8);
        if (i + 4 <= b1) {
            f32x2 c0[6], c1[6], n0[6], n1[6];
            auto load2 = [&](int at, f32x2 (&r0)[6], f32x2 (&r1)[6]) {
#pragma unroll
                for (int k = 0; k < 6; ++k) { r0[k] = rec[(size_t)(at >> 1) * 8 + k]; r1[k] = rec[(size_t)(at >> 1) * 8 + 8 + k]; }
                __builtin_amdgcn_sched_barrier(0);       // (the loads stay ahead of the arithmetic that follows: left alone the scheduler sinks them to their use)
            };
            load2(i, c0, c1);
            // ping-pong between two register sets (no copies); the last load of a sub-block re-reads its own records: no read past the stream
            while (i + 4 <= b1) {
                // (wait for the records in hand BEFORE the next loads are issued: scalar loads return out of order, a wait placed after
                // them -- where the compiler would put it, at the first use -- drains the prefetch as well)
                __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0)
                load2(i + 8 <= b1 ? i + 4 : i, n0, n1);
                pair_of(c0[0], c0[1], c0[2], c0[3], c0[4], c0[5]);
                pair_of(c1[0], c1[1], c1[2], c1[3], c1[4], c1[5]);
                i += 4;
                if (i + 4 > b1) break;
                __builtin_amdgcn_s_waitcnt(0xC07F);
                load2(i + 8 <= b1 ? i + 4 : i, c0, c1);
                pair_of(n0[0], n0[1], n0[2], n0[3], n0[4], n0[5]);
                pair_of(n1[0], n1[1], n1[2], n1[3], n1[4], n1[5]);
                i += 4;
            }
        }
        if (i < b1) {        // one record left in the sub-block
            const f32x2 *q = rec + (size_t)(i >> 1) * 8;
            pair_of(q[0], q[1], q[2], q[3], q[4], q[5]);
        }
        ssq += q32;
    }
    if (pend < end && begin < end) {      // (a chunk past the end -- begin > end -- owns nothing, not even the odd last correspondence)
        const float d2 = lr_corr_d2(M.Rt, corr8, pend);
        if (d2 < thr2) { cnt += 1u; ssq += lr_score_term(d2); }
    }
}

template <int HEAD>
__global__ void __launch_bounds__(256)
ransac_score_kernel(const float *__restrict__ corr8, const float *__restrict__ corr8s, int m_max, const int32_t *__restrict__ m_dev, float thr2,
                    const float *__restrict__ models, const float *__restrict__ models_s, uint32_t *__restrict__ score_cnt,
                    unsigned long long *__restrict__ score_ssq, const int32_t *__restrict__ counters, lr_score_info *__restrict__ info,
                    const int32_t *__restrict__ perm, const int32_t *__restrict__ glen, int sub, int model_stride, int vslot,
                    int gx, int total, int allow_prune, lr_zargs z)
{
    // 1-D XCD-aware grid -> (block of the pair, pair): the blocks of one pair run on one XCD, whose L2 then serves the pair's
    // record stream (0.5 MB, read by every wave) and its models
    int logical;
    if (!lr_xcd_block(total, logical)) return;
    const int bxi = logical % gx, pair = logical / gx;
    lr_z(corr8, z, pair); lr_z(corr8s, z, pair); lr_z(m_dev, z, pair); lr_z(models, z, pair); lr_z(models_s, z, pair); lr_z(score_cnt, z, pair); lr_z(score_ssq, z, pair);
    lr_z(counters, z, pair); lr_z(info, z, pair); lr_z(perm, z, pair); lr_z(glen, z, pair);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int V = counters[vslot];           // LR_CNT_NVALID, or LR_CNT_NVALID2 behind the SPRT pre-verification
    const int hb = (V + 63) >> 6;
    if (hb == 0 || m <= 0 || reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT)->done) return;
    const int K0 = allow_prune ? lr_sc_head(m, V) : 0;     // (the host leaves the ordering passes out for short batches: same decision here)
    const int lane = threadIdx.x & 63;
    const size_t ms = (size_t)model_stride;
    // a block is four independent waves (one-wave blocks cap the CU at half its wave slots); wave w of the pair's gx blocks takes
    // the work items w, w + W, ...
    // (the wave index is wave-uniform, which the compiler cannot see through threadIdx: without the readfirstlane the record
    // loads become per-lane global loads with VALU address arithmetic instead of scalar loads)
    const int W = gx * 4, w0 = bxi * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (HEAD) {
        if (K0 == 0) return;
        // work item = (group of 64 models, quarter of the head): the head is short, so a group per wave would leave three waves in four
        // idle; the pilot is elected on the first quarter's counts alone (any model is a valid pilot, see above)
        constexpr int HQ = 4, QL = LR_SC_HEAD / HQ;
        for (int w = w0; w < hb * HQ; w += W) {
            const int g = w % hb, qi = w / hb;
            const int slot = g * 64 + lane;
            const bool active = slot < V;
            const lr_model12 M = lr_load_model(models + (active ? slot : 0), ms);
            uint32_t cnt = 0; unsigned long long ssq = 0;
            lr_score_stream(corr8, qi * QL, (qi + 1) * QL, sub, thr2, M, cnt, ssq);
            if (active && cnt) { atomicAdd(&score_cnt[slot], cnt); atomicAdd(&score_ssq[slot], ssq); }
            if (qi == 0) {
                unsigned long long key = active ? ((unsigned long long)cnt << 32) | (unsigned long long)(0xffffffffu - (uint32_t)slot) : 0ull;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) { const unsigned long long k2 = __shfl_xor(key, o); key = k2 > key ? k2 : key; }
                if (lane == 0) atomicMax(&info->pilot_key, key);
            }
        }
        return;
    }
    const bool prune = K0 > 0;
    const float *__restrict__ stream = prune ? corr8s : corr8;
    const int L = prune ? m - K0 : m;
    int chunks = W / hb;
    const int cmax = L / LR_SCORE_CHUNK > 0 ? L / LR_SCORE_CHUNK : 1;   // at least LR_SCORE_CHUNK correspondences per work item
    if (chunks > cmax) chunks = cmax;
    if (chunks < 1) chunks = 1;
    const int per = ((L + chunks - 1) / chunks + 1) & ~1;      // even: chunks start on a pair boundary
    for (int w = w0; w < hb * chunks; w += W) {
        const int g = w % hb, c = w / hb;
        const int len = prune ? min(glen[g], (L + 1) & ~1) : L;      // records this group has to look at
        const int begin = c * per, end = min(len, begin + per);
        if (begin >= end) continue;
        const int spos = g * 64 + lane;        // position in the model order of this batch's scoring (reach-sorted, or the list as it lies)
        const bool active = spos < V;
        const lr_model12 M = lr_load_model((prune ? models_s : models) + (active ? spos : 0), ms);
        uint32_t cnt = 0;
        unsigned long long ssq = 0;
        lr_score_stream(stream, begin, end, sub, thr2, M, cnt, ssq);
        if (active && cnt) {
            const int slot = prune ? perm[spos] : spos;
            atomicAdd(&score_cnt[slot], cnt); atomicAdd(&score_ssq[slot], ssq);
        }
    }
}

// order pass, part 1 (a thread per correspondence): residual under the pilot model -> bucket; bucket histogram and the bounding box of
// the source points through one atomic per block and value
__global__ void __launch_bounds__(256)
ransac_resid_kernel(const float *__restrict__ corr8, int m_max, const int32_t *__restrict__ m_dev, const float *__restrict__ models,
                    const int32_t *__restrict__ counters, lr_score_info *__restrict__ info, uint8_t *__restrict__ cb, int model_stride, int vslot, lr_zargs z)
{
    __shared__ int s_h[LR_SC_NB];
    __shared__ float s_red[4][6];
    __shared__ int s_bad;
    lr_z(corr8, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(models, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(info, z, blockIdx.z); lr_z(cb, z, blockIdx.z);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int V = counters[vslot];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x * 256 + tid;
    if (V <= 0 || blockIdx.x * 256 >= m || reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT)->done) return;
    const int K0 = lr_sc_head(m, V);
    if (K0 == 0) return;
    if (tid < LR_SC_NB) s_h[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int ps = (int)(0xffffffffu - (uint32_t)info->pilot_key);
    ps = min(max(ps, 0), V - 1);
    const lr_model12 P = lr_load_model(models + ps, (size_t)model_stride);
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    if (c < m) {
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float v = corr8[lr_corr_at(c, a)]; bad |= !(fabsf(v) < 3.0e38f); lo[a] = v; hi[a] = v; }
        if (bad) s_bad = 1;
        if (c >= K0) {
            constexpr float INVW = 1.0f / LR_SC_W, RMAX = LR_SC_NB * LR_SC_W;
            const float r = sqrtf(lr_corr_d2(P.Rt, corr8, c));
            int b = LR_SC_NB - 1;
            if (r < RMAX) b = min((int)(r * INVW), LR_SC_NB - 1);      // (NaN, inf: last bucket)
            cb[c] = (uint8_t)b;
            atomicAdd(&s_h[b], 1);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o)); }
    if (lane == 0) { for (int a = 0; a < 3; ++a) { s_red[wave][a] = lo[a]; s_red[wave][3 + a] = hi[a]; } }
    __syncthreads();
    if (tid < LR_SC_NB && s_h[tid]) atomicAdd(&info->hist[tid], s_h[tid]);
    if (tid < 6) {
        float v = s_red[0][tid];
        for (int w = 1; w < 4; ++w) v = tid < 3 ? fminf(v, s_red[w][tid]) : fmaxf(v, s_red[w][tid]);
        if (tid < 3) atomicMin(&info->box[tid], lr_ford(v)); else atomicMax(&info->box[tid], lr_ford(v));
    }
    if (tid == 0 && s_bad) info->bad = 1;
}

// order pass, part 2 (one block per pair): bucket offsets; reach of every model = the last bucket it has to look at; models sorted by
// reach, longest first; records every group of 64 sorted models scans
__global__ void __launch_bounds__(1024)
ransac_order_kernel(int m_max, const int32_t *__restrict__ m_dev, float thr2, const float *__restrict__ models, int32_t *__restrict__ counters,
                    lr_score_info *__restrict__ info, int32_t *__restrict__ perm, int32_t *__restrict__ glen, uint8_t *__restrict__ mb,
                    float *__restrict__ models_s, int model_stride, int vslot, lr_zargs z)
{
    __shared__ int s_h[LR_SC_NB], s_off[LR_SC_NB + 1], s_fill[LR_SC_NB];
    __shared__ unsigned long long s_ev[16];
    lr_z(m_dev, z, blockIdx.z); lr_z(models, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(models_s, z, blockIdx.z);
    lr_z(info, z, blockIdx.z); lr_z(perm, z, blockIdx.z); lr_z(glen, z, blockIdx.z); lr_z(mb, z, blockIdx.z);
    lr_ransac_state *state = reinterpret_cast<lr_ransac_state *>(counters + LR_CNT_COUNT);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int V = counters[vslot];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (V <= 0 || m <= 0 || state->done) return;
    const int K0 = lr_sc_head(m, V);
    if (K0 == 0) return;      // the main pass scans the list as it lies (prune stays 0)
    const size_t ms = (size_t)model_stride;
    int ps = (int)(0xffffffffu - (uint32_t)info->pilot_key);
    ps = min(max(ps, 0), V - 1);
    const lr_model12 P = lr_load_model(models + ps, ms);
    // exclusive scan of the bucket histogram: wave 0, two buckets per lane
    if (tid < 64) {
        const int h0 = info->hist[2 * tid], h1 = info->hist[2 * tid + 1];
        int inc = h0 + h1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (tid >= o) inc += v; }
        const int ex = inc - (h0 + h1);
        s_off[2 * tid] = ex; s_off[2 * tid + 1] = ex + h0;
        info->offs[2 * tid] = ex; info->offs[2 * tid + 1] = ex + h0;
        info->fill[2 * tid] = ex; info->fill[2 * tid + 1] = ex + h0;
        if (tid == 63) { s_off[LR_SC_NB] = inc; info->offs[LR_SC_NB] = inc; }
    }
    if (tid < LR_SC_NB) s_h[tid] = 0;
    __syncthreads();
    // ball around the source points: centre and half diagonal of their bounding box
    const float b0 = lr_ford_inv(info->box[0]), b1 = lr_ford_inv(info->box[1]), b2 = lr_ford_inv(info->box[2]);
    const float b3 = lr_ford_inv(info->box[3]), b4 = lr_ford_inv(info->box[4]), b5 = lr_ford_inv(info->box[5]);
    const float cx = 0.5f * (b0 + b3), cy = 0.5f * (b1 + b4), cz = 0.5f * (b2 + b5);
    const float ex = b3 - b0, ey = b4 - b1, ez = b5 - b2;
    float rho = 0.5f * sqrtf(ex * ex + ey * ey + ez * ez) * 1.0001f + 1e-6f;
    if (info->bad) rho = LR_INF_F;                       // a non-finite coordinate: every model keeps the whole list (eps below is inf or NaN)
    const float amax = fmaxf(fmaxf(fmaxf(fabsf(b0), fabsf(b3)), fmaxf(fabsf(b1), fabsf(b4))), fmaxf(fabsf(b2), fabsf(b5)));
    constexpr float INVW = 1.0f / LR_SC_W, RMAX = LR_SC_NB * LR_SC_W;
    const float thr = sqrtf(thr2);
    const float *Pm = P.Rt;
    const float pt1 = fabsf(Pm[3]) + fabsf(Pm[7]) + fabsf(Pm[11]);
    for (int v = tid; v < V; v += 1024) {
        const lr_model12 M = lr_load_model(models + v, ms);
        const float *Mm = M.Rt;
        const float d00 = Mm[0] - Pm[0], d01 = Mm[1] - Pm[1], d02 = Mm[2] - Pm[2], d10 = Mm[4] - Pm[4], d11 = Mm[5] - Pm[5], d12 = Mm[6] - Pm[6],
                    d20 = Mm[8] - Pm[8], d21 = Mm[9] - Pm[9], d22 = Mm[10] - Pm[10];
        const float F = sqrtf(d00 * d00 + d01 * d01 + d02 * d02 + d10 * d10 + d11 * d11 + d12 * d12 + d20 * d20 + d21 * d21 + d22 * d22);
        const float ux = d00 * cx + d01 * cy + d02 * cz + (Mm[3] - Pm[3]), uy = d10 * cx + d11 * cy + d12 * cz + (Mm[7] - Pm[7]),
                    uz = d20 * cx + d21 * cy + d22 * cz + (Mm[11] - Pm[11]);
        const float eps = (F * rho + sqrtf(ux * ux + uy * uy + uz * uz)) * 1.001f;
        const float slack = 0.01f + 4e-6f * (3.0f * amax + pt1 + fabsf(Mm[3]) + fabsf(Mm[7]) + fabsf(Mm[11]));
        const float cut = thr + eps + slack;
        int bv = LR_SC_NB - 1;
        if (cut < RMAX) bv = min((int)(cut * INVW), LR_SC_NB - 1);      // (NaN, inf: everything)
        mb[v] = (uint8_t)bv;
        atomicAdd(&s_h[LR_SC_NB - 1 - bv], 1);      // longest reach first
    }
    __syncthreads();
    if (tid < 64) {
        const int h0 = s_h[2 * tid], h1 = s_h[2 * tid + 1];
        int inc = h0 + h1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (tid >= o) inc += v; }
        s_fill[2 * tid] = inc - (h0 + h1); s_fill[2 * tid + 1] = inc - h1;
    }
    __syncthreads();
    // the models in that order: a copy (the main pass then reads a group's 64 models with coalesced loads) and the way back to their slots
    for (int v = tid; v < V; v += 1024) {
        const int pos = atomicAdd(&s_fill[LR_SC_NB - 1 - (int)mb[v]], 1);
        perm[pos] = v;
#pragma unroll
        for (int k = 0; k < 12; ++k) models_s[(size_t)k * ms + pos] = models[(size_t)k * ms + v];
    }
    __syncthreads();
    const int L = m - K0;
    const int hb = (V + 63) >> 6;
    unsigned long long ev = 0;
    for (int g = tid; g < hb; g += 1024) {
        const int len = (s_off[(int)mb[perm[g * 64]] + 1] + 1) & ~1;       // the group's first model reaches furthest
        glen[g] = len;
        ev += (unsigned long long)min(len, L) * (unsigned long long)min(64, V - g * 64);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ev += __shfl_xor(ev, o);
    if (lane == 0) s_ev[wave] = ev;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) ev += s_ev[w];
        state->evals += ev + (unsigned long long)V * (unsigned long long)K0;
        state->evals_full += (unsigned long long)V * (unsigned long long)m;
        info->prune = 1; info->n_sorted = L;
    }
}

// order pass, part 3 (a thread per correspondence): the records behind the head copied in bucket order (within a bucket in any order:
// the sums are integers).  A block reserves its share of every bucket with one atomic, its threads take positions inside that.
__global__ void __launch_bounds__(256)
ransac_scatter_kernel(const float *__restrict__ corr8, float *__restrict__ corr8s, int m_max, const int32_t *__restrict__ m_dev,
                      const int32_t *__restrict__ counters, lr_score_info *__restrict__ info, const uint8_t *__restrict__ cb, int vslot, lr_zargs z)
{
    __shared__ int s_h[LR_SC_NB], s_base[LR_SC_NB];
    lr_z(corr8, z, blockIdx.z); lr_z(corr8s, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(info, z, blockIdx.z); lr_z(cb, z, blockIdx.z);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int V = counters[vslot];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * 256 + tid;
    if (V <= 0 || blockIdx.x * 256 >= m || reinterpret_cast<const lr_ransac_state *>(counters + LR_CNT_COUNT)->done) return;
    const int K0 = lr_sc_head(m, V);
    if (K0 == 0) return;
    if (tid < LR_SC_NB) s_h[tid] = 0;
    __syncthreads();
    const bool live = c >= K0 && c < m;
    const int b = live ? (int)cb[c] : 0;
    int rank = 0;
    if (live) rank = atomicAdd(&s_h[b], 1);
    __syncthreads();
    if (tid < LR_SC_NB && s_h[tid]) s_base[tid] = atomicAdd(&info->fill[tid], s_h[tid]);
    __syncthreads();
    if (live) {
        const int pos = s_base[b] + rank;
#pragma unroll
        for (int k = 0; k < 6; ++k) corr8s[lr_corr_at(pos, k)] = corr8[lr_corr_at(c, k)];
    }
    const int L = m - K0;
    if (blockIdx.x == 0 && tid == 0 && (L & 1)) {      // an odd list ends with a record that is nobody's inlier
#pragma unroll
        for (int k = 0; k < 6; ++k) corr8s[lr_corr_at(L, k)] = k < 3 ? 0.0f : 3.0e38f;
    }
}

// ------------------------------------------------------------------ one batch
// Scores the model list `models` (its live length: counters[vslot]) of a batch of `h_count` hypothesis ids into ws->score_cnt / score_ssq.
// Pilot-ordered: head (every model over the first records) -> order (one block per pair) -> main; or the main pass alone over everything.
void lr_score_run(const lr_call &c, const float *corr8, int m_max, const int32_t *m_dev, float thr2, const float *models, int h_count, int vslot)
{
    lr_workspace *ws = c.ws; hipStream_t st = c.st;
    lr_score_info *info = reinterpret_cast<lr_score_info *>(ws->sc_info);
    // correspondences per 32-bit error sum of lr_score_stream: sub * thr2 * 2^20 < 2^32
    int sub = (int)((4294967296.0 / (double)LR_SCORE_SCALE - 1.0) / ((double)thr2 * 1.0000001 + 1e-6));
    if (sub > 4096) sub = 4096;
    sub &= ~1;                  // the scoring loop takes correspondences two at a time
    if (sub < 2) sub = 2;       // 2 * thr2 * 2^20 < 2^32 for every admissible thr2 (< 2048)
    // (the device decides from the live counts; a batch of up to 1 024 ids is scored in full -- its four ordering launches cost
    // more than they save, and with the pre-check fewer than LR_SC_MIN_V of its ids survive anyway)
    // Nor with a few pairs in the call: the GPU is not full, the main pass over everything costs a lone 30k pair 37 us where the
    // pruned pass costs 39 us AFTER 39 us of ordering launches (FR() 296 -> 254 us; one call of 2 / 4 / 8 / 16 pairs:
    // 0.50 -> 0.46, 0.69 -> 0.65, 1.00 -> 1.03, 1.67 -> 1.76 ms).
    const bool may_prune = m_max >= LR_SC_MIN_M && h_count >= 2048 && c.pairs > LR_SC_MIN_PAIRS;
    if (may_prune) {
        const int hgx = 64, htotal = hgx * c.pairs;
        hipLaunchKernelGGL(ransac_score_kernel<1>, dim3(8 * lr_cdiv(htotal, 8)), dim3(256), 0, st, corr8, (const float *)ws->corr8s, m_max, m_dev, thr2,
                           models, (const float *)ws->models_s, ws->score_cnt, ws->score_ssq, ws->counters, info, (const int32_t *)ws->sc_perm, (const int32_t *)ws->sc_glen, sub,
                           ws->max_iters, vslot, hgx, htotal, 1, c.z);
        const dim3 cgrid(lr_cdiv(m_max, 256), 1, c.pairs);
        hipLaunchKernelGGL(ransac_resid_kernel, cgrid, dim3(256), 0, st, corr8, m_max, m_dev, models, (const int32_t *)ws->counters, info, ws->sc_cb,
                           ws->max_iters, vslot, c.z);
        hipLaunchKernelGGL(ransac_order_kernel, dim3(1, 1, c.pairs), dim3(1024), 0, st, m_max, m_dev, thr2, models, ws->counters, info,
                           ws->sc_perm, ws->sc_glen, ws->sc_mb, ws->models_s, ws->max_iters, vslot, c.z);
        hipLaunchKernelGGL(ransac_scatter_kernel, cgrid, dim3(256), 0, st, corr8, ws->corr8s, m_max, m_dev, (const int32_t *)ws->counters, info,
                           (const uint8_t *)ws->sc_cb, vslot, c.z);
    }
    // (main: LR_SCORE_BLOCKS / 4 blocks for EVERY pair of a batched call: 64 per pair -- the GPU filled exactly once -- measured
    // 32 % slower, the few large work items of a pair do not balance)
    const int sgx = LR_SCORE_BLOCKS / 4, stotal = sgx * c.pairs;
    hipLaunchKernelGGL(ransac_score_kernel<0>, dim3(8 * lr_cdiv(stotal, 8)), dim3(256), 0, st, corr8, (const float *)ws->corr8s, m_max, m_dev, thr2,
                       models, (const float *)ws->models_s, ws->score_cnt, ws->score_ssq, ws->counters, info, (const int32_t *)ws->sc_perm, (const int32_t *)ws->sc_glen, sub,
                       ws->max_iters, vslot, sgx, stotal, may_prune ? 1 : 0, c.z);
}
