// Fast exact nearest / second-nearest neighbour search: f16 matrix-core filter + exact fp32 verification.
//
// Contract: reference Experiments/algorithms/matching.py:22-65 with the arithmetic of oracle/oracle.c -- the RESULT is
// bit-identical to the fp32 fma-chain definition.  What is free is how the N0 x N1 candidates are pruned.  On gfx950 the
// fp32-input MFMA runs at the fp32 VALU rate (round 1, profiles/r01a_*: 1024 + ~800 cycles per 32x32 tile), so the pruning
// runs in f16:
//
//   sample  f16 MFMA (v_mfma_f32_16x16x32_f16, the real matrix pipe) over every `sstride`-th column tile; per query row
//           the 2nd smallest (1st for top-1) approximate value u' = n1[j] - 2 dot16(i,j) of that subset: U_i
//   thresh  tau_i = U_i + 2 E_i (+ a sqrt-rounding band), E_i a rigorous bound on |d2_exact - (n0_i + u')|
//   walk    f16 MFMA over ALL column tiles; a column is a candidate of row i iff u' <= tau_i.  The accumulator starts
//           at tau_i/2 (minus the smallest column term when all column norms are alike), so the test of a lane's 16
//           accumulator registers is the AND of their sign bits (or, with spread-out norms, their maximum against n1[j]/2):
//           9 VALU ops per 1024 elements, interleaved with the next tile's MFMAs; candidates are ~1e-4 of the elements;
//           a hit only parks { column, lane group }, the rows and filter values are re-derived later by the same MFMA on
//           the gathered columns, and the thresholds tighten as the walk finds better neighbours (sample, thresholds and
//           walk are ONE kernel, nn16_passb_kernel)
//   reverse (mutual filter) thresholds from the forward result, rows / columns ordered by forward NN distance so that
//           each row block walks only a prefix of the column tiles (lr_nn16_reverse)
//   exact   per row, the fp32 fma-chain distance of its few candidates, ordered by (sqrt value, index) --
//           this is exactly torch.min's "first minimal value" order, so no separate tie-break path is needed;
//           rows whose candidate list overflowed (duplicate-heavy inputs) or could not be filled (non-finite
//           f16 conversions) are re-done in place by an exact scan of all columns.
//
// Why the candidate set is a superset of what the exact order needs: let S be the sampled columns and j1, j2 in S the
// two with the smallest u'.  Their exact distances are <= n0_i + U_i + E_i, hence so is the exact 2nd smallest x2 of
// the whole row.  Every j whose sqrt value ties with or beats the 2nd smallest has d2(j) <= x2 (1 + 2^-21), therefore
// u'(j) <= d2(j) - n0_i + E_i <= U_i + 2 E_i + 2^-21 (n0_i + U_i + E_i)  -- the threshold of the filter pass.
//
// Error bound (u = 2^-24; n0, n1 squared norms; all terms worst case):
//   exact chain vs real arithmetic      <= (2 g32 + 3u)(n0 + n1),  g32 = 32u/(1-32u)          ~  67 u (n0+n1)
//   f16 input rounding (RN, 2^-11 rel.) <= (2^-10 + 2^-22) 2 sqrt(n0 n1) <= (2^-10 + 2^-22)(n0+n1)
//   f16 underflow (|x| < 2^-14)         <= 2 * 2^-25 (|a|_1 + |b|_1) <= 3.4e-7 (1 + (n0+n1)/2)
//   MFMA fp32 accumulation of exact f16 products, norms, final fma             <= ~162 u (n0+n1) (generous)
//   => E_ij <= 9.91e-4 (n0+n1) + 3.4e-7 ;  used: 1.05e-3 (n0_i + max_j n1_j) + 4e-7 (lr_nn16_err).
//
// This file: the prep and range kernels and the forward direction.  lr_nn16_pass.hip: the filter pass; lr_nn16_exact.hip: the exact stage;
// lr_nn16_rev.hip: the reverse direction; lr_nn16_dev.h: what more than one of them compiles, and the launch plans.
#include "lr_nn16_dev.h"

// ------------------------------------------------------------------ prep: norms + f16 copy
// Eight threads per row (coalesced 16-byte loads).  The norm is the sequential fp32 fma chain over k = 0..31 of the
// arithmetic contract: thread t continues the chain over its four values from where thread t-1 stopped.
// H[row] (64 B) = f16 of k0..31 in order: lane group kb of an MFMA operand reads bytes [16 kb, 16 kb + 16).
__global__ void __launch_bounds__(256)
nn16_prep_kernel(const float *__restrict__ Fa, int na, _Float16 *__restrict__ Ha, float *__restrict__ nrma, float *__restrict__ bmaxa, float *__restrict__ bmina,
                 const float *__restrict__ Fb, int nb, _Float16 *__restrict__ Hb, float *__restrict__ nrmb, float *__restrict__ bmaxb, float *__restrict__ bminb,
                 uint32_t *__restrict__ seed_b, unsigned long long *__restrict__ seed64_b, int32_t *__restrict__ counters, int zero_counters, int nblk_a,
                 uint32_t *__restrict__ yshare_a, lr_zargs z)
{
    __shared__ float s_m[4], s_n[4];
    if (z.descs) { const lr_pair_desc d = z.descs[blockIdx.z]; Fa = d.F0; na = d.n0; Fb = d.F1; nb = d.n1; }
    lr_z(bmina, z, blockIdx.z); lr_z(bminb, z, blockIdx.z);
    lr_z(Ha, z, blockIdx.z); lr_z(nrma, z, blockIdx.z); lr_z(bmaxa, z, blockIdx.z); lr_z(Hb, z, blockIdx.z); lr_z(nrmb, z, blockIdx.z);
    lr_z(bmaxb, z, blockIdx.z); lr_z(seed_b, z, blockIdx.z); lr_z(seed64_b, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(yshare_a, z, blockIdx.z);
    // first kernel of a pair: the counter block starts from zero (lr_register_pair) and the distance range of
    // lr_nn16_reverse from { 0x7f7f7f7f, 0 }
    if (counters && blockIdx.x == 0 && (int)threadIdx.x < LR_CNT_TOTAL) {
        const int k = threadIdx.x;
        if (k == LR_CNT_RLO) counters[k] = 0x7f7f7f7f;
        else if (k == LR_CNT_RHI || k == LR_CNT_FORM_MISS_F || k == LR_CNT_FORM_MISS_R || zero_counters) counters[k] = 0;
    }
    // blocks [0, nblk_a) prepare cloud a, the rest cloud b (one launch for the pair; nblk_a = ceil(na/32) of the largest
    // cloud of a batch: blocks past a pair's own rows only write a zero maximum)
    const bool second = (int)blockIdx.x >= nblk_a;
    const float *__restrict__ F = second ? Fb : Fa;
    _Float16 *__restrict__ H = second ? Hb : Ha;
    float *__restrict__ nrm = second ? nrmb : nrma;
    float *__restrict__ block_max = second ? bmaxb : bmaxa;
    float *__restrict__ block_min = second ? bminb : bmina;
    const int n = second ? nb : na;
    const int blk = second ? blockIdx.x - nblk_a : blockIdx.x;
    const int gid = blk * 256 + threadIdx.x;
    const int row = gid >> 3, t = gid & 7, lane = threadIdx.x & 63;
    const bool live = row < n;
    f32x4 v = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (live) v = reinterpret_cast<const f32x4 *>(F + (size_t)row * 32)[t];
    float run = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        float in = __shfl(run, (lane & ~7) | (s > 0 ? s - 1 : 0));
        if (s == 0) in = 0.0f;
        float out = __builtin_fmaf(v.x, v.x, in);
        out = __builtin_fmaf(v.y, v.y, out);
        out = __builtin_fmaf(v.z, v.z, out);
        out = __builtin_fmaf(v.w, v.w, out);
        if (t == s) run = out;
    }
    const float norm = __shfl(run, (lane & ~7) | 7);
    if (live) {
        if (t == 0) {
            nrm[row] = norm;
            if (!second && yshare_a) yshare_a[row] = LR_ORD_INF;      // "no strip of the forward filter pass has a threshold for this row yet"
            if (second && seed_b) { seed_b[row] = 0x7f7f7f7fu; seed64_b[row] = ~0ull; }      // "no query points at this row yet" (lr_nn16_reverse)
        }
        const int pos = 4 * t;
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        f16x4 hv = { (_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w };
        *reinterpret_cast<f16x4 *>(H + (size_t)row * 32 + pos) = hv;
    }
    // largest norm of the block (32 rows) -> block_max[blockIdx.x]; the threshold kernel reduces that short array
    // (no same-address atomics: thousands of them serialise at ~12 ns each)
    // (a NaN norm drops out of fmaxf: such rows are re-done exactly anyway.  For the minimum a norm that is not finite -- NaN, or an
    // overflowing sum -- counts as -1: the range kernel's minimum is then negative, which tells the filter pass not to select the sign
    // form of its test (it needs all norms alike) and the exact kernel to re-do EVERY row of the other cloud by the full scan: a NaN
    // column is every row's nearest neighbour under the contract -- fmaxf(NaN, 1e-30) is 1e-30, torch.min returns the NaN -- and no
    // filter value says so)
    float m = live ? norm : 0.0f, mn = live ? ((norm - norm == 0.0f) ? norm : -1.0f) : LR_INF;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { m = fmaxf(m, __shfl_xor(m, k)); mn = fminf(mn, __shfl_xor(mn, k)); }
    if (lane == 0) { s_m[threadIdx.x >> 6] = m; s_n[threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_max[blk] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        if (block_min) block_min[blk] = fminf(fminf(s_n[0], s_n[1]), fminf(s_n[2], s_n[3]));
    }
}

// largest / smallest squared norm of both clouds from the per-32-row values of the prep kernel: range[0..1] cloud a, range[2..3] cloud b
// (one block per cloud and pair; the filter-pass blocks then read two floats instead of reducing ~1000 each)
__global__ void __launch_bounds__(256)
nn16_range_kernel(int na, const float *__restrict__ bmaxa, const float *__restrict__ bmina, int nb, const float *__restrict__ bmaxb,
                  const float *__restrict__ bminb, float *__restrict__ range, int32_t *__restrict__ form_out, lr_zargs z)
{
    __shared__ float s_m[4], s_n[4];
    if (z.descs) { na = z.descs[blockIdx.z].n0; nb = z.descs[blockIdx.z].n1; }
    lr_z(bmaxa, z, blockIdx.z); lr_z(bmina, z, blockIdx.z); lr_z(bmaxb, z, blockIdx.z); lr_z(bminb, z, blockIdx.z); lr_z(range, z, blockIdx.z);
    const bool second = blockIdx.x == 1;
    const float *__restrict__ bmax = second ? bmaxb : bmaxa, *__restrict__ bmin = second ? bminb : bmina;
    const int nblk = ((second ? nb : na) + 31) >> 5;
    float mx = 0.0f, mn = LR_INF;
    for (int b = threadIdx.x; b < nblk; b += 256) { mx = fmaxf(mx, bmax[b]); mn = fminf(mn, bmin[b]); }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, k)); mn = fminf(mn, __shfl_xor(mn, k)); }
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = mx; s_n[threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float hi = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])), lo = fminf(fminf(s_n[0], s_n[1]), fminf(s_n[2], s_n[3]));
        range[2 * second] = hi;
        range[2 * second + 1] = lo;
        // (single-pair calls: which form of the filter pass this cloud's norms ask for when it is the column cloud -- nn16_passb_kernel's
        // own rule --, left in pinned host memory for the NEXT call on the workspace, which then launches that form alone)
        if (form_out) form_out[second] = (lo > 0.0f && hi < LR_INF && hi - lo <= 1e-4f * hi) ? 1 : 2;
    }
}

// ------------------------------------------------------------------ host side
int lr_nn16_prep(const lr_call &c, const float *F0, int n0, const float *F1, int n1, bool zero_counters)
{
    lr_workspace *ws = c.ws;
    hipLaunchKernelGGL(nn16_prep_kernel, dim3(lr_cdiv(n0, 32) + lr_cdiv(n1, 32), 1, c.pairs), dim3(256), 0, c.st, F0, n0, ws->H0, ws->nrm0, ws->bmax0, ws->bmin0,
                       F1, n1, ws->H1, ws->nrm1, ws->bmax1, ws->bmin1, ws->rev_seed, ws->rev_seed64, ws->counters, zero_counters ? 1 : 0, lr_cdiv(n0, 32), ws->yshare, c.z);
    hipLaunchKernelGGL(nn16_range_kernel, dim3(2, 1, c.pairs), dim3(256), 0, c.st, n0, (const float *)ws->bmax0, (const float *)ws->bmin0, n1, (const float *)ws->bmax1,
                       (const float *)ws->bmin1, ws->nn_range, c.pairs == 1 ? ws->form_dev : (int32_t *)nullptr, c.z);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

int lr_nn16_run(const lr_call &c, const float *Fq, int na, const float *Fc, int nb,
                int32_t *idx1, int32_t *idx2, float *s1, float *s2, bool seed_reverse)
{
    lr_workspace *ws = c.ws;
    const int need = idx2 ? 2 : 1;
    const lr_nn16_plan p = lr_nn16_plan_fwd(na, nb, c.pairs, ws->nn_blocks_target, ws->nn_blocks_batch, ws->nn_sample_stride);
    lr_pb_args a = {};      // (no row / column maps, bounds or start thresholds in this direction)
    a.Hq = ws->H0; a.na = na; a.Hc = ws->H1; a.nC = ws->nrm1; a.nb = nb; a.tps = p.tps;
    a.yfin = ws->yfin; a.yfin_stride = ws->max_n; a.yshare = ws->yshare;
    a.thr = lr_thr_in{ ws->nrm0, ws->nn_range + 2, need, p.sstride };
    a.row_blocks = p.row_blocks; a.strips = p.strips; a.dir = 0;
    LR_TRY_HIP(lr_nn16_passb(c, a));
    const lr_ex_out eo = { idx1, idx2, s1, idx2 ? s2 : (float *)nullptr, seed_reverse ? ws->rev_seed : (uint32_t *)nullptr, ws->rev_s1,
                           reinterpret_cast<uint32_t *>(ws->counters + LR_CNT_RLO), ws->rev_seed64 };
    return lr_nn16_exact(c, 0, Fq, na, Fc, nb, p.strips, need, ws->yfin, nullptr, nullptr, eo);
}
