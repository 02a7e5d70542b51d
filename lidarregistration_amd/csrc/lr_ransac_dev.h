// Device text that more than one stage of the RANSAC back end compiles: lr_ransac.hip (hypotheses, merge of a batch), lr_score.hip
// (pilot-ordered scoring), lr_lo.hip (local optimisation).  Device-only and header-only: there is no relocatable device code, so
// every translation unit inlines its own copy.  What a single stage uses stays in that stage's file.
//
// Arithmetic is spelled out op by op and is the oracle's (build: -ffp-contract=off): what both sides compute is one text,
// lr_contract.h; the packed form of its fp32 scoring is below.
#pragma once
#include "lr_internal.h"
#include <math.h>

// ------------------------------------------------------------------ Philox4x32-10
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

#include "lr_contract.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the scoring arithmetic on the device (lr_contract.h, "fp32 scoring")
// A model as lr_score_d2 takes it: R | t, row-major.  The model lists hold coefficient k of slot s at [k * stride + s].
struct lr_model12 { float Rt[12]; };
__device__ __forceinline__ lr_model12 lr_load_model(const float *__restrict__ mp, size_t ms)
{
    lr_model12 M;
#pragma unroll
    for (int k = 0; k < 12; ++k) M.Rt[k] = mp[k * ms];
    return M;
}
__device__ __forceinline__ void lr_store_model(float *__restrict__ mp, size_t ms, const lr_model12 &M)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) mp[k * ms] = M.Rt[k];
}
// correspondence i of a packed list (lr_corr_at) under the model
__device__ __forceinline__ float lr_corr_d2(const float Rt[12], const float *__restrict__ corr8, int i)
{
    return lr_score_d2(Rt, corr8[lr_corr_at(i, 0)], corr8[lr_corr_at(i, 1)], corr8[lr_corr_at(i, 2)], corr8[lr_corr_at(i, 3)],
                       corr8[lr_corr_at(i, 4)], corr8[lr_corr_at(i, 5)]);
}

// The packed form: the two correspondences of a 64-byte record per packed fp32 instruction, every half in lr_score_d2's fma order.
// Device-only (ext_vector arithmetic has no C99 spelling), and the one place where it is written.
struct lr_model12x2 {        // every coefficient in both halves; from a float[12] (lr_model12::Rt, an LDS row) or a double[12] rounded to float
    f32x2 c[12];
    template <class T>
    __device__ __forceinline__ explicit lr_model12x2(const T *Rt)
    {
#pragma unroll
        for (int k = 0; k < 12; ++k) { const float v = (float)Rt[k]; c[k] = f32x2{ v, v }; }
    }
};
__device__ __forceinline__ f32x2 lr_d2x2(const lr_model12x2 &S, const f32x2 px, const f32x2 py, const f32x2 pz, const f32x2 qx, const f32x2 qy, const f32x2 qz)
{
    const f32x2 x = __builtin_elementwise_fma(S.c[0], px, __builtin_elementwise_fma(S.c[1], py, __builtin_elementwise_fma(S.c[2], pz, S.c[3])));
    const f32x2 y = __builtin_elementwise_fma(S.c[4], px, __builtin_elementwise_fma(S.c[5], py, __builtin_elementwise_fma(S.c[6], pz, S.c[7])));
    const f32x2 z = __builtin_elementwise_fma(S.c[8], px, __builtin_elementwise_fma(S.c[9], py, __builtin_elementwise_fma(S.c[10], pz, S.c[11])));
    const f32x2 dx = x - qx, dy = y - qy, dz = z - qz;
    return __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy, dz * dz));
}
__device__ __forceinline__ f32x2 lr_d2x2(const lr_model12x2 &S, const f32x2 *o) { return lr_d2x2(S, o[0], o[1], o[2], o[3], o[4], o[5]); }
// the three 16-byte loads of a record -> its six operands px py pz qx qy qz (x: correspondence 2 r, y: 2 r + 1)
__device__ __forceinline__ void lr_record_operands(const f32x4 A, const f32x4 B, const f32x4 C, f32x2 (&o)[6])
{
    o[0] = f32x2{ A.x, A.y }; o[1] = f32x2{ A.z, A.w }; o[2] = f32x2{ B.x, B.y }; o[3] = f32x2{ B.z, B.w }; o[4] = f32x2{ C.x, C.y }; o[5] = f32x2{ C.z, C.w };
}
// count and error terms of the two halves, each under its own predicate (Q: 32-bit where the caller bounds the sum, else 64-bit)
template <class Q>
__device__ __forceinline__ void lr_add_pair(const f32x2 d2, bool in0, bool in1, uint32_t &cnt, Q &q)
{
    const f32x2 fx = d2 * f32x2{ LR_SCORE_SCALE, LR_SCORE_SCALE };
    cnt += (in0 ? 1u : 0u) + (in1 ? 1u : 0u);
    q += (Q)(in0 ? (uint32_t)fx.x : 0u) + (Q)(in1 ? (uint32_t)fx.y : 0u);
}

// ------------------------------------------------------------------ pilot-ordered scoring: shared state (lr_score.hip; ransac_gen_kernel resets it for every batch)
#define LR_SC_HEAD 256
#define LR_SC_NB 128
#define LR_SC_W 0.0625f
#define LR_SC_MIN_M 2048
#define LR_SC_MIN_V 128
#define LR_SC_MIN_PAIRS 4       // calls of at most this many pairs score every model over every correspondence (no ordering passes)
// what the head and order passes leave for the main pass (one per pair arena)
struct lr_score_info {
    unsigned long long pilot_key;     // max over the models of (head inliers << 32 | ~slot): the pilot
    int32_t prune;                    // 1: corr8s / perm / glen describe this batch
    int32_t n_sorted;                 // records in the sorted copy (M - head)
    uint32_t box[6];                  // bounding box of the source points (lr_ford: order-preserving bit patterns; min x y z, max x y z)
    int32_t bad;                      // a source coordinate is not finite: no pruning
    int32_t pad;
    int32_t hist[LR_SC_NB];           // records per residual bucket
    int32_t fill[LR_SC_NB];           // next free position of every bucket while the sorted copy is written
    int32_t offs[LR_SC_NB + 1];       // start of every residual bucket in the sorted copy (offs[b + 1]: its end)
};
// float <-> unsigned with the same order (atomicMin / atomicMax on floats of either sign)
__device__ __forceinline__ uint32_t lr_ford(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float lr_ford_inv(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
static_assert(sizeof(lr_score_info) <= LR_SC_INFO_BYTES, "lr_score_info does not fit its scratch block");

__device__ __forceinline__ void lr_score_info_reset(lr_score_info *info)      // by one block of >= LR_SC_NB threads
{
    const int t = threadIdx.x;
    if (t < LR_SC_NB) info->hist[t] = 0;
    if (t < 3) { info->box[t] = 0xffffffffu; info->box[3 + t] = 0u; }
    if (t == 0) { info->pilot_key = 0ull; info->bad = 0; info->prune = 0; }
}
__device__ __forceinline__ int lr_sc_head(int m, int V) { return (m >= LR_SC_MIN_M && V >= LR_SC_MIN_V) ? LR_SC_HEAD : 0; }

// re-design of the SPRT for the next batch: eps follows the best model (its inlier count `nc` of `mm` correspondences), delta the
// models rejected so far
__device__ __forceinline__ void lr_sprt_redesign(lr_ransac_state *state, uint32_t nc, int mm)
{
    double eps = state->sprt_eps > 0.0 ? state->sprt_eps : LR_SPRT_EPS0, delta = state->sprt_delta > 0.0 ? state->sprt_delta : LR_SPRT_DELTA0;
    if (nc > 0) { const double e = (double)nc / (double)mm; if (e > eps && e < 1.0) eps = e; }
    if (state->rej_pts > 0) {
        const double d = (double)state->rej_inl / (double)state->rej_pts;
        if (d > 0.0 && d < 0.9 * eps && fabs(d - delta) > 0.05 * delta) delta = d;
    }
    if (!(delta < 0.9 * eps)) delta = 0.9 * eps * 0.5;
    state->sprt_eps = eps; state->sprt_delta = delta;
}

// ------------------------------------------------------------------ local optimisation: the helper blocks' control block (protocol: lr_lo.hip)
// Here because ransac_final_kernel (lr_ransac.hip) zeroes the job slots before every launch of ransac_lo_kernel that has helper blocks.
#define LO_CHUNK_REC 384
#define LO_JOBS 16
struct lr_lo_job { int32_t next_chunk, done_chunks, nchunks, pad0;
                   float Rt[LR_LO_TRIALS][12]; unsigned cnt[LR_LO_TRIALS]; unsigned long long ssq[LR_LO_TRIALS]; };
struct lr_lo_ctl { int32_t phase, pad[3]; lr_lo_job job[LO_JOBS]; };      // phase: 0 nothing yet; k > 0: job k - 1 is published; -1: the master is done
static_assert(sizeof(lr_lo_ctl) <= LR_LO_CTL_BYTES, "lr_lo_ctl does not fit its scratch block");
