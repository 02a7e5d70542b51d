// The device text of the wide (33..128) exact feature NN, shared by its two hosts: lr_nnw.hip (lr_nn_wide: one pair, caller scratch) and
// lr_nnw_ws.hip (the NN stage of a wide workspace: pairs as blockIdx.z, both directions, lists in the arenas).  Not part of the ABI.
// The contract is a1/a2 of oracle/oracle.c at the wider D, bit for bit:
//   norm, dot  fmaf chains over k = 0..D-1 from +0;  d2 = fmaf(-2, dot, n0[i] + n1[j]);  s = sqrtf(fmaxf(d2, 1e-30f));
//   order      ascending (s, j): the first minimal value wins, for the first and for the second neighbour; n1 = 1: second = -1 / inf.
// (fmaxf drops a NaN: a non-finite d2 becomes 1e-30 or stays +inf, so no NaN distance is ever compared -- as in the oracle.)
//
//   nnw_block<NS, TOP2>   the hot path, the work of one block.  It owns 128 rows of the row cloud A (32 per wave, resident in registers as
//                     the A operand of v_mfma_f32_32x32x2_f32, which is bit for bit the fmaf chain; D zero-padded to 2 NS, a zero term
//                     leaves the chain as it is) and one strip of the column cloud's 32-column tiles, which stream through LDS transposed
//                     ([k][j], pitch 33), the next tile in flight in registers while the matrix cores work on the current one.  In the
//                     accumulator a lane owns one column residue and 16 rows: it keeps a running top-2 (TOP2 = false: top-1) per owned row
//                     -- as the clamped d2 of the entries, so that the square roots are taken only when a column gets below the last one
//                     kept (sqrtf is monotone: d2 >= d2(last) cannot win under strict '<').  Columns ascend within a lane, so strict '<'
//                     on s keeps the first.  The 32 lanes of a row are merged once per block under the full (s, j) order; no rows x columns
//                     matrix is stored.  The rows may be gathered: logical row i of the block is row rowof(i) of A and of its norms.
//   nnw_merge2        top-2 of two sorted pairs under (s, j): the lanes of a row, and the strips of a row, meet through it -- a total
//                     order, so neither the lane layout nor the strip count can change a result
#pragma once
#include "lr_scratch.h"
#include <math.h>

#define NNW_MAX_N 4194304        // rows of either cloud
#define NNW_MIN_DIM 33
#define NNW_MAX_DIM 128
#define NNW_ROWS 128             // rows of the row cloud per block
#define NNW_PITCH 33             // floats between consecutive k of the transposed tile in LDS
#define NNW_BLOCKS 1024          // column strips are chosen so that about this many blocks run
#define NNW_MAX_STRIPS 64

struct __attribute__((aligned(16))) nnw_part { float s1; int32_t i1; float s2; int32_t i2; };      // a row's top-2 within one strip

// steps of two the kernel is built for: the smallest that holds dim
static inline int nnw_steps(int dim) { return dim <= 36 ? 18 : dim <= 48 ? 24 : dim <= 64 ? 32 : dim <= 96 ? 48 : 64; }

#ifdef __HIPCC__
typedef float nnw_f32x16 __attribute__((ext_vector_type(16)));

// (s, j) order; an empty entry is (inf, -1) and no live entry has s = inf
__device__ __forceinline__ bool nnw_before(float s, int32_t j, float t, int32_t k) { return s < t || (s == t && j < k); }

// top-2 of two sorted pairs
__device__ __forceinline__ void nnw_merge2(float &a1, int32_t &ia1, float &a2, int32_t &ia2, float c1, int32_t ic1, float c2, int32_t ic2)
{
    // the first is the earlier head; the second the earlier of the other head and the winner's own second
    const bool cf = nnw_before(c1, ic1, a1, ia1);
    const float x = cf ? a1 : c1, y = cf ? c2 : a2;
    const int32_t ix = cf ? ia1 : ic1, iy = cf ? ic2 : ia2;
    const bool xf = nnw_before(x, ix, y, iy);
    a1 = cf ? c1 : a1; ia1 = cf ? ic1 : ia1;
    a2 = xf ? x : y; ia2 = xf ? ix : iy;
}

// Row block rb of the `na` (logical) rows against the column tiles [t0, t1) of B's nb columns; emit(row, s1, j1, s2, j2) is called once per
// live logical row, by one lane (TOP2 = false: s2 / j2 are inf / -1).  The caller has made sure that the block has rows (rb * 128 < na);
// every thread of the block must come here (barriers).
template <int NS, bool TOP2, class RowOf, class Emit>
__device__ __forceinline__ void nnw_block(const float *A, const float *nrmA, size_t na, RowOf rowof, const float *B, const float *nrmB, size_t nb,
                                          int D, int rb, int t0, int t1, Emit emit)
{
    constexpr int NF = NS / 4 + (NS % 4 != 0);       // floats of a tile (32 x 2 NS at most) per thread
    constexpr int NK = TOP2 ? 16 : 1;                // (the second neighbour's registers exist in the top-2 form only)
    __shared__ float s_b[2][2 * NS * NNW_PITCH];
    __shared__ float s_n[2][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, jl = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)rb * NNW_ROWS + (size_t)wave * 32;

    // the A operand: row jl of the wave's 32, k = 2 s + h
    float areg[NS];
    {
        const size_t i = row0 + jl;
        const float *x = A + (i < na ? rowof(i) : 0) * (size_t)D;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 2 * s + h;
            areg[s] = (i < na && k < D) ? x[k] : 0.0f;
        }
    }
    // the 16 rows this lane owns in the accumulator
    float ni[16], d1[16], d2[NK];
    int32_t i1[16], i2[NK];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const size_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        ni[r] = row < na ? nrmA[rowof(row)] : 0.0f;
        d1[r] = INFINITY; i1[r] = -1;
        if constexpr (TOP2) { d2[r] = INFINITY; i2[r] = -1; }
    }
    // rows k >= D of both buffers stay zero: the tile stores touch k < D only
    for (int e = tid; e < 2 * 2 * NS * NNW_PITCH; e += 256) (&s_b[0][0])[e] = 0.0f;
    __syncthreads();

    // element e = tid + 256 f of a tile's 32 x D contiguous floats: column e / D, component e % D
    const int step_j = 256 / D, step_k = 256 % D;
    const size_t total = nb * (size_t)D;
    float pre[NF], pre_n = 0.0f;
    auto fetch = [&](int t) {
        const size_t base = (size_t)t * 32 * (size_t)D;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int e = tid + 256 * f;
            pre[f] = (e < 32 * D && base + e < total) ? B[base + e] : 0.0f;
        }
        if (tid < 32) pre_n = (size_t)t * 32 + tid < nb ? nrmB[(size_t)t * 32 + tid] : 0.0f;
    };
    auto store = [&](int buf) {
        int j = tid / D, k = tid % D;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (tid + 256 * f < 32 * D) s_b[buf][k * NNW_PITCH + j] = pre[f];
            j += step_j; k += step_k;
            if (k >= D) { k -= D; ++j; }
        }
        if (tid < 32) s_n[buf][tid] = pre_n;
    };
    int buf = 0;
    if (t0 < t1) { fetch(t0); store(0); }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;
        if (more) fetch(t + 1);
        nnw_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float *b = &s_b[buf][h * NNW_PITCH + jl];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[s], b[2 * s * NNW_PITCH], acc, 0, 0, 0);
        const int j = t * 32 + jl;
        const float nj = s_n[buf][jl];
        if ((size_t)j < nb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float sum = ni[r] + nj;
                const float dc = fmaxf(fmaf(-2.0f, acc[r], sum), 1e-30f);
                if constexpr (TOP2) {
                    if (dc < d2[r]) {
                        const float s = __builtin_sqrtf(dc), b1 = __builtin_sqrtf(d1[r]), b2 = __builtin_sqrtf(d2[r]);
                        if (s < b1) { d2[r] = d1[r]; i2[r] = i1[r]; d1[r] = dc; i1[r] = j; }
                        else if (s < b2) { d2[r] = dc; i2[r] = j; }
                    }
                } else {
                    // (the first neighbour of the top-2 form changes exactly when s < b1, and d2 >= d1 there too: the same first)
                    if (dc < d1[r]) {
                        const float s = __builtin_sqrtf(dc), b1 = __builtin_sqrtf(d1[r]);
                        if (s < b1) { d1[r] = dc; i1[r] = j; }
                    }
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // the 32 lanes of a row (one half-wave) -> one top-2 (top-1) under (s, j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float b1 = __builtin_sqrtf(d1[r]), b2 = INFINITY;
        int32_t j1 = i1[r], j2 = -1;
        if constexpr (TOP2) { b2 = __builtin_sqrtf(d2[r]); j2 = i2[r]; }
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            const float c1 = __shfl_xor(b1, m);
            const int32_t k1 = __shfl_xor(j1, m);
            if constexpr (TOP2) {
                const float c2 = __shfl_xor(b2, m);
                const int32_t k2 = __shfl_xor(j2, m);
                nnw_merge2(b1, j1, b2, j2, c1, k1, c2, k2);
            } else {
                const bool cf = nnw_before(c1, k1, b1, j1);
                b1 = cf ? c1 : b1; j1 = cf ? k1 : j1;
            }
        }
        const size_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (jl == 0 && row < na) emit(row, b1, j1, b2, j2);
    }
}
#endif
