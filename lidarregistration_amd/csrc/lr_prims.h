// The building blocks the cloud-level kernels share (lr_filter.hip, lr_icp.hip, lr_voxel.hip, lr_overlap.hip, lr_nn3.hip, lr_bbrf.hip, lr_symicp.hip,
// lr_sm.hip, lr_teaser.hip, lr_pdsc.hip, lr_pdsc_solve.hip, lr_dgr.hip; not part of the ABI): wave and block scans, flag counting and
// ordered compaction, the fixed summation tree over a block and its wave levels, the total order of the doubles as integers, the
// three-term dot product, the 64-bit mix hash.  Device only, inlined, no state; a wave is 64 lanes.  The NN files (lr_nn16*.hip) and the RANSAC files (lr_ransac.hip, lr_score.hip, lr_lo.hip) keep their own spellings: the helper re-schedules their kernels.
#pragma once
#include <hip/hip_runtime.h>

// inclusive scan of v over the wave, lane = this thread's lane (int, long long)
template <typename T> __device__ __forceinline__ T lr_wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}

// Flag + ordered compaction in blocks of 256, two small launches instead of a scan: (1) flags + per-block counts, (2) every block sums
// the counts of the blocks before it (<= n/256 values, one coalesced read) and scatters its survivors in order.
// (1) blk_cnt[blockIdx.x] = flags set in this block
__device__ __forceinline__ void lr_block_count(bool flag, int32_t *__restrict__ blk_cnt)
{
    __shared__ int s_wave[4];
    const unsigned long long bal = __ballot(flag);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
// (2) this wave's share of the flags set in the blocks before this one (taken before the caller loads its flag), then this thread's output
// position in ascending-index order across the grid's x dimension (meaningful where flag is set); prefix = flags set in the blocks before
// this one.  s_w, s_p: four LDS words each, the caller's; s_w keeps the waves' counts of this block (prefix + their sum = the grand total).
__device__ __forceinline__ int lr_blocks_before(const int32_t *__restrict__ blk_cnt)
{
    int c = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) c += blk_cnt[b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    return c;
}
__device__ __forceinline__ int lr_ordered_slot(bool flag, int before, int *s_w, int *s_p, int &prefix)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) { s_p[wave] = before; s_w[wave] = __popcll(bal); }
    __syncthreads();
    prefix = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += s_w[w];
    return prefix + woff + __popcll(bal & ((1ull << lane) - 1ull));
}
// exclusive prefix of a flag over a block of NT threads in thread order, and the block's total; s_cnt: NT / 64 LDS words, the caller's
template <int NT> __device__ __forceinline__ int lr_block_rank(bool flag, int *s_cnt, int &total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) { const int n = s_cnt[w]; off += w < wave ? n : 0; tot += n; }
    total = tot;
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}
// exclusive scan of a[0..len) in place by one block of 1024 threads, 4096 entries per round
__device__ __forceinline__ void lr_block_exscan(int32_t *a, size_t len)
{
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (size_t base = 0; base < len; base += 4096) {
        int v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const size_t t = base + 4 * (size_t)tid + k; v[k] = t < len ? a[t] : 0; sum += v[k]; }
        const int incl = lr_wave_incl_scan(sum, lane);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int run = s_carry;
        for (int w = 0; w < wave; ++w) run += s_w[w];
        run += incl - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const size_t t = base + 4 * (size_t)tid + k; if (t < len) a[t] = run; run += v[k]; }
        __syncthreads();
        if (tid == 1023) s_carry = run;
        __syncthreads();
    }
}
// the levels h = 32 .. 1 of a fixed summation tree inside a wave: v_l = v_l + v_(l + h); lane 0 ends with the sum (float, double)
template <typename T> __device__ __forceinline__ T lr_wave_tree_sum(T v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h);
    return v;
}
// The fixed summation tree over a block of n threads (a power of two; the kernel is launched with exactly n), one double per thread:
// s[t] = s[t] + s[t + h] for h = n / 2 .. 1, a barrier per level; every thread returns the sum.  s: n doubles of LDS, the caller's.
// The ORDER is contract, not an implementation choice: G2 (DGR), E2 (PointDSC) and DESIGN.md §11.1 (SM) state this tree, and the numpy
// restatements the kernels are held to bit for bit add in it.  (dg_loop_kernel keeps its own in-loop form of the same tree.)
// <NT>: the width at compile time, what every caller but one uses; sm_fit_kernel passes blockDim.x.
__device__ __forceinline__ double lr_block_tree_sum(double v, double *s, int n)
{
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int h = n / 2; h >= 1; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    return s[0];
}
template <int NT> __device__ __forceinline__ double lr_block_tree_sum(double v, double *s) { return lr_block_tree_sum(v, s, NT); }
// the total order of the doubles as unsigned integers (for atomicMin / atomicMax over doubles), and back
__device__ __forceinline__ unsigned long long lr_ord_enc(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double lr_ord_dec(unsigned long long e)
{
    return __longlong_as_double((long long)((e >> 63) ? (e & 0x7fffffffffffffffull) : ~e));
}
// u . v of three doubles; the association (u0 v0 + u1 v1) + u2 v2 is what the fp64 restatements evaluate
__device__ __forceinline__ double lr_dot3(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
// row a of M.v and the product P Q of 3 x 3 row-major matrices under the same association (lr_symicp.hip; lr_bbrf.hip keeps its own
// spellings of the two, bb_row / bb_mat3: the source of its loop kernels is left as it was)
__device__ __forceinline__ double lr_row3(const double *M, int a, double x, double y, double z) { return (M[3 * a] * x + M[3 * a + 1] * y) + M[3 * a + 2] * z; }
__device__ __forceinline__ void lr_mat3(const double *P, const double *Q, double *R)
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[3 * a + b] = (P[3 * a] * Q[b] + P[3 * a + 1] * Q[3 + b]) + P[3 * a + 2] * Q[6 + b];
}
// 64-bit finaliser mix (MurmurHash3's fmix64): every input bit reaches every output bit
__device__ __forceinline__ unsigned long long lr_mix64(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}
