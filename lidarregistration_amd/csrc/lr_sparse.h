// What the two sparse-convolution networks share (lr_fcgf.hip: three dimensions, 27 / 125 offsets; lr_dgr6.hip: six dimensions, 729
// offsets) and that does not depend on how a cell is packed into its 64-bit key (not part of the ABI): the lookup in a table of
// lr_cells.h, the key-only bitonic sort that puts a coarse level's cells in ascending key order, and the ReLU of the epilogue F6.
// The kernels are static: each of the two translation units gets its own copy.
#pragma once
#include "lr_cells.h"

#define FC_SORT_CHUNK 2048

typedef unsigned long long fc_u64;
typedef float fc_f32x16 __attribute__((ext_vector_type(16)));

// the slot of `key`, -1 when the table does not hold it (at most half of the slots are taken: an empty one is met)
__device__ __forceinline__ int fc_find(const fc_u64 *__restrict__ keys, unsigned mask, fc_u64 key)
{
    unsigned s = (unsigned)lr_mix64(key) & mask;
    for (;;) {
        const fc_u64 k = keys[s];
        if (k == key) return (int)s;
        if (k == LR_CELL_EMPTY) return -1;
        s = (s + 1) & mask;
    }
}

// bitonic sort, ascending, of n_sort = 2^p >= 2048 keys: the steps with a distance below 2048 run in LDS, 2048 keys per block
static __global__ void __launch_bounds__(1024) fc_sort_local_kernel(fc_u64 *__restrict__ keys, unsigned k_lo, unsigned k_hi)
{
    __shared__ fc_u64 s[FC_SORT_CHUNK];
    const unsigned tid = threadIdx.x, base = blockIdx.x * FC_SORT_CHUNK;
    s[tid] = keys[base + tid]; s[tid + 1024] = keys[base + tid + 1024];
    __syncthreads();
    for (unsigned k = k_lo; k <= k_hi; k <<= 1)
        for (unsigned j = (k >> 1) < 1024u ? (k >> 1) : 1024u; j >= 1; j >>= 1) {
            const unsigned i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1));
            const bool up = ((base + i) & k) == 0;
            const fc_u64 a = s[i], b = s[i + j];
            if ((a > b) == up) { s[i] = b; s[i + j] = a; }
            __syncthreads();
        }
    keys[base + tid] = s[tid]; keys[base + tid + 1024] = s[tid + 1024];
}
static __global__ void __launch_bounds__(256) fc_sort_global_kernel(fc_u64 *__restrict__ keys, unsigned j, unsigned k, unsigned half)
{
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const bool up = (i & k) == 0;
    const fc_u64 a = keys[i], b = keys[i + j];
    if ((a > b) == up) { keys[i] = b; keys[i + j] = a; }
}

// the whole sort of buf[0 .. n_sort), n_sort a power of two >= FC_SORT_CHUNK, on stream st
static inline void fc_sort_launch(fc_u64 *buf, unsigned n_sort, hipStream_t st)
{
    const unsigned half_blocks = (n_sort / 2 + 255) / 256;
    hipLaunchKernelGGL(fc_sort_local_kernel, dim3(n_sort / FC_SORT_CHUNK), dim3(1024), 0, st, buf, 2u, (unsigned)FC_SORT_CHUNK);
    for (unsigned k = 2 * FC_SORT_CHUNK; k <= n_sort; k <<= 1) {
        for (unsigned j = k >> 1; j >= FC_SORT_CHUNK; j >>= 1)
            hipLaunchKernelGGL(fc_sort_global_kernel, dim3(half_blocks), dim3(256), 0, st, buf, j, k, n_sort / 2);
        hipLaunchKernelGGL(fc_sort_local_kernel, dim3(n_sort / FC_SORT_CHUNK), dim3(1024), 0, st, buf, k, k);
    }
}

__device__ __forceinline__ float fc_relu(float y) { return y > 0.0f ? y : (y != y ? y : 0.0f); }
