// lr_nn_wide: exact top-2 feature nearest neighbour for descriptors of 33..128 numbers (FPFH's 33, any other hand-made descriptor), a
// stand-alone entry point with caller-owned scratch.  The contract and the hot path (nnw_block) are in lr_nnw_dev.h, which the NN stage of
// a wide workspace (lr_nnw_ws.hip) compiles too.
//
//   nnw_norm_kernel   a thread per row of either cloud: the norm chain
//   nnw_kernel<NS>    a block = nnw_block<NS, top-2> over 128 rows of F0 and one strip of F1's column tiles
//   nnw_merge_kernel  more than one strip: a thread per row merges the strips' partials in ascending strip order under (s, j) -- plain
//                     loads and stores, no atomics
#include "lr_nnw_dev.h"
#include <string.h>

struct nnw_layout {
    size_t nrm0, nrm1, part;     // byte offsets: norms of F0 [n0], of F1 [n1], partials [strips][n0] (strips > 1 only)
    int rblocks, tiles, strips, tiles_per_strip;
};

static inline size_t nnw_make_layout(nnw_layout *L, size_t n0, size_t n1)
{
    L->rblocks = (int)((n0 + NNW_ROWS - 1) / NNW_ROWS);
    L->tiles = (int)((n1 + 31) / 32);
    int strips = L->rblocks ? (NNW_BLOCKS + L->rblocks - 1) / L->rblocks : 1;
    if (strips > NNW_MAX_STRIPS) strips = NNW_MAX_STRIPS;
    if (strips > L->tiles) strips = L->tiles;
    if (strips < 1) strips = 1;
    L->tiles_per_strip = (L->tiles + strips - 1) / strips;
    L->strips = L->tiles_per_strip ? (L->tiles + L->tiles_per_strip - 1) / L->tiles_per_strip : 1;      // (no empty strip)
    size_t off = 0;
    L->nrm0 = off; off += lr_al(n0 * sizeof(float));
    L->nrm1 = off; off += lr_al(n1 * sizeof(float));
    L->part = off; off += L->strips > 1 ? lr_al(n0 * (size_t)L->strips * sizeof(nnw_part)) : 0;
    return off < 256 ? 256 : off;
}

struct nnw_args {
    char *base; size_t stride;       // (the scratch, as lr_ptr takes it; one arena)
    nnw_layout L;
    const float *F0, *F1;
    int n0, n1, dim;
    int32_t *idx1, *idx2; float *s1, *s2;
};

__global__ void __launch_bounds__(256) nnw_norm_kernel(nnw_args g)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)g.n0 + (size_t)g.n1) return;
    const bool second = r >= (size_t)g.n0;
    const size_t row = second ? r - (size_t)g.n0 : r;
    const float *x = (second ? g.F1 : g.F0) + row * (size_t)g.dim;
    float acc = 0.0f;
    for (int k = 0; k < g.dim; ++k) acc = fmaf(x[k], x[k], acc);
    lr_ptr<float>(g, 0, second ? g.L.nrm1 : g.L.nrm0)[row] = acc;
}

__device__ __forceinline__ void nnw_emit(const nnw_args &g, int strip, size_t row, float b1, int32_t i1, float b2, int32_t i2)
{
    if (g.L.strips > 1) {
        lr_ptr<nnw_part>(g, 0, g.L.part)[(size_t)strip * (size_t)g.n0 + row] = nnw_part{ b1, i1, b2, i2 };
    } else {
        g.idx1[row] = i1;
        if (g.idx2) g.idx2[row] = i2;
        if (g.s1) g.s1[row] = b1;
        if (g.s2) g.s2[row] = b2;
    }
}

template <int NS> __global__ void __launch_bounds__(256) nnw_kernel(nnw_args g)
{
    const int rb = (int)blockIdx.x % g.L.rblocks, strip = (int)blockIdx.x / g.L.rblocks;
    const int t0 = strip * g.L.tiles_per_strip, t1 = min(t0 + g.L.tiles_per_strip, g.L.tiles);
    nnw_block<NS, true>(g.F0, lr_ptr<const float>(g, 0, g.L.nrm0), (size_t)g.n0, [](size_t i) { return i; }, g.F1, lr_ptr<const float>(g, 0, g.L.nrm1),
                        (size_t)g.n1, g.dim, rb, t0, t1,
                        [&](size_t row, float b1, int32_t j1, float b2, int32_t j2) { nnw_emit(g, strip, row, b1, j1, b2, j2); });
}

__global__ void __launch_bounds__(256) nnw_merge_kernel(nnw_args g)
{
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= (size_t)g.n0) return;
    const nnw_part *part = lr_ptr<const nnw_part>(g, 0, g.L.part);
    const nnw_part a = part[row];
    float b1 = a.s1, b2 = a.s2;
    int32_t j1 = a.i1, j2 = a.i2;
    for (int s = 1; s < g.L.strips; ++s) {
        const nnw_part c = part[(size_t)s * (size_t)g.n0 + row];
        nnw_merge2(b1, j1, b2, j2, c.s1, c.i1, c.s2, c.i2);
    }
    g.idx1[row] = j1;
    if (g.idx2) g.idx2[row] = j2;
    if (g.s1) g.s1[row] = b1;
    if (g.s2) g.s2[row] = b2;
}

extern "C" size_t lr_nn_wide_scratch_bytes(int n0, int n1, int dim)
{
    if (n0 < 0 || n0 > NNW_MAX_N || n1 < 0 || n1 > NNW_MAX_N || dim < NNW_MIN_DIM || dim > NNW_MAX_DIM) return 0;
    nnw_layout L;
    return nnw_make_layout(&L, (size_t)n0, (size_t)n1);
}

extern "C" int lr_nn_wide(const float *F0, int n0, const float *F1, int n1, int dim, int32_t *idx1, int32_t *idx2, float *s1, float *s2,
                          void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_nn_wide";
    LR_REFUSE_UNLESS(dim < 1 || dim > 32, LR_EINVAL, "dim must lie in 33..128: for 1..32 use lr_nn_top2");
    LR_REFUSE_UNLESS(dim >= NNW_MIN_DIM && dim <= NNW_MAX_DIM, LR_EINVAL, "dim must lie in 33..128");
    LR_REFUSE_UNLESS(n0 >= 0 && n0 <= NNW_MAX_N && n1 >= 0 && n1 <= NNW_MAX_N, LR_EINVAL, "n0 / n1 must lie in 0..4194304");
    LR_REFUSE_UNLESS(n0 == 0 || F0, LR_EINVAL, "null F0");
    LR_REFUSE_UNLESS(n1 == 0 || F1, LR_EINVAL, "null F1");
    LR_REFUSE_UNLESS(n0 == 0 || idx1, LR_EINVAL, "null idx1");
    nnw_args g;
    memset(&g, 0, sizeof g);
    g.stride = nnw_make_layout(&g.L, (size_t)n0, (size_t)n1);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, g.stride, "lr_nn_wide_scratch_bytes(n0, n1, dim)", LR_EINVAL, stream, nullptr));
    if (n0 == 0) return LR_OK;
    g.base = reinterpret_cast<char *>(scratch);
    g.F0 = F0; g.F1 = F1; g.n0 = n0; g.n1 = n1; g.dim = dim;
    g.idx1 = idx1; g.idx2 = idx2; g.s1 = s1; g.s2 = s2;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)n0 + (size_t)n1;
    nnw_norm_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st>>>(g);
    const dim3 grid((unsigned)(g.L.rblocks * g.L.strips));
    switch (nnw_steps(dim)) {
    case 18: nnw_kernel<18><<<grid, dim3(256), 0, st>>>(g); break;
    case 24: nnw_kernel<24><<<grid, dim3(256), 0, st>>>(g); break;
    case 32: nnw_kernel<32><<<grid, dim3(256), 0, st>>>(g); break;
    case 48: nnw_kernel<48><<<grid, dim3(256), 0, st>>>(g); break;
    default: nnw_kernel<64><<<grid, dim3(256), 0, st>>>(g); break;
    }
    if (g.L.strips > 1) nnw_merge_kernel<<<dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st>>>(g);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
