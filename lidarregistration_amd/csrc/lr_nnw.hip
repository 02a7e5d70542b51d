// lr_nn_wide: exact top-2 feature nearest neighbour for descriptors of 33..128 numbers (FPFH's 33, any other hand-made descriptor), a
// stand-alone entry point with caller-owned scratch.  The contract is a1/a2 of oracle/oracle.c at the wider D, bit for bit:
//   norm, dot  fmaf chains over k = 0..D-1 from +0;  d2 = fmaf(-2, dot, n0[i] + n1[j]);  s = sqrtf(fmaxf(d2, 1e-30f));
//   order      ascending (s, j): the first minimal value wins, for the first and for the second neighbour; n1 = 1: second = -1 / inf.
// (fmaxf drops a NaN: a non-finite d2 becomes 1e-30 or stays +inf, so no NaN distance is ever compared -- as in the oracle.)
//
//   nnw_norm_kernel   a thread per row of either cloud: the norm chain
//   nnw_kernel<NS>    the hot path.  A block owns 128 rows of F0 (32 per wave, resident in registers as the A operand of
//                     v_mfma_f32_32x32x2_f32, which is bit for bit the fmaf chain; D zero-padded to 2 NS, a zero term leaves the chain as it
//                     is) and one strip of F1's 32-column tiles, which stream through LDS transposed ([k][j], pitch 33), the next tile in
//                     flight in registers while the matrix cores work on the current one.  In the accumulator a lane owns one column
//                     residue and 16 rows: it keeps a running top-2 per owned row -- as the clamped d2 of the two entries, so that the
//                     square roots are taken only when a column gets below the second one (sqrtf is monotone: d2 >= d2(second) cannot win
//                     under strict '<').  Columns ascend within a lane, so strict '<' on s keeps the first.  The 32 lanes of a row are
//                     merged once per block under the full (s, j) order; no n0 x n1 matrix is stored
//   nnw_merge_kernel  more than one strip: a thread per row merges the strips' partials in ascending strip order under (s, j) -- plain
//                     loads and stores, no atomics
#include "lr_scratch.h"
#include <math.h>
#include <string.h>

#define NNW_MAX_N 4194304        // rows of either cloud
#define NNW_MIN_DIM 33
#define NNW_MAX_DIM 128
#define NNW_ROWS 128             // rows of F0 per block
#define NNW_PITCH 33             // floats between consecutive k of the transposed tile in LDS
#define NNW_BLOCKS 1024          // column strips are chosen so that about this many blocks run
#define NNW_MAX_STRIPS 64

struct __attribute__((aligned(16))) nnw_part { float s1; int32_t i1; float s2; int32_t i2; };      // a row's top-2 within one strip

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

// steps of two the kernel is built for: the smallest that holds dim
static inline int nnw_steps(int dim) { return dim <= 36 ? 18 : dim <= 48 ? 24 : dim <= 64 ? 32 : dim <= 96 ? 48 : 64; }

struct nnw_args {
    char *base; size_t stride;       // (the scratch, as lr_ptr takes it; one arena)
    nnw_layout L;
    const float *F0, *F1;
    int n0, n1, dim;
    int32_t *idx1, *idx2; float *s1, *s2;
};

typedef float nnw_f32x16 __attribute__((ext_vector_type(16)));

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
    constexpr int NF = NS / 4 + (NS % 4 != 0);       // floats of a tile (32 x 2 NS at most) per thread
    __shared__ float s_b[2][2 * NS * NNW_PITCH];
    __shared__ float s_n[2][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, jl = lane & 31, h = lane >> 5;
    const int rb = (int)blockIdx.x % g.L.rblocks, strip = (int)blockIdx.x / g.L.rblocks;
    const int D = g.dim;
    const int t0 = strip * g.L.tiles_per_strip, t1 = min(t0 + g.L.tiles_per_strip, g.L.tiles);
    const float *nrm0 = lr_ptr<const float>(g, 0, g.L.nrm0), *nrm1 = lr_ptr<const float>(g, 0, g.L.nrm1);
    const size_t row0 = (size_t)rb * NNW_ROWS + (size_t)wave * 32;

    // the A operand: row jl of the wave's 32, k = 2 s + h
    float areg[NS];
    {
        const size_t i = row0 + jl;
        const float *x = g.F0 + i * (size_t)D;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 2 * s + h;
            areg[s] = (i < (size_t)g.n0 && k < D) ? x[k] : 0.0f;
        }
    }
    // the 16 rows this lane owns in the accumulator
    float ni[16], d1[16], d2[16];
    int32_t i1[16], i2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const size_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        ni[r] = row < (size_t)g.n0 ? nrm0[row] : 0.0f;
        d1[r] = d2[r] = INFINITY; i1[r] = i2[r] = -1;
    }
    // rows k >= D of both buffers stay zero: the tile stores touch k < D only
    for (int e = tid; e < 2 * 2 * NS * NNW_PITCH; e += 256) (&s_b[0][0])[e] = 0.0f;
    __syncthreads();

    // element e = tid + 256 f of a tile's 32 x D contiguous floats: column e / D, component e % D
    const int step_j = 256 / D, step_k = 256 % D;
    const size_t total = (size_t)g.n1 * (size_t)D;
    float pre[NF], pre_n = 0.0f;
    auto fetch = [&](int t) {
        const size_t base = (size_t)t * 32 * (size_t)D;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int e = tid + 256 * f;
            pre[f] = (e < 32 * D && base + e < total) ? g.F1[base + e] : 0.0f;
        }
        if (tid < 32) pre_n = (size_t)t * 32 + tid < (size_t)g.n1 ? nrm1[(size_t)t * 32 + tid] : 0.0f;
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
        if (j < g.n1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float sum = ni[r] + nj;
                const float dc = fmaxf(fmaf(-2.0f, acc[r], sum), 1e-30f);
                if (dc < d2[r]) {
                    const float s = __builtin_sqrtf(dc), b1 = __builtin_sqrtf(d1[r]), b2 = __builtin_sqrtf(d2[r]);
                    if (s < b1) { d2[r] = d1[r]; i2[r] = i1[r]; d1[r] = dc; i1[r] = j; }
                    else if (s < b2) { d2[r] = dc; i2[r] = j; }
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // the 32 lanes of a row (one half-wave) -> one top-2 under (s, j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float b1 = __builtin_sqrtf(d1[r]), b2 = __builtin_sqrtf(d2[r]);
        int32_t j1 = i1[r], j2 = i2[r];
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            const float c1 = __shfl_xor(b1, m), c2 = __shfl_xor(b2, m);
            const int32_t k1 = __shfl_xor(j1, m), k2 = __shfl_xor(j2, m);
            nnw_merge2(b1, j1, b2, j2, c1, k1, c2, k2);
        }
        const size_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (jl == 0 && row < (size_t)g.n0) nnw_emit(g, strip, row, b1, j1, b2, j2);
    }
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
