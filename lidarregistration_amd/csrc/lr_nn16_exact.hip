// Exact stage of the NN path (contract and error bound: lr_nn16.hip): the fp32 fma-chain distances of the candidates the filter pass
// (lr_nn16_pass.hip) left in the candidate store, in both directions.  One kernel, one launch site (lr_nn16_exact).
#include "lr_nn16_dev.h"

#define LR_EX_EMPTY 0xffffffffffffffffull
// The two best candidates of a row under the (sqrt value, index) order -- torch.min's "first minimal value" -- are kept as 64-bit keys (value
// bits << 32 | index) with two LDS atomics per candidate:  old = atomicMin(best, key);  atomicMin(second, max(old, key)).  Whatever the
// order of arrival, `best` ends as the smallest key and `second` as the second smallest (every loser max(old, key) is at least the second
// smallest, and the second smallest itself loses exactly once).
__device__ __forceinline__ void ex_offer(unsigned long long *best, unsigned long long *second, float sv, int j)
{
    const unsigned long long key = ((unsigned long long)__float_as_uint(sv) << 32) | (unsigned)j;       // sv > 0: bits order like values
    const unsigned long long old = atomicMin(best, key);
    atomicMin(second, old > key ? old : key);
}
// results of one row (the calling lane's): neighbours and distances by data row; forward direction of a pair: seed the reverse pass (what
// nn16_rev_seed_kernel would recompute bit for bit): best forward distance per target, the row's own column key.  sv / key: the lane's
// contribution to the range the ordering buckets of the reverse pass span (ex_range reduces them over the wave)
__device__ __forceinline__ void ex_write_row(const lr_ex_out &o, int rowd, unsigned long long kb, unsigned long long ks, int nb, int need, float &sv, float &key)
{
    const int i1 = kb == LR_EX_EMPTY ? -1 : (int)(unsigned)kb;
    const float b1 = kb == LR_EX_EMPTY ? LR_INF : __uint_as_float((unsigned)(kb >> 32));
    o.idx1[rowd] = i1;
    if (o.idx2) o.idx2[rowd] = ks == LR_EX_EMPTY ? (nb > 1 ? LR_IMAX : -1) : (int)(unsigned)ks;
    if (o.s1o) o.s1o[rowd] = b1;
    if (o.s2o) o.s2o[rowd] = ks == LR_EX_EMPTY ? LR_INF : __uint_as_float((unsigned)(ks >> 32));
    if (o.seed_out) {
        sv = b1;
        if (!(sv < 3.0e38f)) sv = 3.0e38f;
        if (i1 >= 0 && i1 < nb) {
            atomicMin(&o.seed_out[i1], __float_as_uint(sv));
            atomicMin(&o.seed64[i1], ((unsigned long long)__float_as_uint(sv) << 32) | (unsigned)rowd);
        }
        // column key of the reverse pass: a lower bound of the row's distance to every point it does NOT point at -- its exact
        // second-smallest distance when the second neighbour was asked for (the thresholds then guarantee it), else the smallest
        key = sv;
        if (need >= 2) { key = ks == LR_EX_EMPTY ? 3.0e38f : __uint_as_float((unsigned)(ks >> 32)); if (!(key < 3.0e38f)) key = 3.0e38f; }
        o.seed_s1[rowd] = key;
    }
}
// (one wave, every lane: writer = the lane wrote a row) the range of the seeds and keys
__device__ __forceinline__ void ex_range(const lr_ex_out &o, bool writer, float sv, float key, int lane)
{
    float lo = writer ? sv : 3.0e38f, hi = writer ? fmaxf(sv, key) : 0.0f;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { lo = fminf(lo, __shfl_xor(lo, k)); hi = fmaxf(hi, __shfl_xor(hi, k)); }
    if (lane == 0) {
        atomicMin(&o.seed_range[0], __float_as_uint(lo));
        atomicMax(&o.seed_range[1], __float_as_uint(hi));
    }
}
// a row whose f16 copy is not finite never produced a meaningful filter value (u, v: eight of its fp32 values)
__device__ __forceinline__ bool ex_bad8(const f32x4 &u, const f32x4 &v)
{
    const float big = fmaxf(fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)), fmaxf(fabsf(u.z), fabsf(u.w))), fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    return !(big <= 65504.0f) || u.x != u.x || u.y != u.y || u.z != u.z || u.w != u.w || v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;
}

// ------------------------------------------------------------------ exact verification of the candidates
// A block takes the 64 query rows of one pass-B wave.  Their fp32 descriptors are staged in LDS once; then every thread
// takes ENTRIES of that wave's segments (one segment per column strip): it gathers the entry's column row (128 B) once and,
// for every register bit of the mask, forms the fp32 fma-chain distance to that query row and offers it to the row's two best
// (ex_offer, above).  The work is spread over the threads by entry, so a row with many candidates does not stall its
// neighbours, and nothing is binned or sorted.
// Rows whose segment overflowed, whose list is too short, or whose f16 copy is not finite are re-done by the whole block
// with an exact scan of all columns (slow, rare, and by construction the reference answer).
#define LR_EX_STRIDE 33          // floats per staged query row (odd: conflict-free column-wise reads)

__global__ void __launch_bounds__(256)
nn16_exact_kernel(const float *__restrict__ Fq, const float *__restrict__ nQ, int na,
                  const float *__restrict__ Fc, const float *__restrict__ nC, int nb,
                  const int32_t *__restrict__ cand_cnt, const int32_t *__restrict__ cand, int nstrips, int need,
                  const float *__restrict__ yfin, int yfin_stride,
                  const int32_t *__restrict__ rowmap, const int32_t *__restrict__ na_dev, lr_ex_out out,
                  int32_t *__restrict__ counters, const float *__restrict__ range_c, int dir, int gx, int total, lr_zargs z)
{
    // 1-D XCD-aware grid -> (row block, pair): the blocks one XCD receives are consecutive row blocks of the same pairs, so the
    // column cloud they gather from (3.84 MB of fp32 rows at 30k points) stays in that XCD's L2
    int logical;
    if (!lr_xcd_block(total, logical)) return;
    const int bxi = logical % gx, pair = logical / gx;
    __shared__ float s_a[LR_EX_ROWS * LR_EX_STRIDE];
    __shared__ float s_nq[LR_EX_ROWS];
    __shared__ unsigned long long s_best[LR_EX_ROWS], s_second[LR_EX_ROWS];
    __shared__ int s_cnt[LR_EX_ROWS], s_rowd[LR_EX_ROWS], s_badrow[LR_EX_ROWS];
    __shared__ int s_bad, s_skip, s_nredo, s_redo[LR_EX_ROWS];
    if (z.descs) {      // dir 0: rows = cloud 0 against cloud 1; 1: the reverse direction
        const lr_pair_desc d = z.descs[pair];
        Fq = dir ? d.F1 : d.F0; na = dir ? d.n1 : d.n0; Fc = dir ? d.F0 : d.F1; nb = dir ? d.n0 : d.n1;
    }
    lr_z(nQ, z, pair); lr_z(nC, z, pair); lr_z(cand_cnt, z, pair); lr_z(cand, z, pair); lr_z(rowmap, z, pair); lr_z(yfin, z, pair);
    lr_z(na_dev, z, pair); lr_z(out.idx1, z, pair); lr_z(out.idx2, z, pair); lr_z(out.s1o, z, pair); lr_z(out.s2o, z, pair);
    lr_z(counters, z, pair); lr_z(out.seed_out, z, pair); lr_z(out.seed_s1, z, pair); lr_z(out.seed_range, z, pair); lr_z(out.seed64, z, pair); lr_z(range_c, z, pair);
    unsigned long long *__restrict__ const seed64 = out.seed64;
    if (na_dev) na = *na_dev;                  // compacted row list (reverse direction): lists by position, data by rowmap[]
    const int row0 = bxi * LR_EX_ROWS;
    if (row0 >= na) return;
    const int tid = threadIdx.x;
    // a filter pass that was launched in one form only while this call's norms asked for the other walked nothing -- and then NOBODY wrote
    // this call's candidate counts: the store is not looked at (s_skip below), every row goes through the full scan
    const int miss = counters[LR_CNT_FORM_MISS_F + (dir ? 1 : 0)] != 0 ? 1 : 0;
    // ---- stage the query rows: thread t moves floats [8 (t & 3) .. +8) of row t >> 2
    {
        const int rl = tid >> 2, part = tid & 3;
        const int rowc = min(row0 + rl, na - 1);
        const int rowd = rowmap ? rowmap[rowc] : rowc;
        const f32x4 *pa = reinterpret_cast<const f32x4 *>(Fq + (size_t)rowd * 32 + 8 * part);
        const f32x4 u = pa[0], v = pa[1];
        float *dst = &s_a[rl * LR_EX_STRIDE + 8 * part];
        dst[0] = u.x; dst[1] = u.y; dst[2] = u.z; dst[3] = u.w; dst[4] = v.x; dst[5] = v.y; dst[6] = v.z; dst[7] = v.w;
        const bool bad = ex_bad8(u, v);          // a query row whose f16 copy is not finite never produced a meaningful filter value
        if (tid < LR_EX_ROWS) { s_best[tid] = LR_EX_EMPTY; s_second[tid] = LR_EX_EMPTY; s_cnt[tid] = 0; s_badrow[tid] = 0; }
        // (a column cloud with a norm that is not finite -- the prep kernel's minimum is negative then --: every row by the full scan)
        // ... and so does a form miss (above)
        if (tid == 0) {
            s_bad = ((range_c != nullptr && range_c[1] < 0.0f) || miss) ? 1 : 0; s_skip = miss; s_nredo = 0;
        }
        if (part == 0) { s_nq[rl] = nQ[rowd]; s_rowd[rl] = rowd; }
        __syncthreads();
        if (bad) s_badrow[rl] = 1;
        // reverse direction seeded by this library's forward pass: the best of the points that POINT AT the row is known (distance and
        // smallest index at that distance); the scan below only adds points that do not point at it (see lr_nn16_reverse)
        if (dir == 1 && seed64 && tid < LR_EX_ROWS && row0 + tid < na) { s_best[tid] = seed64[s_rowd[tid]]; s_cnt[tid] = 1; }
    }
    __syncthreads();
    // exact distance of staged row rl to a column row held in registers, the arithmetic contract's fma chain
    auto dist = [&](int rl, const f32x4 (&t)[8], float ncj) {
        const float *a = &s_a[rl * LR_EX_STRIDE];
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc = __builtin_fmaf(a[4 * k], t[k].x, acc);
            acc = __builtin_fmaf(a[4 * k + 1], t[k].y, acc);
            acc = __builtin_fmaf(a[4 * k + 2], t[k].z, acc);
            acc = __builtin_fmaf(a[4 * k + 3], t[k].w, acc);
        }
        const float d2 = __builtin_fmaf(-2.0f, acc, s_nq[rl] + ncj);
        return __builtin_sqrtf(fmaxf(d2, 1e-30f));
    };
    // ---- the candidates: entries { column | kb << 22 | LR_PB_HASG, 16-bit row mask | g16 << 16 } of the filter-pass wave (LR_PB_*, lr_nn16_dev.h)
    if (!s_skip) {
        const int32_t *cw = cand_cnt + bxi * (nstrips + 1);
        const int used = min(max(cw[nstrips], 1), nstrips);        // strips the pass-B row block really used
        const int seg_cap = lr_seg_cap(used);
        // the rows' final thresholds of the filter pass (the tightest over the strips: a threshold is a property of the row, any valid
        // one applies to all of its entries): an entry that carries its filter value g and fails g >= -y is not a candidate any more
        __shared__ float s_yf[LR_EX_ROWS];
        if (tid < LR_EX_ROWS) {
            float yv = LR_INF;
            if (yfin && row0 + tid < na) for (int sidx = 0; sidx < used; ++sidx) yv = fminf(yv, yfin[(size_t)sidx * yfin_stride + row0 + tid]);
            s_yf[tid] = yv;
        }
        __syncthreads();
        const uint2 *__restrict__ segs = reinterpret_cast<const uint2 *>(cand) + (size_t)bxi * LR_NN16_SEG;
        for (int sidx = 0; sidx < used; ++sidx) {
            const int c = cw[sidx];
            if (c < 0) { if (tid == 0) s_bad = 1; continue; }      // segment overflowed: all 64 rows are re-done
            // (two entries in flight per thread measured slower: 118 VGPRs, 4 instead of 6 waves per SIMD)
            for (int e = tid; e < c; e += 256) {
                const uint2 v = segs[(size_t)sidx * seg_cap + e];
                const int j = (int)(v.x & LR_PB_COLMASK), ekb = lr_pb_kb(v.x);
                if (v.x & LR_PB_HASG) {       // (single-row entry with its g, rounded up to 16 bits)
                    const int rl = lr_pb_row(ekb, __builtin_ctz((v.y & 0xffffu) | 0x8000u));
                    const float gv = __uint_as_float(v.y & 0xffff0000u), yr = s_yf[rl];
                    if (gv + 1e-5f * (fabsf(gv) + fabsf(yr)) < -yr) continue;
                }
                f32x4 t[8];
                const f32x4 *pb = reinterpret_cast<const f32x4 *>(Fc + (size_t)j * 32);
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = pb[k];
                const float ncj = nC[j];
                unsigned m = v.y & 0xffffu;
                while (m) {
                    const int bit = __builtin_ctz(m);
                    m &= m - 1;
                    const int rl = lr_pb_row(ekb, bit);
                    ex_offer(&s_best[rl], &s_second[rl], dist(rl, t, ncj), j);
                    atomicAdd(&s_cnt[rl], 1);
                }
            }
        }
    }
    __syncthreads();
    // ---- rows to re-do by an exact scan of all columns
    if (tid < LR_EX_ROWS && row0 + tid < na && (s_bad || s_badrow[tid] || s_cnt[tid] < min(need, nb))) s_redo[atomicAdd(&s_nredo, 1)] = tid;
    __syncthreads();
    const int nredo = s_nredo;
    for (int r = 0; r < nredo; ++r) {
        const int rl = s_redo[r];
        if (tid == 0) { s_best[rl] = LR_EX_EMPTY; s_second[rl] = LR_EX_EMPTY; atomicAdd(&counters[LR_CNT_FIX_TOTAL], 1); }
        __syncthreads();
        for (int j = tid; j < nb; j += 256) {
            f32x4 t[8];
            const f32x4 *pb = reinterpret_cast<const f32x4 *>(Fc + (size_t)j * 32);
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = pb[k];
            ex_offer(&s_best[rl], &s_second[rl], dist(rl, t, nC[j]), j);
        }
    }
    __syncthreads();
    // ---- results: one thread per row
    float sv = 3.0e38f, key = 0.0f;
    const bool writer = tid < LR_EX_ROWS && row0 + tid < na;
    if (writer) ex_write_row(out, s_rowd[tid], s_best[tid], s_second[tid], nb, need, sv, key);
    if (out.seed_out && tid < 64) ex_range(out, writer, sv, key, tid);          // (the rows live in wave 0)
}

// ------------------------------------------------------------------ host side
// Both directions: the query rows' and the columns' norms and the column cloud's norm range are the workspace's, by direction.
int lr_nn16_exact(const lr_call &c, int dir, const float *Fq, int na, const float *Fc, int nb, int strips, int need,
                  const float *yfin, const int32_t *rowmap, const int32_t *na_dev, const lr_ex_out &out)
{
    lr_workspace *ws = c.ws;
    const float *nQ = dir ? ws->nrm1 : ws->nrm0, *nC = dir ? ws->nrm0 : ws->nrm1, *range_c = ws->nn_range + (dir ? 0 : 2);
    // 1-D XCD-aware grid over (block of LR_EX_ROWS rows, pair), padded to a multiple of 8
    const int ex_gx = lr_cdiv(na, LR_EX_ROWS), ex_total = ex_gx * c.pairs;
    hipLaunchKernelGGL(nn16_exact_kernel, dim3(8 * lr_cdiv(ex_total, 8)), dim3(256), 0, c.st, Fq, nQ, na, Fc, nC, nb, (const int32_t *)ws->cand_cnt, (const int32_t *)ws->cand,
                       strips, need, yfin, yfin ? ws->max_n : 0, rowmap, na_dev, out, ws->counters, range_c, dir, ex_gx, ex_total, c.z);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
