// Reverse direction of the NN path (the mutual filter): seeds, the ordering of rows and columns, lr_nn16_reverse.  The walk itself is
// the filter pass of lr_nn16_pass.hip, the verification the exact stage of lr_nn16_exact.hip.
#include "lr_nn16_dev.h"

// ------------------------------------------------------------------ reverse NN seeded by the forward result
// The mutual test only asks, for a cloud-1 point j that some query i points at, whether any other cloud-0 point beats
// that pair.  So the reverse direction needs no sampling pass: the exact distance s*_j of the best forward pair (i*, j)
// IS an upper bound of j's minimum, and pass B looks for points with u' <= s*^2 (1 + 4e-7) - n_j + E.
//   - points j nobody points at are left out (their reverse NN is reported as -1; the reference does not compute it
//     either, matching.py:224-225);
//   - a cloud-0 point i' that does NOT point at j is at least as far from j as from its own second neighbour: d(i', j) >= s2(i')
//     holds exactly in fp32 because both directions form bit-identical distances (key = s2, or s1 when no second neighbour was
//     asked for; a by-product of the forward exact kernel).  The points that DO point at j need no search: the forward exact kernel
//     leaves the best of them per target, with the smallest index among equals, in a 64-bit seed.  The rows (pointed-at j) are
//     therefore ordered by descending s*, the columns (all i') by ascending key (a counting sort on LR_RS_BUCKETS linear buckets;
//     any order is valid, a better one only prunes more), and each 256-row block walks only the prefix of column tiles that can
//     matter to it: the columns in the buckets up to the bucket of its first row's bound (nn16_passb_kernel).
// seeds: seed_bits[j] = min over i with idx1[i] == j of the exact distance; s1[i] = that distance; range = their min / max
__global__ void __launch_bounds__(256)
nn16_rev_seed_kernel(const float *__restrict__ F0, const float *__restrict__ n0v, int n0, const float *__restrict__ F1,
                     const float *__restrict__ n1v, const int32_t *__restrict__ idx1, uint32_t *__restrict__ seed_bits,
                     float *__restrict__ s1, uint32_t *__restrict__ range)
{
    __shared__ float s_lo[4], s_hi[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float sv = 0.0f;
    if (i < n0) {
    const int j = idx1[i];
    const f32x4 *pa = reinterpret_cast<const f32x4 *>(F0 + (size_t)i * 32);
    const f32x4 *pb = reinterpret_cast<const f32x4 *>(F1 + (size_t)j * 32);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f32x4 a = pa[k], b = pb[k];
        acc = __builtin_fmaf(a.x, b.x, acc);
        acc = __builtin_fmaf(a.y, b.y, acc);
        acc = __builtin_fmaf(a.z, b.z, acc);
        acc = __builtin_fmaf(a.w, b.w, acc);
    }
    // same value the reverse direction forms for (j, i): the sum n1 + n0 and the products commute bit for bit
    const float d2 = __builtin_fmaf(-2.0f, acc, n0v[i] + n1v[j]);
    sv = __builtin_sqrtf(fmaxf(d2, 1e-30f));
    if (!(sv < 3.0e38f)) sv = 3.0e38f;                  // non-finite features: keep the bit pattern below the "empty" fill
    atomicMin(&seed_bits[j], __float_as_uint(sv));      // sv > 0: bit patterns order like the values
    s1[i] = sv;
    }
    float lo = i < n0 ? sv : 3.0e38f, hi = i < n0 ? sv : 0.0f;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { lo = fminf(lo, __shfl_xor(lo, k)); hi = fmaxf(hi, __shfl_xor(hi, k)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&range[0], __float_as_uint(fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]))));
        atomicMax(&range[1], __float_as_uint(fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]))));
    }
}

// The ordering of the reverse pass in ONE launch (round 6; rounds 2-5: histogram + scan in a one-block kernel, ranks in a second, the
// permuted f16 copy in a third -- 15 + 39 + 41 us per call of 32 pairs and two dependent launch boundaries between the forward result
// and the reverse walk).  A counting sort on LR_RS_BUCKETS linear buckets per side: cloud-0 points (the columns) by ascending key, cloud-1
// points with a seed (the rows) by descending seed.  `parts` blocks per pair (a power of two), and NO exchange between them:
//   1. every block builds the histograms of ALL keys of its pair in LDS and scans them (redundantly: 4 bytes per key from L2; what the
//      one-block kernel did in 15 us, now without a launch of its own); part 0 writes the offsets the filter pass reads (bucket b ends
//      where bucket b + 1 starts) and the row count;
//   2. a block OWNS the buckets whose first position falls into its share [part, part + 1) n / parts of the order -- a contiguous range
//      per side, found from the block's own offsets;
//   3. it walks all keys again, 8192 per round: the rank of an owned element inside its bucket is an LDS atomic (any order inside a
//      bucket is valid); owned cloud-0 elements are queued as (point, position) in LDS and then moved by FOUR threads per row -- the f16
//      row (64 B) to its position in the permuted copy the reverse walk streams, with colmap and the norm: full lanes and whole 64-byte
//      segments, where a thread that ranks and copies its own element had 1 lane in 8 at work; owned cloud-1 elements get their position
//      in the row list and their threshold at once (4 + 4 bytes).
// Rows nobody points at get rev = -1; the segment counters of the reverse filter pass start from zero (row blocks that use fewer strips
// than offered leave the others untouched).
#define LR_RO_ROUND 8192         // keys per round (1024 threads x 8 keys, all eight loads in flight)
#define LR_RO_QUEUE 3072         // capacity of the round's copy queue: a block owns 1/parts of the keys (1/8 .. 1/32), three times the expected share
                                 // of a round; an element that finds the queue full is moved by its own thread (slow, correct: one bucket holding
                                 // most of a cloud -- hundreds of identical descriptors)
__global__ void __launch_bounds__(1024)
nn16_rev_order_kernel(int n0, int n1, const float *__restrict__ s1, const uint32_t *__restrict__ seed_bits, const uint32_t *__restrict__ range,
                      int32_t *__restrict__ offs, int32_t *__restrict__ n_rows, const float *__restrict__ block_max_c, int nblk_c,
                      const float *__restrict__ nrm1, const _Float16 *__restrict__ H0, const float *__restrict__ nrm0, int32_t *__restrict__ colmap,
                      _Float16 *__restrict__ H0s, float *__restrict__ nrm0s, int32_t *__restrict__ rowmap, float *__restrict__ tau,
                      int32_t *__restrict__ cand_cnt, int32_t *__restrict__ rev_out, int seg_counters, lr_zargs z)
{
    __shared__ int s_pos[2 * LR_RS_BUCKETS];     // histograms, then offsets, then the next free position of every bucket
    __shared__ int2 s_q[LR_RO_QUEUE];            // copy queue of the round: (cloud-0 point, its position)
    __shared__ float s_m[16];
    __shared__ int s_w[16], s_own[4], s_nq, s_nrows;
    if (z.descs) { n0 = z.descs[blockIdx.z].n0; n1 = z.descs[blockIdx.z].n1; nblk_c = (n0 + 31) >> 5; }
    lr_z(s1, z, blockIdx.z); lr_z(seed_bits, z, blockIdx.z); lr_z(range, z, blockIdx.z); lr_z(offs, z, blockIdx.z); lr_z(n_rows, z, blockIdx.z);
    lr_z(block_max_c, z, blockIdx.z); lr_z(nrm1, z, blockIdx.z); lr_z(H0, z, blockIdx.z); lr_z(nrm0, z, blockIdx.z); lr_z(colmap, z, blockIdx.z);
    lr_z(H0s, z, blockIdx.z); lr_z(nrm0s, z, blockIdx.z); lr_z(rowmap, z, blockIdx.z); lr_z(tau, z, blockIdx.z); lr_z(cand_cnt, z, blockIdx.z); lr_z(rev_out, z, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, part = blockIdx.x, parts = gridDim.x;
    for (int k = part * 1024 + tid; k < seg_counters; k += parts * 1024) cand_cnt[k] = 0;
    const float lo = __uint_as_float(range[0]), scale = rs_scale(lo, __uint_as_float(range[1]));
    for (int k = tid; k < 2 * LR_RS_BUCKETS; k += 1024) s_pos[k] = 0;
    if (tid < 4) s_own[tid] = (tid & 1) ? 0 : 0x7fffffff;
    if (tid == 0) s_nq = 0;
    // largest norm of cloud 0 (the columns): part of the rows' thresholds
    float mx = 0.0f;
    for (int b = tid; b < nblk_c; b += 1024) mx = fmaxf(mx, block_max_c[b]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) mx = fmaxf(mx, __shfl_xor(mx, k));
    if (lane == 0) s_m[tid >> 6] = mx;
    __syncthreads();
    float max_nc = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) max_nc = fmaxf(max_nc, s_m[w]);
    // ---- 1. histograms of both sides (sixteen independent loads in flight per thread -- eight keys of each cloud: the loop is bound by load
    //         latency, not by the atomics)
    for (int i0 = tid; i0 < max(n0, n1); i0 += 8 * 1024) {
        float v[8]; uint32_t u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = s1[min(i0 + 1024 * k, n0 - 1)]; u[k] = seed_bits[min(i0 + 1024 * k, n1 - 1)]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + 1024 * k < n0) atomicAdd(&s_pos[rs_bucket(v[k], lo, scale)], 1);
            const float sv = __uint_as_float(u[k]);
            if (i0 + 1024 * k < n1 && sv <= 3.0e38f) atomicAdd(&s_pos[LR_RS_BUCKETS + (LR_RS_BUCKETS - 1 - rs_bucket(sv, lo, scale))], 1);
        }
    }
    __syncthreads();
    // exclusive prefix sums, in place; part 0 publishes them
    for (int side = 0; side < 2; ++side) {
        int *hp = s_pos + side * LR_RS_BUCKETS;
        int v[LR_RS_BUCKETS / 1024], sum = 0;
#pragma unroll
        for (int k = 0; k < LR_RS_BUCKETS / 1024; ++k) { v[k] = hp[tid * (LR_RS_BUCKETS / 1024) + k]; sum += v[k]; }
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        if (lane == 63) s_w[tid >> 6] = inc;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < (tid >> 6); ++w) base += s_w[w];
        int run = base + inc - sum;
#pragma unroll
        for (int k = 0; k < LR_RS_BUCKETS / 1024; ++k) {
            hp[tid * (LR_RS_BUCKETS / 1024) + k] = run;
            if (part == 0) offs[side * LR_RS_BUCKETS + tid * (LR_RS_BUCKETS / 1024) + k] = run;
            run += v[k];
        }
        if (side == 1 && tid == 1023) { s_nrows = run; if (part == 0) *n_rows = run; }
        __syncthreads();
    }
    // ---- 2. the buckets this block owns (contiguous per side: the two threads that sit on a range's ends write them -- no atomics)
    {
        const long long nrows = s_nrows;
        for (int k = tid; k < 2 * LR_RS_BUCKETS; k += 1024) {
            const int side = k >= LR_RS_BUCKETS, kb = k & (LR_RS_BUCKETS - 1);
            const long long n = side ? nrows : (long long)n0, lo_p = (long long)part * n, hi_p = (long long)(part + 1) * n;
            auto own = [&](int idx) { const long long sp = (long long)s_pos[idx] * parts; return sp >= lo_p && sp < hi_p; };
            if (own(k)) {
                if (kb == 0 || !own(k - 1)) s_own[2 * side] = k;
                if (kb == LR_RS_BUCKETS - 1 || !own(k + 1)) s_own[2 * side + 1] = k + 1;
            }
        }
    }
    __syncthreads();
    const int c_lo = s_own[0], c_len = max(s_own[1] - s_own[0], 0), r_lo = s_own[2], r_len = max(s_own[3] - s_own[2], 0);
    // ---- 3a. cloud 0: rank, queue, move (rounds of LR_RO_ROUND keys; every thread runs every round: the barriers are uniform)
    constexpr int U = LR_RO_ROUND / 1024;
    auto move_row = [&](int i, int p, int piece) {
        reinterpret_cast<f32x4 *>(H0s + (size_t)p * 32)[piece] = reinterpret_cast<const f32x4 *>(H0 + (size_t)i * 32)[piece];
        if (piece == 0) { colmap[p] = i; nrm0s[p] = nrm0[i]; }
    };
    for (int i0 = 0; i0 < n0; i0 += LR_RO_ROUND) {
        float v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = s1[min(i0 + tid + 1024 * k, n0 - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = i0 + tid + 1024 * k, b = rs_bucket(v[k], lo, scale);
            if (i < n0 && (unsigned)(b - c_lo) < (unsigned)c_len) {
                const int p = atomicAdd(&s_pos[b], 1), slot = atomicAdd(&s_nq, 1);
                if (slot < LR_RO_QUEUE) s_q[slot] = make_int2(i, p);
                else { for (int piece = 0; piece < 4; ++piece) move_row(i, p, piece); }
            }
        }
        __syncthreads();
        const int nq = min(s_nq, LR_RO_QUEUE);
        __syncthreads();                 // (everybody has read the count before it is reset for the next round)
        if (tid == 0) s_nq = 0;
        for (int e = tid >> 2; e < nq; e += 256) { const int2 ip = s_q[e]; move_row(ip.x, ip.y, tid & 3); }
        __syncthreads();                 // (the queue is consumed and the reset visible before the next round pushes)
    }
    // ---- 3b. cloud 1: position in the row list + threshold, sixteen keys in flight per thread
    constexpr int U1 = 16;
    for (int j0 = tid; j0 < n1; j0 += U1 * 1024) {
        uint32_t v[U1];
#pragma unroll
        for (int k = 0; k < U1; ++k) v[k] = seed_bits[min(j0 + 1024 * k, n1 - 1)];
#pragma unroll
        for (int k = 0; k < U1; ++k) {
            const int row = j0 + 1024 * k;
            if (row >= n1) continue;
            const float sv = __uint_as_float(v[k]);
            if (!(sv <= 3.0e38f)) {      // still the 0x7f7f7f7f fill: no query points at this row
                if ((row & (parts - 1)) == part) rev_out[row] = -1;
                continue;
            }
            const int b = LR_RS_BUCKETS + (LR_RS_BUCKETS - 1 - rs_bucket(sv, lo, scale));
            if ((unsigned)(b - r_lo) >= (unsigned)r_len) continue;
            const int p = atomicAdd(&s_pos[b], 1);
            const float nj = nrm1[row], scl = nj + max_nc;
            const float E = lr_nn16_err(scl);
            const float d2hi = sv * sv * (1.0f + 6e-7f);               // every d2 whose sqrt rounds to <= sv lies below this
            rowmap[p] = row;
            tau[p] = (d2hi - nj) + E + 6e-6f * scl + 2e-6f * d2hi;
        }
    }
}

int lr_nn16_reverse(const lr_call &c, const float *F0, int n0, const float *F1, int n1, const int32_t *fwd_idx1, int32_t *rev, bool seeded)
{
    lr_workspace *ws = c.ws; hipStream_t st = c.st;
    const float *nrm0 = ws->nrm0, *nrm1 = ws->nrm1;
    // rows = cloud 1 (the columns of the forward direction), columns = cloud 0
    const int na = n1, nb = n0;
    const lr_nn16_plan p = lr_nn16_plan_rev(na, nb, c.pairs, ws->rev_strips);
    uint32_t *seed = ws->rev_seed;          // filled with 0x7f7f7f7f, and range reset to { 0x7f7f7f7f, 0 }, by the prep kernel of this pair
    uint32_t *range = reinterpret_cast<uint32_t *>(ws->counters + LR_CNT_RLO);
    int32_t *n_rows = ws->counters + LR_CNT_NREV;
    if (!seeded)     // (the forward pass of lr_register_pair seeds from its exact kernel: same values, one launch less)
        hipLaunchKernelGGL(nn16_rev_seed_kernel, dim3(lr_cdiv(n0, 256)), dim3(256), 0, st, F0, nrm0, n0, F1, nrm1, fwd_idx1, seed, ws->rev_s1, range);
    const int order_parts = c.pairs >= 16 ? 8 : c.pairs >= 4 ? 16 : 32;      // (a power of two; few pairs: more, smaller shares)
    hipLaunchKernelGGL(nn16_rev_order_kernel, dim3(order_parts, 1, c.pairs), dim3(1024), 0, st, n0, n1, (const float *)ws->rev_s1, (const uint32_t *)seed,
                       (const uint32_t *)range, ws->rev_hist, n_rows, (const float *)ws->bmax0, lr_cdiv(nb, 32), nrm1, (const _Float16 *)ws->H0, nrm0, ws->rev_cols, ws->Hs, ws->nrms,
                       ws->rev_rows, ws->tau, ws->cand_cnt, rev, p.row_blocks * 4 * (p.strips + 1), c.z);
    // grids are sized for all rows; blocks past the compacted count (or past their row block's strips) leave at once.
    // The column-prefix pruning (flagged by a non-null tile_min) rests on the keys being true lower bounds: that holds when
    // the list comes from this library's own forward pass (`seeded`, lr_register_pair).  A caller-supplied list (lr_nn_to_mutual,
    // lr_gpf*) may be anything -- the reference's nn_to_mutual accepts any corres_idx1 -- so every row block walks all column
    // tiles there: the seeds are still upper bounds of the row minima, only the prefix cut is given up.
    lr_pb_args a = {};      // (no final thresholds kept, no pooling of them across strips in this direction)
    a.Hq = ws->H1; a.na = na; a.rowmap = ws->rev_rows; a.na_dev = n_rows; a.Hc = ws->Hs; a.nC = ws->nrms; a.nb = nb; a.tps = p.tps;
    a.tau = ws->tau;
    a.colmap = ws->rev_cols; a.tile_min = seeded ? ws->rev_tmin : nullptr; a.row_bound = seed; a.rev_offs = ws->rev_hist; a.rev_range = range;
    a.thr = lr_thr_in{ nullptr, ws->nn_range, 1, 0 };      // (no tightening: the column norms' range selects the form of the walk's test)
    a.row_blocks = p.row_blocks; a.strips = p.strips; a.dir = 1;
    LR_TRY_HIP(lr_nn16_passb(c, a));
    const lr_ex_out reo = { rev, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, seeded ? ws->rev_seed64 : (unsigned long long *)nullptr };
    return lr_nn16_exact(c, 1, F1, na, F0, nb, p.strips, 1, nullptr, ws->rev_rows, n_rows, reo);
}
