// TEASER++ global registration on gfx950 -- the second back end of the reference's survey (--algo TEASER,
// Experiments/algorithms/TEASER_plus_plus.py:78-126; TEASER++ itself is not vendored: the algorithm is the contract stated in
// include/lidarreg.h and DESIGN.md §10, restated in numpy in tests/teaser_cpu.py).
//
// Stages (each kernel is launched ONCE for a batch, the pair is the grid's last dimension; a single-pair call is a batch of one):
//   1. graph      tz_graph_kernel      pairwise consistency test -> bitset adjacency (uint64 rows, both triangles).  A float32 test
//                                      with a guard band decides the clear cases; pairs inside the band are re-tested in fp64, which
//                                      makes the bits identical to the fp64 definition.
//   2. clique     tz_peel_kernel       one workgroup per pair: degrees, level-synchronous k-core peeling (core numbers, k-core
//                                      shortcut), 16 greedy cliques (lower bound LB), reduction to the core >= LB vertices and removal
//                                      of the vertices adjacent to all others of that set (they join the clique).
//                 tz_compact_kernel    adjacency of what is left, re-indexed compactly.
//                 tz_search_kernel     one wave per pair: bitset branch and bound with a greedy-colouring bound, explicit stack in
//                                      scratch, bounded by a node budget and a device-clock budget; writes the clique in ascending order
//                                      (the wave scan of the extraction is lr_prims.h's, the header of the shared integer steps).
//   3. rotation   tz_rot_kernel        one workgroup per pair, fp64: GNC-TLS over the chain TIMs, 3x3 SVD on one lane.
//   4. translation tz_vote_kernel      every endpoint of the adaptive voting evaluated on its own (no sort: the consensus set at an
//                                      endpoint is the set of intervals whose entry key <= its key < their exit key), then
//                 tz_final_kernel      first minimum per axis, translation inliers, result block.
// All reductions run in a fixed order, so a pair's result does not depend on the batch it is in or on scheduling.
#include "lr_corrset.h"
#include "lr_prims.h"
#include <math.h>

#define TZ_MAX_M CS_MAX_M
#define TZ_MAX_W (TZ_MAX_M / 64)
#define TZ_NWL (TZ_MAX_W / 64)       // bitset words per lane of the search wave
#define TZ_GREEDY_WAVES 16

// per-pair control block at the head of the pair's scratch arena
struct tz_ctl {
    const float *a, *b;
    int32_t *clique_out;
    int32_t m, W;                    // live correspondences, their bitset words
    int32_t maxcore, lb, nU, nR, target, done;
    int32_t K, exact, found, nbest;
    int32_t gnc_iters, n_rot, n_part, status, n_trans, pad;
    unsigned long long nodes;
    double R[9], t[3];
};

struct tz_layout {
    size_t ctl, adj, cadj, stack, core, rlist, cstack, bestc, clique, pidx, bits, tim, wgt, xv, ecost, total;
};

__host__ __device__ static inline int tz_words(int m) { return (m + 63) >> 6; }

static tz_layout tz_make_layout(int max_m)
{
    const size_t W = (size_t)tz_words(max_m < 1 ? 1 : max_m), Mp = W * 64;
    tz_layout L;
    size_t o = 0;
    L.ctl = o;    o += lr_al(sizeof(tz_ctl));
    L.adj = o;    o += lr_al(Mp * W * 8);
    L.cadj = o;   o += lr_al(Mp * W * 8);
    L.stack = o;  o += lr_al((Mp + 1) * W * 8);
    L.core = o;   o += lr_al(Mp * 4);
    L.rlist = o;  o += lr_al(Mp * 4);
    L.cstack = o; o += lr_al(Mp * 4);
    L.bestc = o;  o += lr_al(Mp * 4);
    L.clique = o; o += lr_al(Mp * 4);
    L.pidx = o;   o += lr_al(Mp * 4);
    L.bits = o;   o += lr_al(3 * W * 8);       // [0] incumbent clique, [1] universal vertices, [2] final clique
    L.tim = o;    o += lr_al(6 * Mp * 8);
    L.wgt = o;    o += lr_al(Mp * 8);
    L.xv = o;     o += lr_al(3 * Mp * 8);
    L.ecost = o;  o += lr_al(3 * 2 * Mp * 8);
    L.total = o;
    return L;
}

struct tz_args {
    char *base;                      // scratch arena of pair 0
    size_t stride;                   // bytes between consecutive pairs' arenas
    int Wmax;                        // row stride (words) of every bitset matrix
    tz_layout L;
};

__device__ __forceinline__ void tz_wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- setup: descriptors by value -> control blocks (no host copy, graph-capturable) --------------------------------------
__global__ void tz_setup_kernel(cs_desc_table t, tz_args g, int npairs)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const cs_desc d = t.d[k];
    tz_ctl *c = lr_ptr<tz_ctl>(g, k, g.L.ctl);
    const int m = cs_live_m(d);
    c->a = d.a; c->b = d.b; c->clique_out = (int32_t *)d.out0;
    c->m = m; c->W = tz_words(m);
    c->maxcore = 0; c->lb = 0; c->nU = 0; c->nR = 0; c->target = 0; c->done = 0;
    c->K = 0; c->exact = 1; c->found = 0; c->nbest = 0;
    c->gnc_iters = 0; c->n_rot = 0; c->n_part = 0; c->status = 0; c->n_trans = 0; c->pad = 0;
    c->nodes = 0;
    for (int i = 0; i < 9; ++i) c->R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) c->t[i] = 0.0;
}

// ---- 1. consistency graph ---------------------------------------------------------------------------------------------------
// Edge i~j (i != j) iff | |a_i - a_j| - |b_i - b_j| | <= thr, in fp64 on the promoted inputs: differences, (dx*dx + dy*dy) + dz*dz,
// correctly rounded sqrt (no contraction: -ffp-contract=off).  The float32 image of each distance is within 3 ulp relative of the
// fp64 value (exact inputs, one rounding per operation), so |diff32 - diff64| <= 2.4e-7 (da + db); the band is four times that
// plus a term for the rounding of thr itself.  NaN lands in the band and is decided in fp64 (no edge).
__device__ __forceinline__ bool tz_edge(float aix, float aiy, float aiz, float bix, float biy, float biz,
                                        float ajx, float ajy, float ajz, float bjx, float bjy, float bjz, float thr32, double thr)
{
    const float ax = aix - ajx, ay = aiy - ajy, az = aiz - ajz, bx = bix - bjx, by = biy - bjy, bz = biz - bjz;
    const float da = sqrtf((ax * ax + ay * ay) + az * az), db = sqrtf((bx * bx + by * by) + bz * bz);
    const float diff = fabsf(da - db), band = 1e-6f * (da + db) + 1e-6f * thr32;
    if (diff <= thr32 - band) return true;
    if (diff > thr32 + band) return false;
    const double dax = (double)aix - (double)ajx, day = (double)aiy - (double)ajy, daz = (double)aiz - (double)ajz;
    const double dbx = (double)bix - (double)bjx, dby = (double)biy - (double)bjy, dbz = (double)biz - (double)bjz;
    const double la = sqrt((dax * dax + day * day) + daz * daz), lb = sqrt((dbx * dbx + dby * dby) + dbz * dbz);
    return fabs(la - lb) <= thr;
}

// block = 4 waves; wave v owns column chunk blockIdx.y*4+v (lane = column), the block's 64 rows are walked in turn and every row's
// 64 tests of a chunk become one word by a ballot.  Lane r keeps row r's word and writes it at the end.
__global__ void __launch_bounds__(256) tz_graph_kernel(tz_args g, double thr)
{
    const int pair = blockIdx.z;
    const tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    const int m = c->m, i0 = blockIdx.x * 64, chunk = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i0 >= m || chunk * 64 >= m) return;
    const float *__restrict__ a = c->a, *__restrict__ b = c->b;
    unsigned long long *adj = lr_ptr<unsigned long long>(g, pair, g.L.adj);
    const float thr32 = (float)thr;
    const int j = chunk * 64 + lane;
    const bool jv = j < m;
    float ajx = 0, ajy = 0, ajz = 0, bjx = 0, bjy = 0, bjz = 0;
    if (jv) { ajx = a[3 * j]; ajy = a[3 * j + 1]; ajz = a[3 * j + 2]; bjx = b[3 * j]; bjy = b[3 * j + 1]; bjz = b[3 * j + 2]; }
    unsigned long long mine = 0;
    const int rows = m - i0 < 64 ? m - i0 : 64;
    for (int r = 0; r < rows; ++r) {
        const int i = i0 + r;
        const float aix = a[3 * i], aiy = a[3 * i + 1], aiz = a[3 * i + 2], bix = b[3 * i], biy = b[3 * i + 1], biz = b[3 * i + 2];
        const bool e = jv && j != i && tz_edge(aix, aiy, aiz, bix, biy, biz, ajx, ajy, ajz, bjx, bjy, bjz, thr32, thr);
        const unsigned long long word = __ballot(e);
        if (lane == r) mine = word;
    }
    if (lane < rows) adj[(size_t)(i0 + lane) * g.Wmax + chunk] = mine;
}

// ---- 2a. peeling, greedy lower bound, reduction --------------------------------------------------------------------------------
__device__ __forceinline__ int tz_block_sum(int v, int *s_red)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += s_red[w];
    return s;
}
__device__ __forceinline__ int tz_block_min(int v, int *s_red)
{
    for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = s_red[w] < s ? s_red[w] : s;
    return s;
}

__global__ void __launch_bounds__(1024) tz_peel_kernel(tz_args g, double kcore_threshold)
{
    __shared__ int s_deg[TZ_MAX_M];                       // degrees while peeling; then 32 bitsets of the greedy waves
    __shared__ unsigned long long s_alive[TZ_MAX_W], s_front[TZ_MAX_W];
    __shared__ int s_red[16], s_gsize[TZ_GREEDY_WAVES];
    __shared__ int s_seed[TZ_GREEDY_WAVES];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    const int m = c->m, W = c->W, Ws = g.Wmax;
    if (m == 0) { if (tid == 0) c->done = 1; return; }
    const unsigned long long *adj = lr_ptr<unsigned long long>(g, pair, g.L.adj);
    int32_t *core = lr_ptr<int32_t>(g, pair, g.L.core);
    unsigned long long *bits = lr_ptr<unsigned long long>(g, pair, g.L.bits);
    unsigned long long *inc = bits, *ubits = bits + Ws, *fin = bits + 2 * Ws;

    // degrees (popcount of the rows) and the alive set
    for (int v = wave; v < m; v += 16) {
        int d = 0;
        for (int w = lane; w < W; w += 64) d += __popcll(adj[(size_t)v * Ws + w]);
        for (int o = 32; o >= 1; o >>= 1) d += __shfl_xor(d, o);
        if (lane == 0) s_deg[v] = d;
    }
    for (int w = tid; w < W; w += 1024) {
        const int lo = w * 64;
        s_alive[w] = (m - lo >= 64) ? ~0ull : ((1ull << (m - lo)) - 1ull);
        s_front[w] = 0ull;
    }
    __syncthreads();

    // level-synchronous peeling: every round removes the alive vertices of degree <= k (k = max(k, min degree)), their core number is k
    int k = 0;
    for (;;) {
        int mn = 0x7fffffff, cnt = 0;
        for (int w = tid; w < W; w += 1024) {
            unsigned long long x = s_alive[w];
            cnt += __popcll(x);
            while (x) { const int v = w * 64 + __ffsll((long long)x) - 1; x &= x - 1; const int d = s_deg[v]; mn = d < mn ? d : mn; }
        }
        const int alive = tz_block_sum(cnt, s_red);
        if (alive == 0) break;
        const int dmin = tz_block_min(mn, s_red);
        k = dmin > k ? dmin : k;
        for (int w = tid; w < W; w += 1024) {
            unsigned long long x = s_alive[w], f = 0;
            while (x) {
                const int b = __ffsll((long long)x) - 1; x &= x - 1;
                const int v = w * 64 + b;
                if (s_deg[v] <= k) { f |= 1ull << b; core[v] = k; }
            }
            s_front[w] = f;
            s_alive[w] &= ~f;
        }
        __syncthreads();
        for (int w = wave; w < W; w += 16) {
            unsigned long long f = s_front[w];
            while (f) {
                const int v = w * 64 + __ffsll((long long)f) - 1; f &= f - 1;
                for (int ww = lane; ww < W; ww += 64) {
                    unsigned long long x = adj[(size_t)v * Ws + ww] & s_alive[ww];
                    while (x) { const int u = ww * 64 + __ffsll((long long)x) - 1; x &= x - 1; atomicSub(&s_deg[u], 1); }
                }
            }
        }
        __syncthreads();
    }
    const int maxcore = k;

    // vertices of maximal core number -> s_front
    int nmax = 0;
    for (int w = tid; w < W; w += 1024) {
        unsigned long long f = 0;
        for (int b = 0; b < 64 && w * 64 + b < m; ++b) if (core[w * 64 + b] == maxcore) f |= 1ull << b;
        s_front[w] = f;
        nmax += __popcll(f);
    }
    nmax = tz_block_sum(nmax, s_red);        // (its barriers also publish s_front)

    if ((double)maxcore > kcore_threshold * (double)m) {     // k-core shortcut: the max-core set is the answer
        for (int w = tid; w < W; w += 1024) fin[w] = s_front[w];
        if (tid == 0) { c->maxcore = maxcore; c->lb = 0; c->done = 2; }
        return;
    }

    // greedy cliques: wave j starts from the j-th (mod nmax) max-core vertex, adds max-core candidates in ascending order, then any
    if (lane == 0 && wave < TZ_GREEDY_WAVES) {
        const int want = wave % nmax;
        int seen = 0, seed = 0;
        for (int w = 0; w < W; ++w) {
            const int pc = __popcll(s_front[w]);
            if (seen + pc > want) {
                unsigned long long x = s_front[w];
                for (int r = want - seen; r > 0; --r) x &= x - 1;
                seed = w * 64 + __ffsll((long long)x) - 1;
                break;
            }
            seen += pc;
        }
        s_seed[wave] = seed;
    }
    __syncthreads();
    unsigned long long *gb = reinterpret_cast<unsigned long long *>(s_deg);     // 32 bitsets of W words (W <= 512)
    if (wave < TZ_GREEDY_WAVES) {
        unsigned long long *P = gb + (size_t)wave * 2 * W, *C = P + W;
        const int seed = s_seed[wave];
        for (int w = lane; w < W; w += 64) { P[w] = adj[(size_t)seed * Ws + w]; C[w] = (w == (seed >> 6)) ? (1ull << (seed & 63)) : 0ull; }
        int size = 1;
        tz_wsync();
        for (int pass = 0; pass < 2; ++pass) {
            for (int w = 0; w < W; ++w) {
                const unsigned long long mask = pass == 0 ? s_front[w] : ~0ull;
                unsigned long long x = P[w] & mask;
                while (x) {
                    const int b = __ffsll((long long)x) - 1;
                    const int v = w * 64 + b;
                    if (lane == 0) C[w] |= 1ull << b;
                    ++size;
                    for (int ww = lane; ww < W; ww += 64) P[ww] &= adj[(size_t)v * Ws + ww];
                    tz_wsync();
                    x = P[w] & mask & (b == 63 ? 0ull : ~((2ull << b) - 1ull));
                }
            }
        }
        if (lane == 0) s_gsize[wave] = size;
    }
    __syncthreads();
    int best = 0;
    for (int j = 1; j < TZ_GREEDY_WAVES; ++j) if (s_gsize[j] > s_gsize[best]) best = j;
    const int LB = s_gsize[best];
    {
        const unsigned long long *C = gb + (size_t)best * 2 * W + W;
        for (int w = tid; w < W; w += 1024) inc[w] = C[w];
    }

    // reduction: a clique larger than LB lies in the vertices of core number >= LB; those adjacent to every other one of them join it
    for (int w = tid; w < W; w += 1024) {
        unsigned long long f = 0;
        for (int b = 0; b < 64 && w * 64 + b < m; ++b) if (core[w * 64 + b] >= LB) f |= 1ull << b;
        s_alive[w] = f;
    }
    int nr = 0;
    for (int w = tid; w < W; w += 1024) nr += __popcll(s_alive[w]);
    nr = tz_block_sum(nr, s_red);
    for (int w = tid; w < W; w += 1024) s_front[w] = 0ull;
    __syncthreads();
    for (int w = wave; w < W; w += 16) {
        unsigned long long x = s_alive[w];
        while (x) {
            const int b = __ffsll((long long)x) - 1; x &= x - 1;
            const int v = w * 64 + b;
            int d = 0;
            for (int ww = lane; ww < W; ww += 64) d += __popcll(adj[(size_t)v * Ws + ww] & s_alive[ww]);
            for (int o = 32; o >= 1; o >>= 1) d += __shfl_xor(d, o);
            if (lane == 0 && d == nr - 1) atomicOr(&s_front[w], 1ull << b);
        }
    }
    __syncthreads();
    int nu = 0, nrest = 0;
    for (int w = tid; w < W; w += 1024) {
        ubits[w] = s_front[w];
        nu += __popcll(s_front[w]);
        s_alive[w] &= ~s_front[w];
        nrest += __popcll(s_alive[w]);
    }
    nu = tz_block_sum(nu, s_red);
    nrest = tz_block_sum(nrest, s_red);
    if (nrest == 0) {
        const bool useU = nu > LB;
        for (int w = tid; w < W; w += 1024) fin[w] = useU ? s_front[w] : inc[w];
        if (tid == 0) { c->maxcore = maxcore; c->lb = LB; c->nU = nu; c->nR = 0; c->done = 1; }
        return;
    }
    // compact list of the remaining vertices, ascending
    int32_t *rlist = lr_ptr<int32_t>(g, pair, g.L.rlist);
    if (tid == 0) {
        int off = 0;
        for (int w = 0; w < W; ++w) { const int pc = __popcll(s_alive[w]); s_deg[w] = off; off += pc; }    // (s_deg is free again)
    }
    __syncthreads();
    for (int w = tid; w < W; w += 1024) {
        unsigned long long x = s_alive[w];
        int o = s_deg[w];
        while (x) { rlist[o++] = w * 64 + __ffsll((long long)x) - 1; x &= x - 1; }
    }
    if (tid == 0) { c->maxcore = maxcore; c->lb = LB; c->nU = nu; c->nR = nrest; c->target = LB - nu; c->done = 0; }
}

// ---- 2b. adjacency of the remaining vertices, compact ids ------------------------------------------------------------------
__global__ void __launch_bounds__(256) tz_compact_kernel(tz_args g)
{
    const int pair = blockIdx.y;
    const tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    if (c->done) return;
    const int n = c->nR, Wn = tz_words(n), Ws = g.Wmax;
    const unsigned long long *adj = lr_ptr<unsigned long long>(g, pair, g.L.adj);
    unsigned long long *cadj = lr_ptr<unsigned long long>(g, pair, g.L.cadj);
    const int32_t *rlist = lr_ptr<int32_t>(g, pair, g.L.rlist);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const unsigned long long *row = adj + (size_t)rlist[r] * Ws;
        for (int w = threadIdx.x; w < Wn; w += 256) {
            unsigned long long x = 0;
            for (int b = 0; b < 64; ++b) {
                const int j = w * 64 + b;
                if (j >= n) break;
                const int oj = rlist[j];
                x |= ((row[oj >> 6] >> (oj & 63)) & 1ull) << b;
            }
            cadj[(size_t)r * Ws + w] = x;
        }
    }
}

// ---- 2c. exact search (one wave per pair) ------------------------------------------------------------------------------------
// lowest set bit of a bitset held as TZ_NWL words per lane (word index lane + 64 t): -1 when empty
__device__ __forceinline__ int tz_lowest(const unsigned long long (&x)[TZ_NWL], int lane)
{
    int f = 0x7fffffff;
#pragma unroll
    for (int t = TZ_NWL - 1; t >= 0; --t) if (x[t]) f = (lane + 64 * t) * 64 + __ffsll((long long)x[t]) - 1;
    for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(f, o); f = u < f ? u : f; }
    return f == 0x7fffffff ? -1 : f;
}

__global__ void __launch_bounds__(64) tz_search_kernel(tz_args g, long long node_budget, unsigned long long tick_budget)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    const int m = c->m, W = c->W, Ws = g.Wmax;
    unsigned long long *bits = lr_ptr<unsigned long long>(g, pair, g.L.bits);
    unsigned long long *inc = bits, *ubits = bits + Ws, *fin = bits + 2 * Ws;
    int32_t *clique = lr_ptr<int32_t>(g, pair, g.L.clique);
    if (m == 0) { if (lane == 0) { c->K = 0; c->exact = 1; c->nodes = 0; } return; }
    long long nodes = 0;
    int aborted = 0;
    if (!c->done) {
        const int n = c->nR, Wn = tz_words(n);
        const unsigned long long *cadj = lr_ptr<unsigned long long>(g, pair, g.L.cadj);
        unsigned long long *stack = lr_ptr<unsigned long long>(g, pair, g.L.stack);
        int32_t *cstack = lr_ptr<int32_t>(g, pair, g.L.cstack), *bestc = lr_ptr<int32_t>(g, pair, g.L.bestc);
        const int32_t *rlist = lr_ptr<int32_t>(g, pair, g.L.rlist);
        int best = c->target, found = 0;
        for (int w = lane; w < Wn; w += 64) { const int lo = w * 64; stack[w] = (n - lo >= 64) ? ~0ull : ((1ull << (n - lo)) - 1ull); }
        tz_wsync();
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        int d = 0;
        for (;;) {
            unsigned long long U[TZ_NWL], Q[TZ_NWL];
            const unsigned long long *P = stack + (size_t)d * Ws;
#pragma unroll
            for (int t = 0; t < TZ_NWL; ++t) { const int w = lane + 64 * t; U[t] = w < Wn ? P[w] : 0ull; }
            bool back = false;
            int v = tz_lowest(U, lane);
            if (v < 0) {
                if (d > best) {                                   // a larger clique: cstack[0..d)
                    best = d; found = 1;
                    for (int i = lane; i < d; i += 64) bestc[i] = cstack[i];
                }
                back = true;
            } else {
                // greedy colouring in ascending order; kmax colours, `last` = the last vertex given colour kmax
                int kmax = 0, last = -1;
                while (v >= 0) {
                    ++kmax;
#pragma unroll
                    for (int t = 0; t < TZ_NWL; ++t) Q[t] = U[t];
                    int q = v;
                    while (q >= 0) {
                        const int qw = q >> 6, qt = qw >> 6;
                        const unsigned long long qb = 1ull << (q & 63);
#pragma unroll
                        for (int t = 0; t < TZ_NWL; ++t) {
                            const int w = lane + 64 * t;
                            if (t == qt && lane == (qw & 63)) { U[t] &= ~qb; Q[t] &= ~qb; }
                            if (w < Wn) Q[t] &= ~cadj[(size_t)q * Ws + w];
                        }
                        last = q;
                        q = tz_lowest(Q, lane);
                    }
                    v = tz_lowest(U, lane);
                }
                if (d + kmax <= best) back = true;
                else {
                    if (nodes >= node_budget || __builtin_amdgcn_s_memrealtime() - t0 > tick_budget) { aborted = 1; break; }
                    ++nodes;
                    if (lane == 0) cstack[d] = last;
                    unsigned long long *Pn = stack + (size_t)(d + 1) * Ws;
                    for (int w = lane; w < Wn; w += 64) Pn[w] = P[w] & cadj[(size_t)last * Ws + w];
                    tz_wsync();
                    ++d;
                    continue;
                }
            }
            if (back) {
                --d;
                if (d < 0) break;
                const int u = cstack[d];
                if (lane == 0) stack[(size_t)d * Ws + (u >> 6)] &= ~(1ull << (u & 63));
                tz_wsync();
            }
        }
        // final clique bits
        for (int w = lane; w < W; w += 64) fin[w] = found ? ubits[w] : inc[w];
        tz_wsync();
        if (found && lane == 0)
            for (int i = 0; i < best; ++i) { const int o = rlist[bestc[i]]; fin[o >> 6] |= 1ull << (o & 63); }
        tz_wsync();
        if (lane == 0) { c->found = found; c->nbest = best; }
    }
    // ascending extraction: 64 words at a time, lane = word, exclusive prefix of popcounts
    int base = 0;
    int32_t *out = c->clique_out;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        unsigned long long x = w < W ? fin[w] : 0ull;
        const int pc = __popcll(x);
        const int incl = lr_wave_incl_scan(pc, lane);
        int o = base + incl - pc;
        while (x) { const int v = w * 64 + __ffsll((long long)x) - 1; x &= x - 1; clique[o] = v; if (out) out[o] = v; ++o; }
        base += __shfl(incl, 63);
    }
    if (lane == 0) { c->K = base; c->exact = aborted ? 0 : 1; c->nodes = (unsigned long long)nodes; }
}

// ---- 3. rotation: GNC-TLS on the chain TIMs --------------------------------------------------------------------------------
// R = argmin sum w |B - R A|^2 from H = sum w A B^T = U S V^T: R = V diag(1, 1, det(V U^T)) U^T.  One-sided Jacobi on H (columns of
// H V orthogonalised), singular values sorted descending.  Rank-deficient H (collinear or coincident points) has no unique optimum; any
// proper rotation attaining it is returned: s2 <= 1e-14 s1 (zero or rounding noise) completes u2 by an axis orthogonal to u1, s3 <= 1e-14
// s1 completes u3 = u1 x u2, and H = 0 gives R = I.  Its own routine: lr_contract.h (which RANSAC's results depend on) is not touched.
__device__ void tz_svd_rot(const double H[9], double R[9])
{
    double M[9], V[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    for (int i = 0; i < 9; ++i) M[i] = H[i];
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 3; ++r) { al += M[3 * r + p] * M[3 * r + p]; be += M[3 * r + q] * M[3 * r + q]; ga += M[3 * r + p] * M[3 * r + q]; }
                if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                const double ze = (be - al) / (2.0 * ga);
                const double t = (ze >= 0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; ++r) {
                    const double mp = M[3 * r + p], mq = M[3 * r + q];
                    M[3 * r + p] = cs * mp - sn * mq; M[3 * r + q] = sn * mp + cs * mq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = cs * vp - sn * vq; V[3 * r + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    double s[3];
    int ord[3] = { 0, 1, 2 };
    for (int j = 0; j < 3; ++j) s[j] = sqrt(M[j] * M[j] + M[3 + j] * M[3 + j] + M[6 + j] * M[6 + j]);
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) if (s[ord[j]] > s[ord[i]]) { const int tmp = ord[i]; ord[i] = ord[j]; ord[j] = tmp; }
    const double s1 = s[ord[0]];
    if (!(s1 > 0.0)) {                              // rank 0 (H = 0): every rotation attains the optimum 0
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double U[9], Vs[9];
    for (int j = 0; j < 3; ++j) {
        const int o = ord[j];
        for (int r = 0; r < 3; ++r) { Vs[3 * r + j] = V[3 * r + o]; U[3 * r + j] = s[o] > 0 ? M[3 * r + o] / s[o] : 0.0; }
    }
    if (!(s[ord[1]] > 1e-14 * s1)) {                // rank 1: the second column of H V is zero or rounding noise along u1; u2 = any unit
        int k = 0;                                  // vector orthogonal to u1, from the axis where u1 is smallest
        if (fabs(U[3]) < fabs(U[3 * k])) k = 1;
        if (fabs(U[6]) < fabs(U[3 * k])) k = 2;
        double e[3] = { 0.0, 0.0, 0.0 };
        e[k] = 1.0;
        const double dot = U[3 * k];
        double nn = 0.0;
        for (int r = 0; r < 3; ++r) { U[3 * r + 1] = e[r] - dot * U[3 * r]; nn += U[3 * r + 1] * U[3 * r + 1]; }
        nn = sqrt(nn);
        for (int r = 0; r < 3; ++r) U[3 * r + 1] /= nn;
    }
    if (!(s[ord[2]] > 1e-14 * s1)) {               // rank <= 2: u3 = u1 x u2
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
    // R = Vs diag(1,1,d) U^T, d = det(Vs) det(U)
    const double dV = Vs[0] * (Vs[4] * Vs[8] - Vs[5] * Vs[7]) - Vs[1] * (Vs[3] * Vs[8] - Vs[5] * Vs[6]) + Vs[2] * (Vs[3] * Vs[7] - Vs[4] * Vs[6]);
    const double dU = U[0] * (U[4] * U[8] - U[5] * U[7]) - U[1] * (U[3] * U[8] - U[5] * U[6]) + U[2] * (U[3] * U[7] - U[4] * U[6]);
    const double dd = (dV * dU) < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Vs[3 * i] * U[3 * j] + Vs[3 * i + 1] * U[3 * j + 1] + dd * Vs[3 * i + 2] * U[3 * j + 2];
}

#define TZ_RB 256
// fixed-order block reduction of n doubles (n <= 10): per-thread partials, then a tree
__device__ __forceinline__ void tz_reduce(double *v, int n, double (*s)[TZ_RB], bool is_max)
{
    const int tid = threadIdx.x;
    for (int i = 0; i < n; ++i) s[i][tid] = v[i];
    __syncthreads();
    for (int h = TZ_RB / 2; h >= 1; h >>= 1) {
        if (tid < h)
            for (int i = 0; i < n; ++i) s[i][tid] = is_max ? fmax(s[i][tid], s[i][tid + h]) : s[i][tid] + s[i][tid + h];
        __syncthreads();
    }
    for (int i = 0; i < n; ++i) v[i] = s[i][0];
    __syncthreads();
}

__device__ __forceinline__ double tz_res(const double *tim, size_t Mp, int k, const double *R)
{
    const double ax = tim[k], ay = tim[Mp + k], az = tim[2 * Mp + k], bx = tim[3 * Mp + k], by = tim[4 * Mp + k], bz = tim[5 * Mp + k];
    const double ex = bx - ((R[0] * ax + R[1] * ay) + R[2] * az), ey = by - ((R[3] * ax + R[4] * ay) + R[5] * az),
                 ez = bz - ((R[6] * ax + R[7] * ay) + R[8] * az);
    return (ex * ex + ey * ey) + ez * ez;
}

__global__ void __launch_bounds__(TZ_RB) tz_rot_kernel(tz_args g, double nb2, double gnc_factor, int max_iterations, double cost_threshold)
{
    __shared__ double s_red[10][TZ_RB];
    __shared__ double s_R[9];
    const int pair = blockIdx.x, tid = threadIdx.x;
    tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    const int K = c->K;
    if (K < 3) { if (tid == 0) c->status = 1; return; }
    const size_t Mp = (size_t)g.Wmax * 64;
    const int32_t *clique = lr_ptr<int32_t>(g, pair, g.L.clique);
    double *tim = lr_ptr<double>(g, pair, g.L.tim), *wgt = lr_ptr<double>(g, pair, g.L.wgt);
    const float *a = c->a, *b = c->b;
    double v[10];
    for (int i = 0; i < 10; ++i) v[i] = 0.0;
    for (int k = tid; k < K; k += TZ_RB) {
        const int c0 = clique[k], c1 = clique[k + 1 == K ? 0 : k + 1];
        const double ax = (double)a[3 * c1] - (double)a[3 * c0], ay = (double)a[3 * c1 + 1] - (double)a[3 * c0 + 1], az = (double)a[3 * c1 + 2] - (double)a[3 * c0 + 2];
        const double bx = (double)b[3 * c1] - (double)b[3 * c0], by = (double)b[3 * c1 + 1] - (double)b[3 * c0 + 1], bz = (double)b[3 * c1 + 2] - (double)b[3 * c0 + 2];
        tim[k] = ax; tim[Mp + k] = ay; tim[2 * Mp + k] = az; tim[3 * Mp + k] = bx; tim[4 * Mp + k] = by; tim[5 * Mp + k] = bz;
        wgt[k] = 1.0;
        v[0] += ax * bx; v[1] += ax * by; v[2] += ax * bz; v[3] += ay * bx; v[4] += ay * by; v[5] += ay * bz; v[6] += az * bx; v[7] += az * by; v[8] += az * bz;
    }
    tz_reduce(v, 9, s_red, false);
    if (tid == 0) tz_svd_rot(v, s_R);
    __syncthreads();
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = s_R[i];
    double mx = 0.0;
    for (int k = tid; k < K; k += TZ_RB) mx = fmax(mx, tz_res(tim, Mp, k, R));
    tz_reduce(&mx, 1, s_red, true);
    double mu = 1.0 / (2.0 * mx / nb2 - 1.0);
    int iters = 0;
    if (mu > 0.0) {
        double prev = 0.0;
        for (int it = 0; it < max_iterations; ++it) {
            const double th1 = (mu + 1.0) / mu * nb2, th2 = mu / (mu + 1.0) * nb2;
            for (int i = 0; i < 10; ++i) v[i] = 0.0;
            for (int k = tid; k < K; k += TZ_RB) {
                const double r = tz_res(tim, Mp, k, R);
                v[9] += wgt[k] * r;
                const double w = r >= th1 ? 0.0 : (r <= th2 ? 1.0 : sqrt(nb2 * mu * (mu + 1.0) / r) - mu);
                wgt[k] = w;
                const double ax = tim[k], ay = tim[Mp + k], az = tim[2 * Mp + k], bx = tim[3 * Mp + k], by = tim[4 * Mp + k], bz = tim[5 * Mp + k];
                const double wax = w * ax, way = w * ay, waz = w * az;
                v[0] += wax * bx; v[1] += wax * by; v[2] += wax * bz; v[3] += way * bx; v[4] += way * by; v[5] += way * bz; v[6] += waz * bx; v[7] += waz * by; v[8] += waz * bz;
            }
            tz_reduce(v, 10, s_red, false);
            iters = it + 1;
            mu *= gnc_factor;
            if (fabs(v[9] - prev) < cost_threshold) break;
            prev = v[9];
            if (tid == 0) tz_svd_rot(v, s_R);
            __syncthreads();
            for (int i = 0; i < 9; ++i) R[i] = s_R[i];
            __syncthreads();
        }
    }
    // rotation inliers (w >= 0.5; all when GNC did not start) -> participating clique points, ascending, and their x = b - R a
    __shared__ int s_cnt[TZ_RB / 64 + 1];
    int32_t *pidx = lr_ptr<int32_t>(g, pair, g.L.pidx);
    double *xv = lr_ptr<double>(g, pair, g.L.xv);
    int base = 0;
    for (int k0 = 0; k0 < K; k0 += TZ_RB) {
        const int k = k0 + tid;
        const bool in = k < K && (mu <= 0.0 || wgt[k] >= 0.5);
        const unsigned long long bal = __ballot(in);
        if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < (tid >> 6); ++w) off += s_cnt[w];
        off += __popcll(bal & ((1ull << (tid & 63)) - 1ull));
        if (in) {
            const int p = clique[k];
            pidx[off] = p;
            const double ax = a[3 * p], ay = a[3 * p + 1], az = a[3 * p + 2];
            xv[off] = (double)b[3 * p] - ((R[0] * ax + R[1] * ay) + R[2] * az);
            xv[Mp + off] = (double)b[3 * p + 1] - ((R[3] * ax + R[4] * ay) + R[5] * az);
            xv[2 * Mp + off] = (double)b[3 * p + 2] - ((R[6] * ax + R[7] * ay) + R[8] * az);
        }
        for (int w = 0; w < TZ_RB / 64; ++w) base += s_cnt[w];
        __syncthreads();
    }
    if (tid == 0) {
        c->gnc_iters = iters; c->n_rot = base; c->n_part = base;
        for (int i = 0; i < 9; ++i) c->R[i] = R[i];
        if (base < 3) c->status = 1;
    }
}

// ---- 4. translation: adaptive voting per axis ---------------------------------------------------------------------------------
// endpoint e of point i = e >> 1: value x_i - beta (entry, e even) or x_i + beta (exit); order (value, exit?, i).  The consensus set
// just after e is { j : key(entry_j) <= key(e) < key(exit_j) }; cost = sum_in (x - mean)^2 + beta |out| (+inf when empty).
__device__ __forceinline__ bool tz_key_le(double v1, int t1, int i1, double v2, int t2, int i2)
{
    if (v1 != v2) return v1 < v2;
    if (t1 != t2) return t1 < t2;
    return i1 <= i2;
}

__global__ void __launch_bounds__(256) tz_vote_kernel(tz_args g, double beta)
{
    __shared__ double s_x[256];
    const int pair = blockIdx.z, axis = blockIdx.y, tid = threadIdx.x;
    const tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    if (c->status) return;
    const int n = c->n_part;
    if ((int)blockIdx.x * 256 >= 2 * n) return;
    const size_t Mp = (size_t)g.Wmax * 64;
    const double *x = lr_ptr<double>(g, pair, g.L.xv) + axis * Mp;
    double *ecost = lr_ptr<double>(g, pair, g.L.ecost) + axis * 2 * Mp;
    const int e = blockIdx.x * 256 + tid;
    const bool ev = e < 2 * n;
    const int ie = e >> 1, te = e & 1;
    const double ve = ev ? (te ? x[ie] + beta : x[ie] - beta) : 0.0;
    double s1 = 0, s2 = 0;
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        if (j0 + tid < n) s_x[tid] = x[j0 + tid];
        __syncthreads();
        const int jn = n - j0 < 256 ? n - j0 : 256;
        for (int jj = 0; jj < jn; ++jj) {
            const double xj = s_x[jj];
            const int j = j0 + jj;
            if (tz_key_le(xj - beta, 0, j, ve, te, ie) && !tz_key_le(xj + beta, 1, j, ve, te, ie)) {
                const double dxj = xj - ve;
                s1 += dxj; s2 += dxj * dxj; ++cnt;
            }
        }
    }
    if (ev) ecost[e] = cnt ? (s2 - s1 * s1 / (double)cnt) + beta * (double)(n - cnt) : INFINITY;
}

__global__ void __launch_bounds__(256) tz_final_kernel(tz_args g, double beta, lr_teaser_result *results)
{
    __shared__ double s_c[256], s_v[256];
    __shared__ int s_e[256];
    __shared__ double s_red[10][TZ_RB];
    __shared__ double s_t[3];
    const int pair = blockIdx.x, tid = threadIdx.x;
    tz_ctl *c = lr_ptr<tz_ctl>(g, pair, g.L.ctl);
    lr_teaser_result *res = results + pair;
    const int status = c->status, n = c->n_part;
    const size_t Mp = (size_t)g.Wmax * 64;
    const double *xv = lr_ptr<double>(g, pair, g.L.xv);
    int ntrans = 0;
    if (!status) {
        for (int axis = 0; axis < 3; ++axis) {
            const double *x = xv + axis * Mp;
            const double *ec = lr_ptr<double>(g, pair, g.L.ecost) + axis * 2 * Mp;
            // first minimum: smallest (cost, key)
            double bc = INFINITY, bv = 0; int be = -1;
            for (int e = tid; e < 2 * n; e += 256) {
                const double ce = ec[e];
                const double ve = (e & 1) ? x[e >> 1] + beta : x[e >> 1] - beta;
                if (be < 0 || ce < bc || (ce == bc && tz_key_le(ve, e & 1, e >> 1, bv, be & 1, be >> 1))) { bc = ce; bv = ve; be = e; }
            }
            s_c[tid] = bc; s_v[tid] = bv; s_e[tid] = be;
            __syncthreads();
            for (int h = 128; h >= 1; h >>= 1) {
                if (tid < h) {
                    const int e2 = s_e[tid + h];
                    if (e2 >= 0) {
                        const double c2 = s_c[tid + h], v2 = s_v[tid + h];
                        const int e1 = s_e[tid];
                        if (e1 < 0 || c2 < s_c[tid] || (c2 == s_c[tid] && tz_key_le(v2, e2 & 1, e2 >> 1, s_v[tid], e1 & 1, e1 >> 1))) {
                            s_c[tid] = c2; s_v[tid] = v2; s_e[tid] = e2;
                        }
                    }
                }
                __syncthreads();
            }
            const int we = s_e[0];
            const double wv = s_v[0];
            __syncthreads();
            double v[2] = { 0.0, 0.0 };
            for (int j = tid; j < n; j += 256) {
                const double xj = x[j];
                if (tz_key_le(xj - beta, 0, j, wv, we & 1, we >> 1) && !tz_key_le(xj + beta, 1, j, wv, we & 1, we >> 1)) { v[0] += xj; v[1] += 1.0; }
            }
            tz_reduce(v, 2, s_red, false);
            if (tid == 0) s_t[axis] = v[0] / v[1];
            __syncthreads();
        }
        int cnt = 0;
        for (int j = tid; j < n; j += 256) {
            bool in = true;
            for (int axis = 0; axis < 3; ++axis) in = in && fabs(xv[axis * Mp + j] - s_t[axis]) <= beta;
            cnt += in ? 1 : 0;
        }
        double v[1] = { (double)cnt };
        tz_reduce(v, 1, s_red, false);
        ntrans = (int)v[0];
    }
    if (tid == 0) {
        for (int i = 0; i < 16; ++i) res->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
        if (!status) {
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) res->T[4 * i + j] = c->R[3 * i + j];
                res->T[4 * i + 3] = s_t[i];
            }
        }
        res->status = status; res->K = c->K; res->exact = c->exact; res->max_core = c->maxcore; res->lb = c->lb; res->pad0 = 0;
        res->nodes = c->nodes; res->gnc_iters = c->gnc_iters; res->n_rot_inliers = c->n_rot; res->n_trans_inliers = ntrans; res->pad1 = 0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int g_tz_timing = 0;
static hipEvent_t g_tz_ev[5];
static int g_tz_ev_ok = 0, g_tz_recorded = 0;

extern "C" size_t lr_teaser_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > TZ_MAX_M) return 0;
    return tz_make_layout(max_m).total;
}

extern "C" int lr_teaser_timing(int enable)
{
    if (enable && !g_tz_ev_ok) {
        for (int i = 0; i < 5; ++i) LR_HIP(hipEventCreate(&g_tz_ev[i]));
        g_tz_ev_ok = 1;
    }
    g_tz_timing = enable ? 1 : 0;
    g_tz_recorded = 0;
    return LR_OK;
}

extern "C" int lr_teaser_stage_times(float out[4])
{
    LR_REQUIRE(out, LR_EINVAL, "lr_teaser_stage_times: null pointer");
    LR_REQUIRE(g_tz_recorded, LR_EINVAL, "lr_teaser_stage_times: no timed call since lr_teaser_timing(1)");
    for (int i = 0; i < 4; ++i) LR_HIP(hipEventElapsedTime(&out[i], g_tz_ev[i], g_tz_ev[i + 1]));
    return LR_OK;
}

static int check_teaser_params(const lr_teaser_params *p, const char *who)
{
    LR_CHECK_STRUCT_SIZE(lr_teaser_params, p, who);
    if (!(p->noise_bound > 0.0 && isfinite(p->noise_bound))) { lr_set_error("%s: noise_bound must be positive and finite", who); return LR_EINVAL; }
    if (!(p->cbar2 > 0.0 && isfinite(p->cbar2))) { lr_set_error("%s: cbar2 must be positive and finite", who); return LR_EINVAL; }
    if (!(p->kcore_threshold > 0.0 && p->kcore_threshold <= 1.0)) { lr_set_error("%s: kcore_threshold must lie in (0, 1]", who); return LR_EINVAL; }
    if (!(p->gnc_factor > 1.0 && isfinite(p->gnc_factor))) { lr_set_error("%s: gnc_factor must be > 1 (GNC_TLS)", who); return LR_EINVAL; }
    if (p->max_iterations < 0) { lr_set_error("%s: max_iterations must be >= 0", who); return LR_EINVAL; }
    if (!(p->cost_threshold >= 0.0)) { lr_set_error("%s: cost_threshold must be >= 0", who); return LR_EINVAL; }
    if (p->node_budget < 1) { lr_set_error("%s: node_budget must be >= 1", who); return LR_EINVAL; }
    if (!(p->time_budget_ms > 0.0 && p->time_budget_ms <= 3.6e6)) { lr_set_error("%s: time_budget_ms must lie in (0, 3.6e6]", who); return LR_EINVAL; }
    if (p->rotation_tim_graph != 0 || p->estimate_scaling != 0) {
        lr_set_error("%s: only the CHAIN TIM graph without scale estimation is built (rotation_tim_graph 0, estimate_scaling 0)", who);
        return LR_EINVAL;
    }
    return LR_OK;
}

// `who`: the entry point the params messages name; the checks of the shared front have always reported as lr_teaser_batch
static int tz_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m,
                  const int32_t *const *m_dev, const lr_teaser_params *p, lr_teaser_result *results,
                  int32_t *const *clique_out, void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_teaser_batch", "npairs * lr_teaser_scratch_bytes(max m)", lr_teaser_scratch_bytes, LR_ESIZE };
    LR_TRY_HIP(check_teaser_params(p, who));
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, (void *const *)clique_out, nullptr, results, scratch, scratch_bytes, stream, &f));
    const int mx = f.mx;
    int dev = 0, khz = 0;
    LR_HIP(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    const double ticks = p->time_budget_ms * (double)khz;

    tz_args g;
    g.base = reinterpret_cast<char *>(scratch);
    g.stride = f.per;
    g.Wmax = tz_words(mx < 1 ? 1 : mx);
    g.L = tz_make_layout(mx);
    const double beta = p->noise_bound;
    const double thr = 2.0 * beta * sqrt(p->cbar2);
    const double nb2 = (2.0 * beta) * (2.0 * beta) * p->cbar2;
    hipStream_t st = (hipStream_t)stream;
    const bool tm = g_tz_timing && g_tz_ev_ok;
    if (tm) LR_HIP(hipEventRecord(g_tz_ev[0], st));
    hipLaunchKernelGGL(tz_setup_kernel, dim3(1), dim3(64), 0, st, f.t, g, npairs);
    if (mx > 0)
        hipLaunchKernelGGL(tz_graph_kernel, dim3(lr_cdiv(mx, 64), lr_cdiv(g.Wmax, 4), npairs), dim3(256), 0, st, g, thr);
    if (tm) LR_HIP(hipEventRecord(g_tz_ev[1], st));
    hipLaunchKernelGGL(tz_peel_kernel, dim3(npairs), dim3(1024), 0, st, g, p->kcore_threshold);
    hipLaunchKernelGGL(tz_compact_kernel, dim3(256, npairs), dim3(256), 0, st, g);
    hipLaunchKernelGGL(tz_search_kernel, dim3(npairs), dim3(64), 0, st, g, (long long)p->node_budget, (unsigned long long)ticks);
    if (tm) LR_HIP(hipEventRecord(g_tz_ev[2], st));
    hipLaunchKernelGGL(tz_rot_kernel, dim3(npairs), dim3(TZ_RB), 0, st, g, nb2, p->gnc_factor, p->max_iterations, p->cost_threshold);
    if (tm) LR_HIP(hipEventRecord(g_tz_ev[3], st));
    hipLaunchKernelGGL(tz_vote_kernel, dim3(lr_cdiv(2 * (mx < 1 ? 1 : mx), 256), 3, npairs), dim3(256), 0, st, g, beta);
    hipLaunchKernelGGL(tz_final_kernel, dim3(npairs), dim3(256), 0, st, g, beta, results);
    if (tm) { LR_HIP(hipEventRecord(g_tz_ev[4], st)); g_tz_recorded = 1; }
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_teaser_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m,
                               const int32_t *const *m_dev, const lr_teaser_params *p, lr_teaser_result *results,
                               int32_t *const *clique_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return tz_run("lr_teaser_batch", npairs, src, tgt, m, m_dev, p, results, clique_out, scratch, scratch_bytes, stream);
}

extern "C" int lr_teaser(const float *src, const float *tgt, int m, const int32_t *m_dev, const lr_teaser_params *p,
                         lr_teaser_result *result, int32_t *clique_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return tz_run("lr_teaser", 1, &src, &tgt, &m, &m_dev, p, result, &clique_out, scratch, scratch_bytes, stream);
}
