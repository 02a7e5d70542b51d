// Balanced-set selection (lr_balanced_select) on gfx950: the rejection loop of the reference's balanced-set generator
// (BalancedDatasetGenerator/GenerateBalancedSet.py:456-507, :544-562) as rounds of two stream-ordered launches.  Contract S is stated in
// include/lidarreg.h and DESIGN.md §15 and restated in tests/balanced_cpu.py.
//
// The loop's state -- who is alive, the columns' extremes, the sessions' counts -- changes only at a hit, and well under 1 % of the attempts
// hit.  So a round tests the next SEL_T attempts against every alive candidate at once (sel_eval_kernel: one candidate per thread, the points
// of the unit cube read from scratch, the draws wave-uniform, one integer atomicOr per wave and attempt with anybody inside thresh) and a
// single block then resolves the marked attempts in order (sel_resolve_kernel: the lexicographic minimum of (fullness, d, i) by exact
// comparison, the commit, the cursor, the stop rules).  A commit only removes a candidate, so an unmarked attempt stays a miss and a marked
// one is simply walked again over who is left -- unless the removed candidate held a column's extreme: then the extremes and every point
// are computed again and the round ends there, the next one evaluating from the attempt after it.  A call enqueues a fixed number of
// rounds; the control block's first word ends the loop: every later launch returns at its first instruction.
// No host synchronisation, no floating-point atomic, no block waits on another one; every loop is bounded by n, SEL_T or the round count.
#include "lr_scratch.h"
#include <float.h>
#include <math.h>
#include <string.h>

#define SEL_MAX_N        4194304
#define SEL_MAX_SESSIONS 65536
#ifndef SEL_T
#define SEL_T            1024         // attempts a round tests (chosen from a measurement); a multiple of SEL_TS
#endif
#define SEL_TS           64           // attempts per block of the evaluate kernel: its grid is (candidate tiles, SEL_T / SEL_TS)
#define SEL_PART_BLOCKS  256          // blocks of the extremes pass of a call's start

enum { SEL_OK = 0, SEL_DRAWS = 1, SEL_DEGENERATE = 2, SEL_BAD_SESSION = 3, SEL_ROUNDS = 4, SEL_RUNNING = -1 };

struct sel_ctl {
    int32_t done;                // first: the stop word of every kernel of the rounds
    int32_t pad;
    long long cursor;            // draws of this call consumed so far
    double pre;                  // an attempt's squared distance above this cannot be a hit (a little above thresh^2: the exact test follows)
    uint32_t hits[SEL_T / 32];   // bit t: attempt cursor + t of the round in flight has a candidate inside thresh (zero between rounds)
};

struct sel_args {
    const double *fields;        // [n][6]
    const int32_t *session;      // [n]
    const int32_t *n_cands;      // [n_sessions]
    const double *draws;         // [n_draws][6]
    uint8_t *alive;              // [n]
    int32_t *n_sel;              // [n_sessions]
    int32_t *out;                // [n_request]
    lr_select_result *res;
    sel_ctl *ctl;
    double *part;                // [SEL_PART_BLOCKS][16]: lo[6] hi[6] bad invalid alive-count
    double *pts;                 // [6][n_pad]
    size_t n_pad;
    long long n_draws;
    double thresh;
    int n, n_sessions, n_request, resume, rounds;
};

// the point of candidate i in the unit cube, column c (S1): both operations correctly rounded
__device__ __forceinline__ double sel_point(double f, double lo, double hi) { return __ddiv_rn(f - lo, hi - lo); }

// d of one attempt (S2): numpy's order for six terms
__device__ __forceinline__ double sel_sumsq(const double *__restrict__ r, const double p[6])
{
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double e = r[c] - p[c];
        const double q = e * e;
        s = c == 0 ? q : s + q;
    }
    return s;
}

// ---- extremes of the alive candidates over a block ---------------------------------------------------------------------------------
// acc[0..5] least, acc[6..11] greatest finite value per column, acc[12] > 0: an alive candidate has a non-finite field, acc[13] > 0: a
// session id out of range or without candidates, acc[14]: alive candidates (exact: counts below 2^53)
struct sel_acc { double v[15]; };

__device__ __forceinline__ void sel_acc_init(sel_acc &a)
{
    for (int c = 0; c < 6; ++c) { a.v[c] = INFINITY; a.v[6 + c] = -INFINITY; }
    a.v[12] = 0.0; a.v[13] = 0.0; a.v[14] = 0.0;
}
__device__ __forceinline__ void sel_acc_merge(sel_acc &a, const double *b)
{
    for (int c = 0; c < 6; ++c) { a.v[c] = fmin(a.v[c], b[c]); a.v[6 + c] = fmax(a.v[6 + c], b[6 + c]); }
    a.v[12] += b[12]; a.v[13] += b[13]; a.v[14] += b[14];
}
__device__ __forceinline__ void sel_acc_point(sel_acc &a, const double *__restrict__ f)
{
    for (int c = 0; c < 6; ++c) {
        const double x = f[c];
        if (isfinite(x)) { a.v[c] = fmin(a.v[c], x); a.v[6 + c] = fmax(a.v[6 + c], x); }
        else a.v[12] = 1.0;
    }
    a.v[14] += 1.0;
}
// the block's merged accumulator in s[0..15) (s: 16 * (blockDim.x / 64) doubles + 16); every thread must call
__device__ __forceinline__ void sel_acc_block(sel_acc &a, double *s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = (int)blockDim.x >> 6;
    for (int k = 0; k < 15; ++k) {
        double x = a.v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double o = __shfl_xor(x, m);
            x = k < 6 ? fmin(x, o) : (k < 12 ? fmax(x, o) : x + o);
        }
        if (lane == 0) s[16 + wave * 16 + k] = x;
    }
    __syncthreads();
    if (tid < 15) {
        double x = s[16 + tid];
        for (int w = 1; w < waves; ++w) {
            const double o = s[16 + w * 16 + tid];
            x = tid < 6 ? fmin(x, o) : (tid < 12 ? fmax(x, o) : x + o);
        }
        s[tid] = x;
    }
    __syncthreads();
}
// S's deviation: every column's greatest minus least must be a positive finite number
__device__ __forceinline__ bool sel_degenerate(const double *acc)
{
    if (acc[12] > 0.0) return true;
    for (int c = 0; c < 6; ++c) { const double w = acc[6 + c] - acc[c]; if (!(w > 0.0) || !isfinite(w)) return true; }
    return false;
}

// ---- the start of a call ------------------------------------------------------------------------------------------------------------
// (1) a fresh call makes every candidate alive and every session empty; both kinds take the alive candidates' extremes per block
__global__ __launch_bounds__(256) void sel_begin_kernel(sel_args g)
{
    __shared__ double s[16 * 5];
    sel_acc a;
    sel_acc_init(a);
    const int stride = (int)gridDim.x * 256;
    if (!g.resume) for (int t = (int)blockIdx.x * 256 + (int)threadIdx.x; t < g.n_sessions; t += stride) g.n_sel[t] = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.n; i += stride) {
        if (!g.resume) g.alive[i] = 1;
        const int sid = g.session[i];
        if (sid < 0 || sid >= g.n_sessions || g.n_cands[sid] < 1) { a.v[13] = 1.0; continue; }
        if (g.alive[i]) sel_acc_point(a, g.fields + 6 * (size_t)i);
    }
    sel_acc_block(a, s);
    if (threadIdx.x < 16) g.part[(size_t)blockIdx.x * 16 + threadIdx.x] = threadIdx.x < 15 ? s[threadIdx.x] : 0.0;
}

// (2) one block: the extremes, the call's control block, the stop rules that hold before the first attempt
__global__ __launch_bounds__(256) void sel_setup_kernel(sel_args g, int blocks)
{
    __shared__ double s[16 * 5];
    sel_acc a;
    sel_acc_init(a);
    for (int b = threadIdx.x; b < blocks; b += 256) sel_acc_merge(a, g.part + (size_t)b * 16);
    sel_acc_block(a, s);
    if (threadIdx.x != 0) return;
    lr_select_result *r = g.res;
    if (!g.resume) { r->n_selected = 0; r->attempts = 0; r->misses = 0; r->rounds = 0; r->rescales = 0; }
    r->consumed = 0;
    for (int c = 0; c < 6; ++c) { r->lo[c] = s[c]; r->hi[c] = s[6 + c]; }
    int status = SEL_RUNNING;
    if (s[13] > 0.0) status = SEL_BAD_SESSION;
    else if (r->n_selected < 0 || r->n_selected > g.n_request || (double)r->n_selected + s[14] != (double)g.n) status = SEL_BAD_SESSION;   // a resumed state that is none
    else if (g.n_request == 0 || r->n_selected == g.n_request) status = SEL_OK;
    else if (sel_degenerate(s)) status = SEL_DEGENERATE;
    else if (g.n_draws == 0) status = SEL_DRAWS;
    r->status = status;
    sel_ctl *c = g.ctl;
    c->cursor = 0;
    for (int w = 0; w < SEL_T / 32; ++w) c->hits[w] = 0;
    c->pre = fmax(g.thresh * g.thresh * (1.0 + 1e-7), DBL_MIN);
    c->done = status != SEL_RUNNING;
}

// (3) the points of every candidate, column by column
__global__ __launch_bounds__(256) void sel_points_kernel(sel_args g)
{
    if (g.ctl->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const lr_select_result *r = g.res;
#pragma unroll
    for (int c = 0; c < 6; ++c) g.pts[(size_t)c * g.n_pad + i] = sel_point(g.fields[6 * (size_t)i + c], r->lo[c], r->hi[c]);
}

// ---- a round: evaluate ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sel_eval_kernel(sel_args g)
{
    const sel_ctl *ctl = g.ctl;
    if (ctl->done) return;
    const long long cursor = ctl->cursor;
    const long long left = g.n_draws - cursor;
    const int count = left < SEL_T ? (int)left : SEL_T;
    const int t0 = (int)blockIdx.y * SEL_TS;
    const int t1 = min(t0 + SEL_TS, count);
    if (t0 >= t1) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < g.n && g.alive[i];
    if (__ballot(live) == 0ull) return;
    double p[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) p[c] = live ? g.pts[(size_t)c * g.n_pad + i] : 0.0;
    const double pre = ctl->pre, thresh = g.thresh;
    const double *__restrict__ r = g.draws + 6 * (size_t)(cursor + t0);
    uint32_t *hits = g.ctl->hits;
    for (int t = t0; t < t1; ++t, r += 6) {
        const double s = sel_sumsq(r, p);
        bool hit = live && !(s > pre);
        if (hit) hit = __dsqrt_rn(s) < thresh;
        if (__ballot(hit) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&hits[t >> 5], 1u << (t & 31));
    }
}

// ---- a round: resolve ------------------------------------------------------------------------------------------------------------------
struct sel_key { double fullness, d; int32_t i; };
__device__ __forceinline__ bool sel_less(const sel_key &a, const sel_key &b)
{
    if (a.i < 0 || b.i < 0) return b.i < 0 && a.i >= 0;
    if (a.fullness != b.fullness) return a.fullness < b.fullness;
    if (a.d != b.d) return a.d < b.d;
    return a.i < b.i;
}

__global__ __launch_bounds__(1024) void sel_resolve_kernel(sel_args g, int round)
{
    __shared__ double s_acc[16 * 17];
    __shared__ sel_key s_key[16];
    __shared__ uint32_t s_hits[SEL_T / 32];
    __shared__ double s_ext[12];
    __shared__ int s_flag;                               // what thread 0 decided at a marked attempt: bit 0 rescale, bit 1 the request is met
    sel_ctl *ctl = g.ctl;
    if (ctl->done) return;
    lr_select_result *res = g.res;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long cursor = ctl->cursor;
    const long long left = g.n_draws - cursor;
    const int count = left < SEL_T ? (int)left : SEL_T;
    const double pre = ctl->pre;
    for (int w = tid; w < SEL_T / 32; w += 1024) { s_hits[w] = ctl->hits[w]; ctl->hits[w] = 0; }
    if (tid < 12) s_ext[tid] = tid < 6 ? res->lo[tid] : res->hi[tid - 6];       // (they stand as long as the round goes on)
    int n_selected = res->n_selected;                    // (thread 0's copy is the one that is written back)
    __syncthreads();
    int used = count, commits = 0;                       // (thread 0's count of commits is the one that is written)
    bool degenerate = false;
    for (int t = 0; t < count; ++t) {
        // the next marked attempt at or after t: every thread finds the same one
        int w = t >> 5;
        uint32_t m = s_hits[w] & (0xffffffffu << (t & 31));
        while (m == 0 && ++w < SEL_T / 32) m = s_hits[w];
        if (m == 0) break;
        t = w * 32 + __ffs(m) - 1;
        if (t >= count) break;
        double r[6];
        for (int c = 0; c < 6; ++c) r[c] = g.draws[6 * (size_t)(cursor + t) + c];
        sel_key best; best.fullness = 0.0; best.d = 0.0; best.i = -1;
        // (the square root only where the sum is not above the bound the evaluate kernel uses)
        for (long long i = tid; i < g.n; i += 1024) {
            if (!g.alive[i]) continue;
            double p[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) p[c] = g.pts[(size_t)c * g.n_pad + i];
            const double s = sel_sumsq(r, p);
            if (s > pre) continue;
            const double d = __dsqrt_rn(s);
            if (!(d < g.thresh)) continue;
            const int sid = g.session[i];
            sel_key k; k.fullness = __ddiv_rn((double)g.n_sel[sid], (double)g.n_cands[sid]); k.d = d; k.i = (int32_t)i;
            if (sel_less(k, best)) best = k;
        }
#pragma unroll
        for (int mm = 32; mm >= 1; mm >>= 1) {
            sel_key o; o.fullness = __shfl_xor(best.fullness, mm); o.d = __shfl_xor(best.d, mm); o.i = __shfl_xor(best.i, mm);
            if (sel_less(o, best)) best = o;
        }
        if (lane == 0) s_key[wave] = best;
        __syncthreads();
        if (tid == 0) {
            best = s_key[0];
            for (int q = 1; q < 16; ++q) if (sel_less(s_key[q], best)) best = s_key[q];
            int flag = 0;
            const int sel = best.i;
            if (sel >= 0) {                               // (none: the candidates that marked the attempt are gone -- a miss)
                const int sid = g.session[sel];
                double f[6];
                for (int c = 0; c < 6; ++c) f[c] = g.fields[6 * (size_t)sel + c];      // (loads first: one trip to memory, not one per store)
                const int had = g.n_sel[sid];
                g.alive[sel] = 0;
                g.n_sel[sid] = had + 1;
                g.out[n_selected] = sel;
                ++n_selected;
                ++commits;
                for (int c = 0; c < 6; ++c) if (f[c] == s_ext[c] || f[c] == s_ext[6 + c]) flag |= 1;
                if (n_selected >= g.n_request) flag |= 2;
            }
            s_flag = flag;
        }
        __syncthreads();
        const int flag = s_flag;
        if (flag & 1) {
            // the removed candidate held an extreme: the extremes of the rest (order-independent, so exact), then every point again
            sel_acc a;
            sel_acc_init(a);
            for (long long i = tid; i < g.n; i += 1024) if (g.alive[i]) sel_acc_point(a, g.fields + 6 * (size_t)i);
            sel_acc_block(a, s_acc);
            degenerate = sel_degenerate(s_acc);
            if (!degenerate && !(flag & 2)) {
                for (long long i = tid; i < g.n; i += 1024) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) g.pts[(size_t)c * g.n_pad + i] = sel_point(g.fields[6 * (size_t)i + c], s_acc[c], s_acc[6 + c]);
                }
            }
            if (tid == 0) {
                bool moved = false;
                for (int c = 0; c < 6; ++c) {
                    if (s_acc[c] != res->lo[c] || s_acc[6 + c] != res->hi[c]) moved = true;
                    res->lo[c] = s_acc[c]; res->hi[c] = s_acc[6 + c];
                }
                if (moved && !degenerate) res->rescales += 1;                  // (a commit that ends in status 2 counts none)
            }
        }
        if (flag) { used = t + 1; break; }               // the marks after t were made with other points, or nothing more is wanted
    }
    if (tid != 0) return;
    res->n_selected = n_selected;
    res->attempts += used; res->consumed += used; res->rounds += 1;
    res->misses += used - commits;
    ctl->cursor = cursor + used;
    int status = SEL_RUNNING;
    if (degenerate) status = SEL_DEGENERATE;
    else if (res->n_selected >= g.n_request) status = SEL_OK;
    else if (ctl->cursor >= g.n_draws) status = SEL_DRAWS;
    else if (round + 1 >= g.rounds) status = SEL_ROUNDS;
    if (status != SEL_RUNNING) { res->status = status; ctl->done = 1; }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_select_params) == 24 && sizeof(lr_select_result) == 136,
              "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");
static_assert(sizeof(sel_ctl) <= 1024, "sel_ctl outgrew its slot");
static_assert(SEL_T % SEL_TS == 0 && SEL_T >= SEL_TS, "a round is a whole number of evaluate blocks");

struct sel_layout { size_t ctl, part, pts, n_pad, total; };
static size_t sel_make_layout(sel_layout *L, size_t n)
{
    L->n_pad = (n + 31) & ~(size_t)31;                       // columns of the points start 256-byte aligned
    L->ctl = 0;
    L->part = 1024;
    L->pts = L->part + (size_t)SEL_PART_BLOCKS * 16 * sizeof(double);
    L->total = lr_al(L->pts + 6 * L->n_pad * sizeof(double));
    return L->total;
}

extern "C" size_t lr_balanced_select_scratch_bytes(int n)
{
    if (n < 0 || n > SEL_MAX_N) return 0;
    sel_layout L;
    return sel_make_layout(&L, (size_t)n);
}

// rounds that always suffice: a round commits a selection or consumes SEL_T draws (or the rest of them)
static long long sel_rounds_needed(long long n_draws, int n_request)
{
    if (n_request == 0) return 0;
    const long long full = (long long)n_request + (n_draws + SEL_T - 1) / SEL_T;
    return full < n_draws ? full : n_draws;
}

extern "C" int lr_balanced_select(const double *fields, const int32_t *session, const int32_t *n_cands, int n, int n_sessions,
                                  const double *draws, long long n_draws, const lr_select_params *p, uint8_t *alive, int32_t *n_sel,
                                  int32_t *out, lr_select_result *result, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_balanced_select";
    LR_CHECK_STRUCT_SIZE(lr_select_params, p, who);
    LR_REFUSE_UNLESS(n >= 0 && n <= SEL_MAX_N, LR_EINVAL, "n must lie in 0..4194304");
    LR_REFUSE_UNLESS(n_sessions >= 1 && n_sessions <= SEL_MAX_SESSIONS, LR_EINVAL, "n_sessions must lie in 1..65536");
    LR_REFUSE_UNLESS(p->thresh > 0.0 && isfinite(p->thresh), LR_EINVAL, "thresh must be positive and finite");
    LR_REFUSE_UNLESS(p->n_request >= 0 && p->n_request <= n, LR_EINVAL, "n_request must lie in 0..n");
    LR_REFUSE_UNLESS(n_draws >= 0 && n_draws <= (1ll << 40), LR_EINVAL, "n_draws must lie in 0..2^40");
    LR_REFUSE_UNLESS(p->max_rounds >= 0 && p->max_rounds <= LR_SELECT_MAX_ROUNDS, LR_EINVAL, "max_rounds must lie in 0..65536 (0: as many as the draws can need)");
    LR_REFUSE_UNLESS(p->resume == 0 || p->resume == 1, LR_EINVAL, "resume must be 0 or 1");
    LR_REFUSE_UNLESS(n == 0 || fields, LR_EINVAL, "null fields");
    LR_REFUSE_UNLESS(n == 0 || session, LR_EINVAL, "null session");
    LR_REFUSE_UNLESS(n_cands, LR_EINVAL, "null n_cands");
    LR_REFUSE_UNLESS(n_draws == 0 || draws, LR_EINVAL, "null draws");
    LR_REFUSE_UNLESS(n == 0 || alive, LR_EINVAL, "null alive");
    LR_REFUSE_UNLESS(n_sel, LR_EINVAL, "null n_sel");
    LR_REFUSE_UNLESS(p->n_request == 0 || out, LR_EINVAL, "null out");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    long long rounds = sel_rounds_needed(n_draws, p->n_request);
    if (p->max_rounds > 0 && rounds > p->max_rounds) rounds = p->max_rounds;
    LR_REFUSE_UNLESS(rounds <= LR_SELECT_MAX_ROUNDS, LR_EINVAL, "these draws can need more than 65536 rounds: pass fewer draws per call, or set max_rounds");
    sel_layout L;
    const size_t need = sel_make_layout(&L, (size_t)n);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, need, "lr_balanced_select_scratch_bytes(n)", LR_EINVAL, stream, nullptr));
    sel_args g;
    memset(&g, 0, sizeof g);
    char *base = reinterpret_cast<char *>(scratch);
    g.fields = fields; g.session = session; g.n_cands = n_cands; g.draws = draws; g.alive = alive; g.n_sel = n_sel; g.out = out; g.res = result;
    g.ctl = reinterpret_cast<sel_ctl *>(base + L.ctl); g.part = reinterpret_cast<double *>(base + L.part);
    g.pts = reinterpret_cast<double *>(base + L.pts); g.n_pad = L.n_pad;
    g.n_draws = n_draws; g.thresh = p->thresh; g.n = n; g.n_sessions = n_sessions; g.n_request = p->n_request; g.resume = p->resume;
    g.rounds = (int)rounds;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = lr_cdiv(n > 0 ? n : 1, 256);
    const int pb = tiles < SEL_PART_BLOCKS ? tiles : SEL_PART_BLOCKS;
    hipLaunchKernelGGL(sel_begin_kernel, dim3(pb), dim3(256), 0, st, g);
    hipLaunchKernelGGL(sel_setup_kernel, dim3(1), dim3(256), 0, st, g, pb);
    hipLaunchKernelGGL(sel_points_kernel, dim3(tiles), dim3(256), 0, st, g);
    for (int k = 0; k < g.rounds; ++k) {
        hipLaunchKernelGGL(sel_eval_kernel, dim3(tiles, SEL_T / SEL_TS), dim3(256), 0, st, g);
        hipLaunchKernelGGL(sel_resolve_kernel, dim3(1), dim3(1024), 0, st, g, k);
    }
    LR_LAUNCH_CHECK();
    return LR_OK;
}
