// RANSAC on gfx950: local optimisation of a new best model (GC-RANSAC, --GC_LO) + the final polish.  Runs behind ransac_final_kernel
// (lr_ransac.hip), on the running state that kernel merged the batch into.
//
// One block of 1024 threads per pair; see oracle/oracle.c (lo_optimise / lo_polish) for the algorithm and its sources.
//   mode 0 (after a batch whose winner became the best model): <= LR_LO_ROUNDS rounds of { inlier list of the model; LR_LO_TRIALS
//          least-squares fits on LR_LO_SAMPLE inliers each (all of them when there are no more: one fit); every fit scored over
//          ALL correspondences by 1024 / trials threads; the best replaces the model if strictly better, else stop }, then the
//          confidence test on the optimised model
//   mode 1 (once, after the last batch): iterated least squares over all inliers
// All sums that decide anything are integers (order independent); the fp64 moments of the all-inlier fits run as 1024 strided
// partials + a fixed halving tree, the order oracle.c reproduces, so the models agree bit for bit.
#include "lr_ransac_dev.h"
#define LO_THREADS 1024

#define LO_MAXIT 32              // records (two correspondences) per thread and pass of the list builder
struct lo_shared {
    double T[LR_LO_TRIALS][12];         // candidate models of the round (fp64)
    __attribute__((aligned(16))) float Rt[LR_LO_TRIALS][12];         // ... rounded for the scoring arithmetic
    float pts[LR_LO_TRIALS][LR_LO_SAMPLE][6];     // the sampled correspondences (fetched by one lane each, summed by one thread per trial)
    unsigned cnt[LR_LO_TRIALS];
    unsigned long long ssq[LR_LO_TRIALS];
    double red[4][LO_THREADS];       // block reduction of the fp64 moments, four components at a time
    double mom[16];
    double curT[12];                 // model under optimisation
    unsigned long long curq;
    unsigned curc;
    int wcnt[LO_MAXIT][LO_THREADS / 64];    // inliers per (step, wave) of a list-builder pass, then their offsets in the list
    int wsum[16];
    int nI, flag;
    // near-inlier bound of a round (see lo_build_list): bounding box of the source points, how many correspondences lie within
    // thr + LO_NEAR_CAP of the model under optimisation, whether the round's trial models may be scored over those alone
    float box[6];
    int box_state;                   // 0: not computed yet; 1: valid; -1: a non-finite coordinate (no bound)
    int nNear, near_ok;
    double eps[LR_LO_TRIALS];
    double baseT[12];                // the model near8 was copied around
};

// inliers of sh.curT over the m correspondences, in index order -> list[0 .. sh.nI).
// A thread tests the two correspondences of one 64-byte record per step (three 16-byte loads, the packed arithmetic of the
// scoring kernel: same fma order per component).  A pass covers LO_MAXIT * LO_THREADS records: every thread runs its LO_MAXIT steps
// back to back (independent loads, no barrier in between), keeping the outcomes as a bit mask; the per-(step, wave) counts go to
// LDS, one block-wide exclusive scan turns them into list offsets, and the threads write their inliers.  Four barriers per pass.
//
// NEAR (OUT = 1; the rounds of mode 0): the trial models of a round are least-squares fits over subsets of the current model's inliers, i.e.
// close to it.  For two models t, b and a correspondence (p, q):  |T_t p - q| >= |T_b p - q| - |T_t p - T_b p| >= r_b - eps_t,
//     eps_t = |R_t - R_b|_F rho + |(R_t - R_b) c + t_t - t_b|          (c, rho: centre and half diagonal of the source points' bounding box)
// so (p, q) can be an inlier of t only if r_b < thr + eps_t -- the bound of the pilot-ordered scoring (ransac_order_kernel) with the model
// the optimisation started from as the pilot.  With OUT = 1 the pass copies the correspondences with r_b < (1 + LO_NEAR_CAP) thr, IN INDEX
// ORDER, to `near8` (corr8's record layout) instead of listing the inliers, and reduces the bounding box.  Everything a round does then
// runs over near8 alone -- about a quarter of the list on the balanced-set surrogates -- as long as every model involved stays within
// eps + slack <= LO_NEAR_CAP thr of the base model (checked in fp64 after the fits; otherwise the round scores everything and the next
// one starts from a fresh copy): the inlier list (the same call with OUT = 0 over near8: the same correspondences in the same order, so
// the samples of the trials are the oracle's), the 21-point fits, and the scoring of the 20 trials (113 -> ~30 us per round).  Counts and
// error sums are integer sums over inliers, which all lie in near8: the same integers as a scan of everything (tests/test_gpu_gc.py,
// tools/soak_gc.py against the oracle, which scores all).
#define LO_NEAR_CAP 0.5f
template <int OUT>
__device__ void lo_build_list(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2, int32_t *__restrict__ list, float *__restrict__ near8 = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool want_box = OUT == 1 && sh.box_state == 0;
    float bmn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, bmx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    bool bad = false;
    const lr_model12x2 S(sh.curT);
    const int nrec = (m + 1) >> 1;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int total = 0;
    for (int sbase = 0; sbase < nrec; sbase += LO_MAXIT * LO_THREADS) {
        const int nit = min(LO_MAXIT, (nrec - sbase + LO_THREADS - 1) / LO_THREADS);
        unsigned long long bits = 0ull;          // bit 2 it + b: correspondence b of the record of step it
#pragma unroll 2
        for (int it = 0; it < nit; ++it) {
            const int r = sbase + it * LO_THREADS + tid;
            const f32x4 *rec = reinterpret_cast<const f32x4 *>(corr8) + (size_t)min(r, nrec - 1) * 4;
            const f32x4 A = rec[0], B = rec[1], C = rec[2];
            f32x2 o[6];
            lr_record_operands(A, B, C, o);
            const f32x2 d2 = lr_d2x2(S, o);
            const bool in0 = r < nrec && d2.x < thr2, in1 = r < nrec && 2 * r + 1 < m && d2.y < thr2;
            bits |= (unsigned long long)((in0 ? 1u : 0u) | (in1 ? 2u : 0u)) << (2 * it);
            if (want_box && r < nrec) {
                bmn[0] = fminf(bmn[0], A.x); bmx[0] = fmaxf(bmx[0], A.x); bmn[1] = fminf(bmn[1], A.z); bmx[1] = fmaxf(bmx[1], A.z);
                bmn[2] = fminf(bmn[2], B.x); bmx[2] = fmaxf(bmx[2], B.x);
                const float s0 = A.x + A.z + B.x;
                bad = bad || !(s0 - s0 == 0.0f);
                if (2 * r + 1 < m) {
                    bmn[0] = fminf(bmn[0], A.y); bmx[0] = fmaxf(bmx[0], A.y); bmn[1] = fminf(bmn[1], A.w); bmx[1] = fmaxf(bmx[1], A.w);
                    bmn[2] = fminf(bmn[2], B.y); bmx[2] = fmaxf(bmx[2], B.y);
                    const float s1 = A.y + A.w + B.y;
                    bad = bad || !(s1 - s1 == 0.0f);
                }
            }
        }
        for (int it = 0; it < nit; ++it) {
            const unsigned long long b0 = __ballot((bits >> (2 * it)) & 1ull), b1 = __ballot((bits >> (2 * it + 1)) & 1ull);
            if (lane == 0) sh.wcnt[it][wave] = __popcll(b0) + __popcll(b1);
        }
        __syncthreads();
        // exclusive scan over the entries e = step * 16 + wave (the order of the correspondence indices), one entry per thread
        int *flat = &sh.wcnt[0][0];
        const int ne = nit * (LO_THREADS / 64);
        const int v = tid < ne ? flat[tid] : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
        if (lane == 63) sh.wsum[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LO_THREADS / 64; ++w) { const int x = sh.wsum[w]; all += x; if (w < wave) before += x; }
        if (tid < ne) flat[tid] = total + before + inc - v;
        __syncthreads();
        for (int it = 0; it < nit; ++it) {
            const bool in0 = (bits >> (2 * it)) & 1ull, in1 = (bits >> (2 * it + 1)) & 1ull;
            const unsigned long long b0 = __ballot(in0), b1 = __ballot(in1);
            const int pos = sh.wcnt[it][wave] + (int)__popcll(b0 & lt) + (int)__popcll(b1 & lt);
            const int r = sbase + it * LO_THREADS + tid;
            if constexpr (OUT == 0) {
                if (in0) list[pos] = 2 * r;
                if (in1) list[pos + (in0 ? 1 : 0)] = 2 * r + 1;
            } else if (in0 || in1) {
                // (the record again: it is in L2; keeping LO_MAXIT records in registers across the scan is not an option)
                const f32x4 *rec = reinterpret_cast<const f32x4 *>(corr8) + (size_t)r * 4;
                const f32x4 A = rec[0], B = rec[1], C = rec[2];
                if (in0) { const float w0[6] = { A.x, A.z, B.x, B.z, C.x, C.z };
#pragma unroll
                           for (int k = 0; k < 6; ++k) near8[lr_corr_at(pos, k)] = w0[k]; }
                if (in1) { const float w1[6] = { A.y, A.w, B.y, B.w, C.y, C.w }; const int p1 = pos + (in0 ? 1 : 0);
#pragma unroll
                           for (int k = 0; k < 6; ++k) near8[lr_corr_at(p1, k)] = w1[k]; }
            }
        }
        total += all;
        __syncthreads();          // (the next pass rewrites wcnt / wsum)
    }
    if (tid == 0) { if (OUT == 0) sh.nI = total; else sh.nNear = total; }
    if (want_box) {
        // bounding box of the source points (and "all finite"): wave shuffles, then one thread per component over the waves
        float *scr = reinterpret_cast<float *>(&sh.red[0][0]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { bmn[k] = fminf(bmn[k], __shfl_xor(bmn[k], o)); bmx[k] = fmaxf(bmx[k], __shfl_xor(bmx[k], o)); }
        }
        const bool wbad = __ballot(bad) != 0ull;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { scr[wave * 8 + k] = bmn[k]; scr[wave * 8 + 3 + k] = bmx[k]; }
            scr[wave * 8 + 6] = wbad ? 1.0f : 0.0f;
        }
        __syncthreads();
        if (tid < 7) {
            float v = scr[tid];
            for (int w = 1; w < LO_THREADS / 64; ++w) v = tid < 3 ? fminf(v, scr[w * 8 + tid]) : fmaxf(v, scr[w * 8 + tid]);
            if (tid < 6) sh.box[tid] = v; else sh.box_state = v > 0.0f ? -1 : 1;
        }
    }
    __syncthreads();
}

// least-squares fit over the listed correspondences -> sh.T[0] / sh.Rt[0]; false when fewer than 3 points
__device__ bool lo_fit_all(lo_shared &sh, const float *__restrict__ corr8, const int32_t *__restrict__ list, int n)
{
    const int tid = threadIdx.x;
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.0;
    for (int e = tid; e < n; e += LO_THREADS) {
        const int i = list[e];
        const double p[3] = { (double)corr8[lr_corr_at(i, 0)], (double)corr8[lr_corr_at(i, 1)], (double)corr8[lr_corr_at(i, 2)] };
        const double q[3] = { (double)corr8[lr_corr_at(i, 3)], (double)corr8[lr_corr_at(i, 4)], (double)corr8[lr_corr_at(i, 5)] };
        v[0] += 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { v[1 + a] += p[a]; v[4 + a] += q[a]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] += p[a] * q[b];
    }
    // halving tree red[t] += red[t + s], s = 512 ... 1 (the order oracle.c reproduces): through LDS while the partners sit in
    // different waves, by shuffles inside wave 0 for s <= 32 (the same additions, no barriers)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) sh.red[k][tid] = v[4 * g + k];
        for (int sft = LO_THREADS / 2; sft >= 64; sft >>= 1) {
            __syncthreads();
            if (tid < sft) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sh.red[k][tid] += sh.red[k][tid + sft];
            }
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double x = sh.red[k][tid];
#pragma unroll
                for (int sft = 32; sft >= 1; sft >>= 1) x = x + __shfl_down(x, sft);
                if (tid == 0) sh.mom[4 * g + k] = x;
            }
        }
    }
    __syncthreads();
    const bool ok = sh.mom[0] >= 3.0;
    if (ok && tid == 0) {
        double T[16];
        lr_rt_from_moments(sh.mom, T);
        for (int k = 0; k < 12; ++k) { sh.T[0][k] = T[k]; sh.Rt[0][k] = (float)T[k]; }
    }
    __syncthreads();
    return ok;
}

// score sh.Rt[0 .. ntrial) over all m correspondences -> sh.cnt / sh.ssq (integer atomics in LDS): three forms.
// One model (the polish, or a round with at most LR_LO_SAMPLE inliers): one thread per 64-byte record (two correspondences), 32-bit sums
// per thread (the caller guarantees that a thread's share of the correspondences cannot overflow them), one wave reduction and one
// LDS atomic per wave at the end.
__device__ void lo_score_one(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < LR_LO_TRIALS) { sh.cnt[tid] = 0u; sh.ssq[tid] = 0ull; }
    __syncthreads();
    const lr_model12x2 S(sh.Rt[0]);
    const int nrec = (m + 1) >> 1;
    uint32_t c = 0u, q = 0u;
    // the record walk of lo_build_list (three 16-byte loads per 64-byte record, both correspondences in one packed chain; the scalar
    // form -- 24 strided 4-byte loads per step -- kept the texture addresser busy for 76 us per call at 30k correspondences)
#pragma unroll 4
    for (int r = tid; r < nrec; r += LO_THREADS) {
        const f32x4 *rec = reinterpret_cast<const f32x4 *>(corr8) + (size_t)r * 4;
        const f32x4 A = rec[0], B = rec[1], C = rec[2];
        f32x2 o[6];
        lr_record_operands(A, B, C, o);
        const f32x2 d2 = lr_d2x2(S, o);
        lr_add_pair(d2, d2.x < thr2, 2 * r + 1 < m && d2.y < thr2, c, q);
    }
    unsigned long long qq = q;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c += (uint32_t)__shfl_xor((int)c, o); qq += __shfl_xor(qq, o); }
    if (lane == 0 && c) { atomicAdd(&sh.cnt[0], c); atomicAdd(&sh.ssq[0], qq); }
    __syncthreads();
}

// all LR_LO_TRIALS models of a round: the arithmetic of ransac_score_kernel (one LANE per model, two correspondences per packed
// step), with three correspondence streams side by side in a wave -- lanes [20 s, 20 s + 20) apply the 20 models to the records
// 3 w + s, 3 w + s + 48, ... of wave w -- so 60 of the 64 lanes work and a wave's three 64-byte records come in as three
// broadcast global_load_dwordx4 per lane.  12 coefficient + 12 record registers, sums per lane, 48 LDS atomics per model at the end.
__device__ void lo_score_lanes_range(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2, int rec_begin, int rec_end)
{
    // (adds to sh.cnt / sh.ssq: the caller zeroes them; records [rec_begin, rec_end))
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NS = 64 / LR_LO_TRIALS;                 // streams per wave (3)
    constexpr int STRIDE = NS * (LO_THREADS / 64);     // records between two steps of a stream (48)
    const int t = lane % LR_LO_TRIALS, st = lane / LR_LO_TRIALS;
    const bool act = st < NS;
    const lr_model12x2 S(sh.Rt[t]);
    uint32_t c = 0u;
    unsigned long long q = 0ull;
    const int first = rec_begin + wave * NS + (act ? st : 0);
    const int span = rec_end - rec_begin - wave * NS;
    const int steps = span > 0 ? (span + STRIDE - 1) / STRIDE : 0;        // (wave-uniform: the steps of the wave's first stream)
#pragma unroll 2
    for (int k = 0; k < steps; ++k) {
        const int r = first + k * STRIDE;
        const bool live = act && r < rec_end;
        const f32x4 *rec = reinterpret_cast<const f32x4 *>(corr8) + (size_t)(live ? r : 0) * 4;
        const f32x4 A = rec[0], B = rec[1], C = rec[2];
        f32x2 o[6];
        lr_record_operands(A, B, C, o);
        const f32x2 d2 = lr_d2x2(S, o);
        lr_add_pair(d2, live && d2.x < thr2, live && 2 * r + 1 < m && d2.y < thr2, c, q);
    }
    if (act && c) { atomicAdd(&sh.cnt[t], c); atomicAdd(&sh.ssq[t], q); }
    __syncthreads();
}
__device__ void lo_score_lanes(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2)
{
    if (threadIdx.x < LR_LO_TRIALS) { sh.cnt[threadIdx.x] = 0u; sh.ssq[threadIdx.x] = 0ull; }
    __syncthreads();
    lo_score_lanes_range(sh, corr8, m, thr2, 0, (m + 1) >> 1);
}

// ---- helper blocks (single-pair and small-batch calls: the GPU is idle while one block per pair optimises its model).
// The scoring of a round's 20 models over all correspondences is 2/3 of a round and embarrassingly parallel.  The master block (block 0
// of the pair) PUBLISHES it as a job -- the 20 rounded models, the chunk count -- in a control block in device memory; every block of
// the pair's group, the master included, claims chunks of LO_CHUNK_REC records from the job's counter, scores them with
// lo_score_lanes_range, adds its integer sums to the job's totals and reports the chunks it did.  The master waits only for chunks that
// were CLAIMED, i.e. for blocks that are running: a helper that was never scheduled (other kernels hold the CUs) costs nothing, and no
// block ever waits for a block that is not running -- there is no grid barrier.  Every job has its own slot (counters are never reused
// within a launch, so a slow helper cannot touch a later job); the slots are zeroed by ransac_final_kernel, which precedes every launch.
// Release / acquire follow MI355X_MICROARCH.md ("inter-workgroup visibility"): stores, vmcnt(0), barrier, agent-scope release, flag;
// agent-scope acquire by one lane, vmcnt(0), barrier, plain loads.  Spins are bounded by the wall clock; a master that gives up
// recomputes the job alone.  (lr_lo_job / lr_lo_ctl, LO_CHUNK_REC and LO_JOBS: lr_ransac_dev.h.)

// this block's share of job `jb` (models already in sh.Rt): claims chunks until none is left, then adds its sums to the job's totals
__device__ void lo_job_work(lo_shared &sh, lr_lo_job *jb, const float *__restrict__ corr8, int m, float thr2)
{
    const int tid = threadIdx.x;
    const int nrec = (m + 1) >> 1;
    const int nchunks = (nrec + LO_CHUNK_REC - 1) / LO_CHUNK_REC;
    if (tid < LR_LO_TRIALS) { sh.cnt[tid] = 0u; sh.ssq[tid] = 0ull; }
    __syncthreads();
    int mine = 0;
    for (;;) {
        if (tid == 0) sh.flag = __hip_atomic_fetch_add(&jb->next_chunk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int c = sh.flag;
        __syncthreads();
        if (c >= nchunks) break;
        lo_score_lanes_range(sh, corr8, m, thr2, c * LO_CHUNK_REC, min(nrec, (c + 1) * LO_CHUNK_REC));
        mine += 1;
    }
    if (mine > 0) {
        if (tid < LR_LO_TRIALS && sh.cnt[tid]) {
            __hip_atomic_fetch_add(&jb->cnt[tid], sh.cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&jb->ssq[tid], sh.ssq[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __hip_atomic_fetch_add(&jb->done_chunks, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
}

// master: score sh.Rt[0 .. LR_LO_TRIALS) over all correspondences with whoever helps -> sh.cnt / sh.ssq
__device__ void lo_score_shared(lo_shared &sh, lr_lo_ctl *ctl, int job, const float *__restrict__ corr8, int m, float thr2, int32_t *timeouts)
{
    const int tid = threadIdx.x;
    lr_lo_job *jb = &ctl->job[job];
    const int nrec = (m + 1) >> 1;
    const int nchunks = (nrec + LO_CHUNK_REC - 1) / LO_CHUNK_REC;
    for (int k = tid; k < LR_LO_TRIALS * 12; k += LO_THREADS) jb->Rt[k / 12][k % 12] = sh.Rt[k / 12][k % 12];
    if (tid == 0) jb->nchunks = nchunks;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(&ctl->phase, job + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    lo_job_work(sh, jb, corr8, m, thr2);
    // wait for the chunks other blocks claimed (they are running: this ends), bounded by the wall clock
    if (tid == 0) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        int ok = 1;
        while (__hip_atomic_load(&jb->done_chunks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nchunks) {
            __builtin_amdgcn_s_sleep(2);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 20000000ull) { ok = 0; break; }      // 0.2 s at 100 MHz
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        sh.flag = ok;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int ok = sh.flag;
    __syncthreads();
    if (!ok) {          // (never observed; the sums of the job are abandoned, the event is counted: lr_ransac_result.pad0)
        if (tid == 0 && timeouts) __hip_atomic_fetch_add(timeouts, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lo_score_lanes(sh, corr8, m, thr2);
        return;
    }
    if (tid < LR_LO_TRIALS) {
        sh.cnt[tid] = __hip_atomic_load(&jb->cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh.ssq[tid] = __hip_atomic_load(&jb->ssq[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
}

// helper block: serves the jobs the master publishes until it says it is done (or nothing happens for 0.2 s)
__device__ void lo_helper_loop(lo_shared &sh, lr_lo_ctl *ctl, const float *__restrict__ corr8, int m, float thr2, int32_t *timeouts)
{
    const int tid = threadIdx.x;
    int seen = 0;
    for (;;) {
        if (tid == 0) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            int p;
            while ((p = __hip_atomic_load(&ctl->phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == seen) {
                __builtin_amdgcn_s_sleep(8);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 20000000ull) { p = -1; __hip_atomic_fetch_add(timeouts, 0x10000, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            sh.flag = p;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int p = sh.flag;
        __syncthreads();
        if (p <= 0) return;                       // -1: done (0 cannot be observed as a change)
        seen = p;
        lr_lo_job *jb = &ctl->job[p - 1];
        for (int k = tid; k < LR_LO_TRIALS * 12; k += LO_THREADS) sh.Rt[k / 12][k % 12] = jb->Rt[k / 12][k % 12];
        __syncthreads();
        lo_job_work(sh, jb, corr8, m, thr2);      // (always the full list: the near-inlier copy only exists in launches without helper blocks)
    }
}

// any number of models and any threshold (64-bit sums): LO_THREADS / ntrial threads per model, each striding over the correspondences
__device__ void lo_score_wide(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2, int ntrial)
{
    const int tid = threadIdx.x;
    if (tid < LR_LO_TRIALS) { sh.cnt[tid] = 0u; sh.ssq[tid] = 0ull; }
    __syncthreads();
    const int per = LO_THREADS / ntrial;           // threads per model
    const int t = tid / per, l = tid % per;
    if (t < ntrial) {
        float Rt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = sh.Rt[t][k];
        unsigned c = 0; unsigned long long q = 0;
        for (int i = l; i < m; i += per) {
            const float d2 = lr_corr_d2(Rt, corr8, i);
            if (d2 < thr2) { c += 1u; q += (unsigned long long)lr_score_term(d2); }
        }
        if (c) { atomicAdd(&sh.cnt[t], c); atomicAdd(&sh.ssq[t], q); }
    }
    __syncthreads();
}

__device__ __forceinline__ void lo_score(lo_shared &sh, const float *__restrict__ corr8, int m, float thr2, int ntrial, lr_lo_ctl *ctl = nullptr, int job = -1,
                                         int32_t *timeouts = nullptr)
{
    // 32-bit per-thread error sums hold when (correspondences per thread) * thr2 * 2^20 < 2^32
    if (ntrial > 1) {      // (lanes of trials >= ntrial score stale models nobody reads)
        if (ctl && job >= 0 && job < LO_JOBS) lo_score_shared(sh, ctl, job, corr8, m, thr2, timeouts);
        else lo_score_lanes(sh, corr8, m, thr2);
        return;
    }
    const bool narrow = ((double)(m / LO_THREADS + 2)) * (double)thr2 * (double)LR_SCORE_SCALE < 4.0e9;      // (a thread's correspondences x the largest term)
    if (!narrow) lo_score_wide(sh, corr8, m, thr2, ntrial);
    else lo_score_one(sh, corr8, m, thr2);
}

#ifdef LR_LO_PROBE      // development build (tools/r4_loprobe.sh): 10 ns ticks the master block spends per phase, summed over all launches
__device__ unsigned long long g_lo_probe[16];
extern "C" __attribute__((visibility("default"))) int lr_debug_lo_probe(unsigned long long *out, int reset)
{
    if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lo_probe), sizeof(unsigned long long) * 16);
    if (reset) { unsigned long long z[16] = { 0 }; hipMemcpyToSymbol(HIP_SYMBOL(g_lo_probe), z, sizeof(z)); }
    return 0;
}
#define LO_TICK(slot) do { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); atomicAdd(&g_lo_probe[slot], now_ - tk_); tk_ = now_; } } while (0)
#define LO_COUNT(slot) do { if (threadIdx.x == 0) atomicAdd(&g_lo_probe[slot], 1ull); } while (0)
#else
#define LO_TICK(slot) do { } while (0)
#define LO_COUNT(slot) do { } while (0)
#endif

__global__ void __launch_bounds__(LO_THREADS)
ransac_lo_kernel(const float *__restrict__ corr8, int m_max, const int32_t *__restrict__ m_dev, lr_ransac_params p, int h_end, int mode,
                 int32_t *__restrict__ counters, int32_t *__restrict__ list, double *__restrict__ T_out, lr_ransac_result *__restrict__ res,
                 lr_lo_ctl *__restrict__ ctl, float *__restrict__ near8, lr_zargs z)
{
    lr_z(corr8, z, blockIdx.z); lr_z(m_dev, z, blockIdx.z); lr_z(counters, z, blockIdx.z); lr_z(list, z, blockIdx.z); lr_z(T_out, z, blockIdx.z);
    lr_z(res, z, blockIdx.z); lr_z(ctl, z, blockIdx.z); lr_z(near8, z, blockIdx.z);
    __shared__ lo_shared sh;
    lr_ransac_state *state = reinterpret_cast<lr_ransac_state *>(counters + LR_CNT_COUNT);
    const int m = m_dev ? min(*m_dev, m_max) : m_max;
    const int tid = threadIdx.x;
    const bool helpers = gridDim.x > 1 && mode == 0;              // blocks 1.. of the pair's group serve the master's scoring jobs
    if (blockIdx.x > 0) {
        if (helpers && m > 0) lo_helper_loop(sh, ctl, corr8, m, p.thr2, &state->lo_timeouts);
        return;
    }
    // (every way out of the master tells the helpers: they must not wait for jobs that never come)
    auto release_helpers = [&]() { if (helpers && tid == 0) __hip_atomic_store(&ctl->phase, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    if (state->cnt == 0 || m <= 0) { release_helpers(); return; }                         // no model
    if (mode == 0 && !state->lo_pending) { release_helpers(); return; }                  // best model unchanged by the batch just merged
#ifdef LR_LO_PROBE
    unsigned long long tk_ = __builtin_amdgcn_s_memrealtime();
    const unsigned long long tk0_ = tk_;
#endif
    LO_COUNT(mode == 0 ? 9 : 10);
    const uint32_t msac_T = lr_msac_T(p.scoring, p.thr2);
    if (tid < 12) sh.curT[tid] = state->T[tid];
    if (tid == 0) { sh.curc = state->cnt; sh.curq = state->ssq; }
    const int call = state->lo_calls;
    __syncthreads();
    if (mode == 0) {
        // near8: the correspondences within (1 + LO_NEAR_CAP) thr of the base model, in index order (lo_build_list<1>); while every
        // model involved stays within the cap of the base, a round runs over near8 alone
        const float thr = sqrtf(p.thr2);
        const float thr_near = thr * (1.0f + LO_NEAR_CAP), thr2_near = thr_near * thr_near * 1.000001f;
        // (short lists: nothing to gain; calls with helper blocks -- single pairs -- neither: their scoring is already spread over 16 CUs,
        // the copy would cost more than it saves: 156 -> 178 us per pair measured)
        bool near_on = near8 != nullptr && m >= 4096 && !helpers;
        if (tid == 0) { sh.box_state = 0; sh.near_ok = 0; sh.nNear = 0; }
        __syncthreads();
        bool have_near = false;
        for (int round = 0; round < p.lo_rounds; ++round) {
            LO_COUNT(8);
            const float *cc = corr8; int mm = m;          // what this round's list, fits (and, eps permitting, scoring) run over
            if (near_on) {
                if (!have_near) {
                    if (tid < 12) sh.baseT[tid] = sh.curT[tid];
                    lo_build_list<1>(sh, corr8, m, thr2_near, nullptr, near8);
                    have_near = sh.box_state == 1 && sh.nNear > 0;
                    // (a non-finite source coordinate -- no bounding box, no bound -- or an empty copy: no later round of this call can use one
                    // either; without this every remaining round re-ran the full scan + copy for nothing)
                    if (!have_near) near_on = false;
                    LO_COUNT(13);
                }
                if (have_near) { cc = near8; mm = sh.nNear; }
            }
            lo_build_list<0>(sh, cc, mm, p.thr2, list);
            LO_TICK(0);
            const int nI = sh.nI;
            if (nI <= p.sample_size) break;
            const int ntrial = nI > LR_LO_SAMPLE ? p.lo_trials : 1;
            if (nI > LR_LO_SAMPLE) {
                // LR_LO_SAMPLE distinct positions per trial (word stream keyed by seed, call, round, trial; a word that repeats a position is
                // skipped): 32 lanes per trial, lane j keeps the j-th accepted position, so "already drawn?" is one ballot over the
                // trial's half of the wave instead of a loop over LDS.  Lane j then fetches its correspondence (two dependent loads,
                // all LR_LO_TRIALS * LR_LO_SAMPLE of them in flight at once).
                {
                    const int t = tid >> 5, j = tid & 31, half = (tid >> 5) & 1;
                    if (t < ntrial) {
                        int mine = -1, got = 0;
                        const uint64_t key = p.seed ^ 0x4c4f43414c4f5054ull;
                        for (int blk = 0; blk < 32 && got < LR_LO_SAMPLE; ++blk) {
                            const uint64_t ctr = ((uint64_t)call << 40) | ((uint64_t)round << 32) | ((uint64_t)t << 8) | (uint64_t)blk;
                            uint32_t w[4] = { (uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u };
                            philox4x32_10(w, (uint32_t)key, (uint32_t)(key >> 32));
                            for (int k = 0; k < 4 && got < LR_LO_SAMPLE; ++k) {
                                const int c = (int)__umulhi(w[k], (uint32_t)nI);
                                const bool dup = (uint32_t)(__ballot(mine == c) >> (32 * half)) != 0u;
                                if (!dup) { if (j == got) mine = c; ++got; }
                            }
                        }
                        for (int c = 0; got < LR_LO_SAMPLE; ++c) {
                            const bool dup = (uint32_t)(__ballot(mine == c) >> (32 * half)) != 0u;
                            if (!dup) { if (j == got) mine = c; ++got; }
                        }
                        if (j < LR_LO_SAMPLE) {
                            const int i = list[mine];
#pragma unroll
                            for (int a = 0; a < 6; ++a) sh.pts[t][j][a] = cc[lr_corr_at(i, a)];
                        }
                    }
                }
                __syncthreads();
                // ... and summed by one thread per trial in the order of kabsch_points_kernel / orc_kabsch_points
                if (tid < ntrial) {
                    double cp[3] = { 0, 0, 0 }, cq[3] = { 0, 0, 0 }, W = 0.0;
#pragma unroll 1
                    for (int k = 0; k < LR_LO_SAMPLE; ++k) {      // (rolled: unrolled, the 126 values of both loops are kept live and spill)
                        W = W + 1.0;
                        for (int a = 0; a < 3; ++a) { cp[a] = cp[a] + 1.0 * (double)sh.pts[tid][k][a]; cq[a] = cq[a] + 1.0 * (double)sh.pts[tid][k][3 + a]; }
                    }
                    for (int a = 0; a < 3; ++a) { cp[a] = cp[a] / W; cq[a] = cq[a] / W; }
                    double H[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
#pragma unroll 1
                    for (int k = 0; k < LR_LO_SAMPLE; ++k) {
                        double pc[3], qc[3];
                        for (int a = 0; a < 3; ++a) { pc[a] = (double)sh.pts[tid][k][a] - cp[a]; qc[a] = (double)sh.pts[tid][k][3 + a] - cq[a]; }
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b) H[a][b] = H[a][b] + (1.0 * pc[a]) * qc[b];
                    }
                    double T[16];
                    lr_rt_from_cov(H, cp, cq, T);
                    for (int k = 0; k < 12; ++k) { sh.T[tid][k] = T[k]; sh.Rt[tid][k] = (float)T[k]; }
                    // how far this trial can move a source point away from where the model under optimisation puts it (fp64; see lo_build_list)
                    double e = 1.0e300;
                    if (have_near) {
                        const double cx = 0.5 * ((double)sh.box[0] + (double)sh.box[3]), cy = 0.5 * ((double)sh.box[1] + (double)sh.box[4]), cz = 0.5 * ((double)sh.box[2] + (double)sh.box[5]);
                        const double ex = (double)sh.box[3] - (double)sh.box[0], ey = (double)sh.box[4] - (double)sh.box[1], ez = (double)sh.box[5] - (double)sh.box[2];
                        const double rho = 0.5 * sqrt(ex * ex + ey * ey + ez * ez) * 1.0001 + 1e-6;
                        double d[12], F2 = 0.0;
                        for (int k = 0; k < 12; ++k) d[k] = T[k] - sh.baseT[k];
                        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) F2 += d[4 * a + b] * d[4 * a + b];
                        const double ux = d[0] * cx + d[1] * cy + d[2] * cz + d[3], uy = d[4] * cx + d[5] * cy + d[6] * cz + d[7], uz = d[8] * cx + d[9] * cy + d[10] * cz + d[11];
                        const double amax = fmax(fmax(fmax(fabs((double)sh.box[0]), fabs((double)sh.box[3])), fmax(fabs((double)sh.box[1]), fabs((double)sh.box[4]))),
                                                 fmax(fabs((double)sh.box[2]), fabs((double)sh.box[5])));
                        // (the slack of the pilot-ordered scoring: 1 cm + 4e-6 of the coordinate magnitude, two orders above the fp32 rounding of both residuals)
                        const double slack = 0.01 + 4e-6 * (3.0 * amax + fabs(T[3]) + fabs(T[7]) + fabs(T[11]) + fabs(sh.baseT[3]) + fabs(sh.baseT[7]) + fabs(sh.baseT[11]));
                        e = (sqrt(F2) * rho + sqrt(ux * ux + uy * uy + uz * uz)) * 1.001 + slack;
                    }
                    sh.eps[tid] = e;          // (NaN from a degenerate fit fails the comparison below: the round scores everything)
                }
                __syncthreads();
                if (tid == 0) {
                    bool ok = have_near;
                    for (int t = 0; t < ntrial && ok; ++t) ok = sh.eps[t] <= (double)(LO_NEAR_CAP * thr);
                    sh.near_ok = ok ? 1 : 0;
                }
                __syncthreads();
            } else {
                if (tid == 0) { sh.near_ok = 0; sh.eps[0] = 1.0e300; }      // (one fit over all inliers: not bounded, scored over everything)
                if (!lo_fit_all(sh, cc, list, nI)) break;
            }
            LO_TICK(1);
            // (near_ok implies a launch without helper blocks: the near-inlier copy is never handed to a job)
            if (sh.near_ok) { LO_COUNT(12); lo_score(sh, near8, sh.nNear, p.thr2, ntrial); }
            else lo_score(sh, corr8, m, p.thr2, ntrial, helpers ? ctl : nullptr, round, &state->lo_timeouts);
            LO_TICK(2);
            if (tid == 0) {
                int bt = -1; unsigned bc = 0; unsigned long long bq = 0;
                for (int t = 0; t < ntrial; ++t) {
                    if (sh.cnt[t] == 0u) continue;
                    if (bt < 0 || lr_score_better(sh.cnt[t], sh.ssq[t], t, bc, bq, bt, msac_T)) { bt = t; bc = sh.cnt[t]; bq = sh.ssq[t]; }
                }
                // strictly better than the model under optimisation
                sh.flag = (bt >= 0 && lr_score_better(bc, bq, 1, sh.curc, sh.curq, 0, msac_T)) ? bt : -1;
                if (sh.flag >= 0) { sh.curc = bc; sh.curq = bq; for (int k = 0; k < 12; ++k) sh.curT[k] = sh.T[bt][k]; }
            }
            __syncthreads();
            LO_TICK(3);
            if (sh.flag < 0) break;
            // the next round may keep running over near8 only if the model it optimises lies within the cap of the base model
            // (its inliers are then all in near8); else it starts from a fresh copy around that model
            have_near = have_near && sh.eps[sh.flag] <= (double)(LO_NEAR_CAP * thr);
        }
    } else {
        for (int it = 0; it < LR_LO_POLISH; ++it) {
            LO_COUNT(11);
            lo_build_list<false>(sh, corr8, m, p.thr2, list);
            LO_TICK(4);
            const int nI = sh.nI;
            if (nI <= p.sample_size || !lo_fit_all(sh, corr8, list, nI)) break;
            LO_TICK(5);
            lo_score(sh, corr8, m, p.thr2, 1);
            LO_TICK(6);
            if (tid == 0) {
                // a fit that loses inliers is discarded; an equal count is kept and ends the iteration; more: again
                const unsigned tc = sh.cnt[0];
                sh.flag = tc < sh.curc ? -1 : (tc == sh.curc ? 0 : 1);
                if (sh.flag >= 0) { sh.curc = tc; sh.curq = sh.ssq[0]; for (int k = 0; k < 12; ++k) sh.curT[k] = sh.T[0][k]; }
            }
            __syncthreads();
            if (sh.flag <= 0) break;
        }
    }
    __syncthreads();
    release_helpers();
    // back to the running state; outputs rewritten from it
    if (tid < 16) {
        double v = (tid % 5 == 0) ? 1.0 : 0.0;
        if (tid < 12) { v = sh.curT[tid]; state->T[tid] = v; }
        T_out[tid] = v;
    }
    if (tid == 0) {
        state->cnt = sh.curc; state->ssq = sh.curq;
        if (mode == 0) {
            state->lo_pending = 0; state->lo_calls = call + 1;
            if (p.use_elc == 2) lr_sprt_redesign(state, sh.curc, m);
            if (p.confidence > 0.0f && p.confidence < 1.0f) {
                const double f = (double)sh.curc / (double)m;
                double fn = f;
                for (int q = 1; q < p.sample_size; ++q) fn = fn * f;
                const double kk = lr_det_log(1.0 - (double)p.confidence) / lr_det_log(1.0 - fn);
                if ((double)h_end >= kk && h_end >= p.min_iters) state->done = 1;
            }
        }
        lr_ransac_result r;
        r.best_h = state->h; r.best_count = sh.curc; r.pad0 = (uint32_t)state->lo_timeouts; r.best_ssq = sh.curq;
        r.n_valid = state->n_valid; r.n_ids = state->n_ids;
        *res = r;
    }
#ifdef LR_LO_PROBE
    if (tid == 0) atomicAdd(&g_lo_probe[7], __builtin_amdgcn_s_memrealtime() - tk0_);
#endif
}

// ------------------------------------------------------------------ launches
// blocks per pair of the per-batch launches: with one or a few pairs in the call the GPU is idle next to the one block
// that optimises a pair's model, so helper blocks take shares of its scoring jobs (lo_score_shared); with a full batch the calls of the
// other streams fill the GPU (2 / 4 / 8 helper groups per pair of a 32-pair call: +1 ... -3 % over the list runs, round 4)
int lr_lo_groups(const lr_call &c, const lr_ransac_params &p, int m_max)
{
    return (p.local_opt == 1 && m_max >= 4 * LO_CHUNK_REC) ? (c.pairs <= 2 ? 16 : c.pairs <= 4 ? 8 : 1) : 1;
}

// mode 0: the optimisation behind a batch that ended with id h_end (helper groups by lr_lo_groups); mode 1: the final iterated least squares.
// The near-inlier copy of mode 0 reuses ws->corr8s, the scratch of the pilot-ordered scoring: the batch's scoring is over, and the next
// batch's scatter pass rewrites it before it is read.
void lr_lo_run(const lr_call &c, const float *corr8, int m_max, const int32_t *m_dev, const lr_ransac_params &p, int h_end, int mode,
               double *T_out, lr_ransac_result *res)
{
    lr_workspace *ws = c.ws;
    const int groups = mode == 0 ? lr_lo_groups(c, p, m_max) : 1;
    hipLaunchKernelGGL(ransac_lo_kernel, dim3(groups, 1, c.pairs), dim3(LO_THREADS), 0, c.st, corr8, m_max, m_dev, p, h_end, mode, ws->counters, ws->lo_list,
                       T_out, res, reinterpret_cast<lr_lo_ctl *>(ws->lo_ctl), mode == 0 ? ws->corr8s : (float *)nullptr, c.z);
}
