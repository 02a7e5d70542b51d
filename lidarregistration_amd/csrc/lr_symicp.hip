// Symmetric ICP (lr_symicp) on the grid of the exact nearest neighbour, on gfx950: the third refinement of the reference's refinement
// tester (FCGF_FAST/net/refinement_tester.py:75-93), which shells out to trimesh2's mesh_align (net/symmetric_icp.py:47-82).  That binary
// is outside the reference tree: [upstream-recalled, parity unpinned]; the contract is the algorithm of the paper behind it (Rusinkiewicz,
// A Symmetric Objective Function for ICP, 2019).  Contract Y: include/lidarreg.h f9; restated in tests/symicp_cpu.py.
//
// Structure.  The scratch holds a control block (the stop word first, W, t: wave-uniform, read by the per-point kernels as they are), B' /
// nB', the two index lists, the run sums, and two arenas of lr_nn3's layout: A's grid, built once, and B''s, rebuilt in every iteration.
// An iteration is a fixed sequence of launches -- transform, the six grid launches, the forward and the backward search, the pair kernel
// (one wave per run of 1024 indices of either index space: 16 consecutive candidates per lane, 28 sums, the lanes folded as a tree), the
// one-wave step (run sums in order, Cholesky, the split rotation, log row, stop flags, the next W).  The control block's first word ends
// the loop: every later launch, the grid's and the search's included, returns at its first instruction.  No floating-point atomic; every
// word read was written by a kernel of the call.
#include "lr_prims.h"
#include "lr_nn3.h"
#include <math.h>
#include <string.h>

#define SY_MAX_ITER 1000
#define SY_SEG 16                    // consecutive terms per lane: 64 lanes x 16 = one run (Y4)
#define SY_NSUM 28                   // 21 entries of H (a <= b, row-major), 6 of g, b b
#define SY_SLOT 32                   // doubles per run in the scratch: the 28 sums, the count, padding to 256 bytes
static_assert(SY_SEG * 64 == NN_RUN, "a run is one wave's worth of segments");

struct sy_ctl {
    int32_t done, status, iters_run, converged, n_pairs, pad[3];         // done first: the grid / search kernels' stop word
    double msq, W[9], t[3];
};
static_assert(sizeof(sy_ctl) <= 1024, "sy_ctl outgrew its slot");

struct sy_layout { size_t Bp, nBp, f, r, part, arena_f, arena_b, end; };
struct sy_args {
    char *base;
    size_t stride;
    sy_layout L;
    const double *A, *nA, *B, *nB, *T_init;
    int32_t n0, n1, n_iter;
    double max_d2, min_cos, eps_rot2, eps_trans2, piv_eps;
    lr_symicp_result *res;
    double *log;
};

static size_t sy_make_layout(sy_layout *L, size_t n0, size_t n1)
{
    const size_t m0 = n0 > 0 ? n0 : 1, m1 = n1 > 0 ? n1 : 1;
    nn_layout nl;
    size_t o = 1024;
    L->Bp = o;      o += lr_al(m1 * 24);
    L->nBp = o;     o += lr_al(m1 * 24);
    L->f = o;       o += lr_al(m0 * 4);
    L->r = o;       o += lr_al(m1 * 4);
    L->part = o;    o += lr_al((m0 / NN_RUN + m1 / NN_RUN + 2) * SY_SLOT * 8);       // forward runs, then backward runs
    L->arena_f = o; o += nn_make_layout(&nl, n0, n1, 0);         // queries A, target B'
    L->arena_b = o; o += nn_make_layout(&nl, n1, n0, 0);         // queries B', target A
    L->end = o;
    return o;
}

__device__ __forceinline__ sy_ctl *sy_c(const sy_args &g) { return lr_ptr<sy_ctl>(g, 0, 0); }
__device__ __forceinline__ bool sy_finite3(const double *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// the result block from the control block's pose: B_to_A = [W t; 0 1], T its rigid inverse
__device__ static void sy_write_result(const sy_args &g, const sy_ctl *c)
{
    lr_symicp_result r;
    const double *W = c->W, *t = c->t;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) { r.B_to_A[4 * a + b] = W[3 * a + b]; r.T[4 * a + b] = W[3 * b + a]; }
        r.B_to_A[4 * a + 3] = t[a];
        r.T[4 * a + 3] = -((W[a] * t[0] + W[3 + a] * t[1]) + W[6 + a] * t[2]);
        r.B_to_A[12 + a] = 0.0; r.T[12 + a] = 0.0;
    }
    r.B_to_A[15] = 1.0; r.T[15] = 1.0;
    r.status = c->status; r.iters_run = c->iters_run; r.converged = c->converged; r.n_pairs = c->n_pairs; r.mean_sq = c->msq;
    *g.res = r;
}

__global__ void __launch_bounds__(256) sy_init_kernel(sy_args g)
{
    if (g.log)
        for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < (size_t)g.n_iter * 8; s += (size_t)gridDim.x * 256) g.log[s] = 0.0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sy_ctl *c = sy_c(g);
    c->done = 0; c->status = 0; c->iters_run = 0; c->converged = 0; c->n_pairs = 0;
    c->pad[0] = c->pad[1] = c->pad[2] = 0;
    c->msq = 0.0;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) c->W[3 * a + b] = g.T_init ? g.T_init[4 * a + b] : (a == b ? 1.0 : 0.0);
        c->t[a] = g.T_init ? g.T_init[4 * a + 3] : 0.0;
    }
}

// Y1
__global__ void __launch_bounds__(256) sy_xform_kernel(sy_args g)
{
    const sy_ctl *c = sy_c(g);
    if (c->done) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n1) return;
    const double x = g.B[3 * (size_t)j], y = g.B[3 * (size_t)j + 1], z = g.B[3 * (size_t)j + 2];
    const double nx = g.nB[3 * (size_t)j], ny = g.nB[3 * (size_t)j + 1], nz = g.nB[3 * (size_t)j + 2];
    double *Bp = lr_ptr<double>(g, 0, g.L.Bp) + 3 * (size_t)j, *nBp = lr_ptr<double>(g, 0, g.L.nBp) + 3 * (size_t)j;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Bp[a] = lr_row3(c->W, a, x, y, z) + c->t[a];
        nBp[a] = lr_row3(c->W, a, nx, ny, nz);
    }
}

// Y2 .. Y4, first level: one wave per run of 1024 indices, forward runs (over i) first, then backward runs (over j).  A lane adds its 16
// consecutive candidates in order (a rejected or absent one would add +0.0, which changes no sum that started from +0.0: it is skipped),
// then the lanes fold as the contract's tree.
__global__ void __launch_bounds__(64) sy_pair_kernel(sy_args g)
{
    const sy_ctl *c = sy_c(g);
    if (c->done) return;
    const int lane = threadIdx.x, nr0 = (g.n0 + NN_RUN - 1) / NN_RUN, nr1 = (g.n1 + NN_RUN - 1) / NN_RUN, run = blockIdx.x;
    if (run >= nr0 + nr1) return;
    const bool back = run >= nr0;
    const int n = back ? g.n1 : g.n0, begin = (back ? run - nr0 : run) * NN_RUN + SY_SEG * lane;
    const int32_t *f = lr_ptr<int32_t>(g, 0, g.L.f), *r = lr_ptr<int32_t>(g, 0, g.L.r);
    const double *Bp = lr_ptr<double>(g, 0, g.L.Bp), *nBp = lr_ptr<double>(g, 0, g.L.nBp);
    double acc[SY_NSUM];
#pragma unroll
    for (int k = 0; k < SY_NSUM; ++k) acc[k] = 0.0;
    int count = 0;
#pragma unroll 1
    for (int u = begin; u < begin + SY_SEG && u < n; ++u) {
        int i, j;
        if (!back) { i = u; j = f[i]; if (j < 0) continue; }                         // f_i: -1, or < n1
        else { j = u; i = r[j]; if (i < 0 || f[i] == j) continue; }                  // a mutual pair counts once, forward
        const double *pp = Bp + 3 * (size_t)j, *qp = g.A + 3 * (size_t)i, *nap = g.nA + 3 * (size_t)i, *nbp = nBp + 3 * (size_t)j;
        const double p[3] = { pp[0], pp[1], pp[2] }, q[3] = { qp[0], qp[1], qp[2] };
        const double na[3] = { nap[0], nap[1], nap[2] }, nb[3] = { nbp[0], nbp[1], nbp[2] };
        if (!(sy_finite3(p) && sy_finite3(q) && sy_finite3(na) && sy_finite3(nb))) continue;
        const double d[3] = { p[0] - q[0], p[1] - q[1], p[2] - q[2] };
        const double dot = lr_dot3(na, nb);
        if (!(lr_dot3(d, d) <= g.max_d2) || !(fabs(dot) >= g.min_cos)) continue;
        const double s = dot < 0.0 ? -1.0 : 1.0;
        const double nv[3] = { na[0] + s * nb[0], na[1] + s * nb[1], na[2] + s * nb[2] };
        const double m[3] = { p[0] + q[0], p[1] + q[1], p[2] + q[2] };
        const double cv[6] = { m[1] * nv[2] - m[2] * nv[1], m[2] * nv[0] - m[0] * nv[2], m[0] * nv[1] - m[1] * nv[0], nv[0], nv[1], nv[2] };
        const double b = -lr_dot3(d, nv);
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int e = a; e < 6; ++e) { acc[k] = acc[k] + cv[a] * cv[e]; ++k; }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + cv[a] * b;
        acc[27] = acc[27] + b * b;
        ++count;
    }
#pragma unroll
    for (int k = 0; k < SY_NSUM; ++k) acc[k] = lr_wave_tree_sum(acc[k]);
    count = lr_wave_tree_sum(count);
    if (lane == 0) {
        double *part = lr_ptr<double>(g, 0, g.L.part) + SY_SLOT * (size_t)run;
#pragma unroll
        for (int k = 0; k < SY_NSUM; ++k) part[k] = acc[k];
        part[SY_NSUM] = (double)count;
    }
}

// Y5: Cholesky of H (S[0 .. 20], the upper triangle row-major) and the two substitutions on g (S[21 .. 26]); 0, or 2 where a pivot fails
__device__ static int sy_solve(const double *S, double piv_eps, double *x)
{
    double H[6][6], L[6][6], y[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int e = a; e < 6; ++e) { H[a][e] = S[k]; H[e][a] = S[k]; ++k; }
    for (int j = 0; j < 6; ++j) {
        double d = H[j][j];
        for (int q = 0; q < j; ++q) d = d - L[j][q] * L[j][q];
        if (!(d > piv_eps * H[j][j])) return 2;
        L[j][j] = __dsqrt_rn(d);
        for (int i = j + 1; i < 6; ++i) {
            double s = H[i][j];
            for (int q = 0; q < j; ++q) s = s - L[i][q] * L[j][q];
            L[i][j] = s / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = S[21 + i];
        for (int q = 0; q < i; ++q) s = s - L[i][q] * y[q];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int q = i + 1; q < 6; ++q) s = s - L[q][i] * x[q];
        x[i] = s / L[i][i];
    }
    return 0;
}

// second level of the sums (lane q adds sum q's run sums in run order, forward then backward), Y5 .. Y7, the result block and the stop word
__global__ void __launch_bounds__(64) sy_step_kernel(sy_args g, int k)
{
    __shared__ double S[SY_SLOT];
    sy_ctl *c = sy_c(g);
    if (c->done) return;
    const int lane = threadIdx.x, nr0 = (g.n0 + NN_RUN - 1) / NN_RUN, nr1 = (g.n1 + NN_RUN - 1) / NN_RUN;
    if (lane <= SY_NSUM) {
        const double *part = lr_ptr<double>(g, 0, g.L.part) + lane;
        double fw = 0.0, bw = 0.0;
        for (int r = 0; r < nr0; ++r) fw = fw + part[SY_SLOT * (size_t)r];
        for (int r = nr0; r < nr0 + nr1; ++r) bw = bw + part[SY_SLOT * (size_t)r];
        S[lane] = fw + bw;
    }
    __syncthreads();
    if (lane != 0) return;
    const int n_pairs = (int)S[SY_NSUM];                     // a sum of integers below 2^23: exact
    const double msq = n_pairs > 0 ? S[27] / (double)n_pairs : 0.0;
    double *row = g.log ? g.log + 8 * (size_t)k : nullptr;
    if (row) { row[0] = (double)n_pairs; row[1] = msq; }
    c->iters_run = k + 1; c->n_pairs = n_pairs; c->msq = msq;
    bool stop = k + 1 >= g.n_iter;
    double x[6];
    if (n_pairs < 6) { c->status = 1; stop = true; }
    else if (sy_solve(S, g.piv_eps, x)) { c->status = 2; stop = true; }
    else if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(x[3]) && isfinite(x[4]) && isfinite(x[5]))) { c->status = 3; stop = true; }
    else {
        // Y6: the rotation by the half step, applied twice
        const double aa = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
        const double cs = 1.0 / __dsqrt_rn(1.0 + aa), k2 = (cs * cs) / (1.0 + cs);
        const double Sk[9] = { 0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0 };
        double R[9], dW[9], Wn[9], dt[3], tn[3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) R[3 * a + b] = ((a == b ? cs : 0.0) + cs * Sk[3 * a + b]) + k2 * (x[a] * x[b]);
        lr_mat3(R, R, dW);
        for (int a = 0; a < 3; ++a) dt[a] = lr_row3(R, a, cs * x[3], cs * x[4], cs * x[5]);
        lr_mat3(dW, c->W, Wn);
        for (int a = 0; a < 3; ++a) tn[a] = lr_row3(dW, a, c->t[0], c->t[1], c->t[2]) + dt[a];
        for (int a = 0; a < 9; ++a) c->W[a] = Wn[a];
        for (int a = 0; a < 3; ++a) c->t[a] = tn[a];
        const double tt = (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2];
        if (row) { row[2] = aa; row[3] = tt; }
        if (aa <= g.eps_rot2 && tt <= g.eps_trans2) { c->converged = 1; stop = true; }
    }
    if (stop) {
        sy_write_result(g, c);
        __threadfence();
        c->done = 1;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_symicp_params) == 64 && sizeof(lr_symicp_result) == 280,
              "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_symicp_scratch_bytes(int n0, int n1)
{
    if (n0 < 0 || n0 > NN_MAX_N || n1 < 0 || n1 > NN_MAX_N) return 0;
    sy_layout L;
    return sy_make_layout(&L, (size_t)n0, (size_t)n1);
}

extern "C" int lr_symicp(const double *xyzA, const double *nrmA, int n0, const double *xyzB, const double *nrmB, int n1,
                         const lr_symicp_params *p, lr_symicp_result *result, double *log, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_symicp";
    LR_CHECK_STRUCT_SIZE(lr_symicp_params, p, who);
    LR_REFUSE_UNLESS(p->n_iter >= 1 && p->n_iter <= SY_MAX_ITER, LR_EINVAL, "n_iter must lie in 1..1000");
    LR_REFUSE_UNLESS(p->max_dist > 0.0 && isfinite(p->max_dist), LR_EINVAL, "max_dist must be positive and finite");
    LR_REFUSE_UNLESS(p->min_cos >= 0.0 && p->min_cos <= 1.0, LR_EINVAL, "min_cos must lie in [0, 1]");
    LR_REFUSE_UNLESS(p->eps_rot > 0.0 && isfinite(p->eps_rot), LR_EINVAL, "eps_rot must be positive and finite");
    LR_REFUSE_UNLESS(p->eps_trans > 0.0 && isfinite(p->eps_trans), LR_EINVAL, "eps_trans must be positive and finite");
    LR_REFUSE_UNLESS(p->piv_eps > 0.0 && isfinite(p->piv_eps), LR_EINVAL, "piv_eps must be positive and finite");
    LR_REFUSE_UNLESS(p->cell == 0.0 || (p->cell > 0.0 && isfinite(p->cell)), LR_EINVAL, "cell must be 0 (automatic) or positive and finite");
    LR_REFUSE_UNLESS(n0 >= 0 && n0 <= NN_MAX_N && n1 >= 0 && n1 <= NN_MAX_N, LR_EINVAL, "n0 / n1 must lie in 0..4194304");
    LR_REFUSE_UNLESS(n0 == 0 || xyzA, LR_EINVAL, "null xyzA");
    LR_REFUSE_UNLESS(n0 == 0 || nrmA, LR_EINVAL, "null nrmA");
    LR_REFUSE_UNLESS(n1 == 0 || xyzB, LR_EINVAL, "null xyzB");
    LR_REFUSE_UNLESS(n1 == 0 || nrmB, LR_EINVAL, "null nrmB");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    sy_args g;
    memset(&g, 0, sizeof g);
    const size_t need = sy_make_layout(&g.L, (size_t)n0, (size_t)n1);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, need, "lr_symicp_scratch_bytes(n0, n1)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch); g.stride = need;
    g.A = xyzA; g.nA = nrmA; g.B = xyzB; g.nB = nrmB; g.T_init = p->T_init; g.n0 = n0; g.n1 = n1; g.n_iter = p->n_iter;
    g.max_d2 = p->max_dist * p->max_dist; g.min_cos = p->min_cos; g.eps_rot2 = p->eps_rot * p->eps_rot; g.eps_trans2 = p->eps_trans * p->eps_trans;
    g.piv_eps = p->piv_eps;
    g.res = result; g.log = log;
    const int32_t *stop = reinterpret_cast<const int32_t *>(g.base);                 // sy_ctl.done
    const double *Bp = reinterpret_cast<const double *>(g.base + g.L.Bp);
    nn_args gf, gb;
    nn_set_args(&gf, g.base + g.L.arena_f, xyzA, n0, Bp, n1, p->cell, reinterpret_cast<int32_t *>(g.base + g.L.f), stop);
    nn_set_args(&gb, g.base + g.L.arena_b, Bp, n1, xyzA, n0, p->cell, reinterpret_cast<int32_t *>(g.base + g.L.r), stop);
    hipStream_t st = (hipStream_t)stream;
    const int nb1 = lr_cdiv(n1 > 0 ? n1 : 1, 256), runs = lr_cdiv(n0, NN_RUN) + lr_cdiv(n1, NN_RUN);
    const int ib = lr_cdiv(p->n_iter * 8, 256);
    hipLaunchKernelGGL(sy_init_kernel, dim3(ib), dim3(256), 0, st, g);
    nn_launch_grid(gb, st);                                  // A's grid stands for the whole call
    for (int k = 0; k < p->n_iter; ++k) {
        hipLaunchKernelGGL(sy_xform_kernel, dim3(nb1), dim3(256), 0, st, g);
        nn_launch_grid(gf, st);
        nn_launch_search(gf, st);
        nn_launch_search(gb, st);
        hipLaunchKernelGGL(sy_pair_kernel, dim3(runs > 0 ? runs : 1), dim3(64), 0, st, g);
        hipLaunchKernelGGL(sy_step_kernel, dim3(1), dim3(64), 0, st, g, k);
    }
    LR_LAUNCH_CHECK();
    return LR_OK;
}
