// Best-Buddies refinement (lr_bbrf) and hybrid-search point normals (lr_normals, lr_normals2: the same with the neighbour counts) on the grid of the exact nearest neighbour, on gfx950.
//
// Replaces FCGF_FAST/net/BBR_F.py:267-322 (BBR_F: 100 Adam steps over the mutual nearest neighbours of two clouds under a symmetric
// point-to-plane loss) and its calc_normals (:236-241).  Contract B and the normals contract: include/lidarreg.h; restated
// in tests/bbrf_cpu.py.
//
// Structure.  The scratch holds a control block (parameters, moments, W and its derivative matrices: wave-uniform, read by the per-point
// kernels as they are), B' / nB', the two index lists, the run sums, and two arenas of lr_nn3's layout: A's grid, built once, and B''s,
// rebuilt in every iteration.  An iteration is a fixed sequence of launches -- transform, the six grid launches, the forward and the
// backward search, the pair kernel (one wave per run of 1024 source indices, seven sums in index order on every lane), the one-wave
// step (run sums in order, loss, Adam, log row, running argmin, stop flags, the next W).  The control block's first word ends the loop:
// every later launch, the grid's and the search's included, returns at its first instruction.  No floating-point atomic; every word read
// was written by a kernel of the call.
#include "lr_prims.h"
#include "lr_nn3.h"
#include <math.h>
#include <string.h>

#define BB_ANGLE_MAX 0.5
#define BB_MAX_ITER 1000
#define BB_MAX_NN 32
#define BB_SWEEPS 8

struct bb_ctl {
    int32_t done, status, best_iter, n_best, iters_run, pad[3];          // done first: the grid / search kernels' stop word
    double p[6], m[6], v[6], pw1, pw2, best_loss, best_p[6];
    double W[9], t[3], dW[27];
};
static_assert(sizeof(bb_ctl) <= 1024, "bb_ctl outgrew its slot");

struct bb_layout { size_t Bp, nBp, f, r, part, arena_f, arena_b, end; };
struct bb_args {
    char *base;
    size_t stride;
    bb_layout L;
    const double *A, *nA, *B, *nB;
    int32_t n0, n1, n_iter;
    double lr_a, lr_t, beta1, beta2, eps;
    lr_bbrf_result *res;
    double *log;
};

static size_t bb_make_layout(bb_layout *L, size_t n0, size_t n1)
{
    const size_t m0 = n0 > 0 ? n0 : 1, m1 = n1 > 0 ? n1 : 1;
    nn_layout nl;
    size_t o = 1024;
    L->Bp = o;      o += lr_al(m1 * 24);
    L->nBp = o;     o += lr_al(m1 * 24);
    L->f = o;       o += lr_al(m0 * 4);
    L->r = o;       o += lr_al(m1 * 4);
    L->part = o;    o += lr_al((m0 / NN_RUN + 1) * 64);
    L->arena_f = o; o += nn_make_layout(&nl, n0, n1, 0);         // queries A, target B'
    L->arena_b = o; o += nn_make_layout(&nl, n1, n0, 0);         // queries B', target A
    L->end = o;
    return o;
}

__device__ __forceinline__ bb_ctl *bb_c(const bb_args &g) { return lr_ptr<bb_ctl>(g, 0, 0); }

// ---- B2 ----------------------------------------------------------------------------------------------------------------------------
#define BB_F3 6.0
#define BB_F5 120.0
#define BB_F7 5040.0
#define BB_F9 362880.0
#define BB_F11 39916800.0
#define BB_F13 6227020800.0
#define BB_F15 1307674368000.0
#define BB_F17 355687428096000.0
#define BB_F2 2.0
#define BB_F4 24.0
#define BB_F6 720.0
#define BB_F8 40320.0
#define BB_F10 3628800.0
#define BB_F12 479001600.0
#define BB_F14 87178291200.0
#define BB_F16 20922789888000.0

__device__ static double bb_sin(double x)
{
    const double z = x * x;
    double q = 1.0 / BB_F17;
    q = q * z + -1.0 / BB_F15;
    q = q * z + 1.0 / BB_F13;
    q = q * z + -1.0 / BB_F11;
    q = q * z + 1.0 / BB_F9;
    q = q * z + -1.0 / BB_F7;
    q = q * z + 1.0 / BB_F5;
    q = q * z + -1.0 / BB_F3;
    return x + (x * z) * q;
}

__device__ static double bb_cos(double x)
{
    const double z = x * x;
    double q = 1.0 / BB_F16;
    q = q * z + -1.0 / BB_F14;
    q = q * z + 1.0 / BB_F12;
    q = q * z + -1.0 / BB_F10;
    q = q * z + 1.0 / BB_F8;
    q = q * z + -1.0 / BB_F6;
    q = q * z + 1.0 / BB_F4;
    q = q * z + -1.0 / BB_F2;
    return 1.0 + z * q;
}

__device__ static void bb_mat3(const double *P, const double *Q, double *R)
{
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = (P[3 * a] * Q[b] + P[3 * a + 1] * Q[3 + b]) + P[3 * a + 2] * Q[6 + b];
}

// W and, where dW is given, dW/dtheta, dW/dphi, dW/dpsi (27 doubles)
__device__ static void bb_rotation(double theta, double phi, double psi, double *W, double *dW)
{
    const double s1 = bb_sin(theta), c1 = bb_cos(theta), s2 = bb_sin(phi), c2 = bb_cos(phi), s3 = bb_sin(psi), c3 = bb_cos(psi);
    const double Rx[9] = { 1.0, 0.0, 0.0, 0.0, c1, -s1, 0.0, s1, c1 };
    const double Ry[9] = { c2, 0.0, s2, 0.0, 1.0, 0.0, -s2, 0.0, c2 };
    const double Rz[9] = { c3, -s3, 0.0, s3, c3, 0.0, 0.0, 0.0, 1.0 };
    double YX[9], tmp[9];
    bb_mat3(Ry, Rx, YX);
    bb_mat3(Rz, YX, W);
    if (!dW) return;
    const double dRx[9] = { 0.0, 0.0, 0.0, 0.0, -s1, -c1, 0.0, c1, -s1 };
    const double dRy[9] = { -s2, 0.0, c2, 0.0, 0.0, 0.0, -c2, 0.0, -s2 };
    const double dRz[9] = { -s3, -c3, 0.0, c3, -s3, 0.0, 0.0, 0.0, 0.0 };
    bb_mat3(Ry, dRx, tmp); bb_mat3(Rz, tmp, dW);
    bb_mat3(dRy, Rx, tmp); bb_mat3(Rz, tmp, dW + 9);
    bb_mat3(dRz, YX, dW + 18);
}

// lane j's value on every lane, j wave-uniform: two scalar lane reads instead of a trip through the LDS crossbar
__device__ __forceinline__ double bb_lane(double v, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bb_row(const double *M, int a, double x, double y, double z) { return (M[3 * a] * x + M[3 * a + 1] * y) + M[3 * a + 2] * z; }

// B8 from the control block's best parameters
__device__ static void bb_write_result(const bb_args &g, const bb_ctl *c)
{
    lr_bbrf_result r;
    double W[9];
    bb_rotation(c->best_p[0], c->best_p[1], c->best_p[2], W, nullptr);
    const double t[3] = { c->best_p[3], c->best_p[4], c->best_p[5] };
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) { r.B_to_A[4 * a + b] = W[3 * a + b]; r.T[4 * a + b] = W[3 * b + a]; }
        r.B_to_A[4 * a + 3] = t[a];
        r.T[4 * a + 3] = -((W[a] * t[0] + W[3 + a] * t[1]) + W[6 + a] * t[2]);
        r.B_to_A[12 + a] = 0.0; r.T[12 + a] = 0.0;
    }
    r.B_to_A[15] = 1.0; r.T[15] = 1.0;
    r.status = c->status; r.best_iter = c->best_iter; r.best_loss = c->best_loss; r.n_pairs_best = c->n_best; r.iters_run = c->iters_run;
    *g.res = r;
}

// ---- the loop's kernels ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bb_init_kernel(bb_args g)
{
    if (g.log)
        for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < (size_t)g.n_iter * 8; s += (size_t)gridDim.x * 256) g.log[s] = 0.0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    bb_ctl *c = bb_c(g);
    c->done = 0; c->status = 0; c->best_iter = -1; c->n_best = 0; c->iters_run = 0;
    c->pad[0] = c->pad[1] = c->pad[2] = 0;
    for (int k = 0; k < 6; ++k) { c->p[k] = 0.0; c->m[k] = 0.0; c->v[k] = 0.0; c->best_p[k] = 0.0; }
    c->pw1 = 1.0; c->pw2 = 1.0; c->best_loss = INFINITY;
    c->t[0] = c->t[1] = c->t[2] = 0.0;
    bb_rotation(0.0, 0.0, 0.0, c->W, c->dW);
}

__global__ void __launch_bounds__(256) bb_xform_kernel(bb_args g)
{
    const bb_ctl *c = bb_c(g);
    if (c->done) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n1) return;
    const double x = g.B[3 * (size_t)j], y = g.B[3 * (size_t)j + 1], z = g.B[3 * (size_t)j + 2];
    const double nx = g.nB[3 * (size_t)j], ny = g.nB[3 * (size_t)j + 1], nz = g.nB[3 * (size_t)j + 2];
    double *Bp = lr_ptr<double>(g, 0, g.L.Bp) + 3 * (size_t)j, *nBp = lr_ptr<double>(g, 0, g.L.nBp) + 3 * (size_t)j;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Bp[a] = bb_row(c->W, a, x, y, z) + c->t[a];
        nBp[a] = bb_row(c->W, a, nx, ny, nz);
    }
}

// B4 .. B6, first level: every run of 1024 source indices by one wave, the additions in index order on every lane
__global__ void __launch_bounds__(256) bb_pair_kernel(bb_args g)
{
    const bb_ctl *c = bb_c(g);
    if (c->done) return;
    const int lane = threadIdx.x & 63, run = blockIdx.x * 4 + (threadIdx.x >> 6), nruns = (g.n0 + NN_RUN - 1) / NN_RUN;
    if (run >= nruns) return;
    const int32_t *f = lr_ptr<int32_t>(g, 0, g.L.f), *r = lr_ptr<int32_t>(g, 0, g.L.r);
    const double *Bp = lr_ptr<double>(g, 0, g.L.Bp), *nBp = lr_ptr<double>(g, 0, g.L.nBp);
    const int begin = run * NN_RUN, end = begin + NN_RUN < g.n0 ? begin + NN_RUN : g.n0;
    double sum[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int count = 0;
    for (int base = begin; base < end; base += 64) {
        const int cnt = end - base < 64 ? end - base : 64, i = base + lane;
        double v[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        bool pair = false;
        if (lane < cnt) {
            const int j = f[i];                              // -1, or < n1
            pair = j >= 0 && r[j] == i;
            if (pair) {
                const double *a = g.A + 3 * (size_t)i, *na = g.nA + 3 * (size_t)i, *b = g.B + 3 * (size_t)j, *nb = g.nB + 3 * (size_t)j;
                const double *bp = Bp + 3 * (size_t)j, *nbp = nBp + 3 * (size_t)j;
                const double nav[3] = { na[0], na[1], na[2] }, nbv[3] = { nbp[0], nbp[1], nbp[2] };
                const double s = lr_dot3(nav, nbv) < 0.0 ? -1.0 : 1.0;
                const double m[3] = { nav[0] + s * nbv[0], nav[1] + s * nbv[1], nav[2] + s * nbv[2] };
                const double d[3] = { a[0] - bp[0], a[1] - bp[1], a[2] - bp[2] };
                const double dot = lr_dot3(d, m), ad = fabs(dot);
                v[0] = ad > 1e-15 ? ad : 1e-15;
                if (!(dot * dot < 1e-30)) {
                    const double sg = dot < 0.0 ? -1.0 : 1.0;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const double *D = c->dW + 9 * q;
                        const double u[3] = { bb_row(D, 0, b[0], b[1], b[2]), bb_row(D, 1, b[0], b[1], b[2]), bb_row(D, 2, b[0], b[1], b[2]) };
                        const double w[3] = { s * bb_row(D, 0, nb[0], nb[1], nb[2]), s * bb_row(D, 1, nb[0], nb[1], nb[2]), s * bb_row(D, 2, nb[0], nb[1], nb[2]) };
                        v[1 + q] = sg * (lr_dot3(d, w) - lr_dot3(u, m));
                    }
#pragma unroll
                    for (int a3 = 0; a3 < 3; ++a3) v[4 + a3] = sg * (-m[a3]);
                }
            }
        }
        count += __popcll(__ballot(pair));
        for (int j = 0; j < cnt; ++j) {
#pragma unroll
            for (int k = 0; k < 7; ++k) sum[k] += bb_lane(v[k], j);
        }
    }
    if (lane == 0) {
        double *part = lr_ptr<double>(g, 0, g.L.part) + 8 * (size_t)run;
#pragma unroll
        for (int k = 0; k < 7; ++k) part[k] = sum[k];
        part[7] = (double)count;
    }
}

// second level of the sums, B1, B7, B8, the stop flags and the next iteration's matrices
__global__ void __launch_bounds__(64) bb_step_kernel(bb_args g, int k)
{
    bb_ctl *c = bb_c(g);
    if (c->done) return;
    const int lane = threadIdx.x, nruns = (g.n0 + NN_RUN - 1) / NN_RUN;
    const double *part = lr_ptr<double>(g, 0, g.L.part);
    double sum[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int base = 0; base < nruns; base += 64) {
        const int cnt = nruns - base < 64 ? nruns - base : 64;
        double v[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        if (lane < cnt)
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = part[8 * (size_t)(base + lane) + q];
        for (int j = 0; j < cnt; ++j) {
#pragma unroll
            for (int q = 0; q < 8; ++q) sum[q] += bb_lane(v[q], j);
        }
    }
    if (lane != 0) return;
    const int n_pairs = (int)sum[7];                         // a sum of integers below 2^22: exact
    const double np = (double)n_pairs, loss = n_pairs > 0 ? sum[0] / np : INFINITY;
    if (g.log) {
        double *row = g.log + 8 * (size_t)k;
        for (int q = 0; q < 6; ++q) row[q] = c->p[q];
        row[6] = loss; row[7] = np;
    }
    c->iters_run = k + 1;
    bool stop = k + 1 >= g.n_iter;
    if (n_pairs == 0) { c->status = 1; stop = true; }
    else {
        if (loss < c->best_loss) {
            c->best_iter = k; c->best_loss = loss; c->n_best = n_pairs;
            for (int q = 0; q < 6; ++q) c->best_p[q] = c->p[q];
        }
        c->pw1 = c->pw1 * g.beta1;
        c->pw2 = c->pw2 * g.beta2;
        const double c1 = 1.0 - c->pw1, c2 = __dsqrt_rn(1.0 - c->pw2);
        for (int q = 0; q < 6; ++q) {
            const double gq = sum[1 + q] / np, lr = q < 3 ? g.lr_a : g.lr_t;
            const double m = g.beta1 * c->m[q] + (1.0 - g.beta1) * gq;
            const double v = g.beta2 * c->v[q] + (1.0 - g.beta2) * (gq * gq);
            c->m[q] = m; c->v[q] = v;
            const double den = __dsqrt_rn(v) / c2 + g.eps;
            c->p[q] = c->p[q] - (lr / c1) * (m / den);
        }
        if (!(fabs(c->p[0]) <= BB_ANGLE_MAX && fabs(c->p[1]) <= BB_ANGLE_MAX && fabs(c->p[2]) <= BB_ANGLE_MAX)) { c->status = 3; stop = true; }
    }
    if (stop) {
        bb_write_result(g, c);
        __threadfence();
        c->done = 1;
        return;
    }
    c->t[0] = c->p[3]; c->t[1] = c->p[4]; c->t[2] = c->p[5];
    bb_rotation(c->p[0], c->p[1], c->p[2], c->W, c->dW);
}

// ---- lr_normals ------------------------------------------------------------------------------------------------------------------------
struct nm_args {
    nn_args nn;                                              // the cloud against itself: the arena, its layout and the grid
    const double *xyz;
    int32_t n, max_nn;
    double r2;
    double *out;
    int32_t *info;
    int32_t *n_nb;                                           // nullable (lr_normals2): the neighbours every point took
};

// one Jacobi rotation on (p, q), r the third index
__device__ __forceinline__ void nm_rot(double (&A)[3][3], double (&V)[3][3], int p, int q, int r)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + __dsqrt_rn(th * th + 1.0));
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0), s = t * c;
    A[p][p] = A[p][p] - t * apq;
    A[q][q] = A[q][q] + t * apq;
    A[p][q] = 0.0; A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
    A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = c * vp - s * vq;
        V[k][q] = s * vp + c * vq;
    }
}

__global__ void __launch_bounds__(256) nm_kernel(nm_args a)
{
    const nn_args &g = a.nn;
    const nn_ctl *c = nn_c(g);
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool bad = false, few = false;
    if (i < a.n) {
        int taken = 0;
        const double q[3] = { a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2] };
        double nrm[3] = { 0.0, 0.0, 1.0 };
        bad = !(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]));
        if (!bad) {
            const int32_t *table = lr_ptr<int32_t>(g, 0, g.L.table), *pidx = lr_ptr<int32_t>(g, 0, g.L.pidx);
            const double *pts = lr_ptr<double>(g, 0, g.L.pts);
            const int dx = c->dim[0], dy = c->dim[1], dz = c->dim[2];
            const int cx = nn_cell(q[0], c->blo[0], c->cell, dx), cy = nn_cell(q[1], c->blo[1], c->cell, dy), cz = nn_cell(q[2], c->blo[2], c->cell, dz);
            const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < dz ? cz + 1 : dz - 1, y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < dy ? cy + 1 : dy - 1;
            const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < dx ? cx + 1 : dx - 1;
            double ld = -1.0, S[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
            int lj = -1, k = 0;
            for (; k < a.max_nn; ++k) {
                // the least (d2, j) above the last one taken
                double best = INFINITY, bp[3] = { 0.0, 0.0, 0.0 };
                int bj = -1;
                for (int zz = z0; zz <= z1; ++zz)
                    for (int yy = y0; yy <= y1; ++yy) {
                        const int row = (zz * dy + yy) * dx, l0 = row + x0, l1 = row + x1;
                        const int e = table[l1];
                        for (int u = l0 > 0 ? table[l0 - 1] : 0; u < e; ++u) {
                            const double px = pts[3 * (size_t)u], py = pts[3 * (size_t)u + 1], pz = pts[3 * (size_t)u + 2];
                            const double ex = q[0] - px, ey = q[1] - py, ez = q[2] - pz, d2 = (ex * ex + ey * ey) + ez * ez;
                            const int j = pidx[u];
                            if (!(d2 <= a.r2) || !(d2 > ld || (d2 == ld && j > lj))) continue;
                            if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; bp[0] = px; bp[1] = py; bp[2] = pz; }
                        }
                    }
                if (bj < 0) break;
                ld = best; lj = bj;
                S[0] += bp[0]; S[1] += bp[1]; S[2] += bp[2];
                S[3] += bp[0] * bp[0]; S[4] += bp[0] * bp[1]; S[5] += bp[0] * bp[2];
                S[6] += bp[1] * bp[1]; S[7] += bp[1] * bp[2]; S[8] += bp[2] * bp[2];
            }
            few = k < 3;
            taken = k;
            if (!few) {
                const double kn = (double)k;
                double E[9];
#pragma unroll
                for (int s = 0; s < 9; ++s) E[s] = S[s] / kn;
                double A[3][3], V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
                A[0][0] = E[3] - E[0] * E[0]; A[0][1] = E[4] - E[0] * E[1]; A[0][2] = E[5] - E[0] * E[2];
                A[1][1] = E[6] - E[1] * E[1]; A[1][2] = E[7] - E[1] * E[2]; A[2][2] = E[8] - E[2] * E[2];
                A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
#pragma unroll 1
                for (int sw = 0; sw < BB_SWEEPS; ++sw) { nm_rot(A, V, 0, 1, 2); nm_rot(A, V, 0, 2, 1); nm_rot(A, V, 1, 2, 0); }
                double v[3] = { V[0][0], V[1][0], V[2][0] }, lam = A[0][0];
                if (A[1][1] < lam) { lam = A[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; }
                if (A[2][2] < lam) { lam = A[2][2]; v[0] = V[0][2]; v[1] = V[1][2]; v[2] = V[2][2]; }
                const double len = __dsqrt_rn((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                if (len > 0.0) { nrm[0] = v[0] / len; nrm[1] = v[1] / len; nrm[2] = v[2] / len; }
            }
        }
        a.out[3 * (size_t)i] = nrm[0]; a.out[3 * (size_t)i + 1] = nrm[1]; a.out[3 * (size_t)i + 2] = nrm[2];
        if (a.n_nb) a.n_nb[i] = taken;
    }
    const unsigned long long nbad = __ballot(bad), nfew = __ballot(few);
    if ((threadIdx.x & 63) == 0) {
        if (nbad) atomicAdd(&a.info[1], __popcll(nbad));
        if (nfew) atomicAdd(&a.info[2], __popcll(nfew));
    }
}

__global__ void nm_info_kernel(nm_args a, int final)
{
    if (threadIdx.x != 0) return;
    if (!final) { a.info[0] = 0; a.info[1] = 0; a.info[2] = 0; a.info[3] = 0; }
    else a.info[0] = nn_c(a.nn)->n1_live > 0 ? 0 : 1;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_bbrf_params) == 56 && sizeof(lr_bbrf_result) == 280,
              "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_bbrf_scratch_bytes(int n0, int n1, int n_iter)
{
    if (n0 < 0 || n0 > NN_MAX_N || n1 < 0 || n1 > NN_MAX_N || n_iter < 1 || n_iter > BB_MAX_ITER) return 0;
    bb_layout L;
    return bb_make_layout(&L, (size_t)n0, (size_t)n1);
}

extern "C" size_t lr_normals_scratch_bytes(int n)
{
    if (n < 0 || n > NN_MAX_N) return 0;
    nn_layout L;
    return nn_make_layout(&L, (size_t)n, (size_t)n, 0);
}

extern "C" int lr_bbrf(const double *xyzA, const double *nrmA, int n0, const double *xyzB, const double *nrmB, int n1,
                       const lr_bbrf_params *p, lr_bbrf_result *result, double *log, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_bbrf";
    LR_CHECK_STRUCT_SIZE(lr_bbrf_params, p, who);
    LR_REFUSE_UNLESS(p->n_iter >= 1 && p->n_iter <= BB_MAX_ITER, LR_EINVAL, "n_iter must lie in 1..1000");
    LR_REFUSE_UNLESS(p->angles_lr > 0.0 && isfinite(p->angles_lr), LR_EINVAL, "angles_lr must be positive and finite");
    LR_REFUSE_UNLESS(p->trans_lr > 0.0 && isfinite(p->trans_lr), LR_EINVAL, "trans_lr must be positive and finite");
    LR_REFUSE_UNLESS(p->beta1 >= 0.0 && p->beta1 < 1.0, LR_EINVAL, "beta1 must lie in [0, 1)");
    LR_REFUSE_UNLESS(p->beta2 >= 0.0 && p->beta2 < 1.0, LR_EINVAL, "beta2 must lie in [0, 1)");
    LR_REFUSE_UNLESS(p->eps > 0.0 && isfinite(p->eps), LR_EINVAL, "eps must be positive and finite");
    LR_REFUSE_UNLESS(p->cell == 0.0 || (p->cell > 0.0 && isfinite(p->cell)), LR_EINVAL, "cell must be 0 (automatic) or positive and finite");
    LR_REFUSE_UNLESS(n0 >= 0 && n0 <= NN_MAX_N && n1 >= 0 && n1 <= NN_MAX_N, LR_EINVAL, "n0 / n1 must lie in 0..4194304");
    LR_REFUSE_UNLESS(n0 == 0 || xyzA, LR_EINVAL, "null xyzA");
    LR_REFUSE_UNLESS(n0 == 0 || nrmA, LR_EINVAL, "null nrmA");
    LR_REFUSE_UNLESS(n1 == 0 || xyzB, LR_EINVAL, "null xyzB");
    LR_REFUSE_UNLESS(n1 == 0 || nrmB, LR_EINVAL, "null nrmB");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    bb_args g;
    memset(&g, 0, sizeof g);
    const size_t need = bb_make_layout(&g.L, (size_t)n0, (size_t)n1);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, need, "lr_bbrf_scratch_bytes(n0, n1, n_iter)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch); g.stride = need;
    g.A = xyzA; g.nA = nrmA; g.B = xyzB; g.nB = nrmB; g.n0 = n0; g.n1 = n1; g.n_iter = p->n_iter;
    g.lr_a = p->angles_lr; g.lr_t = p->trans_lr; g.beta1 = p->beta1; g.beta2 = p->beta2; g.eps = p->eps;
    g.res = result; g.log = log;
    const int32_t *stop = reinterpret_cast<const int32_t *>(g.base);                 // bb_ctl.done
    const double *Bp = reinterpret_cast<const double *>(g.base + g.L.Bp);
    nn_args gf, gb;
    nn_set_args(&gf, g.base + g.L.arena_f, xyzA, n0, Bp, n1, p->cell, reinterpret_cast<int32_t *>(g.base + g.L.f), stop);
    nn_set_args(&gb, g.base + g.L.arena_b, Bp, n1, xyzA, n0, p->cell, reinterpret_cast<int32_t *>(g.base + g.L.r), stop);
    hipStream_t st = (hipStream_t)stream;
    const int nb1 = lr_cdiv(n1 > 0 ? n1 : 1, 256), rb = lr_cdiv(lr_cdiv(n0 > 0 ? n0 : 1, NN_RUN), 4);
    const int ib = lr_cdiv(p->n_iter * 8, 256);
    hipLaunchKernelGGL(bb_init_kernel, dim3(ib), dim3(256), 0, st, g);
    nn_launch_grid(gb, st);                                  // A's grid stands for the whole call
    for (int k = 0; k < p->n_iter; ++k) {
        hipLaunchKernelGGL(bb_xform_kernel, dim3(nb1), dim3(256), 0, st, g);
        nn_launch_grid(gf, st);
        nn_launch_search(gf, st);
        nn_launch_search(gb, st);
        hipLaunchKernelGGL(bb_pair_kernel, dim3(rb), dim3(256), 0, st, g);
        hipLaunchKernelGGL(bb_step_kernel, dim3(1), dim3(64), 0, st, g, k);
    }
    LR_LAUNCH_CHECK();
    return LR_OK;
}

static int nm_run(const char *who, const double *xyz, int n, double radius, int max_nn, double *normals_out, int32_t *n_nb_out, int32_t *info,
                  void *scratch, size_t scratch_bytes, void *stream)
{
    LR_REFUSE_UNLESS(radius > 0.0 && isfinite(radius) && isfinite(radius * radius), LR_EINVAL, "radius must be positive and finite");
    LR_REFUSE_UNLESS(max_nn >= 1 && max_nn <= BB_MAX_NN, LR_EINVAL, "max_nn must lie in 1..32");
    LR_REFUSE_UNLESS(n >= 0 && n <= NN_MAX_N, LR_EINVAL, "n must lie in 0..4194304");
    LR_REFUSE_UNLESS(n == 0 || xyz, LR_EINVAL, "null xyz");
    LR_REFUSE_UNLESS(n == 0 || normals_out, LR_EINVAL, "null normals_out");
    LR_REFUSE_UNLESS(info, LR_EINVAL, "null info");
    nm_args a;
    memset(&a, 0, sizeof a);
    // the cell is a little longer than the radius: two points within the radius then sit in the same or in adjacent cells whatever the
    // rounding of the cell quotients (below 2^-29 of a cell at up to 2^22 cells per axis)
    nn_set_args(&a.nn, scratch, xyz, n, xyz, n, radius * (1.0 + 1.0 / 65536.0), nullptr, nullptr);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, a.nn.stride, "lr_normals_scratch_bytes(n)", LR_EINVAL, stream, nullptr));
    a.xyz = xyz; a.n = n; a.max_nn = max_nn; a.r2 = radius * radius; a.out = normals_out; a.info = info; a.n_nb = n_nb_out;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nm_info_kernel, dim3(1), dim3(64), 0, st, a, 0);
    nn_launch_grid(a.nn, st);
    hipLaunchKernelGGL(nm_kernel, dim3(lr_cdiv(n > 0 ? n : 1, 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(nm_info_kernel, dim3(1), dim3(64), 0, st, a, 1);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_normals(const double *xyz, int n, double radius, int max_nn, double *normals_out, int32_t *info, void *scratch,
                          size_t scratch_bytes, void *stream)
{
    return nm_run("lr_normals", xyz, n, radius, max_nn, normals_out, nullptr, info, scratch, scratch_bytes, stream);
}

extern "C" int lr_normals2(const double *xyz, int n, double radius, int max_nn, double *normals_out, int32_t *n_nb_out, int32_t *info,
                           void *scratch, size_t scratch_bytes, void *stream)
{
    return nm_run("lr_normals2", xyz, n, radius, max_nn, normals_out, n_nb_out, info, scratch, scratch_bytes, stream);
}
