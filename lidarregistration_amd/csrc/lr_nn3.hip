// The exact, unbounded 3-D nearest neighbour (lr_nn3) and the Z-only refinement of a ground-truth motion built on it (lr_refine_z), on gfx950.
//
// Replaces the balanced-set generator's NN (BalancedDatasetGenerator/GenerateBalancedSet.py:149-153, cKDTree.query(k = 1)) and its
// refine_motion_Z_only (:257-291).  Contract N / Z: include/lidarreg.h; restated in tests/refine_z_cpu.py.
//
// Structure.  The target's finite points are bucketed once into a dense uniform grid over their bounding box (counting sort; the order
// inside a cell is irrelevant: the argmin carries (d2, j) and the lowest j wins a tie).  table[c] ends up as the END of cell c in the
// bucketed arrays, so a run of cells along x is one contiguous range behind two loads, and an empty cell costs one.
//   phase 1: one lane per query walks the Chebyshev shells s = 0, 1, .. around its clamped cell and stops once its best d2 is strictly
//            below a lower bound on every point of the shells beyond s (nn_settled: shrunk by 2^-19, which covers the rounding of the cell
//            quotients and of d2), or once the shells cover the grid.  A query still open after NN_SHELL_CAP shells is flagged;
//   phase 2: the flagged queries, compacted in index order, are resolved one per wave by streaming the bucketed target.
// lr_refine_z builds the grid once and runs every repeat as the same fixed sequence of launches: NN, the valid pairs and their weights,
// an exact radix select of the weights' median on their bit patterns (8 passes of 8 bits; every block re-derives the prefix from the
// finished histograms, so no pass needs a host decision), the two-level sums in their contractual order, the step.  A finished call's
// remaining launches return at their first instruction.  No floating-point atomic; every word read was written by a kernel of the call.
#include "lr_prims.h"
#include "lr_nn3.h"
#include <math.h>
#include <string.h>

// (d2, j) argmin: smaller d2, then smaller j; j = -1 (nothing yet) loses to every j
__device__ __forceinline__ void nn_take(double d2, int j, double &best, int &bj)
{
    if (d2 < best || (d2 == best && (unsigned)j < (unsigned)bj)) { best = d2; bj = j; }
}

// ---- the grid ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nn_init_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    int32_t *table = lr_ptr<int32_t>(g, 0, g.L.table);
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < (size_t)g.ncell_max; s += (size_t)gridDim.x * 256) table[s] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        nn_ctl *c = nn_c(g);
        for (int a = 0; a < 3; ++a) { c->lo[a] = ~0ull; c->hi[a] = 0ull; c->blo[a] = 0.0; c->bhi[a] = 0.0; c->dim[a] = 1; }
        c->cell = 1.0; c->ncell = 1;
        c->n1_live = 0; c->n1_dropped = 0; c->n0_dropped = 0; c->n_strag = 0;
        c->done = 0; c->repeats = 0; c->n_valid = 0; c->status = 0;
        c->dz = 0.0; c->pending = 0.0; c->last_step = 0.0; c->med = 0.0; c->hi_key = ~0ull;
    }
}

__global__ void __launch_bounds__(256) nn_bounds_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    nn_ctl *c = nn_c(g);
    const int j = blockIdx.x * 256 + threadIdx.x;
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    bool bad = false;
    if (j < g.n1) {
        const double p[3] = { g.xyz1[3 * (size_t)j], g.xyz1[3 * (size_t)j + 1], g.xyz1[3 * (size_t)j + 2] };
        bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
        if (!bad)
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = p[a]; hi[a] = p[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], m)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], m)); }
    const unsigned long long nbad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (lo[a] <= hi[a]) { atomicMin(&c->lo[a], lr_ord_enc(lo[a])); atomicMax(&c->hi[a], lr_ord_enc(hi[a])); }
        if (nbad) atomicAdd(&c->n1_dropped, __popcll(nbad));
    }
}

// cells per axis at edge `cell`, as doubles; false when the grid would outgrow the table
__device__ static bool nn_fits(const double ext[3], double cell, double cap, int dim[3])
{
    double prod = 1.0;
    for (int a = 0; a < 3; ++a) {
        double d = floor(ext[a] / cell) + 1.0;
        if (!(d >= 1.0)) d = 1.0;                    // NaN (inf / inf)
        if (!(d <= cap)) return false;
        dim[a] = (int)d;
        prod *= d;
    }
    return prod <= cap;
}

// The cell rule (N6).  cell == 0: the finest edge E 2^(-k/2), k = 0 .. 80, E the bounding box's longest edge, whose grid has at most
// max(4096, 4 n1) cells; cell > 0: that edge, doubled until the grid fits.  A box without extent is one cell.
__global__ void nn_grid_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    if (threadIdx.x != 0) return;
    nn_ctl *c = nn_c(g);
    c->n1_live = g.n1 - c->n1_dropped;
    if (c->n1_live <= 0) { c->n1_live = 0; return; }
    double ext[3], E = 0.0;
    for (int a = 0; a < 3; ++a) {
        c->blo[a] = lr_ord_dec(c->lo[a]); c->bhi[a] = lr_ord_dec(c->hi[a]);
        ext[a] = c->bhi[a] - c->blo[a];
        E = ext[a] > E ? ext[a] : E;
    }
    const double cap = (double)g.ncell_max;
    int dim[3] = { 1, 1, 1 }, trial[3];
    double cell = 1.0;
    if (E > 0.0) {
        if (g.cell_user > 0.0) {
            cell = g.cell_user;
            for (int k = 0; k < 2200 && !nn_fits(ext, cell, cap, trial); ++k) cell = cell * 2.0;
            if (!nn_fits(ext, cell, cap, dim)) { dim[0] = dim[1] = dim[2] = 1; }
        } else {
            cell = E;                                // k = 0: at most 2 x 2 x 2 cells
            nn_fits(ext, cell, cap, dim);
            double pw = 1.0;
            for (int k = 1; k <= 80; ++k) {
                if (!(k & 1)) pw = pw * 0.5;
                const double t = (k & 1) ? (E * pw) * 0.70710678118654752 : E * pw;
                if (!(t > 0.0) || !nn_fits(ext, t, cap, trial)) break;
                cell = t; dim[0] = trial[0]; dim[1] = trial[1]; dim[2] = trial[2];
            }
        }
    }
    c->cell = cell;
    for (int a = 0; a < 3; ++a) c->dim[a] = dim[a];
    c->ncell = dim[0] * dim[1] * dim[2];
}

__device__ __forceinline__ int nn_lin(const nn_ctl *c, const double *p)
{
    const int x = nn_cell(p[0], c->blo[0], c->cell, c->dim[0]), y = nn_cell(p[1], c->blo[1], c->cell, c->dim[1]), z = nn_cell(p[2], c->blo[2], c->cell, c->dim[2]);
    return (z * c->dim[1] + y) * c->dim[0] + x;      // < ncell <= ncell_max
}

__global__ void __launch_bounds__(256) nn_count_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    const nn_ctl *c = nn_c(g);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n1) return;
    const double p[3] = { g.xyz1[3 * (size_t)j], g.xyz1[3 * (size_t)j + 1], g.xyz1[3 * (size_t)j + 2] };
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return;
    atomicAdd(&lr_ptr<int32_t>(g, 0, g.L.table)[nn_lin(c, p)], 1);
}

__global__ void __launch_bounds__(1024) nn_scan_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    lr_block_exscan(lr_ptr<int32_t>(g, 0, g.L.table), (size_t)nn_c(g)->ncell);
}

// after this kernel table[c] = end of cell c; its start is table[c - 1] (0 for c = 0)
__global__ void __launch_bounds__(256) nn_scatter_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    const nn_ctl *c = nn_c(g);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n1) return;
    const double p[3] = { g.xyz1[3 * (size_t)j], g.xyz1[3 * (size_t)j + 1], g.xyz1[3 * (size_t)j + 2] };
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return;
    // starts + fills stay below n1_live <= n1 (the counts sum to it)
    const int at = atomicAdd(&lr_ptr<int32_t>(g, 0, g.L.table)[nn_lin(c, p)], 1);
    double *out = lr_ptr<double>(g, 0, g.L.pts) + 3 * (size_t)at;
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
    lr_ptr<int32_t>(g, 0, g.L.pidx)[at] = j;
}

// ---- phase 1 -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void nn_scan_range(const double *__restrict__ pts, const int32_t *__restrict__ pidx, int s, int e, double qx, double qy, double qz,
                                              double &best, int &bj)
{
    for (int u = s; u < e; ++u) {
        const double dx = qx - pts[3 * (size_t)u], dy = qy - pts[3 * (size_t)u + 1], dz = qz - pts[3 * (size_t)u + 2];
        nn_take((dx * dx + dy * dy) + dz * dz, pidx[u], best, bj);
    }
}

// Lower bound on the computed d2 of every target point in a shell beyond s: along the axis that puts the point there
// the distance is at least ex + s cell (1 - 2^-26), along the others at least ex (the query's distance to the box, 0 inside), so
// d2 >= ex2 + (s cell)^2 up to rounding; the factor 1 - 2^-19 covers the quotients' and d2's rounding.  Outside 1e-290 .. 1e300 the
// relative-error argument does not hold (underflow, overflow): no bound, the walk goes on.
__device__ __forceinline__ bool nn_settled(double best, double ex2, int s, double cell)
{
    const double sc = (double)s * cell, lb2 = (ex2 + sc * sc) * NN_MARGIN;
    return lb2 > 1e-290 && lb2 < 1e300 && best < lb2;
}

__global__ void __launch_bounds__(256) nn_walk_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    nn_ctl *c = nn_c(g);
    if (g.refine && c->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int32_t *idx_out = g.refine ? lr_ptr<int32_t>(g, 0, g.L.idx) : g.idx_out;
    bool open = false, bad = false;
    if (i < g.n0) {
        double q[3];
        if (g.refine) {
            double *P0 = lr_ptr<double>(g, 0, g.L.P0) + 3 * (size_t)i;
            q[0] = P0[0]; q[1] = P0[1];
            q[2] = P0[2] - c->pending;               // the previous repeat's step (Z7); 0 before the first
            P0[2] = q[2];
        } else {
            q[0] = g.xyz0[3 * (size_t)i]; q[1] = g.xyz0[3 * (size_t)i + 1]; q[2] = g.xyz0[3 * (size_t)i + 2];
        }
        bad = !(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]));
        double best = INFINITY;
        int bj = -1;
        if (!bad && c->n1_live > 0) {
            const int32_t *table = lr_ptr<int32_t>(g, 0, g.L.table), *pidx = lr_ptr<int32_t>(g, 0, g.L.pidx);
            const double *pts = lr_ptr<double>(g, 0, g.L.pts);
            const int dx = c->dim[0], dy = c->dim[1], dz = c->dim[2];
            const double cell = c->cell;
            const int cx = nn_cell(q[0], c->blo[0], cell, dx), cy = nn_cell(q[1], c->blo[1], cell, dy), cz = nn_cell(q[2], c->blo[2], cell, dz);
            double ex2 = 0.0;
            {
                double e[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double below = c->blo[a] - q[a], above = q[a] - c->bhi[a];
                    e[a] = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
                }
                ex2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            }
            open = true;
            for (int s = 0; s <= NN_SHELL_CAP && open; ++s) {
                const int z0 = cz - s > 0 ? cz - s : 0, z1 = cz + s < dz - 1 ? cz + s : dz - 1;
                const int y0 = cy - s > 0 ? cy - s : 0, y1 = cy + s < dy - 1 ? cy + s : dy - 1;
                const int x0 = cx - s > 0 ? cx - s : 0, x1 = cx + s < dx - 1 ? cx + s : dx - 1;
                for (int zz = z0; zz <= z1; ++zz)
                    for (int yy = y0; yy <= y1; ++yy) {
                        const int row = (zz * dy + yy) * dx;
                        const bool face = zz - cz == s || cz - zz == s || yy - cy == s || cy - yy == s;
                        if (face) {                  // the whole run of cells along x
                            const int l0 = row + x0, l1 = row + x1;
                            nn_scan_range(pts, pidx, l0 > 0 ? table[l0 - 1] : 0, table[l1], q[0], q[1], q[2], best, bj);
                        } else {                     // the shell's two end cells of this row (s >= 1)
                            if (cx - s >= 0) { const int l = row + cx - s; nn_scan_range(pts, pidx, l > 0 ? table[l - 1] : 0, table[l], q[0], q[1], q[2], best, bj); }
                            if (cx + s <= dx - 1) { const int l = row + cx + s; nn_scan_range(pts, pidx, table[l - 1], table[l], q[0], q[1], q[2], best, bj); }
                        }
                    }
                const bool all = cx - s <= 0 && cx + s >= dx - 1 && cy - s <= 0 && cy + s >= dy - 1 && cz - s <= 0 && cz + s >= dz - 1;
                if (all || nn_settled(best, ex2, s, cell)) open = false;
            }
        }
        idx_out[i] = open ? NN_OPEN : bj;
        if (!open && g.dist_out) g.dist_out[i] = __dsqrt_rn(best);
    }
    const unsigned long long nbad = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && nbad && c->repeats == 0) atomicAdd(&c->n0_dropped, __popcll(nbad));
    lr_block_count(open, lr_ptr<int32_t>(g, 0, g.L.blk));
}

// the open queries in index order; block 0 also clears the words the repeat's later kernels accumulate into
__global__ void __launch_bounds__(256) nn_strag_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    __shared__ int s_w[4], s_p[4];
    nn_ctl *c = nn_c(g);
    if (g.refine && c->done) return;
    if (g.refine && blockIdx.x == 0) {
        int32_t *hist = lr_ptr<int32_t>(g, 0, g.L.hist);
        for (int k = threadIdx.x; k < 8 * 256; k += 256) hist[k] = 0;
        if (threadIdx.x == 0) { c->n_valid = 0; c->hi_key = ~0ull; }
    }
    const int before = lr_blocks_before(lr_ptr<int32_t>(g, 0, g.L.blk)), i = blockIdx.x * 256 + threadIdx.x;
    const int32_t *idx = g.refine ? lr_ptr<int32_t>(g, 0, g.L.idx) : g.idx_out;
    const bool k = i < g.n0 && idx[i] == NN_OPEN;
    int prefix;
    const int slot = lr_ordered_slot(k, before, s_w, s_p, prefix);
    if (k) lr_ptr<int32_t>(g, 0, g.L.strag)[slot] = i;      // slot < n0: the flags set number at most n0
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) c->n_strag = prefix + s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// ---- phase 2: one wave per open query streams the bucketed target ------------------------------------------------------------------
__global__ void __launch_bounds__(256) nn_far_kernel(nn_args g)
{
    if (nn_stopped(g)) return;
    const nn_ctl *c = nn_c(g);
    if (g.refine && c->done) return;
    const int ns = c->n_strag, n1 = c->n1_live, lane = threadIdx.x & 63;
    const int32_t *strag = lr_ptr<int32_t>(g, 0, g.L.strag), *pidx = lr_ptr<int32_t>(g, 0, g.L.pidx);
    const double *pts = lr_ptr<double>(g, 0, g.L.pts);
    int32_t *idx_out = g.refine ? lr_ptr<int32_t>(g, 0, g.L.idx) : g.idx_out;
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < ns; k += gridDim.x * 4) {
        const int i = strag[k];
        double q[3];
        if (g.refine) { const double *P0 = lr_ptr<double>(g, 0, g.L.P0) + 3 * (size_t)i; q[0] = P0[0]; q[1] = P0[1]; q[2] = P0[2]; }
        else { q[0] = g.xyz0[3 * (size_t)i]; q[1] = g.xyz0[3 * (size_t)i + 1]; q[2] = g.xyz0[3 * (size_t)i + 2]; }
        double best = INFINITY;
        int bj = -1;
        for (int u = lane; u < n1; u += 64) {
            const double dx = q[0] - pts[3 * (size_t)u], dy = q[1] - pts[3 * (size_t)u + 1], dz = q[2] - pts[3 * (size_t)u + 2];
            nn_take((dx * dx + dy * dy) + dz * dz, pidx[u], best, bj);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nn_take(__shfl_xor(best, m), __shfl_xor(bj, m), best, bj);
        if (lane == 0) {
            idx_out[i] = bj;
            if (g.dist_out) g.dist_out[i] = __dsqrt_rn(best);
        }
    }
}

__global__ void nn_info_kernel(nn_args g, int32_t *info)
{
    if (threadIdx.x != 0) return;
    const nn_ctl *c = nn_c(g);
    info[0] = c->n1_live > 0 ? 0 : 1; info[1] = c->n0_dropped; info[2] = c->n1_dropped; info[3] = c->n_strag;
}

// ---- lr_refine_z ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rz_xform_kernel(nn_args g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n0) return;
    const double x = g.xyz0[3 * (size_t)i], y = g.xyz0[3 * (size_t)i + 1], z = g.xyz0[3 * (size_t)i + 2];
    double p[3] = { x, y, z };
    if (g.T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = ((g.T[4 * a] * x + g.T[4 * a + 1] * y) + g.T[4 * a + 2] * z) + g.T[4 * a + 3];
    }
    double *P0 = lr_ptr<double>(g, 0, g.L.P0) + 3 * (size_t)i;
    P0[0] = p[0]; P0[1] = p[1]; P0[2] = p[2];
}

// block-wide (256 threads): adds this block's digit counts s_h[0..255] to the pass's histogram
__device__ __forceinline__ void rz_flush(int *s_h, int32_t *hist)
{
    __syncthreads();
    const int v = s_h[threadIdx.x];
    if (v) atomicAdd(&hist[threadIdx.x], v);
}

// Z2 / Z3 and the select's first pass (the keys' top byte)
__global__ void __launch_bounds__(256) rz_pair_kernel(nn_args g)
{
    __shared__ int s_h[256];
    nn_ctl *c = nn_c(g);
    if (c->done) return;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (i < g.n0) {
        const int j = lr_ptr<int32_t>(g, 0, g.L.idx)[i];
        double zd = 0.0, w = -1.0;
        if (j >= 0) {
            const double *P0 = lr_ptr<double>(g, 0, g.L.P0) + 3 * (size_t)i, *b = g.xyz1 + 3 * (size_t)j;
            const double dx = P0[0] - b[0], dy = P0[1] - b[1];
            if (__dsqrt_rn(dx * dx + dy * dy) <= g.gate) {
                valid = true;
                zd = P0[2] - b[2];
                w = 1.0 / fabs(zd);
                atomicAdd(&s_h[(int)((unsigned long long)__double_as_longlong(w) >> 56)], 1);
            }
        }
        lr_ptr<double>(g, 0, g.L.zd)[i] = zd;
        lr_ptr<double>(g, 0, g.L.w)[i] = w;          // negative: not a valid pair
    }
    const unsigned long long bal = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&c->n_valid, __popcll(bal));
    rz_flush(s_h, lr_ptr<int32_t>(g, 0, g.L.hist));
}

// block-wide (256 threads): the leading 8 npass bits of the key of rank `rank` (0-based, ascending) from the finished histograms of
// passes 0 .. npass - 1; less = keys below that prefix, eq = keys with it.  The keys number more than `rank`.
__device__ __forceinline__ unsigned long long rz_select(const int32_t *hist, int npass, int rank, int &less, int &eq)
{
    __shared__ int s_w[4], s_d, s_ex, s_cn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long key = 0;
    less = 0; eq = 0;
    for (int p = 0; p < npass; ++p) {
        const int cn = hist[p * 256 + tid], incl = lr_wave_incl_scan(cn, lane);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int ex = incl - cn;
        for (int w = 0; w < wave; ++w) ex += s_w[w];
        if (cn > 0 && ex <= rank && rank < ex + cn) { s_d = tid; s_ex = ex; s_cn = cn; }     // exactly one digit
        __syncthreads();
        key = (key << 8) | (unsigned long long)s_d;
        less += s_ex; rank -= s_ex; eq = s_cn;
        __syncthreads();
    }
    return key;
}

// pass 1 .. 7: the next digit's counts among the keys that share the prefix found so far
__global__ void __launch_bounds__(256) rz_hist_kernel(nn_args g, int pass)
{
    __shared__ int s_h[256];
    const nn_ctl *c = nn_c(g);
    if (c->done) return;
    const int nv = c->n_valid;
    if (nv == 0) return;
    int32_t *hist = lr_ptr<int32_t>(g, 0, g.L.hist);
    int less, eq;
    const unsigned long long prefix = rz_select(hist, pass, (nv - 1) >> 1, less, eq);
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.n0) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(lr_ptr<double>(g, 0, g.L.w)[i]);
        if (!(key >> 63) && (key >> (64 - 8 * pass)) == prefix) atomicAdd(&s_h[(int)((key >> (56 - 8 * pass)) & 255)], 1);
    }
    rz_flush(s_h, hist + pass * 256);
}

// the lower middle key `lo` is known after 8 passes; an even count whose upper middle is not a copy of lo needs the smallest key above lo
__device__ __forceinline__ bool rz_needs_hi(int nv, int less, int eq) { return !(nv & 1) && less + eq < ((nv - 1) >> 1) + 2; }

__global__ void __launch_bounds__(256) rz_min_kernel(nn_args g)
{
    nn_ctl *c = nn_c(g);
    if (c->done) return;
    const int nv = c->n_valid;
    if (nv == 0) return;
    int less, eq;
    const unsigned long long lo = rz_select(lr_ptr<int32_t>(g, 0, g.L.hist), 8, (nv - 1) >> 1, less, eq);
    if (!rz_needs_hi(nv, less, eq)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long m = ~0ull;
    if (i < g.n0) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(lr_ptr<double>(g, 0, g.L.w)[i]);
        if (!(key >> 63) && key > lo) m = key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(m, d); m = o < m ? o : m; }
    if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(&c->hi_key, m);
}

// Z4 .. Z6, first level: the median, the capped weights, and every run of 1024 indices summed left to right by one wave -- 64 loads in
// flight, the additions in index order on every lane
__global__ void __launch_bounds__(256) rz_runs_kernel(nn_args g)
{
    nn_ctl *c = nn_c(g);
    if (c->done) return;
    const int nv = c->n_valid;
    if (nv == 0) return;
    int less, eq;
    const unsigned long long lo = rz_select(lr_ptr<int32_t>(g, 0, g.L.hist), 8, (nv - 1) >> 1, less, eq);
    const double vlo = __longlong_as_double((long long)lo);
    double med = vlo;
    if (!(nv & 1)) {
        const double vhi = rz_needs_hi(nv, less, eq) ? __longlong_as_double((long long)c->hi_key) : vlo;
        med = (vlo + vhi) / 2.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) c->med = med;
    const int lane = threadIdx.x & 63, run = blockIdx.x * 4 + (threadIdx.x >> 6), nruns = (g.n0 + NN_RUN - 1) / NN_RUN;
    if (run >= nruns) return;
    const double *zd = lr_ptr<double>(g, 0, g.L.zd), *w = lr_ptr<double>(g, 0, g.L.w);
    const int begin = run * NN_RUN, end = begin + NN_RUN < g.n0 ? begin + NN_RUN : g.n0;
    double num = 0.0, den = 0.0;
    for (int base = begin; base < end; base += 64) {
        const int m = end - base < 64 ? end - base : 64;
        double tn = 0.0, td = 0.0;
        if (lane < m) {
            const double wi = w[base + lane];
            if (!(wi < 0.0)) { td = wi > med ? med : wi; tn = td * zd[base + lane]; }
        }
        for (int j = 0; j < m; ++j) { num += __shfl(tn, j); den += __shfl(td, j); }
    }
    if (lane == 0) { double *part = lr_ptr<double>(g, 0, g.L.part) + 2 * (size_t)run; part[0] = num; part[1] = den; }
}

// Z6 second level, Z7, Z8 and the result block
__global__ void __launch_bounds__(64) rz_step_kernel(nn_args g)
{
    nn_ctl *c = nn_c(g);
    if (c->done) return;
    const int lane = threadIdx.x, nv = c->n_valid, nruns = (g.n0 + NN_RUN - 1) / NN_RUN;
    double num = 0.0, den = 0.0;
    if (nv > 0) {
        const double *part = lr_ptr<double>(g, 0, g.L.part);
        for (int base = 0; base < nruns; base += 64) {
            const int m = nruns - base < 64 ? nruns - base : 64;
            double tn = 0.0, td = 0.0;
            if (lane < m) { tn = part[2 * (size_t)(base + lane)]; td = part[2 * (size_t)(base + lane) + 1]; }
            for (int j = 0; j < m; ++j) { num += __shfl(tn, j); den += __shfl(td, j); }
        }
    }
    if (lane != 0) return;
    int status = 0;
    double mean = 0.0;
    if (nv == 0) status = 1;
    else if (c->med == INFINITY) status = 2;
    else mean = num / den;
    c->pending = mean;
    c->dz = c->dz - mean;
    c->last_step = mean;
    c->repeats = c->repeats + 1;
    c->status = status;
    if (status != 0 || fabs(mean) < g.min_change || c->repeats >= g.max_repeats) c->done = 1;
    lr_refine_z_result r;
    r.status = status; r.repeats = c->repeats; r.n_valid = nv; r.n0_dropped = c->n0_dropped; r.n1_dropped = c->n1_dropped; r.reserved = 0;
    r.dz = c->dz; r.last_step = mean;
    *g.res = r;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_nn3_params) == 16 && sizeof(lr_refine_z_params) == 32 && sizeof(lr_refine_z_result) == 40,
              "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

extern "C" size_t lr_nn3_scratch_bytes(int n0, int n1)
{
    if (n0 < 0 || n0 > NN_MAX_N || n1 < 0 || n1 > NN_MAX_N) return 0;
    nn_layout L;
    return nn_make_layout(&L, (size_t)n0, (size_t)n1, 0);
}

extern "C" size_t lr_refine_z_scratch_bytes(int n0, int n1)
{
    if (n0 < 0 || n0 > NN_MAX_N || n1 < 0 || n1 > NN_MAX_N) return 0;
    nn_layout L;
    return nn_make_layout(&L, (size_t)n0, (size_t)n1, 1);
}

// the cloud checks of lr_nn3 / lr_refine_z; g = the call's arguments as far as the two share them, g->stride = the scratch it needs
static int nn_check_common(const char *who, const double *xyz0, int n0, const double *xyz1, int n1, double cell, int refine, nn_args *g)
{
    LR_REFUSE_UNLESS(cell == 0.0 || (cell > 0.0 && isfinite(cell)), LR_EINVAL, "cell must be 0 (automatic) or positive and finite");
    LR_REFUSE_UNLESS(n0 >= 0 && n0 <= NN_MAX_N && n1 >= 0 && n1 <= NN_MAX_N, LR_EINVAL, "n0 / n1 must lie in 0..4194304");
    LR_REFUSE_UNLESS(n0 == 0 || xyz0, LR_EINVAL, "null xyz0");
    LR_REFUSE_UNLESS(n1 == 0 || xyz1, LR_EINVAL, "null xyz1");
    memset(g, 0, sizeof *g);
    g->stride = nn_make_layout(&g->L, (size_t)n0, (size_t)n1, refine);
    g->xyz0 = xyz0; g->xyz1 = xyz1; g->n0 = n0; g->n1 = n1;
    g->ncell_max = (int32_t)nn_cells_max((size_t)n1);
    g->refine = refine; g->cell_user = cell;
    return LR_OK;
}

void nn_set_args(nn_args *g, void *arena, const double *xyz0, int n0, const double *xyz1, int n1, double cell, int32_t *idx_out,
                 const int32_t *stop)
{
    memset(g, 0, sizeof *g);
    g->stride = nn_make_layout(&g->L, (size_t)n0, (size_t)n1, 0);
    g->base = reinterpret_cast<char *>(arena);
    g->xyz0 = xyz0; g->xyz1 = xyz1; g->n0 = n0; g->n1 = n1;
    g->ncell_max = (int32_t)nn_cells_max((size_t)n1);
    g->cell_user = cell; g->idx_out = idx_out; g->stop = stop;
}

void nn_launch_grid(const nn_args &g, hipStream_t st)
{
    const int nb1 = lr_cdiv(g.n1 > 0 ? g.n1 : 1, 256);
    const int ib = lr_cdiv(g.ncell_max, 256) < 1024 ? lr_cdiv(g.ncell_max, 256) : 1024;
    hipLaunchKernelGGL(nn_init_kernel, dim3(ib), dim3(256), 0, st, g);
    hipLaunchKernelGGL(nn_bounds_kernel, dim3(nb1), dim3(256), 0, st, g);
    hipLaunchKernelGGL(nn_grid_kernel, dim3(1), dim3(64), 0, st, g);
    hipLaunchKernelGGL(nn_count_kernel, dim3(nb1), dim3(256), 0, st, g);
    hipLaunchKernelGGL(nn_scan_kernel, dim3(1), dim3(1024), 0, st, g);
    hipLaunchKernelGGL(nn_scatter_kernel, dim3(nb1), dim3(256), 0, st, g);
}

void nn_launch_search(const nn_args &g, hipStream_t st)
{
    const int nb0 = lr_cdiv(g.n0 > 0 ? g.n0 : 1, 256);
    const int fb = lr_cdiv(g.n0 > 0 ? g.n0 : 1, 4) < NN_FAR_BLOCKS ? lr_cdiv(g.n0 > 0 ? g.n0 : 1, 4) : NN_FAR_BLOCKS;
    hipLaunchKernelGGL(nn_walk_kernel, dim3(nb0), dim3(256), 0, st, g);
    hipLaunchKernelGGL(nn_strag_kernel, dim3(nb0), dim3(256), 0, st, g);
    hipLaunchKernelGGL(nn_far_kernel, dim3(fb), dim3(256), 0, st, g);
}

extern "C" int lr_nn3(const double *xyz0, int n0, const double *xyz1, int n1, const lr_nn3_params *p, int32_t *idx, double *dist,
                      int32_t *info, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_nn3";
    LR_CHECK_STRUCT_SIZE(lr_nn3_params, p, who);
    LR_REFUSE_UNLESS(info, LR_EINVAL, "null info");
    LR_REFUSE_UNLESS(n0 <= 0 || (idx && dist), LR_EINVAL, "null idx / dist");
    nn_args g;
    LR_TRY_HIP(nn_check_common(who, xyz0, n0, xyz1, n1, p->cell, 0, &g));
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, g.stride, "lr_nn3_scratch_bytes(n0, n1)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch);
    g.idx_out = idx; g.dist_out = dist;
    hipStream_t st = (hipStream_t)stream;
    nn_launch_grid(g, st);
    nn_launch_search(g, st);
    hipLaunchKernelGGL(nn_info_kernel, dim3(1), dim3(64), 0, st, g, info);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_refine_z(const double *xyz0, int n0, const double *xyz1, int n1, const double *T, const lr_refine_z_params *p,
                           lr_refine_z_result *result, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_refine_z";
    LR_CHECK_STRUCT_SIZE(lr_refine_z_params, p, who);
    LR_REFUSE_UNLESS(p->max_repeats >= 1 && p->max_repeats <= 64, LR_EINVAL, "max_repeats must lie in 1..64");
    LR_REFUSE_UNLESS(p->xy_gate > 0.0 && isfinite(p->xy_gate), LR_EINVAL, "xy_gate must be positive and finite");
    LR_REFUSE_UNLESS(p->min_change >= 0.0 && isfinite(p->min_change), LR_EINVAL, "min_change must be finite and not negative");
    LR_REFUSE_UNLESS(result, LR_EINVAL, "null result");
    nn_args g;
    LR_TRY_HIP(nn_check_common(who, xyz0, n0, xyz1, n1, p->cell, 1, &g));
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, g.stride, "lr_refine_z_scratch_bytes(n0, n1)", LR_EINVAL, stream, nullptr));
    g.base = reinterpret_cast<char *>(scratch);
    g.T = T; g.gate = p->xy_gate; g.min_change = p->min_change; g.max_repeats = p->max_repeats; g.res = result;
    hipStream_t st = (hipStream_t)stream;
    const int nb0 = lr_cdiv(n0 > 0 ? n0 : 1, 256), rb = lr_cdiv(lr_cdiv(n0 > 0 ? n0 : 1, NN_RUN), 4);
    nn_launch_grid(g, st);
    hipLaunchKernelGGL(rz_xform_kernel, dim3(nb0), dim3(256), 0, st, g);
    for (int rep = 0; rep < p->max_repeats; ++rep) {
        nn_launch_search(g, st);
        hipLaunchKernelGGL(rz_pair_kernel, dim3(nb0), dim3(256), 0, st, g);
        for (int pass = 1; pass < 8; ++pass) hipLaunchKernelGGL(rz_hist_kernel, dim3(nb0), dim3(256), 0, st, g, pass);
        hipLaunchKernelGGL(rz_min_kernel, dim3(nb0), dim3(256), 0, st, g);
        hipLaunchKernelGGL(rz_runs_kernel, dim3(rb), dim3(256), 0, st, g);
        hipLaunchKernelGGL(rz_step_kernel, dim3(1), dim3(64), 0, st, g);
    }
    LR_LAUNCH_CHECK();
    return LR_OK;
}
