// The grid and the search launches of the exact 3-D nearest neighbour (lr_nn3.hip), for the translation units that run them inside a
// sequence of their own (lr_bbrf.hip, lr_symicp.hip).  Internal: not part of the ABI.  The layout and the control block are what lr_nn3 / lr_refine_z
// use; *_scratch_bytes of either must not move when this file changes.  Needs lr_scratch.h alone (lr_al, lr_ptr): nothing of the
// correspondence-set front end.
#pragma once
#include "lr_scratch.h"

#define NN_MAX_N 4194304             // points per cloud (2^22)
#define NN_SHELL_CAP 3               // phase 1 walks shells 0..3 (up to 343 cells behind 119 ranges)
#define NN_MARGIN (1.0 - 1.0 / 524288.0)     // 1 - 2^-19
#define NN_OPEN (-2)                 // idx of a query phase 1 left open
#define NN_RUN 1024                  // run length of the two-level sum (contract Z6)
#define NN_FAR_BLOCKS 2048

struct nn_ctl {
    unsigned long long lo[3], hi[3];         // order-preserving images of the target's min / max
    double blo[3], bhi[3], cell;
    int32_t dim[3], ncell;
    int32_t n1_live, n1_dropped, n0_dropped, n_strag;
    // lr_refine_z
    int32_t done, repeats, n_valid, status;
    double dz, pending, last_step, med;
    unsigned long long hi_key;
};
static_assert(sizeof(nn_ctl) <= 512, "nn_ctl outgrew its slot");

struct nn_layout { size_t table, pts, pidx, blk, strag, idx, P0, zd, w, hist, part, end; };
struct nn_args {
    char *base;
    size_t stride;                           // (lr_ptr's form; always one arena)
    nn_layout L;
    const double *xyz0, *xyz1, *T;
    int32_t n0, n1, ncell_max, refine;
    double cell_user;
    int32_t *idx_out;                        // lr_nn3: the caller's; lr_refine_z: scratch
    double *dist_out;                        // lr_nn3 only
    double gate, min_change;
    int32_t max_repeats;
    lr_refine_z_result *res;
    const int32_t *stop;                     // nullable: a non-zero word here makes every grid / search kernel return at once (lr_bbrf's and lr_symicp's loops)
};

static size_t nn_cells_max(size_t n1) { return 4 * n1 > 4096 ? 4 * n1 : 4096; }
static size_t nn_make_layout(nn_layout *L, size_t n0, size_t n1, int refine)
{
    const size_t m0 = n0 > 0 ? n0 : 1, m1 = n1 > 0 ? n1 : 1;
    size_t o = 512;
    L->table = o; o += lr_al(nn_cells_max(n1) * 4);
    L->pts = o;   o += lr_al(m1 * 24);
    L->pidx = o;  o += lr_al(m1 * 4);
    L->blk = o;   o += lr_al((m0 / 256 + 2) * 4);
    L->strag = o; o += lr_al(m0 * 4);
    L->idx = L->P0 = L->zd = L->w = L->hist = L->part = o;
    if (refine) {
        L->idx = o;  o += lr_al(m0 * 4);
        L->P0 = o;   o += lr_al(m0 * 24);
        L->zd = o;   o += lr_al(m0 * 8);
        L->w = o;    o += lr_al(m0 * 8);
        L->hist = o; o += lr_al(8 * 256 * 4);
        L->part = o; o += lr_al((m0 / NN_RUN + 1) * 16);
    }
    L->end = o;
    return o;
}

#ifdef __HIPCC__
__device__ __forceinline__ nn_ctl *nn_c(const nn_args &g) { return lr_ptr<nn_ctl>(g, 0, 0); }
// a caller that runs these launches inside a device-side loop of its own (lr_bbrf) names the word that ends it; lr_nn3 / lr_refine_z pass none
__device__ __forceinline__ bool nn_stopped(const nn_args &g) { return g.stop && *g.stop; }
// clamped cell of a coordinate: 0 .. dim - 1, NaN and everything below the grid to 0
__device__ __forceinline__ int nn_cell(double p, double lo, double cell, int dim)
{
    double v = floor((p - lo) / cell);
    if (!(v >= 0.0)) v = 0.0;
    if (!(v <= (double)(dim - 1))) v = (double)(dim - 1);
    return (int)v;
}
#endif

// lr_nn3.hip.  g describes one arena (base, L from nn_make_layout), the queries xyz0 [n0] and the target xyz1 [n1], idx_out [n0];
// nn_launch_grid buckets the target (six launches), nn_launch_search writes idx_out (and dist_out where given) by contract N.
void nn_set_args(nn_args *g, void *arena, const double *xyz0, int n0, const double *xyz1, int n1, double cell, int32_t *idx_out,
                 const int32_t *stop);
void nn_launch_grid(const nn_args &g, hipStream_t st);
void nn_launch_search(const nn_args &g, hipStream_t st);
