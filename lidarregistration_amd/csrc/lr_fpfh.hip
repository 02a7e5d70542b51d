// lr_fpfh: Fast Point Feature Histograms (33 numbers per point) on the grid of the exact 3-D nearest neighbour, on gfx950.  Open3D 0.13's
// compute_fpfh_feature is not vendored: its algorithm is upstream-recalled, the contract F1..F6 of include/lidarreg.h is the specification
// (restated in numpy in tests/fpfh_cpu.py) and these kernels equal it bit for bit in fp64 -- every operation below is one IEEE operation in
// the contract's order (the library is built with -ffp-contract=off), the square roots __dsqrt_rn.
//
//   fp_info_kernel   zeroes info / writes the status
//   grid             nn_launch_grid (lr_nn3.h) over the cloud itself, cell = radius (1 + 2^-16) as lr_normals: everything within the radius
//                    of a point sits in the 27 cells around it
//   fp_list_kernel   F1, once: a wave per query gathers the in-radius points of the 27 cells, 64 candidates at a time, into its LDS buffer
//                    of 256 (d2, index) entries; when the buffer runs full, and at the end, every entry counts the entries before it under
//                    (d2, index) -- that rank is its place in the list, ranks >= max_nn leave -- and from then on only candidates before the
//                    list's last entry are let in.  The lists go to scratch ([n][max_nn] indices, [n] lengths); later stages read them twice
//   fp_spfh_kernel   F2..F4: a wave per point, a lane per neighbour: the pair feature's three bins, counted with integer LDS atomics (the
//                    count does not depend on the order), times 100 / k
//   fp_fpfh_kernel   F5: a wave per point, a lane per bin: the serial chain over the list in list order, the 11-block sums, the output(s)
// No host synchronisation, no floating-point atomics, no stop word.
#include "lr_nn3.h"
#include <math.h>
#include <string.h>

#define FP_MAX_NN 128
#define FP_MIN_NN 2
#define FP_BUF 256               // entries of a wave's candidate buffer: max_nn kept + up to two chunks of 64 let in before the next ranking
#define FP_BINS 33

struct fp_layout { size_t nn, cnt, lists, spfh, end; };
struct fp_args {
    nn_args nn;                  // the cloud against itself: the grid's arena (at offset 0 of the scratch)
    char *base; size_t stride;
    fp_layout L;
    const double *xyz, *nrm;
    int32_t n, max_nn;
    double r2;
    double *out64; float *out32;
    int32_t *info;
};

static inline size_t fp_make_layout(fp_layout *L, size_t n, size_t max_nn)
{
    nn_layout G;
    size_t o = 0;
    L->nn = o;    o += lr_al(nn_make_layout(&G, n, n, 0));
    L->cnt = o;   o += lr_al((n > 0 ? n : 1) * sizeof(int32_t));
    L->lists = o; o += lr_al((n > 0 ? n : 1) * max_nn * sizeof(int32_t));
    L->spfh = o;  o += lr_al((n > 0 ? n : 1) * FP_BINS * sizeof(double));
    L->end = o;
    return o;
}

// F3: the ten bin edges of the angle feature turned by pi, direction 2 pi e / 11 for e = 1..10
__device__ static const double fp_edge_c[10] = { 0.8412535328311812, 0.41541501300188644, -0.142314838273285, -0.654860733945285, -0.9594929736144974,
                                                 -0.9594929736144975, -0.6548607339452852, -0.14231483827328523, 0.41541501300188605, 0.8412535328311812 };
__device__ static const double fp_edge_s[10] = { 0.5406408174555976, 0.9096319953545183, 0.9898214418809328, 0.7557495743542583, 0.28173255684142967,
                                                 -0.2817325568414294, -0.7557495743542582, -0.9898214418809327, -0.9096319953545186, -0.5406408174555974 };

__device__ __forceinline__ int fp_angle_bin(double y, double x)
{
    const double xr = -x, yr = -y;
    if (y < 0.0) {
        int b = 0;
#pragma unroll
        for (int e = 0; e < 5; ++e) b += (fp_edge_c[e] * yr - fp_edge_s[e] * xr) >= 0.0;
        return b;
    }
    if (y > 0.0) {
        int b = 5;
#pragma unroll
        for (int e = 5; e < 10; ++e) b += (fp_edge_c[e] * yr - fp_edge_s[e] * xr) >= 0.0;
        return b;
    }
    if (y == 0.0 && x < 0.0) return __builtin_signbit(y) ? 0 : 10;
    return 5;
}

__device__ __forceinline__ int fp_unit_bin(double f)
{
    const double t = (11.0 * (f + 1.0)) * 0.5;
    int b = 0;
#pragma unroll
    for (int e = 1; e <= 10; ++e) b += t >= (double)e;
    return b;
}

__device__ __forceinline__ double fp_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void fp_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// F2 + F3: the three bins of the pair (p1, n1), (p2, n2)
__device__ __forceinline__ void fp_pair_bins(const double (&p1)[3], const double (&n1)[3], const double (&p2)[3], const double (&n2)[3], int (&bin)[3])
{
    double d[3] = { p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2] };
    const double L = __dsqrt_rn(fp_dot(d, d));
    const double a1 = fp_dot(n1, d) / L, a2 = fp_dot(n2, d) / L;
    const bool swap = fabs(a1) < fabs(a2);
    double N1[3], N2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { N1[k] = swap ? n2[k] : n1[k]; N2[k] = swap ? n1[k] : n2[k]; d[k] = swap ? -d[k] : d[k]; }
    const double f3 = swap ? -a2 : a1;
    double v[3], w[3];
    fp_cross(d, N1, v);
    const double vn = __dsqrt_rn(fp_dot(v, v));
    v[0] = v[0] / vn; v[1] = v[1] / vn; v[2] = v[2] / vn;
    fp_cross(N1, v, w);
    const double f2 = fp_dot(v, N2), y = fp_dot(w, N2), x = fp_dot(N1, N2);
    const bool ok = L != 0.0 && vn != 0.0;
    bin[0] = ok ? fp_angle_bin(y, x) : 5;
    bin[1] = ok ? fp_unit_bin(f2) : 5;
    bin[2] = ok ? fp_unit_bin(f3) : 5;
}

__global__ void fp_info_kernel(fp_args a, int final)
{
    if (threadIdx.x != 0) return;
    if (!final) { a.info[0] = 0; a.info[1] = 0; a.info[2] = 0; a.info[3] = 0; }
    else a.info[0] = nn_c(a.nn)->n1_live > 0 ? 0 : 1;
}

// the LDS traffic of one wave with itself: its operations complete in order, the compiler must not move them across this point
#define FP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ bool fp_before(double d, int j, double e, int k) { return d < e || (d == e && j < k); }

// ranks the m <= FP_BUF entries of the wave's buffer under (d2, index), keeps the first `cap` in that order; returns the new length
__device__ __forceinline__ int fp_rank_keep(double *bd, int32_t *bj, int m, int cap, int lane)
{
    double md[FP_BUF / 64]; int32_t mj[FP_BUF / 64]; int rank[FP_BUF / 64];
#pragma unroll
    for (int t = 0; t < FP_BUF / 64; ++t) {
        const int e = lane + 64 * t;
        md[t] = e < m ? bd[e] : INFINITY; mj[t] = e < m ? bj[e] : 0x7fffffff; rank[t] = 0;
    }
    for (int f = 0; f < m; ++f) {
        const double d = bd[f]; const int32_t j = bj[f];
#pragma unroll
        for (int t = 0; t < FP_BUF / 64; ++t) rank[t] += fp_before(d, j, md[t], mj[t]);
    }
    FP_WAVE_SYNC();
#pragma unroll
    for (int t = 0; t < FP_BUF / 64; ++t)
        if (lane + 64 * t < m && rank[t] < cap) { bd[rank[t]] = md[t]; bj[rank[t]] = mj[t]; }
    FP_WAVE_SYNC();
    return m < cap ? m : cap;
}

__global__ void __launch_bounds__(256) fp_list_kernel(fp_args a)
{
    __shared__ double s_d[4][FP_BUF];
    __shared__ int32_t s_j[4][FP_BUF];
    const nn_args &g = a.nn;
    const nn_ctl *c = nn_c(g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= a.n) return;
    double *bd = s_d[wave]; int32_t *bj = s_j[wave];
    int32_t *cnt = lr_ptr<int32_t>(a, 0, a.L.cnt);
    int32_t *list = lr_ptr<int32_t>(a, 0, a.L.lists) + (size_t)i * (size_t)a.max_nn;
    const double q[3] = { a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2] };
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) {
        if (lane == 0) { cnt[i] = 0; atomicAdd(&a.info[1], 1); atomicAdd(&a.info[2], 1); }
        return;
    }
    const int32_t *table = lr_ptr<int32_t>(g, 0, g.L.table), *pidx = lr_ptr<int32_t>(g, 0, g.L.pidx);
    const double *pts = lr_ptr<double>(g, 0, g.L.pts);
    const int dx = c->dim[0], dy = c->dim[1], dz = c->dim[2];
    const int cx = nn_cell(q[0], c->blo[0], c->cell, dx), cy = nn_cell(q[1], c->blo[1], c->cell, dy), cz = nn_cell(q[2], c->blo[2], c->cell, dz);
    const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < dz ? cz + 1 : dz - 1, y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < dy ? cy + 1 : dy - 1;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < dx ? cx + 1 : dx - 1;
    int m = 0;
    bool full = false;                       // the list has max_nn entries: (td, tj) is its last one
    double td = INFINITY; int32_t tj = 0x7fffffff;
    for (int zz = z0; zz <= z1; ++zz)
        for (int yy = y0; yy <= y1; ++yy) {
            const int row = (zz * dy + yy) * dx, l0 = row + x0, l1 = row + x1;
            const int e = table[l1];
            for (int ub = l0 > 0 ? table[l0 - 1] : 0; ub < e; ub += 64) {
                const int u = ub + lane;
                bool in = false;
                double d2 = 0.0; int32_t j = 0;
                if (u < e) {
                    const double ex = q[0] - pts[3 * (size_t)u], ey = q[1] - pts[3 * (size_t)u + 1], ez = q[2] - pts[3 * (size_t)u + 2];
                    d2 = (ex * ex + ey * ey) + ez * ez;
                    j = pidx[u];
                    in = d2 <= a.r2 && (!full || fp_before(d2, j, td, tj));
                }
                const unsigned long long mask = __ballot(in);
                if (mask == 0) continue;
                if (in) {
                    const int at = m + __popcll(mask & ((1ull << lane) - 1ull));      // < m + 64 <= FP_BUF
                    bd[at] = d2; bj[at] = j;
                }
                m += __popcll(mask);
                FP_WAVE_SYNC();
                if (m > FP_BUF - 64) {
                    m = fp_rank_keep(bd, bj, m, a.max_nn, lane);
                    if (m == a.max_nn) { full = true; td = bd[m - 1]; tj = bj[m - 1]; }
                }
            }
        }
    m = fp_rank_keep(bd, bj, m, a.max_nn, lane);
    for (int e = lane; e < m; e += 64) list[e] = bj[e];
    if (lane == 0) {
        cnt[i] = m;
        if (m <= 1) atomicAdd(&a.info[2], 1);
        if (m == a.max_nn) atomicAdd(&a.info[3], 1);
    }
}

__global__ void __launch_bounds__(256) fp_spfh_kernel(fp_args a)
{
    __shared__ int32_t s_h[4][FP_BINS + 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= a.n) return;
    int32_t *h = s_h[wave];
    if (lane < FP_BINS) h[lane] = 0;
    FP_WAVE_SYNC();
    const int len = lr_ptr<const int32_t>(a, 0, a.L.cnt)[i];
    const int32_t *list = lr_ptr<const int32_t>(a, 0, a.L.lists) + (size_t)i * (size_t)a.max_nn;
    double *out = lr_ptr<double>(a, 0, a.L.spfh) + (size_t)i * FP_BINS;
    if (len > 1) {
        const double p1[3] = { a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2] };
        const double n1[3] = { a.nrm[3 * (size_t)i], a.nrm[3 * (size_t)i + 1], a.nrm[3 * (size_t)i + 2] };
        for (int e = 1 + lane; e < len; e += 64) {
            const size_t nb = (size_t)list[e];
            const double p2[3] = { a.xyz[3 * nb], a.xyz[3 * nb + 1], a.xyz[3 * nb + 2] };
            const double n2[3] = { a.nrm[3 * nb], a.nrm[3 * nb + 1], a.nrm[3 * nb + 2] };
            int bin[3];
            fp_pair_bins(p1, n1, p2, n2, bin);
            atomicAdd(&h[bin[0]], 1); atomicAdd(&h[11 + bin[1]], 1); atomicAdd(&h[22 + bin[2]], 1);
        }
    }
    FP_WAVE_SYNC();
    if (lane < FP_BINS) out[lane] = len > 1 ? (double)h[lane] * (100.0 / (double)(len - 1)) : 0.0;
}

__global__ void __launch_bounds__(256) fp_fpfh_kernel(fp_args a)
{
    __shared__ double s_f[4][FP_BINS + 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (i >= a.n) return;
    double *sf = s_f[wave];
    const int len = lr_ptr<const int32_t>(a, 0, a.L.cnt)[i];
    const int32_t *list = lr_ptr<const int32_t>(a, 0, a.L.lists) + (size_t)i * (size_t)a.max_nn;
    const double *spfh = lr_ptr<const double>(a, 0, a.L.spfh);
    const int bin = lane < FP_BINS ? lane : FP_BINS - 1;
    double F = 0.0;
    if (len > 1) {
        const double q[3] = { a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2] };
        for (int e = 1; e < len; ++e) {
            const size_t nb = (size_t)list[e];
            const double ex = q[0] - a.xyz[3 * nb], ey = q[1] - a.xyz[3 * nb + 1], ez = q[2] - a.xyz[3 * nb + 2];
            const double d2 = (ex * ex + ey * ey) + ez * ez;
            if (d2 != 0.0) F = F + spfh[nb * FP_BINS + bin] / d2;
        }
    }
    if (lane < FP_BINS) sf[lane] = F;
    FP_WAVE_SYNC();
    if (lane < FP_BINS) {
        const int b0 = 11 * (lane / 11);
        double gsum = 0.0;
        for (int j = b0; j < b0 + 11; ++j) gsum = gsum + sf[j];
        const double scale = gsum != 0.0 ? 100.0 / gsum : 0.0;
        const double r = len > 1 ? F * scale + spfh[(size_t)i * FP_BINS + lane] : 0.0;
        if (a.out64) a.out64[(size_t)i * FP_BINS + lane] = r;
        if (a.out32) a.out32[(size_t)i * FP_BINS + lane] = (float)r;
    }
}

extern "C" size_t lr_fpfh_scratch_bytes(int n, int max_nn)
{
    if (n < 0 || n > NN_MAX_N || max_nn < FP_MIN_NN || max_nn > FP_MAX_NN) return 0;
    fp_layout L;
    return fp_make_layout(&L, (size_t)n, (size_t)max_nn);
}

extern "C" int lr_fpfh(const double *xyz, const double *normals, int n, double radius, int max_nn, double *out_f64, float *out_f32,
                       int32_t *info, void *scratch, size_t scratch_bytes, void *stream)
{
    const char *who = "lr_fpfh";
    LR_REFUSE_UNLESS(radius > 0.0 && isfinite(radius) && isfinite(radius * radius), LR_EINVAL, "radius must be positive and finite");
    LR_REFUSE_UNLESS(max_nn >= FP_MIN_NN && max_nn <= FP_MAX_NN, LR_EINVAL, "max_nn must lie in 2..128");
    LR_REFUSE_UNLESS(n >= 0 && n <= NN_MAX_N, LR_EINVAL, "n must lie in 0..4194304");
    LR_REFUSE_UNLESS(n == 0 || xyz, LR_EINVAL, "null xyz");
    LR_REFUSE_UNLESS(n == 0 || normals, LR_EINVAL, "null normals");
    LR_REFUSE_UNLESS(n == 0 || out_f64 || out_f32, LR_EINVAL, "null out_f64 and out_f32");
    LR_REFUSE_UNLESS(info, LR_EINVAL, "null info");
    fp_args a;
    memset(&a, 0, sizeof a);
    a.stride = fp_make_layout(&a.L, (size_t)n, (size_t)max_nn);
    LR_TRY_HIP(lr_check_scratch(who, scratch, scratch_bytes, a.stride, "lr_fpfh_scratch_bytes(n, max_nn)", LR_EINVAL, stream, nullptr));
    a.base = reinterpret_cast<char *>(scratch);
    // the cell is a little longer than the radius, as in lr_normals: two points within the radius sit in the same or in adjacent cells
    nn_set_args(&a.nn, a.base + a.L.nn, xyz, n, xyz, n, radius * (1.0 + 1.0 / 65536.0), nullptr, nullptr);
    a.xyz = xyz; a.nrm = normals; a.n = n; a.max_nn = max_nn; a.r2 = radius * radius; a.out64 = out_f64; a.out32 = out_f32; a.info = info;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((size_t)(n > 0 ? n : 1) + 3) / 4));
    hipLaunchKernelGGL(fp_info_kernel, dim3(1), dim3(64), 0, st, a, 0);
    nn_launch_grid(a.nn, st);
    hipLaunchKernelGGL(fp_list_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(fp_spfh_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(fp_fpfh_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(fp_info_kernel, dim3(1), dim3(64), 0, st, a, 1);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
