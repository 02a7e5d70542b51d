// Deep Global Registration's robust pose refinement on gfx950: the half of DeepGlobalRegistration.register that follows the inlier
// weights (DGR/core/deep_global_registration.py:403-459) -- the weight-sum decision and GlobalRegistration (DGR/core/registration.py:16-64,
// :116-194; loss DGR/core/loss.py:42-61): a weighted Huber loss over the correspondences, minimised by Adam over a 6-D rotation and a
// translation.  The contract (G1-G10) is stated in include/lidarreg.h and DESIGN.md §19 and restated in numpy in tests/dgr_cpu.py.
//
// The reference runs up to 1000 dependent iterations of a forward pass, an autograd pass and two .item() round trips; here the whole loop
// is ONE launch, one workgroup of 1024 threads per pair, the parameters, Adam's moments and the stop state in LDS.
//
// Kernels (each launched ONCE for a batch; a single-pair call is a batch of one):
//   dg_ctl_kernel     descriptors by value -> control blocks (src, tgt, m_dev travel in cs_desc_table)
//   dg_setup_kernel   the second by-value table (weights, T_init); a block per pair: G1 (live rows compacted in index order into 32-byte
//                     records { X, Y, w, 0 }), w1, the decision of G9, G3 (the initial parameters)
//   dg_loop_kernel    a block per pair: G4-G8.  Per iteration: 13 partial sums per thread over the pair's records (L2-resident), ONE pass
//                     through LDS for the levels h >= 64 of G2's tree (wave k owns sum k: 16 loads, 15 additions in the tree's order), the
//                     levels h < 64 inside the wave, then one lane runs the back-propagation through G4, Adam and the stop rule and
//                     publishes the next R, t.  Three barriers per iteration; the stop is read from LDS after the third.
// No floating-point atomics, no scratch memory, no host synchronisation.
#include "lr_corrset.h"
#include "lr_prims.h"
#include "lr_contract.h"
#include <math.h>
#include <float.h>

#define DG_NB 1024                   // threads of a pair's workgroup
#define DG_NS 13                     // sums of an iteration: the loss, dt[3], G[3][3]
#define DG_EPS 1.1920928955078125e-07        // 2^-23: np.finfo(np.float32).eps, the loss's eps and the fit's
#define DG_CLAMP 1e-8                // ortho2rotation's clamps
#define DG_BETA1 0.9
#define DG_BETA2 0.999
#define DG_ADAM_EPS 1e-8
#define DG_LOSS_STOP 1e-7

typedef float dg_f32x4 __attribute__((ext_vector_type(4)));

// per-pair control block at the head of the pair's scratch arena
struct dg_ctl {
    const float *a, *b, *w;
    const double *T_init;
    double *log;                     // the single call's log, null in a batch
    int32_t m, L;                    // m_dev clamped to 0..m; live rows
    int32_t status, pad;
    double w1;
    double p0[9];                    // G3
};

struct dg_args {
    char *base;                      // scratch arena of pair 0
    size_t stride;                   // bytes between consecutive pairs' arenas
    size_t rec;                      // offset of the records
};

// the pointers cs_desc has no room for
struct dg_ext { const float *w; const double *T_init; };
struct dg_ext_table { dg_ext d[LR_MAX_BATCH]; };

// what the kernels read of lr_dgr_params
struct dg_consts {
    int max_iter, max_break;
    double q, lr, gamma, ratio, clip, wsum;
};
static_assert(sizeof(dg_ext_table) + sizeof(dg_args) + sizeof(dg_consts) + 64 <= 4096, "the second table no longer fits the kernel arguments");

__global__ void dg_ctl_kernel(cs_desc_table t, dg_args g, int npairs)
{
    const int k = threadIdx.x;
    if (k >= npairs) return;
    const cs_desc d = t.d[k];
    dg_ctl *c = lr_ptr<dg_ctl>(g, k, 0);
    c->a = d.a; c->b = d.b;
    c->m = cs_live_m(d);
}

// ---- G1, G3, the decision of G9 ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DG_NB) dg_setup_kernel(dg_ext_table e, dg_args g, dg_consts P, double *log)
{
    __shared__ double s_red[DG_NB];
    __shared__ int s_cnt[DG_NB / 64];
    const int pair = blockIdx.x, tid = threadIdx.x;
    dg_ctl *c = lr_ptr<dg_ctl>(g, pair, 0);
    float *rec = lr_ptr<float>(g, pair, g.rec);
    const float *wp = e.d[pair].w;
    const double *Ti = e.d[pair].T_init;
    const int m = c->m;

    // G1: live rows in index order
    int L = 0;
    for (int base = 0; base < m; base += DG_NB) {
        const int i = base + tid;
        float r[6], w = 0.0f;
        bool live = false;
        if (i < m) {
            // (cs_load_row in this file's own spelling: the helper's load order re-schedules the kernel)
            for (int x = 0; x < 3; ++x) { r[x] = c->a[(size_t)3 * i + x]; r[3 + x] = c->b[(size_t)3 * i + x]; }
            w = wp ? wp[i] : 1.0f;
            live = fabsf(w) <= FLT_MAX && w > 0.0f && (double)w >= P.clip;      // (false for NaN and inf)
            for (int x = 0; x < 6; ++x) live = live && fabsf(r[x]) <= FLT_MAX;
        }
        int total;
        const int slot = L + lr_block_rank<DG_NB>(live, s_cnt, total);
        if (live) {
            dg_f32x4 *o = reinterpret_cast<dg_f32x4 *>(rec + (size_t)slot * 8);
            o[0] = dg_f32x4{ r[0], r[1], r[2], r[3] };
            o[1] = dg_f32x4{ r[4], r[5], w, 0.0f };
        }
        L += total;
    }
    __syncthreads();                 // (the block reads its own records below)

    double v = 0.0;
    for (int i = tid; i < L; i += DG_NB) v = v + (double)rec[(size_t)i * 8 + 6];
    const double w1 = lr_block_tree_sum<DG_NB>(v, s_red);
    const int status = L == 0 ? 1 : (w1 < P.wsum ? 2 : 0);

    double mom[16];
    if (status == 0 && !Ti) {
        // G3: the raw moments of lr_rt_from_moments under the weights w / (w1 + eps), sixteen sums in G2's tree
        const double den = w1 + DG_EPS;
        double acc[16];
        for (int k = 0; k < 16; ++k) acc[k] = 0.0;
        for (int i = tid; i < L; i += DG_NB) {
            const float *r = rec + (size_t)i * 8;
            const double wn = (double)r[6] / den;
            acc[0] = acc[0] + wn;
            for (int x = 0; x < 3; ++x) {
                const double wx = wn * (double)r[x];
                acc[1 + x] = acc[1 + x] + wx;
                acc[4 + x] = acc[4 + x] + wn * (double)r[3 + x];
                for (int y = 0; y < 3; ++y) acc[7 + 3 * x + y] = acc[7 + 3 * x + y] + wx * (double)r[3 + y];
            }
        }
        for (int k = 0; k < 16; ++k) mom[k] = lr_block_tree_sum<DG_NB>(acc[k], s_red);
    }
    if (tid == 0) {
        c->w = wp; c->T_init = Ti; c->log = log;
        c->L = L; c->status = status; c->pad = 0; c->w1 = w1;
        double T[16];
        for (int k = 0; k < 16; ++k) T[k] = k % 5 == 0 ? 1.0 : 0.0;
        if (status == 0) {
            if (Ti) {
                for (int k = 0; k < 16; ++k) T[k] = Ti[k];
            } else {
                lr_rt_from_moments(mom, T);
                for (int k = 0; k < 12; ++k) T[k] = (double)(float)T[k];       // weighted_procrustes ends in .float()
            }
        }
        for (int x = 0; x < 3; ++x) { c->p0[x] = T[4 * x]; c->p0[3 + x] = T[4 * x + 1]; c->p0[6 + x] = T[4 * x + 3]; }
    }
}

// ---- G4 on one lane ---------------------------------------------------------------------------------------------------------------------
struct dg_rot { double x[3], y[3], z[3], b[3], na, nu, xx, xb, n2, c; };

__device__ __forceinline__ void dg_cross(const double *p, const double *q, double *o)
{
    o[0] = p[1] * q[2] - p[2] * q[1]; o[1] = p[2] * q[0] - p[0] * q[2]; o[2] = p[0] * q[1] - p[1] * q[0];
}
// max(v, 1e-8) as torch.clamp(min=) has it: a NaN stays a NaN
__device__ __forceinline__ double dg_clamp(double v) { return v < DG_CLAMP ? DG_CLAMP : v; }

__device__ __forceinline__ void dg_rotation(const double *p, dg_rot &o)
{
    const double *a = p;
    for (int k = 0; k < 3; ++k) o.b[k] = p[3 + k];
    o.na = sqrt(lr_dot3(a, a));
    const double da = dg_clamp(o.na);
    for (int k = 0; k < 3; ++k) o.x[k] = a[k] / da;
    o.xx = lr_dot3(o.x, o.x);
    o.n2 = dg_clamp(o.xx);
    o.xb = lr_dot3(o.x, o.b);
    o.c = o.xb / o.n2;
    double u[3];
    for (int k = 0; k < 3; ++k) u[k] = o.b[k] - o.c * o.x[k];
    o.nu = sqrt(lr_dot3(u, u));
    const double du = dg_clamp(o.nu);
    for (int k = 0; k < 3; ++k) o.y[k] = u[k] / du;
    dg_cross(o.x, o.y, o.z);
}

// G6's back-propagation: G[a][b] = d loss / d R[a][b] -> grad[0..5] = d loss / d (a, b)
__device__ __forceinline__ void dg_rotation_back(const dg_rot &o, const double *G, double *grad)
{
    double Gx[3], Gy[3], Gz[3], t[3], du[3];
    for (int k = 0; k < 3; ++k) { Gx[k] = G[3 * k]; Gy[k] = G[3 * k + 1]; Gz[k] = G[3 * k + 2]; }
    dg_cross(o.y, Gz, t);
    for (int k = 0; k < 3; ++k) Gx[k] = Gx[k] + t[k];
    dg_cross(Gz, o.x, t);
    for (int k = 0; k < 3; ++k) Gy[k] = Gy[k] + t[k];
    if (o.nu < DG_CLAMP) {
        for (int k = 0; k < 3; ++k) du[k] = Gy[k] / DG_CLAMP;
    } else {
        const double yg = lr_dot3(o.y, Gy);
        for (int k = 0; k < 3; ++k) du[k] = (Gy[k] - o.y[k] * yg) / o.nu;
    }
    const double dc = -lr_dot3(du, o.x);
    for (int k = 0; k < 3; ++k) Gx[k] = Gx[k] - o.c * du[k];
    const double t1 = dc / o.n2;
    for (int k = 0; k < 3; ++k) Gx[k] = Gx[k] + t1 * o.b[k];
    for (int k = 0; k < 3; ++k) grad[3 + k] = du[k] + t1 * o.x[k];
    if (!(o.xx < DG_CLAMP)) {
        const double dn2 = -((dc * o.xb) / (o.n2 * o.n2));
        for (int k = 0; k < 3; ++k) Gx[k] = Gx[k] + (2.0 * dn2) * o.x[k];
    }
    if (o.na < DG_CLAMP) {
        for (int k = 0; k < 3; ++k) grad[k] = Gx[k] / DG_CLAMP;
    } else {
        const double xg = lr_dot3(o.x, Gx);
        for (int k = 0; k < 3; ++k) grad[k] = (Gx[k] - o.x[k] * xg) / o.na;
    }
}

__device__ __forceinline__ bool dg_finite(double v) { return fabs(v) <= DBL_MAX; }

// ---- G4-G8: the loop ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DG_NB) dg_loop_kernel(dg_args g, dg_consts P, lr_dgr_result *results)
{
    __shared__ double s_part[DG_NS][DG_NB];
    __shared__ double s_sum[DG_NS + 3];
    __shared__ double s_Rt[12];                      // R row-major, then t
    __shared__ double s_p[9], s_m[9], s_v[9];
    __shared__ double s_st[4];                       // lr, pw1, pw2, loss_prev
    __shared__ int s_flag[4];                        // stop, break_count, iterations, status
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const dg_ctl *c = lr_ptr<const dg_ctl>(g, pair, 0);
    const float *rec = lr_ptr<const float>(g, pair, g.rec);
    lr_dgr_result *res = results + pair;
    const int L = c->L;
    const double w1 = c->w1;
    double *log = c->log;
    const int st0 = c->status;

    if (st0 != 0) {
        if (tid == 0) {
            for (int k = 0; k < 16; ++k) res->T[k] = k % 5 == 0 ? 1.0 : 0.0;
            res->loss = 0.0; res->w1 = w1; res->iterations = 0; res->break_count = 0; res->L = L; res->status = st0;
        }
        if (log) for (int k = tid; k < P.max_iter * 10; k += DG_NB) log[k] = 0.0;
        return;
    }
    if (tid == 0) {
        dg_rot o;
        for (int k = 0; k < 9; ++k) { s_p[k] = c->p0[k]; s_m[k] = 0.0; s_v[k] = 0.0; }
        dg_rotation(s_p, o);
        for (int k = 0; k < 3; ++k) { s_Rt[3 * k] = o.x[k]; s_Rt[3 * k + 1] = o.y[k]; s_Rt[3 * k + 2] = o.z[k]; s_Rt[9 + k] = s_p[6 + k]; }
        s_st[0] = P.lr; s_st[1] = 1.0; s_st[2] = 1.0; s_st[3] = 0.0;
        s_flag[0] = 0; s_flag[1] = 0; s_flag[2] = P.max_iter - 1; s_flag[3] = 0;
    }
    __syncthreads();

    int rows = 0;                                    // log rows written
    for (int it = 0; it < P.max_iter; ++it) {
        double R[12];
        for (int k = 0; k < 12; ++k) R[k] = s_Rt[k];
        double acc[DG_NS];
#pragma unroll
        for (int k = 0; k < DG_NS; ++k) acc[k] = 0.0;
        for (int i = tid; i < L; i += DG_NB) {
            const dg_f32x4 r0 = *reinterpret_cast<const dg_f32x4 *>(rec + (size_t)i * 8), r1 = *reinterpret_cast<const dg_f32x4 *>(rec + (size_t)i * 8 + 4);
            const double X[3] = { (double)r0[0], (double)r0[1], (double)r0[2] }, Y[3] = { (double)r0[3], (double)r1[0], (double)r1[1] };
            const double w = (double)r1[2];
            double r[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] = ((((R[3 * a] * X[0] + R[3 * a + 1] * X[1]) + R[3 * a + 2] * X[2]) + R[9 + a]) - Y[a]) / P.q;
            const double s = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            const bool small = s < 1.0;
            const double rt = sqrt(s + DG_EPS);
            const double l = small ? 0.5 * s : 0.5 * (rt - 0.5);
            const double k = small ? 1.0 : 0.5 / rt;
            const double cf = ((k * w) / w1) / P.q;
            acc[0] = acc[0] + w * l;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double ga = cf * r[a];
                acc[1 + a] = acc[1 + a] + ga;
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[4 + 3 * a + b] = acc[4 + 3 * a + b] + ga * X[b];
            }
        }
#pragma unroll
        for (int k = 0; k < DG_NS; ++k) s_part[k][tid] = acc[k];
        __syncthreads();
        // G2's tree: the levels h = 512 .. 64 pair the waves (j, j + 8), (j, j + 4), (j, j + 2), (0, 1) lane by lane; wave k owns sum k
        if (wave < DG_NS) {
            double q[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = s_part[wave][64 * j + lane];
#pragma unroll
            for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
                for (int j = 0; j < h; ++j) q[j] = q[j] + q[j + h];
            const double tot = lr_wave_tree_sum(q[0]);
            if (lane == 0) s_sum[wave] = tot;
        }
        __syncthreads();
        if (tid == 0) {
            const double loss = s_sum[0] / w1;
            if (log) { for (int k = 0; k < 9; ++k) log[(size_t)it * 10 + k] = s_p[k]; log[(size_t)it * 10 + 9] = loss; }
            s_sum[DG_NS] = loss;
            if (it == 0) s_st[3] = loss;
            if (!dg_finite(loss)) { s_flag[0] = 1; s_flag[2] = it; s_flag[3] = 3; }
            else if (loss < DG_LOSS_STOP) { s_flag[0] = 1; s_flag[2] = it; }
            else {
                // G6's back-propagation, G7
                dg_rot o;
                double grad[9], G[9];
                for (int k = 0; k < 9; ++k) G[k] = s_sum[4 + k];
                dg_rotation(s_p, o);
                dg_rotation_back(o, G, grad);
                for (int k = 0; k < 3; ++k) grad[6 + k] = s_sum[1 + k];
                const double pw1 = s_st[1] * DG_BETA1, pw2 = s_st[2] * DG_BETA2, lr = s_st[0];
                s_st[1] = pw1; s_st[2] = pw2;
                bool ok = true;
                for (int k = 0; k < 9; ++k) {
                    const double gk = grad[k];
                    const double mk = DG_BETA1 * s_m[k] + (1.0 - DG_BETA1) * gk;
                    const double vk = DG_BETA2 * s_v[k] + (1.0 - DG_BETA2) * (gk * gk);
                    const double pk = s_p[k] - (lr / (1.0 - pw1)) * (mk / (sqrt(vk) / sqrt(1.0 - pw2) + DG_ADAM_EPS));
                    s_m[k] = mk; s_v[k] = vk; s_p[k] = pk;
                    ok = ok && dg_finite(pk);
                }
                s_st[0] = lr * P.gamma;
                if (!ok) { s_flag[0] = 1; s_flag[2] = it; s_flag[3] = 3; }
                else {
                    // G8
                    const double prev = s_st[3];
                    if (fabs(prev - loss) < prev * P.ratio) {
                        const int bc = s_flag[1] + 1;
                        s_flag[1] = bc;
                        if (bc >= P.max_break) { s_flag[0] = 1; s_flag[2] = it; }
                    }
                    s_st[3] = loss;
                    dg_rotation(s_p, o);
                    for (int k = 0; k < 3; ++k) { s_Rt[3 * k] = o.x[k]; s_Rt[3 * k + 1] = o.y[k]; s_Rt[3 * k + 2] = o.z[k]; s_Rt[9 + k] = s_p[6 + k]; }
                }
            }
        }
        __syncthreads();
        rows = it + 1;
        if (s_flag[0]) break;                        // (workgroup-uniform)
    }
    if (log) for (int k = rows * 10 + tid; k < P.max_iter * 10; k += DG_NB) log[k] = 0.0;
    if (tid == 0) {
        const int status = s_flag[3];
        double p[9];
        for (int k = 0; k < 9; ++k) p[k] = status == 3 ? c->p0[k] : s_p[k];
        dg_rot o;
        dg_rotation(p, o);
        for (int k = 0; k < 3; ++k) { res->T[4 * k] = o.x[k]; res->T[4 * k + 1] = o.y[k]; res->T[4 * k + 2] = o.z[k]; res->T[4 * k + 3] = p[6 + k]; }
        res->T[12] = 0.0; res->T[13] = 0.0; res->T[14] = 0.0; res->T[15] = 1.0;
        res->loss = s_sum[DG_NS]; res->w1 = w1;
        res->iterations = s_flag[2]; res->break_count = s_flag[1]; res->L = L; res->status = status;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(lr_dgr_params) == 64 && sizeof(lr_dgr_result) == 160, "ABI structs changed: update include/lidarreg.h, _ext.py and INTEGRATION.md together");

static size_t dg_rec_offset() { return lr_al(sizeof(dg_ctl)); }

extern "C" size_t lr_dgr_scratch_bytes(int max_m)
{
    if (max_m < 0 || max_m > CS_MAX_M) return 0;
    return dg_rec_offset() + lr_al((size_t)(max_m < 1 ? 1 : max_m) * 32);
}

static int check_dgr_params(const lr_dgr_params *p, const char *who)
{
    LR_CHECK_STRUCT_SIZE(lr_dgr_params, p, who);
    if (p->max_iter < 1 || p->max_iter > 1000) { lr_set_error("%s: max_iter must lie in 1..1000", who); return LR_EINVAL; }
    if (p->max_break < 1) { lr_set_error("%s: max_break must be at least 1", who); return LR_EINVAL; }
    if (!(p->quantization_size > 0.0 && isfinite(p->quantization_size))) { lr_set_error("%s: quantization_size must be positive and finite", who); return LR_EINVAL; }
    if (!(p->lr > 0.0 && isfinite(p->lr))) { lr_set_error("%s: lr must be positive and finite", who); return LR_EINVAL; }
    if (!(p->gamma > 0.0 && p->gamma <= 1.0)) { lr_set_error("%s: gamma must lie in (0, 1]", who); return LR_EINVAL; }
    if (!(p->ratio >= 0.0 && isfinite(p->ratio))) { lr_set_error("%s: ratio must be non-negative and finite", who); return LR_EINVAL; }
    if (!(p->clip >= 0.0 && isfinite(p->clip))) { lr_set_error("%s: clip must be non-negative and finite", who); return LR_EINVAL; }
    if (!(p->wsum_threshold >= 0.0 && isfinite(p->wsum_threshold))) { lr_set_error("%s: wsum_threshold must be non-negative and finite", who); return LR_EINVAL; }
    return LR_OK;
}

static int dg_run(const char *who, int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                  const float *const *weights, const double *const *T_init, const lr_dgr_params *p, lr_dgr_result *results, double *log,
                  void *scratch, size_t scratch_bytes, void *stream)
{
    static const cs_backend be = { "lr_dgr_refine_batch", "npairs * lr_dgr_scratch_bytes(max m)", lr_dgr_scratch_bytes, LR_EINVAL };
    LR_TRY_HIP(check_dgr_params(p, who));
    cs_front f;
    LR_TRY_HIP(cs_check_batch(be, npairs, src, tgt, m, m_dev, nullptr, nullptr, results, scratch, scratch_bytes, stream, &f));
    dg_ext_table ext;
    for (int k = 0; k < LR_MAX_BATCH; ++k) ext.d[k] = dg_ext{ nullptr, nullptr };
    for (int k = 0; k < npairs; ++k) {
        ext.d[k] = dg_ext{ weights ? weights[k] : nullptr, T_init ? T_init[k] : nullptr };
        LR_REFUSE_UNLESS(((uintptr_t)ext.d[k].T_init & 7) == 0, LR_EINVAL, "T_init must be 8-byte aligned");
    }
    dg_args g;
    g.base = reinterpret_cast<char *>(scratch);
    g.stride = f.per;
    g.rec = dg_rec_offset();
    dg_consts P;
    P.max_iter = p->max_iter; P.max_break = p->max_break;
    P.q = p->quantization_size; P.lr = p->lr; P.gamma = p->gamma; P.ratio = p->ratio; P.clip = p->clip; P.wsum = p->wsum_threshold;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dg_ctl_kernel, dim3(1), dim3(64), 0, st, f.t, g, npairs);
    hipLaunchKernelGGL(dg_setup_kernel, dim3(npairs), dim3(DG_NB), 0, st, ext, g, P, log);
    hipLaunchKernelGGL(dg_loop_kernel, dim3(npairs), dim3(DG_NB), 0, st, g, P, results);
    LR_LAUNCH_CHECK();
    return LR_OK;
}

extern "C" int lr_dgr_refine_batch(int npairs, const float *const *src, const float *const *tgt, const int32_t *m, const int32_t *const *m_dev,
                                   const float *const *weights, const double *const *T_init, const lr_dgr_params *p, lr_dgr_result *results,
                                   void *scratch, size_t scratch_bytes, void *stream)
{
    return dg_run("lr_dgr_refine_batch", npairs, src, tgt, m, m_dev, weights, T_init, p, results, nullptr, scratch, scratch_bytes, stream);
}

extern "C" int lr_dgr_refine(const float *src, const float *tgt, int m, const int32_t *m_dev, const float *weights, const double *T_init,
                             const lr_dgr_params *p, lr_dgr_result *result, double *log_out, void *scratch, size_t scratch_bytes, void *stream)
{
    return dg_run("lr_dgr_refine", 1, &src, &tgt, &m, &m_dev, &weights, &T_init, p, result, log_out, scratch, scratch_bytes, stream);
}
