/*
 * lr_contract.h -- the arithmetic contract, one text for the HIP kernels and the CPU oracle: the fp64 solvers and decisions, and
 * the fp32 scoring of a model (residual, fixed-point error term, MSAC threshold, winner ordering).
 *
 * Plain C99 that is also valid HIP C++: the .hip files next to it compile it with hipcc for gfx950, oracle/oracle.c with gcc.
 * Everything here is written with + - * / sqrt and explicit fmaf only, in an explicit operation order, and both sides build with
 * -ffp-contract=off, so the device and the oracle produce the same bits.  The GPU-against-oracle tests check for these routines that two compilers and two
 * machines turn this one text into the same bits; the mathematics is verified independently (tests/rigid_hp.py: 40-digit SVD
 * Kabsch; the numpy-SVD test of tests/test_oracle_golden.py; goldens G7 / G11).
 * The dependency points from the test infrastructure to the product: oracle/ includes this file, nothing under
 * lidarregistration_amd/ includes anything from oracle/.
 *
 * What deliberately stays as two texts, one per side:
 *   - Philox, sampling, ELC, the PROSAC table: the device forms are different algorithms (__umulhi; the squared-length ELC that
 *     takes square roots only inside a 1e-13 band; a parallel prefix sum for the growth table).  There the oracle is an
 *     independent restatement.
 *   - the point-form moment loops (kabsch_sample<NS>, the LO trial fit over sh.pts, kabsch_points_kernel, orc_kabsch_points,
 *     hypothesis_T): they read different types (fp64 arrays, fp32 LDS records, weights), and the LO loop is rolled on purpose to
 *     avoid spills; a shared template would be new machinery in a kernel at its register limits.
 *   - eff_params: the structs differ (orc_ransac_params has no struct_size) and the device entry refuses lo_trials > 20 where the
 *     oracle clamps it.  Same rule, two texts.
 *   - the fp64 residual of refit_moments_kernel / ICP (no fma, fp64 threshold): a different contract from the fp32 scoring below.
 *   - the pruning radii eps of ransac_order_kernel (fp32) and of the LO near list (fp64): bounds on where inliers can lie, not
 *     results; the oracle scores everything and has neither.
 *   - the packed two-correspondence form of the scoring residual (lr_ransac_dev.h, lr_d2x2): ext_vector arithmetic has no C99
 *     spelling; it applies lr_score_d2's fma order to each half.
 */
#ifndef LR_CONTRACT_H
#define LR_CONTRACT_H

#if defined(__HIPCC__)
#  include <hip/hip_runtime.h>
#  define LRC_FN     __host__ __device__ __forceinline__
#  define LRC_UNROLL _Pragma("unroll")
#else
#  define LRC_FN     static inline
#  define LRC_UNROLL
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>

/* ------------------------------------------------------------------ logarithm for the decisions (fp64, + - * / only) */
/* The confidence exit and the SPRT design compare against values made of logarithms; libm's and ocml's log differ in the last
 * place, which can flip such a comparison on one side only (found by tools/soak_gc.py).
 * x = m 2^e with m in [sqrt(1/2), sqrt(2)), log x = e ln 2 + 2 atanh((m - 1) / (m + 1)), the odd series up to t^25. */
LRC_FN double lr_det_log(double x)
{
    if (!(x > 0.0)) return x == 0.0 ? -HUGE_VAL : NAN;
    if (x > 1.7976931348623157e308) return HUGE_VAL;      /* +inf */
    unsigned long long b;
    memcpy(&b, &x, 8);
    int e = (int)((b >> 52) & 0x7ffull);
    if (e == 0) { x = x * 18014398509481984.0; memcpy(&b, &x, 8); e = (int)((b >> 52) & 0x7ffull) - 54; }
    e -= 1023;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    memcpy(&m, &b, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double t = (m - 1.0) / (m + 1.0), t2 = t * t;
    double s = 1.0 / 25.0;
    s = s * t2 + 1.0 / 23.0; s = s * t2 + 1.0 / 21.0; s = s * t2 + 1.0 / 19.0; s = s * t2 + 1.0 / 17.0; s = s * t2 + 1.0 / 15.0;
    s = s * t2 + 1.0 / 13.0; s = s * t2 + 1.0 / 11.0; s = s * t2 + 1.0 / 9.0; s = s * t2 + 1.0 / 7.0; s = s * t2 + 1.0 / 5.0;
    s = s * t2 + 1.0 / 3.0; s = s * t2 + 1.0;
    return (double)e * 0.6931471805599453 + (2.0 * t) * s;
}

/* ------------------------------------------------------------------ SPRT design (sources and the test itself: oracle.c, sprt_test) */
#define LR_SPRT_HORIZON 256      /* the test runs over the first LR_SPRT_HORIZON correspondences in list order */
#define LR_SPRT_EPS0 0.1
#define LR_SPRT_DELTA0 0.01

/* A solves A = K + ln A,  K = t_M C / m_S + 1 (t_M = 200 verifications per model estimate, m_S = 1 model per sample) */
LRC_FN double lr_sprt_threshold(double eps, double delta)
{
    const double C = (1.0 - delta) * lr_det_log((1.0 - delta) / (1.0 - eps)) + delta * lr_det_log(delta / eps);
    const double K = (200.0 * C) / 1.0 + 1.0;
    double A = K;
    for (int i = 0; i < 10; ++i) A = K + lr_det_log(A);
    return A;
}

/* ------------------------------------------------------------------ local optimisation (algorithm and sources: oracle.c, lo_optimise / lo_polish) */
#define LR_LO_ROUNDS 10          /* rounds of one local optimisation (default of lo_rounds) */
#define LR_LO_TRIALS 20          /* least-squares fits per round (default and upper bound of lo_trials) */
#define LR_LO_SAMPLE 21          /* points per fit: 7 x the minimal sample */
#define LR_LO_POLISH 10          /* fits of the final iterated least squares */

/* ------------------------------------------------------------------ Kabsch (fp64, + - * / sqrt only) */
/* Kabsch through Horn's quaternion form.  Reference semantics: R = V diag(1,1,det) U^T, t = mu_B - R mu_A
 * (Experiments/models/common.py:7-45). */
#define LR_JACOBI_SWEEPS 10      /* upper bound; sweeps stop once the off-diagonal mass is below 1e-15 of the diagonal */

/* Largest-eigenvalue eigenvector of a symmetric 4x4 by cyclic Jacobi: the path for degenerate input. */
LRC_FN void lr_jacobi4_maxvec(double A[4][4], double q[4])
{
    double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
    for (int sweep = 0; sweep < LR_JACOBI_SWEEPS; ++sweep) {
        double off2 = ((((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[0][3] * A[0][3]) + A[1][2] * A[1][2]) + A[1][3] * A[1][3]) + A[2][3] * A[2][3];
        double dia2 = ((A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2]) + A[3][3] * A[3][3];
        if (off2 <= 1e-30 * dia2) break;
LRC_UNROLL
        for (int p = 0; p < 3; ++p)
LRC_UNROLL
            for (int r = p + 1; r < 4; ++r) {
                double apq = A[p][r];
                if (apq != 0.0) {
                    double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
                    double at = fabs(theta);
                    double t = 1.0 / (at + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    double c = 1.0 / sqrt(t * t + 1.0);
                    double s = t * c;
                    double tau = s / (1.0 + c);
                    double h = t * apq;
                    A[p][p] = A[p][p] - h;
                    A[r][r] = A[r][r] + h;
                    A[p][r] = 0.0; A[r][p] = 0.0;
LRC_UNROLL
                    for (int k = 0; k < 4; ++k) {
                        if (k == p || k == r) continue;
                        double g = A[k][p], f = A[k][r];
                        double gn = g - s * (f + g * tau);
                        double fn = f + s * (g - f * tau);
                        A[k][p] = gn; A[p][k] = gn;
                        A[k][r] = fn; A[r][k] = fn;
                    }
LRC_UNROLL
                    for (int k = 0; k < 4; ++k) {
                        double g = V[k][p], f = V[k][r];
                        V[k][p] = g - s * (f + g * tau);
                        V[k][r] = f + s * (g - f * tau);
                    }
                }
            }
    }
    double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0], best = A[0][0];
LRC_UNROLL
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) { best = A[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
    double nn = sqrt(((w * w + x * x) + y * y) + z * z);
    q[0] = w / nn; q[1] = x / nn; q[2] = y / nn; q[3] = z / nn;
}

/* Largest-eigenvalue eigenvector of a symmetric 4x4 in closed form (the cyclic Jacobi above is a chain of 36-48 dependent rotations of 4
 * divisions and 2 square roots -- 60 us of one lane for the hypothesis fits, 50 for the refit).
 *   1. the characteristic polynomial from the trace, the principal 2x2 / 3x3 minors and the determinant;
 *   2. its largest root by Newton's iteration from Gershgorin's upper bound: beyond the largest root the polynomial is positive, increasing
 *      and convex, so the iterates decrease monotonically and the loop ends when one no longer does (6-8 steps of one division; a close
 *      second eigenvalue -- near-collinear points -- takes 20-30);
 *   3. the eigenvector as the column of adj(N - lambda I) = prod(lambda_k - lambda) v v^T with the largest diagonal cofactor;
 *   4. step 3 once more at the Rayleigh quotient lambda' = q^T N q of that vector.
 * Returns 0 -- the caller runs Jacobi -- when the matrix is zero / not finite or either adjugate is at rounding level (a double largest
 * eigenvalue: collinear points).
 * Accuracy: the root of the characteristic polynomial carries eps |N| kappa (kappa = |N| / gap, gap = distance to the second eigenvalue),
 * so step 3's vector is off by delta ~ eps kappa^2 -- up to 1e5 times what the conditioning allows for near-collinear samples.  The
 * Rayleigh quotient is accurate to |N| (delta^2 / kappa + eps), so step 4's vector is off by eps kappa + delta^2: the backward-stable
 * bound that Jacobi attains.  tests/test_rigid_hp_cpu.py holds both paths to angle <= 32 eps kappa against a 40-digit SVD Kabsch. */
LRC_FN double lr_det3_(double a, double b, double c, double d, double e, double f, double g, double h, double i)
{
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}
LRC_FN int lr_horn4_maxvec_newton(const double N[4][4], double q[4])
{
    const double a = N[0][0], b = N[1][1], c = N[2][2], d = N[3][3];
    const double n01 = N[0][1], n02 = N[0][2], n03 = N[0][3], n12 = N[1][2], n13 = N[1][3], n23 = N[2][3];
    /* elementary symmetric functions of the eigenvalues: trace, principal 2x2 and 3x3 minors, determinant */
    const double e1 = (a + b) + (c + d);
    const double e2 = (((a * b - n01 * n01) + (a * c - n02 * n02)) + ((a * d - n03 * n03) + (b * c - n12 * n12))) + ((b * d - n13 * n13) + (c * d - n23 * n23));
    const double m0 = lr_det3_(b, n12, n13, n12, c, n23, n13, n23, d);      /* without row / column 0 */
    const double m1 = lr_det3_(a, n02, n03, n02, c, n23, n03, n23, d);
    const double m2 = lr_det3_(a, n01, n03, n01, b, n13, n03, n13, d);
    const double m3 = lr_det3_(a, n01, n02, n01, b, n12, n02, n12, c);
    const double e3 = (m0 + m1) + (m2 + m3);
    /* det N by the first row */
    const double k1 = lr_det3_(n01, n12, n13, n02, c, n23, n03, n23, d);
    const double k2 = lr_det3_(n01, b, n13, n02, n12, n23, n03, n13, d);
    const double k3 = lr_det3_(n01, b, n12, n02, n12, c, n03, n13, n23);
    const double e4 = ((a * m0 - n01 * k1) + n02 * k2) - n03 * k3;
    /* Gershgorin: an upper bound of the largest eigenvalue */
    const double r0 = ((a + fabs(n01)) + fabs(n02)) + fabs(n03), r1 = ((b + fabs(n01)) + fabs(n12)) + fabs(n13);
    const double r2 = ((c + fabs(n02)) + fabs(n12)) + fabs(n23), r3 = ((d + fabs(n03)) + fabs(n13)) + fabs(n23);
    double lam = r0 > r1 ? r0 : r1; { const double r = r2 > r3 ? r2 : r3; lam = lam > r ? lam : r; }
    const double bound = lam;
    if (!(bound > 0.0 && bound < 1.0e150)) return 0;
    int it = 0;
    for (; it < 64; ++it) {
        const double p = (((lam - e1) * lam + e2) * lam - e3) * lam + e4;
        const double dp = ((4.0 * lam - 3.0 * e1) * lam + 2.0 * e2) * lam - e3;
        if (!(dp > 0.0)) break;
        const double nl = lam - p / dp;
        if (!(nl < lam)) break;
        lam = nl;
    }
    /* B = N - lam I; its adjugate is (a multiple of) v v^T.  Pass 0 takes lam from Newton, pass 1 the Rayleigh quotient of pass 0's
     * vector (see above) */
    double w = 0.0, x = 0.0, y = 0.0, z = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            const double y0 = ((a * w + n01 * x) + n02 * y) + n03 * z, y1 = ((n01 * w + b * x) + n12 * y) + n13 * z;
            const double y2 = ((n02 * w + n12 * x) + c * y) + n23 * z, y3 = ((n03 * w + n13 * x) + n23 * y) + d * z;
            lam = ((w * y0 + x * y1) + y * y2) + z * y3;
        }
        const double A = a - lam, B = b - lam, C = c - lam, D = d - lam;
        const double c00 = lr_det3_(B, n12, n13, n12, C, n23, n13, n23, D);
        const double c11 = lr_det3_(A, n02, n03, n02, C, n23, n03, n23, D);
        const double c22 = lr_det3_(A, n01, n03, n01, B, n13, n03, n13, D);
        const double c33 = lr_det3_(A, n01, n02, n01, B, n12, n02, n12, C);
        const double c01 = -lr_det3_(n01, n12, n13, n02, C, n23, n03, n23, D);
        const double c02 = lr_det3_(n01, B, n13, n02, n12, n23, n03, n13, D);
        const double c03 = -lr_det3_(n01, B, n12, n02, n12, C, n03, n13, n23);
        const double c12 = -lr_det3_(A, n01, n03, n02, n12, n23, n03, n13, D);
        const double c13 = lr_det3_(A, n01, n02, n02, n12, C, n03, n13, n23);
        const double c23 = -lr_det3_(A, n01, n02, n01, B, n12, n03, n13, n23);
        double best = fabs(c00);
        w = c00; x = c01; y = c02; z = c03;
        if (fabs(c11) > best) { best = fabs(c11); w = c01; x = c11; y = c12; z = c13; }
        if (fabs(c22) > best) { best = fabs(c22); w = c02; x = c12; y = c22; z = c23; }
        if (fabs(c33) > best) { best = fabs(c33); w = c03; x = c13; y = c23; z = c33; }
        if (!(best > 1.0e-6 * ((bound * bound) * bound))) return 0;
        const double nn = sqrt(((w * w + x * x) + y * y) + z * z);
        if (!(nn > 0.0)) return 0;
        w = w / nn; x = x / nn; y = y / nn; z = z / nn;
    }
    q[0] = w; q[1] = x; q[2] = y; q[3] = z;
    return 1;
}

/* H = sum (p - cp)(q - cq)^T  (3x3, row = source axis, col = target axis)  ->  T (row-major 4x4, q ~ R p + t) */
LRC_FN void lr_rt_from_cov(const double H[3][3], const double cp[3], const double cq[3], double T[16])
{
    double Sxx = H[0][0], Sxy = H[0][1], Sxz = H[0][2];
    double Syx = H[1][0], Syy = H[1][1], Syz = H[1][2];
    double Szx = H[2][0], Szy = H[2][1], Szz = H[2][2];
    double N[4][4];
    N[0][0] = (Sxx + Syy) + Szz; N[0][1] = Syz - Szy;         N[0][2] = Szx - Sxz;         N[0][3] = Sxy - Syx;
    N[1][0] = N[0][1];           N[1][1] = (Sxx - Syy) - Szz; N[1][2] = Sxy + Syx;         N[1][3] = Szx + Sxz;
    N[2][0] = N[0][2];           N[2][1] = N[1][2];           N[2][2] = (Syy - Sxx) - Szz; N[2][3] = Syz + Szy;
    N[3][0] = N[0][3];           N[3][1] = N[1][3];           N[3][2] = N[2][3];           N[3][3] = (Szz - Sxx) - Syy;
    double q[4];
    if (!lr_horn4_maxvec_newton(N, q)) lr_jacobi4_maxvec(N, q);
    double w = q[0], x = q[1], y = q[2], z = q[3];
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z);       R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z);       R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y);       R[2][1] = 2.0 * (y * z + w * x);       R[2][2] = 1.0 - 2.0 * (x * x + y * y);
LRC_UNROLL
    for (int a = 0; a < 3; ++a) {
        double rc = (R[a][0] * cp[0] + R[a][1] * cp[1]) + R[a][2] * cp[2];
        T[4 * a + 0] = R[a][0]; T[4 * a + 1] = R[a][1]; T[4 * a + 2] = R[a][2];
        T[4 * a + 3] = cq[a] - rc;
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

/* Raw moments mom = { n, sum p [3], sum q [3], sum p q^T [9] } (what the refit, ICP and all-inlier LO fits accumulate)  ->  T */
LRC_FN void lr_rt_from_moments(const double mom[16], double T[16])
{
    const double n = mom[0];
    double cp[3], cq[3], H[3][3];
    for (int a = 0; a < 3; ++a) { cp[a] = mom[1 + a] / n; cq[a] = mom[4 + a] / n; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a][b] = mom[7 + 3 * a + b] - (n * cp[a]) * cq[b];
    lr_rt_from_cov(H, cp, cq, T);
}

/* ------------------------------------------------------------------ fp32 scoring (fmaf in this order, nothing else) */
/* Counts and error sums are integers -- sums over the inliers of (uint32)(d2 * 2^20) -- so they do not depend on the order of
 * summation; they are the same on both sides because every site evaluates d2 through this chain. */
#define LR_SCORE_SCALE 1048576.0f      /* 2^20: fixed point of the squared residual */

/* squared residual of the correspondence (p, q) under the model Rt = R | t, row-major 3x4 */
LRC_FN float lr_score_d2(const float Rt[12], float px, float py, float pz, float qx, float qy, float qz)
{
    const float x = fmaf(Rt[0], px, fmaf(Rt[1], py, fmaf(Rt[2], pz, Rt[3])));
    const float y = fmaf(Rt[4], px, fmaf(Rt[5], py, fmaf(Rt[6], pz, Rt[7])));
    const float z = fmaf(Rt[8], px, fmaf(Rt[9], py, fmaf(Rt[10], pz, Rt[11])));
    const float dx = x - qx, dy = y - qy, dz = z - qz;
    return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

/* what an inlier (d2 < thr2) adds to the error sum */
LRC_FN uint32_t lr_score_term(float d2) { return (uint32_t)(d2 * LR_SCORE_SCALE); }

/* MSAC's threshold in the fixed point of the error sum; 0 selects the ordering by count (scoring: 0 count then error, 1 MSAC) */
LRC_FN uint32_t lr_msac_T(int scoring, float thr2) { return scoring == 1 ? lr_score_term(thr2) : 0u; }

/* is the model (inlier count c, error sum q, id h) better than (bc, bq, bh)?  More inliers, then lower error, then lower id. */
LRC_FN int lr_score_better(uint32_t c, uint64_t q, long long h, uint32_t bc, uint64_t bq, long long bh, uint32_t msac_T)
{
    if (msac_T == 0u) return c > bc || (c == bc && (q < bq || (q == bq && h < bh)));
    /* MSAC: larger sum over inliers of (thr2 - d2) in the fixed point of the error sum; a model without inliers never wins */
    if (c == 0u) return 0;
    if (bc == 0u) return 1;
    const long long k = (long long)c * (long long)msac_T - (long long)q, bk = (long long)bc * (long long)msac_T - (long long)bq;
    return k > bk || (k == bk && h < bh);
}

#endif /* LR_CONTRACT_H */
