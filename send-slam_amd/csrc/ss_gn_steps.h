/*
 * ss_gn_steps.h -- the steps every damped Gauss-Newton of the library shares, whatever its rule (DESIGN.md "Gauss-Newton core"): the
 * tree of a sum, the damped Cholesky solve, the Huber weight, R <- dR.R, the identity and the all-finite test.  The pose-only
 * optimisation (ss_pose_steps.h), the Sim3 refinement (ss_sim3opt_steps.h) and the local bundle adjustment (ss_ba_steps.h) build
 * their rules on it; the kernels, the host twins and the programs under tests/native compile this text.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it.  Compile with -ffp-contract=off.  Division and square root are correctly rounded on both sides (hipcc's default);
 * there is no other library function.  Arrays are indexed by constants only once the loops are unrolled, so they live in registers
 * on the device.
 */
#ifndef SS_GN_STEPS_H
#define SS_GN_STEPS_H

#include "ss_float_steps.h" /* SS_HD, math.h */

#if defined(__HIPCC__) || defined(__clang__)
#define SS_GN_UNROLL _Pragma("unroll")
#else
#define SS_GN_UNROLL
#endif

#define SS_GN_SLOTS 256   /* the partial sums of a tree: slot s adds the terms s, s + 256, ... */
#define SS_GN_BEHIND 1e30 /* the chi-square of a term whose depth is not > 0 */

SS_HD bool ss_gn_is_finite(double x) { return x - x == 0.0; }

SS_HD bool ss_gn_all_finite(const double R[9], const double t[3])
{
    bool ok = true;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) ok = ok && ss_gn_is_finite(R[k]);
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) ok = ok && ss_gn_is_finite(t[k]);
    return ok;
}

/* R = I, t = 0 */
SS_HD void ss_gn_identity(double R[9], double t[3])
{
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
}

/* the Huber weight of a term of weight w and squared error e2 = w * |r|^2 under the threshold d = sqrt(chi2) */
SS_HD double ss_gn_huber(bool robust, double e2, double d, double w) { return (robust && e2 > d * d) ? w * d / sqrt(e2) : w; }

/* R <- dR.R, each entry (a*b + c*d) + e*f.  The translation's rule is the caller's: it reads dR and the old t only */
SS_HD void ss_gn_rotate(const double dR[9], double R[9])
{
    double Rn[9];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) Rn[3 * i + j] = (dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j];
    }
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
}

/* the four group results of a tree */
SS_HD double ss_gn_combine(double r0, double r1, double r2, double r3) { return (r0 + r1) + (r2 + r3); }

/* a tree on the host: the SS_GN_SLOTS partial sums (overwritten) -> the sum.  Each group of 64 consecutive slots is folded by
 * halving, a[l] += a[l + h] for h = 32 .. 1; the kernels do the same through cross-lane moves (ss_gn.h) */
SS_HD double ss_gn_tree(double a[SS_GN_SLOTS])
{
    for (int g = 0; g < SS_GN_SLOTS; g += 64)
        for (int h = 32; h >= 1; h >>= 1)
            for (int l = 0; l < h; l++) a[g + l] = a[g + l] + a[g + l + h];
    return ss_gn_combine(a[0], a[64], a[128], a[192]);
}

/* The solve of a step: H (its upper triangle filled; overwritten) and the gradient g -> delta[0 .. N).  H symmetric from its upper
 * triangle, H_aa += lambda * (1 + H_aa), g negated, Cholesky by columns and the two triangular solves.  False when a pivot is not
 * > 0 */
template <int N> SS_HD bool ss_gn_solve(double H[N][N], const double *g, double lambda, double *delta)
{
    SS_GN_UNROLL
    for (int a = 1; a < N; a++) {
        SS_GN_UNROLL
        for (int b = 0; b < a; b++) H[a][b] = H[b][a];
    }
    SS_GN_UNROLL
    for (int a = 0; a < N; a++) {
        H[a][a] = H[a][a] + lambda * (1.0 + H[a][a]);
        delta[a] = -g[a];
    }
    bool ok = true;
    SS_GN_UNROLL
    for (int j = 0; j < N; j++) {
        double s = H[j][j];
        SS_GN_UNROLL
        for (int k = 0; k < j; k++) s = s - H[j][k] * H[j][k];
        ok = ok && s > 0.0;
        H[j][j] = sqrt(s);
        SS_GN_UNROLL
        for (int i = j + 1; i < N; i++) {
            double v = H[i][j];
            SS_GN_UNROLL
            for (int k = 0; k < j; k++) v = v - H[i][k] * H[j][k];
            H[i][j] = v / H[j][j];
        }
    }
    SS_GN_UNROLL
    for (int i = 0; i < N; i++) {
        double v = delta[i];
        SS_GN_UNROLL
        for (int k = 0; k < i; k++) v = v - H[i][k] * delta[k];
        delta[i] = v / H[i][i];
    }
    SS_GN_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double v = delta[i];
        SS_GN_UNROLL
        for (int k = i + 1; k < N; k++) v = v - H[k][i] * delta[k];
        delta[i] = v / H[i][i];
    }
    return ok;
}

/* The same text for a run-time order n (the reduced system of the bundle adjustment, ss_ba_steps.h): H is n rows of ld doubles, its
 * lower triangle filled.  The factor: Cholesky by columns, L over H's lower triangle; every inner sum subtracts in ascending k.
 * Each entry's subtractions being sequential in k, the rows of a column may be computed in parallel, and a right-looking schedule
 * (column k taken off every later entry once it is final) gives the same bits.  False when a pivot is not > 0 */
SS_HD bool ss_gn_chol_n(double *H, int n, int ld)
{
    bool ok = true;
    for (int j = 0; j < n; j++) {
        double s = H[(size_t)j * ld + j];
        for (int k = 0; k < j; k++) s = s - H[(size_t)j * ld + k] * H[(size_t)j * ld + k];
        ok = ok && s > 0.0;
        H[(size_t)j * ld + j] = sqrt(s);
        for (int i = j + 1; i < n; i++) {
            double v = H[(size_t)i * ld + j];
            for (int k = 0; k < j; k++) v = v - H[(size_t)i * ld + k] * H[(size_t)j * ld + k];
            H[(size_t)i * ld + j] = v / H[(size_t)j * ld + j];
        }
    }
    return ok;
}

/* the two triangular solves on the factor: delta (the right-hand side on entry) <- L^-T L^-1 delta */
SS_HD void ss_gn_subst_n(const double *L, int n, int ld, double *delta)
{
    for (int i = 0; i < n; i++) {
        double v = delta[i];
        for (int k = 0; k < i; k++) v = v - L[(size_t)i * ld + k] * delta[k];
        delta[i] = v / L[(size_t)i * ld + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = delta[i];
        for (int k = i + 1; k < n; k++) v = v - L[(size_t)k * ld + i] * delta[k];
        delta[i] = v / L[(size_t)i * ld + i];
    }
}

/* ss_gn_solve for a run-time order: H's upper triangle filled (overwritten), the gradient g -> delta[0 .. n) */
SS_HD bool ss_gn_solve_n(double *H, int n, int ld, const double *g, double lambda, double *delta)
{
    for (int a = 1; a < n; a++)
        for (int b = 0; b < a; b++) H[(size_t)a * ld + b] = H[(size_t)b * ld + a];
    for (int a = 0; a < n; a++) {
        H[(size_t)a * ld + a] = H[(size_t)a * ld + a] + lambda * (1.0 + H[(size_t)a * ld + a]);
        delta[a] = -g[a];
    }
    const bool ok = ss_gn_chol_n(H, n, ld);
    ss_gn_subst_n(H, n, ld, delta);
    return ok;
}

#endif
