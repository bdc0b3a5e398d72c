/*
 * ss_sim3opt_steps.h -- the steps of the Sim3 refinement (the rule: include/sendslam_orb.h): a
 * correspondence's twelve floats widened, the start, the rows of both edges, the 35 terms of an edge added into the sums, the
 * damped 6 x 6 or 7 x 7 Cholesky solve, the retraction, both chi-squares, the result's floats, and the whole pair on the host.  The
 * kernels (ss_sim3opt.hip), the host twin ss_sim3_opt_host (ss_api_search.cpp) and tests/native/sim3opt_steps_asan.cpp compile this
 * text.  The start rotation, the rotation's series and the table of 1 / n! are ss_pose_steps.h's; the tree of a sum, the damped
 * Cholesky solve and the Huber weight are ss_gn_steps.h's.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it (but for the step-size test of ss_pose_exp).  Compile with -ffp-contract=off.  Arrays are indexed by constants only
 * once the loops are unrolled, so they live in registers on the device.
 */
#ifndef SS_SIM3OPT_STEPS_H
#define SS_SIM3OPT_STEPS_H

#include "ss_pose_steps.h"
#include "ss_sim3_steps.h"

#define SS_SIM3OPT_SUMS 35   /* H_ab, a <= b < 7, row by row (28), then g0 .. g6 */
#define SS_SIM3OPT_SERIES 20 /* terms of the scale's exponential: the first one left out, 1 / 20!, is below 2^-60 at |sigma| = 1 */

/* what a pair's steps read of its two views and of the parameters */
struct ss_sim3opt_cams {
    double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    double chi2, delta; /* delta = sqrt(chi2) */
};

SS_HD ss_sim3opt_cams ss_sim3opt_cams_of(const ss_proj_view &v1, const ss_proj_view &v2, double chi2)
{
    ss_sim3opt_cams c;
    c.fx1 = (double)v1.fx, c.fy1 = (double)v1.fy, c.cx1 = (double)v1.cx, c.cy1 = (double)v1.cy;
    c.fx2 = (double)v2.fx, c.fy2 = (double)v2.fy, c.cx2 = (double)v2.cx, c.cy2 = (double)v2.cy;
    c.chi2 = chi2, c.delta = sqrt(chi2);
    return c;
}

/* one correspondence: the float32 camera coordinates of step 1, both keypoints and both scales, widened */
struct ss_sim3opt_corr {
    double x1[3], x2[3], u1, v1, u2, v2, w1, w2;
};

SS_HD ss_sim3opt_corr ss_sim3opt_corr_of(const float x1[3], const float x2[3], float u1, float v1, float u2, float v2, float s1, float s2)
{
    ss_sim3opt_corr c;
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) c.x1[k] = (double)x1[k], c.x2[k] = (double)x2[k];
    c.u1 = (double)u1, c.v1 = (double)v1, c.u2 = (double)u2, c.v2 = (double)v2;
    const double a = (double)s1, b = (double)s2;
    c.w1 = 1.0 / (a * a);
    c.w2 = 1.0 / (b * b);
    return c;
}

/* step 2: s the norm of row 0 of sr12 (exactly 1.0 with fix_scale), R the Gram-Schmidt rotation of its rows, t = t12.  False when an
 * entry is not finite or s is not > 0: then R = I, t = 0, s = 1 */
SS_HD bool ss_sim3opt_start(const ss_sim3_result &m, bool fix_scale, double R[9], double t[3], double *s)
{
    double st[12];
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) st[k] = (double)m.sr12[k];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) st[9 + k] = (double)m.t12[k];
    const double n0 = sqrt((st[0] * st[0] + st[1] * st[1]) + st[2] * st[2]);
    bool ok = ss_pose_start(st, R, t);
    *s = fix_scale ? 1.0 : n0;
    ok = ok && *s > 0.0 && ss_gn_is_finite(*s);
    if (!ok) {
        ss_gn_identity(R, t);
        *s = 1.0;
    }
    return ok;
}

/* the rows of one edge: r = observation - projection, J the derivative of r by the left increment (omega, upsilon, sigma) */
struct ss_sim3opt_edge {
    double J0[7], J1[7], rx, ry, w;
};

/* Y = s.(R.X2) + t, each component s*((r0*x + r1*y) + r2*z) + t */
SS_HD void ss_sim3opt_map12(const ss_sim3opt_corr &c, const double R[9], const double t[3], double s, double *x, double *y, double *z)
{
    *x = s * ((R[0] * c.x2[0] + R[1] * c.x2[1]) + R[2] * c.x2[2]) + t[0];
    *y = s * ((R[3] * c.x2[0] + R[4] * c.x2[1]) + R[5] * c.x2[2]) + t[1];
    *z = s * ((R[6] * c.x2[0] + R[7] * c.x2[1]) + R[8] * c.x2[2]) + t[2];
}

/* M = (1/s).R^T entry by entry, Z = M.(X1 - t), each component (m0*d0 + m1*d1) + m2*d2 */
SS_HD void ss_sim3opt_map21(const ss_sim3opt_corr &c, const double R[9], const double t[3], double s, double M[9], double *x, double *y, double *z)
{
    const double is = 1.0 / s;
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) M[3 * i + j] = is * R[3 * j + i];
    }
    const double d0 = c.x1[0] - t[0], d1 = c.x1[1] - t[1], d2 = c.x1[2] - t[2];
    *x = (M[0] * d0 + M[1] * d1) + M[2] * d2;
    *y = (M[3] * d0 + M[4] * d1) + M[5] * d2;
    *z = (M[6] * d0 + M[7] * d1) + M[8] * d2;
}

/* step 3, edge e12: keypoint 1 against X2 through the model.  Y moves by (-[Y]x, I, Y): the rotation and translation entries are
 * the pose rule's, and the sigma column is the structural 0 (a scale about camera 1's centre moves no projection).  False, and no
 * rows, when the depth is not > 0 */
SS_HD bool ss_sim3opt_edge12(const ss_sim3opt_corr &c, const ss_sim3opt_cams &k, const double R[9], const double t[3], double s, ss_sim3opt_edge &e)
{
    double x, y, z;
    ss_sim3opt_map12(c, R, t, s, &x, &y, &z);
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z, iz2 = iz * iz;
    e.rx = c.u1 - (k.fx1 * x * iz + k.cx1);
    e.ry = c.v1 - (k.fy1 * y * iz + k.cy1);
    e.w = c.w1;
    e.J0[0] = x * y * iz2 * k.fx1, e.J0[1] = -(1.0 + x * x * iz2) * k.fx1, e.J0[2] = y * iz * k.fx1;
    e.J0[3] = -iz * k.fx1, e.J0[4] = 0.0, e.J0[5] = x * iz2 * k.fx1, e.J0[6] = 0.0;
    e.J1[0] = (1.0 + y * y * iz2) * k.fy1, e.J1[1] = -x * y * iz2 * k.fy1, e.J1[2] = -x * iz * k.fy1;
    e.J1[3] = 0.0, e.J1[4] = -iz * k.fy1, e.J1[5] = y * iz2 * k.fy1, e.J1[6] = 0.0;
    return true;
}

/* step 3, edge e21: keypoint 2 against X1 through the inverse.  X1 moves by E = ([X1]x, -I, -X1), then by M: D = M.E column by
 * column, and J0[c] = pxz*D2c - px*D0c, J1[c] = pyz*D2c - py*D1c with px = fx*iz, pxz = fx*x*iz2, py = fy*iz, pyz = fy*y*iz2 */
SS_HD bool ss_sim3opt_edge21(const ss_sim3opt_corr &c, const ss_sim3opt_cams &k, const double R[9], const double t[3], double s, ss_sim3opt_edge &e)
{
    double M[9], x, y, z;
    ss_sim3opt_map21(c, R, t, s, M, &x, &y, &z);
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z, iz2 = iz * iz;
    e.rx = c.u2 - (k.fx2 * x * iz + k.cx2);
    e.ry = c.v2 - (k.fy2 * y * iz + k.cy2);
    e.w = c.w2;
    const double px = k.fx2 * iz, pxz = k.fx2 * x * iz2, py = k.fy2 * iz, pyz = k.fy2 * y * iz2;
    const double a = c.x1[0], b = c.x1[1], g = c.x1[2];
    double D[3][7];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        const double m0 = M[3 * i], m1 = M[3 * i + 1], m2 = M[3 * i + 2];
        D[i][0] = m1 * g - m2 * b;
        D[i][1] = m2 * a - m0 * g;
        D[i][2] = m0 * b - m1 * a;
        D[i][3] = -m0, D[i][4] = -m1, D[i][5] = -m2;
        D[i][6] = -((m0 * a + m1 * b) + m2 * g);
    }
    SS_GN_UNROLL
    for (int q = 0; q < 7; q++) {
        e.J0[q] = pxz * D[2][q] - px * D[0][q];
        e.J1[q] = pyz * D[2][q] - py * D[1][q];
    }
    return true;
}

/* step 3: the 35 terms of one edge, each added to its sum: acc = acc + term */
SS_HD void ss_sim3opt_add(const ss_sim3opt_edge &e, const ss_sim3opt_cams &k, bool robust, double acc[SS_SIM3OPT_SUMS])
{
    const double e2 = e.w * (e.rx * e.rx + e.ry * e.ry);
    const double wq = ss_gn_huber(robust, e2, k.delta, e.w);
    int n = 0;
    SS_GN_UNROLL
    for (int a = 0; a < 7; a++) {
        const double w0 = wq * e.J0[a], w1 = wq * e.J1[a];
        SS_GN_UNROLL
        for (int b = a; b < 7; b++, n++) acc[n] = acc[n] + (w0 * e.J0[b] + w1 * e.J1[b]);
        acc[28 + a] = acc[28 + a] + (w0 * e.rx + w1 * e.ry);
    }
}

/* the sum of H_ab, a <= b */
SS_HD constexpr int ss_sim3opt_h(int a, int b) { return a * 7 - a * (a - 1) / 2 + (b - a); }

/* The solve of a step over the leading N x N (6 with fix_scale, else 7) */
template <int N> SS_HD bool ss_sim3opt_solve(const double sum[SS_SIM3OPT_SUMS], double lambda, double delta[7])
{
    double H[N][N];
    SS_GN_UNROLL
    for (int a = 0; a < N; a++) {
        SS_GN_UNROLL
        for (int b = a; b < N; b++) H[a][b] = sum[ss_sim3opt_h(a, b)];
    }
    return ss_gn_solve<N>(H, sum + 28, lambda, delta);
}

/* ds = sum sigma^k / k!, k < SS_SIM3OPT_SERIES, a Horner sum from the last term */
SS_HD double ss_sim3opt_exp_scale(double sigma)
{
    const double f[2 * SS_POSE_SERIES + 2] = SS_POSE_INV_FACT;
    double v = f[SS_SIM3OPT_SERIES - 1];
    SS_GN_UNROLL
    for (int k = SS_SIM3OPT_SERIES - 2; k >= 0; k--) v = v * sigma + f[k];
    return v;
}

/* One step from its 35 sums: 0 the model moved, 2 a pivot was not > 0, 4 the step was too large (the model stays in both).
 * R <- dR.R, s <- ds*s, t <- ds*(dR.t) + upsilon.  *small: every |delta_a| < step_eps, the round ends after this step */
SS_HD int ss_sim3opt_step(const double sum[SS_SIM3OPT_SUMS], bool fix_scale, double lambda, double step_eps, double R[9], double t[3], double *s, bool *small)
{
    double delta[7], dR[9], dt[3];
    *small = false;
    delta[6] = 0.0;
    if (!(fix_scale ? ss_sim3opt_solve<6>(sum, lambda, delta) : ss_sim3opt_solve<7>(sum, lambda, delta))) return 2;
    if (!ss_pose_exp(delta, dR, dt)) return 4;
    if (!fix_scale && !(fabs(delta[6]) <= 1.0)) return 4;
    const double ds = fix_scale ? 1.0 : ss_sim3opt_exp_scale(delta[6]);
    double tn[3];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) tn[i] = ds * ((dR[3 * i] * t[0] + dR[3 * i + 1] * t[1]) + dR[3 * i + 2] * t[2]) + delta[3 + i];
    ss_gn_rotate(dR, R);
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) t[k] = tn[k];
    if (!fix_scale) *s = ds * *s;
    bool all = true;
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) all = all && fabs(delta[a]) < step_eps;
    if (!fix_scale) all = all && fabs(delta[6]) < step_eps;
    *small = all;
    return 0;
}

/* step 4: the chi-squares of both edges; the projection is formed with / z; SS_GN_BEHIND when the depth is not > 0 */
SS_HD double ss_sim3opt_chi2_12(const ss_sim3opt_corr &c, const ss_sim3opt_cams &k, const double R[9], const double t[3], double s)
{
    double x, y, z;
    ss_sim3opt_map12(c, R, t, s, &x, &y, &z);
    if (!(z > 0.0)) return SS_GN_BEHIND;
    const double ex = c.u1 - (k.fx1 * x / z + k.cx1), ey = c.v1 - (k.fy1 * y / z + k.cy1);
    return c.w1 * (ex * ex + ey * ey);
}

SS_HD double ss_sim3opt_chi2_21(const ss_sim3opt_corr &c, const ss_sim3opt_cams &k, const double R[9], const double t[3], double s)
{
    double M[9], x, y, z;
    ss_sim3opt_map21(c, R, t, s, M, &x, &y, &z);
    if (!(z > 0.0)) return SS_GN_BEHIND;
    const double ex = c.u2 - (k.fx2 * x / z + k.cx2), ey = c.v2 - (k.fy2 * y / z + k.cy2);
    return c.w2 * (ex * ex + ey * ey);
}

/* removed iff not both */
SS_HD bool ss_sim3opt_inlier(const ss_sim3opt_cams &k, double chi2_12, double chi2_21) { return chi2_12 <= k.chi2 && chi2_21 <= k.chi2; }

/* step 5 and the result's floats, formed as ss_sim3_model_of forms them and rounded once.  False when R, t, s or one of the 25
 * floats is not finite */
SS_HD bool ss_sim3opt_floats(const double R[9], const double t[3], double s, ss_sim3_result *m)
{
    const double s21 = 1.0 / s;
    const float big = 3.4028234663852886e38f;
    bool ok = ss_gn_all_finite(R, t) && ss_gn_is_finite(s);
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) {
            m->sr12[3 * i + j] = (float)(s * R[3 * i + j]);
            m->sr21[3 * i + j] = (float)(s21 * R[3 * j + i]);
        }
        m->t12[i] = (float)t[i];
        m->t21[i] = (float)-(s21 * ss_sim3_dot(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2]));
    }
    m->s12 = (float)s;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) ok = ok && fabsf(m->sr12[k]) <= big && fabsf(m->sr21[k]) <= big;
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) ok = ok && fabsf(m->t12[k]) <= big && fabsf(m->t21[k]) <= big;
    ok = ok && fabsf(m->s12) <= big;
    return ok;
}

/* the record of a pair from what its loop ends with; the floats of the embedded model are all 0.0f unless state == 0 */
SS_HD void ss_sim3opt_record(double R[9], double t[3], double s, const double R0[9], const double t0[3], double s0, double cost, int state, int status,
                             int n_corr, int n_removed, int n_inliers, int steps0, int steps1, ss_sim3_opt_result *out)
{
    ss_sim3_result m;
    if (!ss_sim3opt_floats(R, t, s, &m)) {
        state = 2;
        SS_GN_UNROLL
        for (int k = 0; k < 9; k++) R[k] = R0[k];
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) t[k] = t0[k];
        s = s0;
    }
    if (state != 0) {
        SS_GN_UNROLL
        for (int k = 0; k < 9; k++) m.sr12[k] = m.sr21[k] = 0.0f;
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) m.t12[k] = m.t21[k] = 0.0f;
        m.s12 = 0.0f;
    }
    m.state = state, m.n_corr = n_corr, m.n_inliers = state == 0 ? n_inliers : 0, m.best_inliers = 0, m.iteration = -1, m.status = status, m.reserved = 0;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) out->r12[k] = R[k];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) out->t12[k] = t[k];
    out->s12 = s;
    out->cost = cost;
    out->state = state, out->status = status, out->n_corr = n_corr, out->n_removed = n_removed, out->n_inliers = n_inliers;
    out->steps[0] = steps0, out->steps[1] = steps1;
    out->reserved = 0;
    out->model = m;
}

/* the start is usable: a model of a pair nothing voided */
SS_HD bool ss_sim3opt_start_usable(const ss_sim3_result &m) { return m.state == 0 && m.status == SS_OK; }

/* The whole pair on the host the way the kernel runs it: corr[0 .. n) in numbering order; active: n bytes, 1 = inlier on return;
 * slot: (SS_SIM3OPT_SUMS + 1) * SS_GN_SLOTS doubles of scratch.  status: the pair's (a voided pair has n = 0) */
static inline void ss_sim3opt_pair_host(const ss_sim3opt_corr *corr, int n, const ss_sim3opt_cams &cam, const ss_sim3_result &start, int status,
                                        const ss_sim3_opt_params &p, uint8_t *active, double *slot, ss_sim3_opt_result *out)
{
    const bool fix = p.fix_scale != 0;
    double R[9], t[3], s, R0[9], t0[3], s0;
    const bool usable = ss_sim3opt_start_usable(start);
    const bool start_ok = ss_sim3opt_start(start, fix, R, t, &s);
    for (int k = 0; k < 9; k++) R0[k] = R[k];
    for (int k = 0; k < 3; k++) t0[k] = t[k];
    s0 = s;
    for (int k = 0; k < n; k++) active[k] = 1;
    int state = (status != 0 || !usable) ? 1 : !start_ok ? 2 : n < p.min_corr ? 1 : 0;
    int n_in = n, n_removed = 0, steps[2] = {0, 0};
    double cost = 0.0;
    for (int round = 0; state == 0 && round < 2; round++) {
        const bool robust = round == 0;
        const int iterations = round == 0 ? p.iterations0 : n_removed > 0 ? p.iterations_more : p.iterations_same;
        for (int it = 0; it < iterations; it++) {
            for (int k = 0; k < SS_SIM3OPT_SUMS * SS_GN_SLOTS; k++) slot[k] = 0.0;
            double acc[SS_SIM3OPT_SUMS];
            for (int k = 0; k < n; k++) {
                if (!active[k]) continue;
                for (int q = 0; q < SS_SIM3OPT_SUMS; q++) acc[q] = slot[(size_t)q * SS_GN_SLOTS + k % SS_GN_SLOTS];
                ss_sim3opt_edge e;
                if (ss_sim3opt_edge12(corr[k], cam, R, t, s, e)) ss_sim3opt_add(e, cam, robust, acc);
                if (ss_sim3opt_edge21(corr[k], cam, R, t, s, e)) ss_sim3opt_add(e, cam, robust, acc);
                for (int q = 0; q < SS_SIM3OPT_SUMS; q++) slot[(size_t)q * SS_GN_SLOTS + k % SS_GN_SLOTS] = acc[q];
            }
            double sum[SS_SIM3OPT_SUMS];
            for (int q = 0; q < SS_SIM3OPT_SUMS; q++) sum[q] = ss_gn_tree(&slot[(size_t)q * SS_GN_SLOTS]);
            bool small;
            const int rc = ss_sim3opt_step(sum, fix, p.lambda, p.step_eps, R, t, &s, &small);
            if (rc != 0) {
                state = rc;
                break;
            }
            steps[round]++;
            if (small) break;
        }
        if (state != 0) break;
        double *c = &slot[(size_t)SS_SIM3OPT_SUMS * SS_GN_SLOTS];
        for (int k = 0; k < SS_GN_SLOTS; k++) c[k] = 0.0;
        n_in = 0;
        for (int k = 0; k < n; k++) {
            if (!active[k]) continue; /* a removed correspondence stays removed */
            const double c12 = ss_sim3opt_chi2_12(corr[k], cam, R, t, s), c21 = ss_sim3opt_chi2_21(corr[k], cam, R, t, s);
            active[k] = ss_sim3opt_inlier(cam, c12, c21) ? 1 : 0;
            if (!active[k]) continue;
            c[k % SS_GN_SLOTS] = c[k % SS_GN_SLOTS] + (c12 + c21);
            n_in++;
        }
        cost = ss_gn_tree(c);
        if (round == 0) {
            n_removed = n - n_in;
            if (n_in < p.min_inliers) state = 3;
        }
    }
    ss_sim3opt_record(R, t, s, R0, t0, s0, cost, state, status, n, n_removed, n_in, steps[0], steps[1], out);
}

#endif
