/*
 * ss_ba_steps.h -- the steps of the local bundle adjustment (the rule: include/sendslam_orb.h): one
 * observation's terms of V, b and W, a point's factor and its triangular solves, the terms of a block of the reduced system, the
 * back-substitution, the chi-term of the cost, and the whole problem on the host.  The observation's pose terms, the start rotation,
 * the exponential, the update and the chi-square are ss_pose_steps.h's; the tree of a sum, the Cholesky of a run-time order and the
 * Huber weight are ss_gn_steps.h's.  The kernels (ss_ba.hip), the host twin ss_local_ba_host (ss_api_search.cpp) and
 * tests/native/ba_steps_asan.cpp compile this text.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it.  Compile with -ffp-contract=off.  Division and square root are correctly rounded on both sides; there is no other
 * library function.
 */
#ifndef SS_BA_STEPS_H
#define SS_BA_STEPS_H

#include <vector>

#include "ss_pose_steps.h"

#define SS_BA_V 6    /* V00 V01 V02 V11 V12 V22 */
#define SS_BA_W 18   /* W[a][b] at 3 a + b: a = 0 .. 5 the pose's, b = 0 .. 2 the point's */
#define SS_BA_DIAG 21 /* the upper triangle of a 6 x 6 block, row by row */

/* what the gather keeps of an observation: the keypoint's coordinates, its right coordinate (-1: monocular) and its octave's scale */
struct ss_ba_meas {
    float u, v, ur, scale;
};

SS_HD ss_pose_obs ss_ba_obs_of(const double *X, const ss_ba_meas &m)
{
    ss_pose_obs o;
    o.X = X[0], o.Y = X[1], o.Z = X[2], o.u = (double)m.u, o.v = (double)m.v;
    o.stereo = m.ur > 0.0f;
    o.ur = o.stereo ? (double)m.ur : 0.0;
    const double s = (double)m.scale;
    o.w = 1.0 / (s * s);
    return o;
}

/* step 2: the terms of V (6), b (3) and W (18) of one observation under (R, t).  False, and no term, when z is not > 0.  The rows of J
 * are those of ss_pose_terms, term by term */
SS_HD bool ss_ba_lin(const ss_pose_obs &o, const ss_pose_cam &c, const double R[9], const double t[3], bool robust, double V[SS_BA_V], double b[3],
                     double W[SS_BA_W])
{
    double x, y, z;
    ss_pose_transform(R, t, o, &x, &y, &z);
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z, iz2 = iz * iz;
    const double up = c.fx * x * iz + c.cx;
    const double rx = o.u - up, ry = o.v - (c.fy * y * iz + c.cy);
    const double a0 = x * y * iz2 * c.fx, a1 = -(1.0 + x * x * iz2) * c.fx, a2 = y * iz * c.fx, a3 = -iz * c.fx, a5 = x * iz2 * c.fx;
    const double c0 = (1.0 + y * y * iz2) * c.fy, c1 = -x * y * iz2 * c.fy, c2 = -x * iz * c.fy, c4 = -iz * c.fy, c5 = y * iz2 * c.fy;
    const double J0[6] = {a0, a1, a2, a3, 0.0, a5}, J1[6] = {c0, c1, c2, 0.0, c4, c5};
    double Jp0[3], Jp1[3];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) Jp0[k] = a3 * R[k] + a5 * R[6 + k], Jp1[k] = c4 * R[3 + k] + c5 * R[6 + k];
    if (!o.stereo) {
        const double e2 = o.w * (rx * rx + ry * ry);
        const double q = ss_gn_huber(robust, e2, c.delta_mono, o.w);
        double q0[3], q1[3];
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) q0[k] = q * Jp0[k], q1[k] = q * Jp1[k];
        V[0] = q0[0] * Jp0[0] + q1[0] * Jp1[0];
        V[1] = q0[0] * Jp0[1] + q1[0] * Jp1[1];
        V[2] = q0[0] * Jp0[2] + q1[0] * Jp1[2];
        V[3] = q0[1] * Jp0[1] + q1[1] * Jp1[1];
        V[4] = q0[1] * Jp0[2] + q1[1] * Jp1[2];
        V[5] = q0[2] * Jp0[2] + q1[2] * Jp1[2];
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) b[k] = q0[k] * rx + q1[k] * ry;
        SS_GN_UNROLL
        for (int a = 0; a < 6; a++) {
            const double w0 = q * J0[a], w1 = q * J1[a];
            SS_GN_UNROLL
            for (int k = 0; k < 3; k++) W[3 * a + k] = w0 * Jp0[k] + w1 * Jp1[k];
        }
        return true;
    }
    const double rr = o.ur - (up - c.bf * iz);
    const double d0 = a0 - c.bf * y * iz2, d1 = a1 + c.bf * x * iz2, d5 = a5 - c.bf * iz2;
    const double J2[6] = {d0, d1, a2, a3, 0.0, d5};
    double Jp2[3];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) Jp2[k] = a3 * R[k] + d5 * R[6 + k];
    const double e2 = o.w * ((rx * rx + ry * ry) + rr * rr);
    const double q = ss_gn_huber(robust, e2, c.delta_stereo, o.w);
    double q0[3], q1[3], q2[3];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) q0[k] = q * Jp0[k], q1[k] = q * Jp1[k], q2[k] = q * Jp2[k];
    V[0] = (q0[0] * Jp0[0] + q1[0] * Jp1[0]) + q2[0] * Jp2[0];
    V[1] = (q0[0] * Jp0[1] + q1[0] * Jp1[1]) + q2[0] * Jp2[1];
    V[2] = (q0[0] * Jp0[2] + q1[0] * Jp1[2]) + q2[0] * Jp2[2];
    V[3] = (q0[1] * Jp0[1] + q1[1] * Jp1[1]) + q2[1] * Jp2[1];
    V[4] = (q0[1] * Jp0[2] + q1[1] * Jp1[2]) + q2[1] * Jp2[2];
    V[5] = (q0[2] * Jp0[2] + q1[2] * Jp1[2]) + q2[2] * Jp2[2];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) b[k] = (q0[k] * rx + q1[k] * ry) + q2[k] * rr;
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) {
        const double w0 = q * J0[a], w1 = q * J1[a], w2 = q * J2[a];
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) W[3 * a + k] = (w0 * Jp0[k] + w1 * Jp1[k]) + w2 * Jp2[k];
    }
    return true;
}

/* step 3: the sums V and b of a point -> its factor L (L00 L10 L11 L20 L21 L22).  False when a pivot is not > 0: the point is frozen */
SS_HD bool ss_ba_point_factor(const double V[SS_BA_V], const double b[3], double lambda, double L[6])
{
    double H[3][3], unused[3];
    H[0][0] = V[0], H[0][1] = V[1], H[0][2] = V[2], H[1][1] = V[3], H[1][2] = V[4], H[2][2] = V[5];
    const bool ok = ss_gn_solve<3>(H, b, lambda, unused);
    L[0] = H[0][0], L[1] = H[1][0], L[2] = H[1][1], L[3] = H[2][0], L[4] = H[2][1], L[5] = H[2][2];
    return ok;
}

/* v <- V^-1.v by the two triangular solves of ss_gn_solve<3> on the factor */
SS_HD void ss_ba_point_subst(const double L[6], double v[3])
{
    v[0] = v[0] / L[0];
    v[1] = (v[1] - L[1] * v[0]) / L[2];
    v[2] = ((v[2] - L[3] * v[0]) - L[4] * v[1]) / L[5];
    v[2] = v[2] / L[5];
    v[1] = (v[1] - L[4] * v[2]) / L[2];
    v[0] = ((v[0] - L[1] * v[1]) - L[3] * v[2]) / L[0];
}

/* Y = W.V^-1, row by row */
SS_HD void ss_ba_coupling(const double L[6], const double W[SS_BA_W], double Y[SS_BA_W])
{
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) {
        double v[3] = {W[3 * a], W[3 * a + 1], W[3 * a + 2]};
        ss_ba_point_subst(L, v);
        Y[3 * a] = v[0], Y[3 * a + 1] = v[1], Y[3 * a + 2] = v[2];
    }
}

/* step 4: entry (a, b) of Y_k.W_l^T, and entry a of Y_k.b */
SS_HD double ss_ba_c_term(const double Y[SS_BA_W], const double W[SS_BA_W], int a, int b)
{
    return (Y[3 * a] * W[3 * b] + Y[3 * a + 1] * W[3 * b + 1]) + Y[3 * a + 2] * W[3 * b + 2];
}

SS_HD double ss_ba_yb_term(const double Y[SS_BA_W], const double b[3], int a) { return (Y[3 * a] * b[0] + Y[3 * a + 1] * b[1]) + Y[3 * a + 2] * b[2]; }

/* the 26 sums of a keyframe -> the 21 entries of U's upper triangle row by row, damped, and g */
SS_HD void ss_ba_unpack_u(const double sum[SS_POSE_SUMS], double lambda, double U[SS_BA_DIAG], double g[6])
{
    /* SS_POSE_SUMS order: H00 .. H05, H11 .. H15, H22 .. H25, H33, H35, H44, H45, H55; H34 is the structural 0 */
    SS_GN_UNROLL
    for (int k = 0; k < 16; k++) U[k] = sum[k];
    U[16] = 0.0, U[17] = sum[16], U[18] = sum[17], U[19] = sum[18], U[20] = sum[19];
    U[0] = U[0] + lambda * (1.0 + U[0]);
    U[6] = U[6] + lambda * (1.0 + U[6]);
    U[11] = U[11] + lambda * (1.0 + U[11]);
    U[15] = U[15] + lambda * (1.0 + U[15]);
    U[18] = U[18] + lambda * (1.0 + U[18]);
    U[20] = U[20] + lambda * (1.0 + U[20]);
    SS_GN_UNROLL
    for (int k = 0; k < 6; k++) g[k] = sum[20 + k];
}

/* step 6: one free keyframe's part of a point's right-hand side, v_b -= (W^T.dc)_b */
SS_HD void ss_ba_point_rhs(const double W[SS_BA_W], const double dc[6], double v[3])
{
    SS_GN_UNROLL
    for (int b = 0; b < 3; b++)
        v[b] = v[b] - (((((W[b] * dc[0] + W[3 + b] * dc[1]) + W[6 + b] * dc[2]) + W[9 + b] * dc[3]) + W[12 + b] * dc[4]) + W[15 + b] * dc[5]);
}

/* step 7: the chi-term of an observation */
SS_HD double ss_ba_cost_term(const ss_pose_obs &o, const ss_pose_cam &c, const double R[9], const double t[3], bool robust)
{
    const double e2 = ss_pose_chi2(o, c, R, t);
    const double d = o.stereo ? c.delta_stereo : c.delta_mono;
    if (!robust || e2 <= d * d) return e2;
    return 2.0 * d * sqrt(e2) - d * d;
}

/* lambda after a step */
SS_HD double ss_ba_next_lambda(double lambda, bool accepted, double factor, double lambda_min)
{
    if (!accepted) return lambda * factor;
    const double l = lambda / factor;
    return l > lambda_min ? l : lambda_min;
}

/* the trial pose of a free keyframe: false when the step is too large (state 4); *small: every |dc_a| < step_eps */
SS_HD bool ss_ba_trial_pose(const double dc[6], double step_eps, double R[9], double t[3], bool *small)
{
    double dR[9], dt[3];
    if (!ss_pose_exp(dc, dR, dt)) return false;
    ss_pose_update(dR, dt, R, t);
    bool all = true;
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) all = all && fabs(dc[a]) < step_eps;
    *small = all;
    return true;
}

/* The whole problem on the host the way the kernels run it.  cam, start (12 doubles each) per keyframe; meas and obs [n_kf][P]; obs
 * on entry 0 = an observation, 2 = none, on return the rule's bytes; X [P][3] the points widened (+0.0 where pflag is 2), on return
 * the result; pflag [P] on entry 0 = a point, 2 = none; poses n_kf x 12.  Every field of *out is written; its status is 0 */
static inline void ss_ba_problem_host(int n_kf, int n_free, int P, const ss_pose_cam *cam, const double *start, const ss_ba_meas *meas,
                                      const ss_ba_params &p, uint8_t *obs, double *X, uint8_t *pflag, double *poses, ss_ba_result *out)
{
    const size_t zP = (size_t)P;
    const int n = 6 * n_free;
    bool start_ok = true;
    for (int k = 0; k < n_kf; k++) start_ok = ss_pose_start(start + 12 * k, poses + 12 * k, poses + 12 * k + 9) && start_ok;
    int n_obs = 0, n_stereo = 0, n_active = 0;
    for (int i = 0; i < P; i++) {
        if (pflag[i] != 0) continue;
        int cnt = 0;
        for (int k = 0; k < n_kf; k++)
            if (obs[k * zP + i] == 0) cnt++, n_stereo += meas[k * zP + i].ur > 0.0f ? 1 : 0;
        n_obs += cnt;
        if (cnt < p.min_point_obs) pflag[i] = 1;
        else n_active++;
    }
    int state = !start_ok ? 2 : n_active == 0 ? 1 : 0, n_frozen_max = 0;
    double lambda = p.lambda, cost0 = 0.0, cost_before = 0.0;
    for (int r = 0; r < 4; r++) out->steps[r] = out->accepted[r] = 0;

    std::vector<double> Wv((size_t)n_free * zP * SS_BA_W), Yv((size_t)n_free * zP * SS_BA_W), Lv(zP * 6), bv(zP * 3), A((size_t)n * n), rhs((size_t)n);
    std::vector<double> trial((size_t)n_kf * 12), Xt(zP * 3), slot((size_t)(SS_BA_DIAG + 6 + SS_POSE_SUMS) * SS_GN_SLOTS), cost_k((size_t)n_kf);
    std::vector<uint8_t> lin((size_t)n_kf * zP), solved(zP);

    auto cost_of = [&](const double *ps, const double *Xs, bool robust) {
        for (int k = 0; k < n_kf; k++) {
            for (int s = 0; s < SS_GN_SLOTS; s++) slot[(size_t)s] = 0.0;
            for (int i = 0; i < P; i++) {
                if (pflag[i] != 0 || obs[k * zP + i] != 0) continue;
                const double term = ss_ba_cost_term(ss_ba_obs_of(Xs + 3 * (size_t)i, meas[k * zP + i]), cam[k], ps + 12 * k, ps + 12 * k + 9, robust);
                slot[(size_t)(i % SS_GN_SLOTS)] = slot[(size_t)(i % SS_GN_SLOTS)] + term;
            }
            cost_k[(size_t)k] = ss_gn_tree(slot.data());
        }
        double c = 0.0;
        for (int k = 0; k < n_kf; k++) c = c + cost_k[(size_t)k];
        return c;
    };

    for (int round = 0; state == 0 && round < p.n_rounds; round++) {
        const bool robust = round < p.robust_rounds;
        const double cost_now = cost_of(poses, X, robust);
        if (!ss_gn_is_finite(cost_now)) { /* an input that is not finite: nothing the steps could do about it */
            state = 2;
            break;
        }
        cost0 = cost_now;
        if (round == 0) cost_before = cost0;
        for (int it = 0; it < p.iterations[round]; it++) {
            /* steps 2 and 3 */
            int n_frozen = 0;
            for (int i = 0; i < P; i++) {
                solved[(size_t)i] = 0;
                for (int k = 0; k < n_kf; k++) lin[k * zP + i] = 0;
                if (pflag[i] != 0) continue;
                double V[SS_BA_V] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < n_kf; k++) {
                    if (obs[k * zP + i] != 0) continue;
                    double tV[SS_BA_V], tb[3], tW[SS_BA_W];
                    if (!ss_ba_lin(ss_ba_obs_of(X + 3 * (size_t)i, meas[k * zP + i]), cam[k], poses + 12 * k, poses + 12 * k + 9, robust, tV, tb, tW)) continue;
                    lin[k * zP + i] = 1;
                    for (int e = 0; e < SS_BA_V; e++) V[e] = V[e] + tV[e];
                    for (int e = 0; e < 3; e++) b[e] = b[e] + tb[e];
                    if (k < n_free)
                        for (int e = 0; e < SS_BA_W; e++) Wv[((size_t)k * zP + i) * SS_BA_W + e] = tW[e];
                }
                double *L = &Lv[(size_t)i * 6];
                if (!ss_ba_point_factor(V, b, lambda, L)) {
                    n_frozen++;
                    continue;
                }
                solved[(size_t)i] = 1;
                for (int e = 0; e < 3; e++) bv[(size_t)i * 3 + e] = b[e];
                for (int k = 0; k < n_free; k++)
                    if (lin[k * zP + i]) ss_ba_coupling(L, &Wv[((size_t)k * zP + i) * SS_BA_W], &Yv[((size_t)k * zP + i) * SS_BA_W]);
            }
            n_frozen_max = n_frozen > n_frozen_max ? n_frozen : n_frozen_max;
            /* step 4 */
            for (size_t e = 0; e < A.size(); e++) A[e] = 0.0;
            for (int k = 0; k < n_free; k++) {
                for (int l = k; l < n_free; l++) {
                    const bool diag = k == l;
                    const int ns = diag ? SS_BA_DIAG + 6 + SS_POSE_SUMS : 36;
                    for (int e = 0; e < ns * SS_GN_SLOTS; e++) slot[(size_t)e] = 0.0;
                    for (int i = 0; i < P; i++) {
                        if (!lin[k * zP + i] || !lin[l * zP + i]) continue;
                        double term[SS_BA_DIAG + 6 + SS_POSE_SUMS];
                        int m = 0;
                        const double *Yk = &Yv[((size_t)k * zP + i) * SS_BA_W], *Wl = &Wv[((size_t)l * zP + i) * SS_BA_W];
                        if (solved[(size_t)i]) {
                            for (int a = 0; a < 6; a++)
                                for (int b = diag ? a : 0; b < 6; b++) term[m++] = ss_ba_c_term(Yk, Wl, a, b);
                            if (diag)
                                for (int a = 0; a < 6; a++) term[m++] = ss_ba_yb_term(Yk, &bv[(size_t)i * 3], a);
                        } else if (!diag) {
                            continue;
                        }
                        const int first = solved[(size_t)i] ? 0 : SS_BA_DIAG + 6;
                        if (diag) {
                            m = SS_BA_DIAG + 6;
                            (void)ss_pose_terms(ss_ba_obs_of(X + 3 * (size_t)i, meas[k * zP + i]), cam[k], poses + 12 * k, poses + 12 * k + 9, robust, term + m);
                            m += SS_POSE_SUMS;
                        }
                        for (int e = first; e < m; e++) {
                            double &a = slot[(size_t)e * SS_GN_SLOTS + i % SS_GN_SLOTS];
                            a = a + term[e];
                        }
                    }
                    double sum[SS_BA_DIAG + 6 + SS_POSE_SUMS];
                    for (int e = 0; e < ns; e++) sum[e] = ss_gn_tree(&slot[(size_t)e * SS_GN_SLOTS]);
                    if (diag) {
                        double U[SS_BA_DIAG], g[6];
                        ss_ba_unpack_u(sum + SS_BA_DIAG + 6, lambda, U, g);
                        int m = 0;
                        for (int a = 0; a < 6; a++)
                            for (int b = a; b < 6; b++, m++) A[(size_t)(6 * k + b) * n + 6 * k + a] = U[m] - sum[m];
                        for (int a = 0; a < 6; a++) rhs[(size_t)6 * k + a] = g[a] - sum[SS_BA_DIAG + a];
                    } else {
                        for (int a = 0; a < 6; a++)
                            for (int b = 0; b < 6; b++) A[(size_t)(6 * l + b) * n + 6 * k + a] = 0.0 - sum[6 * a + b];
                    }
                }
            }
            /* step 5 */
            for (int a = 0; a < n; a++) rhs[(size_t)a] = -rhs[(size_t)a];
            if (!ss_gn_chol_n(A.data(), n, n)) {
                state = 2;
                break;
            }
            ss_gn_subst_n(A.data(), n, n, rhs.data());
            /* step 6 */
            bool small = true, finite = true, large = false;
            for (int k = 0; k < n_kf; k++) {
                for (int e = 0; e < 12; e++) trial[(size_t)12 * k + e] = poses[12 * k + e];
                if (k >= n_free) continue;
                bool sm = false;
                if (!ss_ba_trial_pose(&rhs[(size_t)6 * k], p.step_eps, &trial[(size_t)12 * k], &trial[(size_t)12 * k + 9], &sm)) large = true;
                small = small && sm;
                finite = finite && ss_gn_all_finite(&trial[(size_t)12 * k], &trial[(size_t)12 * k + 9]);
            }
            if (large) {
                state = 4;
                break;
            }
            for (int i = 0; i < P; i++) {
                for (int e = 0; e < 3; e++) Xt[(size_t)i * 3 + e] = X[(size_t)i * 3 + e];
                if (pflag[i] != 0 || !solved[(size_t)i]) continue;
                double v[3] = {-bv[(size_t)i * 3], -bv[(size_t)i * 3 + 1], -bv[(size_t)i * 3 + 2]};
                for (int k = 0; k < n_free; k++)
                    if (lin[k * zP + i]) ss_ba_point_rhs(&Wv[((size_t)k * zP + i) * SS_BA_W], &rhs[(size_t)6 * k], v);
                ss_ba_point_subst(&Lv[(size_t)i * 6], v);
                for (int e = 0; e < 3; e++) {
                    Xt[(size_t)i * 3 + e] = X[(size_t)i * 3 + e] + v[e];
                    small = small && fabs(v[e]) < p.step_eps;
                    finite = finite && ss_gn_is_finite(Xt[(size_t)i * 3 + e]);
                }
            }
            /* step 7 */
            const double cost1 = cost_of(trial.data(), Xt.data(), robust);
            const bool accepted = finite && ss_gn_is_finite(cost1) && cost1 <= cost0;
            out->steps[round]++;
            lambda = ss_ba_next_lambda(lambda, accepted, p.lambda_factor, p.lambda_min);
            if (!accepted) continue;
            out->accepted[round]++;
            cost0 = cost1;
            for (int e = 0; e < n_kf * 12; e++) poses[e] = trial[(size_t)e];
            for (size_t e = 0; e < zP * 3; e++) X[e] = Xt[e];
            if (small) break;
        }
        if (state != 0) break;
        /* step 8 */
        for (int i = 0; i < P; i++) {
            if (pflag[i] != 0) continue;
            int cnt = 0;
            for (int k = 0; k < n_kf; k++) {
                if (obs[k * zP + i] != 0) continue;
                const ss_pose_obs o = ss_ba_obs_of(X + 3 * (size_t)i, meas[k * zP + i]);
                if (ss_pose_inlier(o, cam[k], ss_pose_chi2(o, cam[k], poses + 12 * k, poses + 12 * k + 9))) cnt++;
                else obs[k * zP + i] = 1;
            }
            if (cnt < p.min_point_obs) pflag[i] = 1;
        }
    }
    int n_in = 0, n_act = 0;
    for (int i = 0; i < P; i++) n_act += pflag[i] == 0 ? 1 : 0;
    for (size_t e = 0; e < (size_t)n_kf * zP; e++) n_in += obs[e] == 0 ? 1 : 0;
    out->lambda = lambda, out->cost_before = cost_before, out->cost_after = cost0;
    out->state = state, out->status = 0;
    out->n_obs = n_obs, out->n_stereo = n_stereo, out->n_inliers = n_in, out->n_points_active = n_act, out->n_frozen_max = n_frozen_max;
    out->reserved = 0;
}

#endif
