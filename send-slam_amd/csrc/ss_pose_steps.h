/*
 * ss_pose_steps.h -- the steps of the pose-only optimisation (the rule: include/sendslam_orb.h): the start
 * rotation, one observation's 26 terms, the unpacking of the 6 x 6 system, the exponential by fixed-length series, the update, the
 * chi-square, and the whole frame on the host.  The tree of a sum, the damped Cholesky solve and the Huber weight are
 * ss_gn_steps.h's.  The kernels (ss_pose.hip), the host twin ss_pose_opt_host (ss_api_search.cpp) and
 * tests/native/pose_steps_asan.cpp compile this text.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it (but for the step-size test of ss_pose_exp).  Compile with -ffp-contract=off.  Division and square root are correctly
 * rounded on both sides (hipcc's default); there is no other library function.  Arrays are indexed by constants only once the loops
 * are unrolled, so they live in registers on the device.
 */
#ifndef SS_POSE_STEPS_H
#define SS_POSE_STEPS_H

#include "../../include/sendslam_orb.h"
#include "ss_gn_steps.h"

#define SS_POSE_SUMS 26   /* H00 H01 H02 H03 H04 H05 H11 H12 H13 H14 H15 H22 H23 H24 H25 H33 H35 H44 H45 H55 (H34 = 0), then g0 .. g5 */
#define SS_POSE_SERIES 15 /* terms of each series of the exponential: the first one left out is below 2^-60 for q <= pi^2 */
#define SS_POSE_PI2 0x1.3bd3cc9be45dep+3 /* the double next to pi^2 */

/* ss_pose_inv_fact[n] is the double next to 1 / n!, n = 0 .. 2 * SS_POSE_SERIES + 1 (tests/pose_ref.py holds the same table) */
#define SS_POSE_INV_FACT                                                                                                              \
    {                                                                                                                                 \
        0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5,                   \
        0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19,               \
        0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33, 0x1.93974a8c07c9dp-37,              \
        0x1.ae7f3e733b81fp-41, 0x1.ae7f3e733b81fp-45, 0x1.952c77030ad4ap-49, 0x1.6827863b97d97p-53, 0x1.2f49b46814157p-57,              \
        0x1.e542ba4020225p-62, 0x1.71b8ef6dcf572p-66, 0x1.0ce396db7f853p-70, 0x1.761b41316381ap-75, 0x1.f2cf01972f578p-80,              \
        0x1.3f3ccdd165fa9p-84, 0x1.88e85fc6a4e5ap-89, 0x1.d1ab1c2dccea3p-94, 0x1.0a18a2635085dp-98, 0x1.259f98b4358adp-103,             \
        0x1.3932c5047d60ep-108, 0x1.434d2e783f5bcp-113                                                                                  \
    }

/* what a frame's steps read of its view and of the parameters */
struct ss_pose_cam {
    double fx, fy, cx, cy, bf;
    double chi2_mono, chi2_stereo, delta_mono, delta_stereo; /* delta = sqrt(chi2) */
};

SS_HD ss_pose_cam ss_pose_cam_of(const ss_proj_view &v, double chi2_mono, double chi2_stereo)
{
    ss_pose_cam c;
    c.fx = (double)v.fx, c.fy = (double)v.fy, c.cx = (double)v.cx, c.cy = (double)v.cy, c.bf = (double)v.bf;
    c.chi2_mono = chi2_mono, c.chi2_stereo = chi2_stereo;
    c.delta_mono = sqrt(chi2_mono), c.delta_stereo = sqrt(chi2_stereo);
    return c;
}

/* one observation: the float32 inputs widened; stereo iff ur_f > 0 (the gather stores -1 for a monocular one) */
struct ss_pose_obs {
    double X, Y, Z, u, v, ur, w;
    bool stereo;
};

SS_HD ss_pose_obs ss_pose_obs_of(float X, float Y, float Z, float u, float v, float ur_f, float scale)
{
    ss_pose_obs o;
    o.X = (double)X, o.Y = (double)Y, o.Z = (double)Z, o.u = (double)u, o.v = (double)v;
    o.stereo = ur_f > 0.0f;
    o.ur = o.stereo ? (double)ur_f : 0.0;
    const double s = (double)scale;
    o.w = 1.0 / (s * s);
    return o;
}

/* what the gather stores for the right coordinate of a keypoint row (right: the row's value, or absent) */
SS_HD float ss_pose_stored_right(bool check_right, bool have_right, float right) { return (check_right && have_right && right > 0.0f) ? right : -1.0f; }

/* step 2: the rotation next to start[0 .. 8] (rows by Gram-Schmidt, the third as a cross product) and start[9 .. 11].  False when an
 * entry of the result is not finite: the pose is then the identity */
SS_HD bool ss_pose_start(const double *start, double R[9], double t[3])
{
    const double n0 = sqrt((start[0] * start[0] + start[1] * start[1]) + start[2] * start[2]);
    const double a0 = start[0] / n0, a1 = start[1] / n0, a2 = start[2] / n0;
    const double d01 = (start[3] * a0 + start[4] * a1) + start[5] * a2;
    const double b0 = start[3] - d01 * a0, b1 = start[4] - d01 * a1, b2 = start[5] - d01 * a2;
    const double n1 = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    const double c0 = b0 / n1, c1 = b1 / n1, c2 = b2 / n1;
    R[0] = a0, R[1] = a1, R[2] = a2;
    R[3] = c0, R[4] = c1, R[5] = c2;
    R[6] = a1 * c2 - a2 * c1;
    R[7] = a2 * c0 - a0 * c2;
    R[8] = a0 * c1 - a1 * c0;
    t[0] = start[9], t[1] = start[10], t[2] = start[11];
    const bool ok = ss_gn_all_finite(R, t);
    if (!ok) ss_gn_identity(R, t);
    return ok;
}

/* the camera coordinates of an observation's point: each ((r0*X + r1*Y) + r2*Z) + t */
SS_HD void ss_pose_transform(const double R[9], const double t[3], const ss_pose_obs &o, double *x, double *y, double *z)
{
    *x = ((R[0] * o.X + R[1] * o.Y) + R[2] * o.Z) + t[0];
    *y = ((R[3] * o.X + R[4] * o.Y) + R[5] * o.Z) + t[1];
    *z = ((R[6] * o.X + R[7] * o.Y) + R[8] * o.Z) + t[2];
}

/* step 3: the 26 terms of one observation under (R, t), in the order of SS_POSE_SUMS.  False, and no term, when z is not > 0 */
SS_HD bool ss_pose_terms(const ss_pose_obs &o, const ss_pose_cam &c, const double R[9], const double t[3], bool robust, double term[SS_POSE_SUMS])
{
    double x, y, z;
    ss_pose_transform(R, t, o, &x, &y, &z);
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z, iz2 = iz * iz;
    const double up = c.fx * x * iz + c.cx;
    const double rx = o.u - up, ry = o.v - (c.fy * y * iz + c.cy);
    /* the rows of the Jacobians: J0 = {a0 a1 a2 a3 - a5}, J1 = {c0 c1 c2 - c4 c5}, J2 = {d0 d1 a2 a3 - d5} */
    const double a0 = x * y * iz2 * c.fx, a1 = -(1.0 + x * x * iz2) * c.fx, a2 = y * iz * c.fx, a3 = -iz * c.fx, a5 = x * iz2 * c.fx;
    const double c0 = (1.0 + y * y * iz2) * c.fy, c1 = -x * y * iz2 * c.fy, c2 = -x * iz * c.fy, c4 = -iz * c.fy, c5 = y * iz2 * c.fy;
    if (!o.stereo) {
        const double e2 = o.w * (rx * rx + ry * ry);
        const double wq = ss_gn_huber(robust, e2, c.delta_mono, o.w);
        const double wa0 = wq * a0, wa1 = wq * a1, wa2 = wq * a2, wa3 = wq * a3, wa5 = wq * a5;
        const double wc0 = wq * c0, wc1 = wq * c1, wc2 = wq * c2, wc4 = wq * c4, wc5 = wq * c5;
        term[0] = wa0 * a0 + wc0 * c0;
        term[1] = wa0 * a1 + wc0 * c1;
        term[2] = wa0 * a2 + wc0 * c2;
        term[3] = wa0 * a3;
        term[4] = wc0 * c4;
        term[5] = wa0 * a5 + wc0 * c5;
        term[6] = wa1 * a1 + wc1 * c1;
        term[7] = wa1 * a2 + wc1 * c2;
        term[8] = wa1 * a3;
        term[9] = wc1 * c4;
        term[10] = wa1 * a5 + wc1 * c5;
        term[11] = wa2 * a2 + wc2 * c2;
        term[12] = wa2 * a3;
        term[13] = wc2 * c4;
        term[14] = wa2 * a5 + wc2 * c5;
        term[15] = wa3 * a3;
        term[16] = wa3 * a5;
        term[17] = wc4 * c4;
        term[18] = wc4 * c5;
        term[19] = wa5 * a5 + wc5 * c5;
        term[20] = wa0 * rx + wc0 * ry;
        term[21] = wa1 * rx + wc1 * ry;
        term[22] = wa2 * rx + wc2 * ry;
        term[23] = wa3 * rx;
        term[24] = wc4 * ry;
        term[25] = wa5 * rx + wc5 * ry;
        return true;
    }
    const double rr = o.ur - (up - c.bf * iz);
    const double d0 = a0 - c.bf * y * iz2, d1 = a1 + c.bf * x * iz2, d5 = a5 - c.bf * iz2;
    const double e2 = o.w * ((rx * rx + ry * ry) + rr * rr);
    const double wq = ss_gn_huber(robust, e2, c.delta_stereo, o.w);
    const double wa0 = wq * a0, wa1 = wq * a1, wa2 = wq * a2, wa3 = wq * a3, wa5 = wq * a5;
    const double wc0 = wq * c0, wc1 = wq * c1, wc2 = wq * c2, wc4 = wq * c4, wc5 = wq * c5;
    const double wd0 = wq * d0, wd1 = wq * d1, wd2 = wq * a2, wd3 = wq * a3, wd5 = wq * d5;
    term[0] = (wa0 * a0 + wc0 * c0) + wd0 * d0;
    term[1] = (wa0 * a1 + wc0 * c1) + wd0 * d1;
    term[2] = (wa0 * a2 + wc0 * c2) + wd0 * a2;
    term[3] = wa0 * a3 + wd0 * a3;
    term[4] = wc0 * c4;
    term[5] = (wa0 * a5 + wc0 * c5) + wd0 * d5;
    term[6] = (wa1 * a1 + wc1 * c1) + wd1 * d1;
    term[7] = (wa1 * a2 + wc1 * c2) + wd1 * a2;
    term[8] = wa1 * a3 + wd1 * a3;
    term[9] = wc1 * c4;
    term[10] = (wa1 * a5 + wc1 * c5) + wd1 * d5;
    term[11] = (wa2 * a2 + wc2 * c2) + wd2 * a2;
    term[12] = wa2 * a3 + wd2 * a3;
    term[13] = wc2 * c4;
    term[14] = (wa2 * a5 + wc2 * c5) + wd2 * d5;
    term[15] = wa3 * a3 + wd3 * a3;
    term[16] = wa3 * a5 + wd3 * d5;
    term[17] = wc4 * c4;
    term[18] = wc4 * c5;
    term[19] = (wa5 * a5 + wc5 * c5) + wd5 * d5;
    term[20] = (wa0 * rx + wc0 * ry) + wd0 * rr;
    term[21] = (wa1 * rx + wc1 * ry) + wd1 * rr;
    term[22] = (wa2 * rx + wc2 * ry) + wd2 * rr;
    term[23] = wa3 * rx + wd3 * rr;
    term[24] = wc4 * ry;
    term[25] = (wa5 * rx + wc5 * ry) + wd5 * rr;
    return true;
}

/* step 4: the chi-square of an observation under (R, t); the projection is formed with / z */
SS_HD double ss_pose_chi2(const ss_pose_obs &o, const ss_pose_cam &c, const double R[9], const double t[3])
{
    double x, y, z;
    ss_pose_transform(R, t, o, &x, &y, &z);
    if (!(z > 0.0)) return SS_GN_BEHIND;
    const double up = c.fx * x / z + c.cx;
    const double ex = o.u - up, ey = o.v - (c.fy * y / z + c.cy);
    if (!o.stereo) return o.w * (ex * ex + ey * ey);
    const double er = o.ur - (up - c.bf / z);
    return o.w * ((ex * ex + ey * ey) + er * er);
}

/* an outlier iff not chi2 <= th */
SS_HD bool ss_pose_inlier(const ss_pose_obs &o, const ss_pose_cam &c, double chi2) { return chi2 <= (o.stereo ? c.chi2_stereo : c.chi2_mono); }

/* The solve of a step: the 26 sums -> delta.  H_34 is the structural 0 */
SS_HD bool ss_pose_solve(const double sum[SS_POSE_SUMS], double lambda, double delta[6])
{
    double H[6][6];
    H[0][0] = sum[0], H[0][1] = sum[1], H[0][2] = sum[2], H[0][3] = sum[3], H[0][4] = sum[4], H[0][5] = sum[5];
    H[1][1] = sum[6], H[1][2] = sum[7], H[1][3] = sum[8], H[1][4] = sum[9], H[1][5] = sum[10];
    H[2][2] = sum[11], H[2][3] = sum[12], H[2][4] = sum[13], H[2][5] = sum[14];
    H[3][3] = sum[15], H[3][4] = 0.0, H[3][5] = sum[16];
    H[4][4] = sum[17], H[4][5] = sum[18];
    H[5][5] = sum[19];
    return ss_gn_solve<6>(H, sum + 20, lambda, delta);
}

/* The exponential of delta = (omega, upsilon): dR = I + A.W + B.W^2, dt = (I + B.W + C.W^2).upsilon with A = sum (-q)^k / (2k+1)!,
 * B = sum (-q)^k / (2k+2)!, C = sum (-q)^k / (2k+3)!, k < SS_POSE_SERIES, each a Horner sum from the last term (a product, then a
 * sum, per term); q = (w0^2 + w1^2) + w2^2.  False when q > pi^2 */
SS_HD bool ss_pose_exp(const double delta[6], double dR[9], double dt[3])
{
    const double f[2 * SS_POSE_SERIES + 2] = SS_POSE_INV_FACT;
    const double w0 = delta[0], w1 = delta[1], w2 = delta[2];
    const double s00 = w0 * w0, s11 = w1 * w1, s22 = w2 * w2;
    const double q = (s00 + s11) + s22;
    if (q > SS_POSE_PI2) return false; /* a NaN q passes: the pose is then not finite, which ends the frame in state 2 */
    const double mq = -q;
    double A = f[2 * SS_POSE_SERIES - 1], B = f[2 * SS_POSE_SERIES], C = f[2 * SS_POSE_SERIES + 1];
    SS_GN_UNROLL
    for (int k = SS_POSE_SERIES - 2; k >= 0; k--) {
        A = A * mq + f[2 * k + 1];
        B = B * mq + f[2 * k + 2];
        C = C * mq + f[2 * k + 3];
    }
    const double p01 = w0 * w1, p02 = w0 * w2, p12 = w1 * w2;
    const double m00 = -(s11 + s22), m11 = -(s00 + s22), m22 = -(s00 + s11); /* the diagonal of W^2 */
    dR[0] = 1.0 + B * m00;
    dR[1] = B * p01 - A * w2;
    dR[2] = B * p02 + A * w1;
    dR[3] = B * p01 + A * w2;
    dR[4] = 1.0 + B * m11;
    dR[5] = B * p12 - A * w0;
    dR[6] = B * p02 - A * w1;
    dR[7] = B * p12 + A * w0;
    dR[8] = 1.0 + B * m22;
    const double v0 = 1.0 + C * m00, v1 = C * p01 - B * w2, v2 = C * p02 + B * w1;
    const double v3 = C * p01 + B * w2, v4 = 1.0 + C * m11, v5 = C * p12 - B * w0;
    const double v6 = C * p02 - B * w1, v7 = C * p12 + B * w0, v8 = 1.0 + C * m22;
    dt[0] = (v0 * delta[3] + v1 * delta[4]) + v2 * delta[5];
    dt[1] = (v3 * delta[3] + v4 * delta[4]) + v5 * delta[5];
    dt[2] = (v6 * delta[3] + v7 * delta[4]) + v8 * delta[5];
    return true;
}

/* R <- dR.R, t <- dR.t + dt, each entry ((a*b + c*d) + e*f) [+ g] */
SS_HD void ss_pose_update(const double dR[9], const double dt[3], double R[9], double t[3])
{
    double tn[3];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) tn[i] = ((dR[3 * i] * t[0] + dR[3 * i + 1] * t[1]) + dR[3 * i + 2] * t[2]) + dt[i];
    ss_gn_rotate(dR, R);
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) t[k] = tn[k];
}

/* One step from its 26 sums: 0 the pose moved, 2 a pivot was not > 0, 4 the step was too large (the pose stays in both).
 * *small: every |delta_a| < step_eps, the round ends after this step */
SS_HD int ss_pose_step(const double sum[SS_POSE_SUMS], double lambda, double step_eps, double R[9], double t[3], bool *small)
{
    double delta[6], dR[9], dt[3];
    *small = false;
    if (!ss_pose_solve(sum, lambda, delta)) return 2;
    if (!ss_pose_exp(delta, dR, dt)) return 4;
    ss_pose_update(dR, dt, R, t);
    bool all = true;
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) all = all && fabs(delta[a]) < step_eps;
    *small = all;
    return 0;
}

/* The whole frame on the host the way the kernel runs it: obs[0 .. n) in numbering order; active: n bytes, 1 = inlier on return;
 * slot: (SS_POSE_SUMS + 1) * SS_GN_SLOTS doubles of scratch.  Every field of *out is written; its status is 0 */
static inline void ss_pose_frame_host(const ss_pose_obs *obs, int n, const ss_pose_cam &cam, const double *start, const ss_pose_opt_params &p,
                                      uint8_t *active, double *slot, ss_pose_result *out)
{
    double R[9], t[3], R0[9], t0[3];
    const bool start_ok = ss_pose_start(start, R, t);
    for (int k = 0; k < 9; k++) R0[k] = R[k];
    for (int k = 0; k < 3; k++) t0[k] = t[k];
    for (int k = 0; k < n; k++) active[k] = 1;
    int state = !start_ok ? 2 : n < p.min_obs ? 1 : 0, n_in = n, n_stereo = 0;
    for (int k = 0; k < 8; k++) out->steps[k] = 0;
    double cost = 0.0;
    for (int round = 0; state == 0 && round < p.n_rounds; round++) {
        const bool robust = round < p.robust_rounds;
        for (int it = 0; it < p.iterations; it++) {
            for (int k = 0; k < SS_POSE_SUMS * SS_GN_SLOTS; k++) slot[k] = 0.0;
            for (int k = 0; k < n; k++) {
                double term[SS_POSE_SUMS];
                if (!active[k] || !ss_pose_terms(obs[k], cam, R, t, robust, term)) continue;
                for (int s = 0; s < SS_POSE_SUMS; s++) {
                    double &a = slot[(size_t)s * SS_GN_SLOTS + k % SS_GN_SLOTS];
                    a = a + term[s];
                }
            }
            double sum[SS_POSE_SUMS];
            for (int s = 0; s < SS_POSE_SUMS; s++) sum[s] = ss_gn_tree(&slot[(size_t)s * SS_GN_SLOTS]);
            bool small;
            const int rc = ss_pose_step(sum, p.lambda, p.step_eps, R, t, &small);
            if (rc != 0) {
                state = rc;
                break;
            }
            out->steps[round]++;
            if (small) break;
        }
        if (state != 0) break;
        /* step 4 */
        double *c = &slot[(size_t)SS_POSE_SUMS * SS_GN_SLOTS];
        for (int k = 0; k < SS_GN_SLOTS; k++) c[k] = 0.0;
        n_in = 0;
        for (int k = 0; k < n; k++) {
            const double chi2 = ss_pose_chi2(obs[k], cam, R, t);
            active[k] = ss_pose_inlier(obs[k], cam, chi2) ? 1 : 0;
            if (!active[k]) continue;
            c[k % SS_GN_SLOTS] = c[k % SS_GN_SLOTS] + chi2;
            n_in++;
        }
        cost = ss_gn_tree(c);
        if (n_in < p.min_obs) state = 3;
    }
    if (!ss_gn_all_finite(R, t)) {
        state = 2;
        for (int k = 0; k < 9; k++) R[k] = R0[k];
        for (int k = 0; k < 3; k++) t[k] = t0[k];
    }
    for (int k = 0; k < n; k++) n_stereo += obs[k].stereo ? 1 : 0;
    for (int k = 0; k < 9; k++) out->rcw[k] = R[k];
    for (int k = 0; k < 3; k++) out->tcw[k] = t[k];
    out->cost = cost;
    out->state = state, out->status = 0;
    out->n_obs = n, out->n_stereo = n_stereo, out->n_inliers = n_in;
    out->reserved = 0;
}

#endif
