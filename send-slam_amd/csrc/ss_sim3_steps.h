/*
 * ss_sim3_steps.h -- the steps of the Sim3 RANSAC (the rule: include/sendslam_orb.h): mix32 and the
 * draws of a hypothesis, the Horn model of a triple in double, a correspondence's twelve floats, one reprojection test and the
 * selection predicate.  The kernels (ss_sim3.hip), the host twins ss_sim3_model_host / ss_sim3_check_host (ss_api_search.cpp) and
 * tests/native/sim3_steps_asan.cpp compile this text.
 *
 * Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a NaN fails it.  Compile
 * with -ffp-contract=off.  Division and square root are correctly rounded on both sides (hipcc's default).  The 4 x 4 arrays are
 * indexed by constants only, so they live in registers on the device; the rotation is the triangulation's (ss_epi_steps.h).
 */
#ifndef SS_SIM3_STEPS_H
#define SS_SIM3_STEPS_H

#include "ss_epi_steps.h" /* ss_tri_rotate, SS_EPI_UNROLL; SS_HD, the public header */

/* the fixed 32-bit multiply-xorshift finaliser of the draw stream: value n of pair `pair` under `seed` */
SS_HD uint32_t ss_sim3_mix32(uint32_t seed, uint32_t pair, uint32_t n)
{
    uint32_t h = (seed ^ (pair * 0x9E3779B1u)) + n * 0x85EBCA77u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

/* K draws of hypothesis t over 0 .. n-1 (n >= K) without replacement, swap-with-last: draw k takes value base + k of the stream
 * (base = K * t), j = (uint64(r) * (n - k)) >> 32, the value at slot j, and slot j then receives the value at slot n-1-k.  At most K
 * slots are ever displaced (slot[e] holds val[e] after draw e; the latest record of a slot wins), so no array of n is kept */
template <int K> SS_HD void ss_sim3_draw_k(uint32_t seed, uint32_t pair, int t, int n, int out[K])
{
    int slot[K] = {}, val[K] = {};
    const uint32_t base = (uint32_t)K * (uint32_t)t;
    SS_EPI_UNROLL
    for (int k = 0; k < K; k++) {
        const int last = n - 1 - k;
        const int j = (int)(((uint64_t)ss_sim3_mix32(seed, pair, base + (uint32_t)k) * (uint64_t)(uint32_t)(n - k)) >> 32);
        int vj = j, vl = last;
        SS_EPI_UNROLL
        for (int e = 0; e < k; e++) {
            if (slot[e] == j) vj = val[e];
            if (slot[e] == last) vl = val[e];
        }
        out[k] = vj;
        slot[k] = j, val[k] = vl;
    }
}

/* the three draws of hypothesis t over 0 .. n-1 (n >= 3) */
SS_HD void ss_sim3_draw(uint32_t seed, uint32_t pair, int t, int n, int out[3]) { ss_sim3_draw_k<3>(seed, pair, t, n, out); }

/* a hypothesis: X1 = sr12.X2 + t12 and its inverse, float32 */
struct ss_sim3_model {
    float sr12[9], t12[3], sr21[9], t21[3], s12;
};

SS_HD double ss_sim3_dot(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

/* Horn's rotation of M = sum Pr2 Pr1^T: the symmetric N, SS_TRI_SWEEPS sweeps of the triangulation's rotation, the quaternion at the
 * largest diagonal entry, its nine polynomial entries.  X1 ~ r.X2 (the PnP model takes the nearest rotation of a matrix from it) */
SS_HD void ss_sim3_horn(const double m[3][3], double r[9])
{
    double N[4][4], V[4][4];
    N[0][0] = (m[0][0] + m[1][1]) + m[2][2];
    N[0][1] = m[1][2] - m[2][1];
    N[0][2] = m[2][0] - m[0][2];
    N[0][3] = m[0][1] - m[1][0];
    N[1][1] = (m[0][0] - m[1][1]) - m[2][2];
    N[1][2] = m[0][1] + m[1][0];
    N[1][3] = m[2][0] + m[0][2];
    N[2][2] = (m[1][1] - m[0][0]) - m[2][2];
    N[2][3] = m[1][2] + m[2][1];
    N[3][3] = (m[2][2] - m[0][0]) - m[1][1];
    N[1][0] = N[0][1], N[2][0] = N[0][2], N[3][0] = N[0][3], N[2][1] = N[1][2], N[3][1] = N[1][3], N[3][2] = N[2][3];
    SS_EPI_UNROLL
    for (int i = 0; i < 4; i++) {
        SS_EPI_UNROLL
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
    }
    SS_EPI_ROLLED
    for (int sweep = 0; sweep < SS_TRI_SWEEPS; sweep++) {
        ss_tri_rotate<0, 1>(N, V);
        ss_tri_rotate<0, 2>(N, V);
        ss_tri_rotate<0, 3>(N, V);
        ss_tri_rotate<1, 2>(N, V);
        ss_tri_rotate<1, 3>(N, V);
        ss_tri_rotate<2, 3>(N, V);
    }
    int best = 0;
    double high = N[0][0];
    if (N[1][1] > high) best = 1, high = N[1][1];
    if (N[2][2] > high) best = 2, high = N[2][2];
    if (N[3][3] > high) best = 3, high = N[3][3];
    const double q0 = best == 0 ? V[0][0] : best == 1 ? V[0][1] : best == 2 ? V[0][2] : V[0][3];
    const double q1 = best == 0 ? V[1][0] : best == 1 ? V[1][1] : best == 2 ? V[1][2] : V[1][3];
    const double q2 = best == 0 ? V[2][0] : best == 1 ? V[2][1] : best == 2 ? V[2][2] : V[2][3];
    const double q3 = best == 0 ? V[3][0] : best == 1 ? V[3][1] : best == 2 ? V[3][2] : V[3][3];
    const double qn = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double w = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
    r[0] = 1.0 - 2.0 * (y * y + z * z);
    r[1] = 2.0 * (x * y - w * z);
    r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (x * y + w * z);
    r[4] = 1.0 - 2.0 * (x * x + z * z);
    r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (x * z - w * y);
    r[7] = 2.0 * (y * z + w * x);
    r[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* step 3b: x1[k], x2[k] the camera coordinates of draw k in keyframe 1 and 2 */
SS_HD ss_sim3_model ss_sim3_model_of(const float x1[9], const float x2[9], int fix_scale)
{
    double o1[3], o2[3], a[3][3], b[3][3]; /* a[k] = Pr1 of draw k, b[k] = Pr2 */
    SS_EPI_UNROLL
    for (int i = 0; i < 3; i++) {
        o1[i] = (((double)x1[i] + (double)x1[3 + i]) + (double)x1[6 + i]) / 3.0;
        o2[i] = (((double)x2[i] + (double)x2[3 + i]) + (double)x2[6 + i]) / 3.0;
    }
    SS_EPI_UNROLL
    for (int k = 0; k < 3; k++) {
        SS_EPI_UNROLL
        for (int i = 0; i < 3; i++) {
            a[k][i] = (double)x1[3 * k + i] - o1[i];
            b[k][i] = (double)x2[3 * k + i] - o2[i];
        }
    }
    double m[3][3];
    SS_EPI_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_EPI_UNROLL
        for (int j = 0; j < 3; j++) m[i][j] = (b[0][i] * a[0][j] + b[1][i] * a[1][j]) + b[2][i] * a[2][j];
    }
    double r[9];
    ss_sim3_horn(m, r);
    double s = 1.0;
    if (!fix_scale) {
        double p3[3][3];
        SS_EPI_UNROLL
        for (int k = 0; k < 3; k++) {
            SS_EPI_UNROLL
            for (int i = 0; i < 3; i++) p3[k][i] = ss_sim3_dot(r[3 * i], r[3 * i + 1], r[3 * i + 2], b[k][0], b[k][1], b[k][2]);
        }
        const double nom = (ss_sim3_dot(a[0][0], a[0][1], a[0][2], p3[0][0], p3[0][1], p3[0][2]) +
                            ss_sim3_dot(a[1][0], a[1][1], a[1][2], p3[1][0], p3[1][1], p3[1][2])) +
                           ss_sim3_dot(a[2][0], a[2][1], a[2][2], p3[2][0], p3[2][1], p3[2][2]);
        const double den = (ss_sim3_dot(p3[0][0], p3[0][1], p3[0][2], p3[0][0], p3[0][1], p3[0][2]) +
                            ss_sim3_dot(p3[1][0], p3[1][1], p3[1][2], p3[1][0], p3[1][1], p3[1][2])) +
                           ss_sim3_dot(p3[2][0], p3[2][1], p3[2][2], p3[2][0], p3[2][1], p3[2][2]);
        s = nom / den;
    }
    double t12[3];
    SS_EPI_UNROLL
    for (int i = 0; i < 3; i++) t12[i] = o1[i] - s * ss_sim3_dot(r[3 * i], r[3 * i + 1], r[3 * i + 2], o2[0], o2[1], o2[2]);
    const double s21 = 1.0 / s;
    ss_sim3_model o;
    bool finite = true;
    SS_EPI_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_EPI_UNROLL
        for (int j = 0; j < 3; j++) {
            o.sr12[3 * i + j] = (float)(s * r[3 * i + j]);
            o.sr21[3 * i + j] = (float)(s21 * r[3 * j + i]);
        }
        o.t12[i] = (float)t12[i];
        o.t21[i] = (float)-(s21 * ss_sim3_dot(r[i], r[3 + i], r[6 + i], t12[0], t12[1], t12[2]));
    }
    o.s12 = (float)s;
    SS_EPI_UNROLL
    for (int k = 0; k < 9; k++) finite = finite && fabsf(o.sr12[k]) <= 3.4028234663852886e38f && fabsf(o.sr21[k]) <= 3.4028234663852886e38f;
    SS_EPI_UNROLL
    for (int k = 0; k < 3; k++) finite = finite && fabsf(o.t12[k]) <= 3.4028234663852886e38f && fabsf(o.t21[k]) <= 3.4028234663852886e38f;
    finite = finite && fabsf(o.s12) <= 3.4028234663852886e38f;
    if (!finite) {
        SS_EPI_UNROLL
        for (int k = 0; k < 9; k++) o.sr12[k] = o.sr21[k] = 0.0f;
        SS_EPI_UNROLL
        for (int k = 0; k < 3; k++) o.t12[k] = o.t21[k] = 0.0f;
        o.s12 = 0.0f;
    }
    return o;
}

/* step 1 of one correspondence: its twelve floats */
struct ss_sim3_corr {
    float x1[3], x2[3]; /* camera coordinates in keyframe 1 and 2 */
    float u1, v1, u2, v2; /* their projections */
    float max1, max2;
};

/* Y = m.P + t (m row-major 3 x 3), each component ((m0*x + m1*y) + m2*z) + t */
SS_HD void ss_sim3_transform(const float *m, const float *t, float x, float y, float z, float out[3])
{
    out[0] = ((m[0] * x + m[1] * y) + m[2] * z) + t[0];
    out[1] = ((m[3] * x + m[4] * y) + m[5] * z) + t[1];
    out[2] = ((m[6] * x + m[7] * y) + m[8] * z) + t[2];
}

SS_HD void ss_sim3_project(const float X[3], float fx, float fy, float cx, float cy, float *u, float *v)
{
    const float invz = 1.0f / X[2];
    *u = fx * X[0] * invz + cx;
    *v = fy * X[1] * invz + cy;
}

/* both octaves inside the table: the caller has checked that */
SS_HD ss_sim3_corr ss_sim3_corr_of(const ss_proj_view &v1, const ss_proj_view &v2, float p1x, float p1y, float p1z, float p2x, float p2y, float p2z,
                                   float chi2, float s1, float s2)
{
    ss_sim3_corr c;
    ss_sim3_transform(v1.rcw, v1.tcw, p1x, p1y, p1z, c.x1);
    ss_sim3_transform(v2.rcw, v2.tcw, p2x, p2y, p2z, c.x2);
    ss_sim3_project(c.x1, v1.fx, v1.fy, v1.cx, v1.cy, &c.u1, &c.v1);
    ss_sim3_project(c.x2, v2.fx, v2.fy, v2.cx, v2.cy, &c.u2, &c.v2);
    c.max1 = chi2 * (s1 * s1);
    c.max2 = chi2 * (s2 * s2);
    return c;
}

/* One reprojection error of step 3c: X of the other keyframe through (m, t) into the camera (fx, fy, cx, cy), against (u, v).
 * Squares and their sum do not depend on the sign of the difference, so one text serves both tests */
SS_HD float ss_sim3_err(const float *m, const float *t, const float X[3], float fx, float fy, float cx, float cy, float u, float v)
{
    float y[3], qu, qv;
    ss_sim3_transform(m, t, X[0], X[1], X[2], y);
    ss_sim3_project(y, fx, fy, cx, cy, &qu, &qv);
    const float du = u - qu, dv = v - qv;
    return du * du + dv * dv;
}

/* the selection predicate: a hypothesis with this count is over the threshold */
SS_HD bool ss_sim3_wins(int count, int min_inliers) { return count > min_inliers; }

/* state 1 */
SS_HD bool ss_sim3_too_few(int n, int min_inliers) { return n < 3 || n < min_inliers; }

#endif
