/*
 * ss_epi_steps.h -- the steps of the epipolar search and of the triangulation (the rule: include/sendslam_orb.h; DESIGN.md
 * section 18): the epipole and epipolar-line tests of one couple in float32, steps 1 - 9 of one match with its map point in
 * double.  The kernels (ss_epi.hip), the host twins ss_epi_check_host / ss_triangulate_host (ss_api_search.cpp) and
 * tests/native/epi_steps_asan.cpp compile this text.
 *
 * Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a NaN fails it.  Compile
 * with -ffp-contract=off.  Division and square root are correctly rounded on both sides (hipcc's default).  The 4 x 4 arrays are
 * indexed by constants only (the pair loop is unrolled through templates), so they live in registers on the device.
 */
#ifndef SS_EPI_STEPS_H
#define SS_EPI_STEPS_H

#include "../../include/sendslam_orb.h"
#include "ss_float_steps.h" /* SS_HD, math.h */
#include "ss_unproject_steps.h" /* ss_unproject_xyz: modes 1 and 2 of the stereo form */

#if defined(__HIPCC__) || defined(__HIP__)
#define SS_EPI_UNROLL _Pragma("unroll")
#define SS_EPI_ROLLED _Pragma("unroll 1")
#else
#define SS_EPI_UNROLL
#define SS_EPI_ROLLED
#endif

/* the epipolar line of query keypoint (x, y) in image 2: once per query row */
struct ss_epi_line {
    float a, b, c;
};
SS_HD ss_epi_line ss_epi_line_of(const float *f, float x, float y)
{
    ss_epi_line l;
    l.a = (x * f[0] + y * f[3]) + f[6];
    l.b = (x * f[1] + y * f[4]) + f[7];
    l.c = (x * f[2] + y * f[5]) + f[8];
    return l;
}

/* tests 1 - 3 of one couple: 0 pass, 1 octave, 2 epipole, 3 line.  scale[octave] is read only for an octave inside the table */
SS_HD int ss_epi_check(float ex, float ey, int epipole_test, int coarse, const ss_epi_line &l, const float *scale, int n_levels, float xj,
                       float yj, int octave_j)
{
    if (!(octave_j >= 0 && octave_j < n_levels)) return 1;
    const float s = scale[octave_j];
    if (epipole_test) {
        const float dx = ex - xj, dy = ey - yj;
        if (!(dx * dx + dy * dy >= 100.0f * s)) return 2;
    }
    if (!coarse) {
        const float num = (l.a * xj + l.b * yj) + l.c;
        const float den = l.a * l.a + l.b * l.b;
        const float sigma2 = s * s;
        if (!(den > 0.0f && num * num / den < 3.84f * sigma2)) return 3;
    }
    return 0;
}

/* ---- triangulation ---- */
struct ss_tri_out {
    ss_tri_info info;
    ss_map_point point; /* all 0.0f unless info.state == 0 */
};

/* one Jacobi rotation on the symmetric M (both triangles kept) and the vectors V, indices known at compile time */
template <int P, int Q> SS_HD void ss_tri_rotate(double (&M)[4][4], double (&V)[4][4])
{
    const double apq = M[P][Q];
    if (apq != 0.0) {
        const double theta = (M[Q][Q] - M[P][P]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        SS_EPI_UNROLL
        for (int k = 0; k < 4; k++) {
            if (k == P || k == Q) continue;
            const double akp = M[k][P], akq = M[k][Q];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            M[k][P] = M[P][k] = np;
            M[k][Q] = M[Q][k] = nq;
        }
        M[P][P] = M[P][P] - t * apq;
        M[Q][Q] = M[Q][Q] + t * apq;
        M[P][Q] = M[Q][P] = 0.0;
        SS_EPI_UNROLL
        for (int k = 0; k < 4; k++) {
            const double vkp = V[k][P], vkq = V[k][Q];
            V[k][P] = c * vkp - s * vkq;
            V[k][Q] = s * vkp + c * vkq;
        }
    }
}

/* the smallest eigenvector of A^T A for the four rows of A: the upper triangle of M, each entry the sum of its four products in
 * row order, mirrored; SS_TRI_SWEEPS sweeps of cyclic Jacobi; the column of the smallest diagonal entry, the first among equals.
 * ss_tri_eval and the two-view CheckRT (ss_two_view_steps.h) triangulate with it */
SS_HD void ss_tri_null4(const double (&A)[4][4], double v[4])
{
    double M[4][4], V[4][4];
    SS_EPI_UNROLL
    for (int i = 0; i < 4; i++) {
        SS_EPI_UNROLL
        for (int j = 0; j < 4; j++) {
            if (j >= i) M[i][j] = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    M[1][0] = M[0][1], M[2][0] = M[0][2], M[3][0] = M[0][3], M[2][1] = M[1][2], M[3][1] = M[1][3], M[3][2] = M[2][3];
    SS_EPI_ROLLED
    for (int sweep = 0; sweep < SS_TRI_SWEEPS; sweep++) {
        ss_tri_rotate<0, 1>(M, V);
        ss_tri_rotate<0, 2>(M, V);
        ss_tri_rotate<0, 3>(M, V);
        ss_tri_rotate<1, 2>(M, V);
        ss_tri_rotate<1, 3>(M, V);
        ss_tri_rotate<2, 3>(M, V);
    }
    int best = 0;
    double low = M[0][0];
    if (M[1][1] < low) best = 1, low = M[1][1];
    if (M[2][2] < low) best = 2, low = M[2][2];
    if (M[3][3] < low) best = 3, low = M[3][3];
    v[0] = best == 0 ? V[0][0] : best == 1 ? V[0][1] : best == 2 ? V[0][2] : V[0][3];
    v[1] = best == 0 ? V[1][0] : best == 1 ? V[1][1] : best == 2 ? V[1][2] : V[1][3];
    v[2] = best == 0 ? V[2][0] : best == 1 ? V[2][1] : best == 2 ? V[2][2] : V[2][3];
    v[3] = best == 0 ? V[3][0] : best == 1 ? V[3][1] : best == 2 ? V[3][2] : V[3][3];
}

SS_HD ss_tri_out ss_tri_rejected(int state, double cosp, double e1, double e2)
{
    ss_tri_out o;
    o.info.state = state;
    o.info.cos_parallax = cosp == cosp ? (float)cosp : 0.0f; /* a NaN is reported as 0: its sign and payload are the machine's */
    o.info.err1_sq = e1 == e1 ? (float)e1 : 0.0f;
    o.info.err2_sq = e2 == e2 ? (float)e2 : 0.0f;
    o.point.x = o.point.y = o.point.z = o.point.nx = o.point.ny = o.point.nz = o.point.min_dist = o.point.max_dist = 0.0f;
    return o;
}

/* steps 1 - 9 of the match (x1, y1, o1) of keyframe 1 with (x2, y2, o2) of keyframe 2, and its map point */
SS_HD ss_tri_out ss_tri_eval(const ss_epi_pair &w, const ss_tri_params &tp, const float *scale, int n_levels, float fx1, float fy1, int o1,
                             float fx2, float fy2, int o2)
{
    if (!(o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels)) return ss_tri_rejected(10, 0.0, 0.0, 0.0);
    const double x1 = (double)fx1, y1 = (double)fy1, x2 = (double)fx2, y2 = (double)fy2;
    const double s1 = (double)scale[o1], s2 = (double)scale[o2];
    const double *R1 = w.rcw1, *t1 = w.tcw1, *R2 = w.rcw2, *t2 = w.tcw2;
    /* 1 */
    const double a1 = (x1 - w.cx1) * w.invfx1, b1 = (y1 - w.cy1) * w.invfy1;
    const double a2 = (x2 - w.cx2) * w.invfx2, b2 = (y2 - w.cy2) * w.invfy2;
    const double r1x = (R1[0] * a1 + R1[3] * b1) + R1[6], r1y = (R1[1] * a1 + R1[4] * b1) + R1[7], r1z = (R1[2] * a1 + R1[5] * b1) + R1[8];
    const double r2x = (R2[0] * a2 + R2[3] * b2) + R2[6], r2y = (R2[1] * a2 + R2[4] * b2) + R2[7], r2z = (R2[2] * a2 + R2[5] * b2) + R2[8];
    const double dot = (r1x * r2x + r1y * r2y) + r1z * r2z;
    const double l1 = sqrt((r1x * r1x + r1y * r1y) + r1z * r1z), l2 = sqrt((r2x * r2x + r2y * r2y) + r2z * r2z);
    const double cosp = dot / (l1 * l2);
    if (!(cosp > 0.0 && cosp < tp.cos_parallax_max)) return ss_tri_rejected(1, cosp, 0.0, 0.0);
    /* 2 */
    double A[4][4], v[4];
    SS_EPI_UNROLL
    for (int c = 0; c < 4; c++) {
        const double p10 = c < 3 ? R1[c] : t1[0], p11 = c < 3 ? R1[3 + c] : t1[1], p12 = c < 3 ? R1[6 + c] : t1[2];
        const double p20 = c < 3 ? R2[c] : t2[0], p21 = c < 3 ? R2[3 + c] : t2[1], p22 = c < 3 ? R2[6 + c] : t2[2];
        A[0][c] = a1 * p12 - p10;
        A[1][c] = b1 * p12 - p11;
        A[2][c] = a2 * p22 - p20;
        A[3][c] = b2 * p22 - p21;
    }
    ss_tri_null4(A, v);
    const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
    if (!(fabs(v3) <= 1.7976931348623157e308 && v3 != 0.0)) return ss_tri_rejected(2, cosp, 0.0, 0.0);
    const double X0 = v0 / v3, X1 = v1 / v3, X2 = v2 / v3;
    /* 3, 4 */
    const double z1 = ((R1[6] * X0 + R1[7] * X1) + R1[8] * X2) + t1[2];
    if (!(z1 > 0.0)) return ss_tri_rejected(3, cosp, 0.0, 0.0);
    const double z2 = ((R2[6] * X0 + R2[7] * X1) + R2[8] * X2) + t2[2];
    if (!(z2 > 0.0)) return ss_tri_rejected(4, cosp, 0.0, 0.0);
    /* 5 */
    const double x1c = ((R1[0] * X0 + R1[1] * X1) + R1[2] * X2) + t1[0], y1c = ((R1[3] * X0 + R1[4] * X1) + R1[5] * X2) + t1[1];
    const double eu1 = ((w.fx1 * x1c) / z1 + w.cx1) - x1, ev1 = ((w.fy1 * y1c) / z1 + w.cy1) - y1;
    const double err1 = eu1 * eu1 + ev1 * ev1;
    if (!(err1 <= tp.chi2 * (s1 * s1))) return ss_tri_rejected(5, cosp, err1, 0.0);
    /* 6 */
    const double x2c = ((R2[0] * X0 + R2[1] * X1) + R2[2] * X2) + t2[0], y2c = ((R2[3] * X0 + R2[4] * X1) + R2[5] * X2) + t2[1];
    const double eu2 = ((w.fx2 * x2c) / z2 + w.cx2) - x2, ev2 = ((w.fy2 * y2c) / z2 + w.cy2) - y2;
    const double err2 = eu2 * eu2 + ev2 * ev2;
    if (!(err2 <= tp.chi2 * (s2 * s2))) return ss_tri_rejected(6, cosp, err1, err2);
    /* 7 */
    const double n1x = X0 - w.ow1[0], n1y = X1 - w.ow1[1], n1z = X2 - w.ow1[2];
    const double n2x = X0 - w.ow2[0], n2y = X1 - w.ow2[1], n2z = X2 - w.ow2[2];
    const double d1 = sqrt((n1x * n1x + n1y * n1y) + n1z * n1z), d2 = sqrt((n2x * n2x + n2y * n2y) + n2z * n2z);
    if (!(d1 > 0.0 && d2 > 0.0)) return ss_tri_rejected(7, cosp, err1, err2);
    /* 8 */
    if (tp.far_limit > 0.0 && !(d1 < tp.far_limit && d2 < tp.far_limit)) return ss_tri_rejected(8, cosp, err1, err2);
    /* 9 */
    const double rd = d2 / d1, ro = s1 / s2;
    if (!(rd * tp.ratio_factor >= ro && rd <= ro * tp.ratio_factor)) return ss_tri_rejected(9, cosp, err1, err2);
    ss_tri_out o = ss_tri_rejected(0, cosp, err1, err2);
    const double max_dist = d1 * s1;
    o.point.x = (float)X0, o.point.y = (float)X1, o.point.z = (float)X2;
    o.point.nx = (float)((n1x / d1 + n2x / d2) / 2.0);
    o.point.ny = (float)((n1y / d1 + n2y / d2) / 2.0);
    o.point.nz = (float)((n1z / d1 + n2z / d2) / 2.0);
    o.point.max_dist = (float)max_dist;
    o.point.min_dist = (float)(max_dist / (double)scale[n_levels - 1]);
    return o;
}

/* ---- triangulation, stereo form (LocalMapping::CreateNewMapPoints with its stereo branch): ss_tri_eval's steps with the stereo
 * parallax, the unprojection modes and the three-term errors.  With both right coordinates below 0 every number is ss_tri_eval's ---- */
struct ss_tri_stereo_out {
    ss_tri_stereo_info info;
    ss_map_point point; /* all 0.0f unless info.state == 0 */
};

SS_HD float ss_tri_f32_or_0(double v) { return v == v ? (float)v : 0.0f; } /* a NaN is reported as 0 */

SS_HD ss_tri_stereo_out ss_tri_stereo_rejected(int state, int mode, double cosr, double cs1, double cs2, double e1, double e2)
{
    ss_tri_stereo_out o;
    o.info.state = state, o.info.mode = mode, o.info.reserved = 0;
    o.info.cos_rays = ss_tri_f32_or_0(cosr), o.info.cs1 = ss_tri_f32_or_0(cs1), o.info.cs2 = ss_tri_f32_or_0(cs2);
    o.info.err1_sq = ss_tri_f32_or_0(e1), o.info.err2_sq = ss_tri_f32_or_0(e2);
    o.point.x = o.point.y = o.point.z = o.point.nx = o.point.ny = o.point.nz = o.point.min_dist = o.point.max_dist = 0.0f;
    return o;
}

/* the stereo parallax of a side: cos(2 atan2(b / 2, depth)) in its closed form */
SS_HD double ss_tri_stereo_cos(double b, float depth)
{
    const double d = (double)depth, h = b / 2.0;
    return (d * d - h * h) / (d * d + h * h);
}

SS_HD ss_tri_stereo_out ss_tri_stereo_eval(const ss_epi_pair &w, const ss_tri_stereo_rig &rig, const ss_tri_stereo_params &sp, const float *scale,
                                           int n_levels, float fx1, float fy1, int o1, float depth1, float right1, float fx2, float fy2, int o2,
                                           float depth2, float right2)
{
    if (!(o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels)) return ss_tri_stereo_rejected(10, -1, 0.0, 0.0, 0.0, 0.0, 0.0);
    const ss_tri_params &tp = sp.tri;
    const double x1 = (double)fx1, y1 = (double)fy1, x2 = (double)fx2, y2 = (double)fy2;
    const double s1 = (double)scale[o1], s2 = (double)scale[o2];
    const double *R1 = w.rcw1, *t1 = w.tcw1, *R2 = w.rcw2, *t2 = w.tcw2;
    /* 1: the rays, then the stereo parallax of one side (upstream's else-if is kept) */
    const double a1 = (x1 - w.cx1) * w.invfx1, b1 = (y1 - w.cy1) * w.invfy1;
    const double a2 = (x2 - w.cx2) * w.invfx2, b2 = (y2 - w.cy2) * w.invfy2;
    const double r1x = (R1[0] * a1 + R1[3] * b1) + R1[6], r1y = (R1[1] * a1 + R1[4] * b1) + R1[7], r1z = (R1[2] * a1 + R1[5] * b1) + R1[8];
    const double r2x = (R2[0] * a2 + R2[3] * b2) + R2[6], r2y = (R2[1] * a2 + R2[4] * b2) + R2[7], r2z = (R2[2] * a2 + R2[5] * b2) + R2[8];
    const double dot = (r1x * r2x + r1y * r2y) + r1z * r2z;
    const double l1 = sqrt((r1x * r1x + r1y * r1y) + r1z * r1z), l2 = sqrt((r2x * r2x + r2y * r2y) + r2z * r2z);
    const double cosr = dot / (l1 * l2);
    const bool stereo1 = right1 >= 0.0f, stereo2 = right2 >= 0.0f;
    double cs1 = cosr + 1.0, cs2 = cosr + 1.0;
    if (stereo1) cs1 = ss_tri_stereo_cos(rig.b1, depth1);
    else if (stereo2) cs2 = ss_tri_stereo_cos(rig.b2, depth2);
    const double cs = cs2 < cs1 ? cs2 : cs1; /* std::min(cs1, cs2) */
    int mode;
    double X0, X1, X2;
    if (cosr < cs && cosr > 0.0 && (stereo1 || stereo2 || cosr < tp.cos_parallax_max)) {
        /* 2 */
        mode = 0;
        double A[4][4], v[4];
        SS_EPI_UNROLL
        for (int c = 0; c < 4; c++) {
            const double p10 = c < 3 ? R1[c] : t1[0], p11 = c < 3 ? R1[3 + c] : t1[1], p12 = c < 3 ? R1[6 + c] : t1[2];
            const double p20 = c < 3 ? R2[c] : t2[0], p21 = c < 3 ? R2[3 + c] : t2[1], p22 = c < 3 ? R2[6 + c] : t2[2];
            A[0][c] = a1 * p12 - p10;
            A[1][c] = b1 * p12 - p11;
            A[2][c] = a2 * p22 - p20;
            A[3][c] = b2 * p22 - p21;
        }
        ss_tri_null4(A, v);
        const double v3 = v[3];
        if (!(fabs(v3) <= 1.7976931348623157e308 && v3 != 0.0)) return ss_tri_stereo_rejected(2, mode, cosr, cs1, cs2, 0.0, 0.0);
        X0 = v[0] / v3, X1 = v[1] / v3, X2 = v[2] / v3;
    } else if (stereo1 && cs1 < cs2) {
        mode = 1;
        double X[3];
        ss_unproject_xyz(R1, w.ow1, w.cx1, w.cy1, w.invfx1, w.invfy1, fx1, fy1, depth1, X);
        X0 = X[0], X1 = X[1], X2 = X[2];
    } else if (stereo2 && cs2 < cs1) {
        mode = 2;
        double X[3];
        ss_unproject_xyz(R2, w.ow2, w.cx2, w.cy2, w.invfx2, w.invfy2, fx2, fy2, depth2, X);
        X0 = X[0], X1 = X[1], X2 = X[2];
    } else {
        return ss_tri_stereo_rejected(1, -1, cosr, cs1, cs2, 0.0, 0.0);
    }
    /* 3, 4 */
    const double z1 = ((R1[6] * X0 + R1[7] * X1) + R1[8] * X2) + t1[2];
    if (!(z1 > 0.0)) return ss_tri_stereo_rejected(3, mode, cosr, cs1, cs2, 0.0, 0.0);
    const double z2 = ((R2[6] * X0 + R2[7] * X1) + R2[8] * X2) + t2[2];
    if (!(z2 > 0.0)) return ss_tri_stereo_rejected(4, mode, cosr, cs1, cs2, 0.0, 0.0);
    /* 5 */
    const double x1c = ((R1[0] * X0 + R1[1] * X1) + R1[2] * X2) + t1[0], y1c = ((R1[3] * X0 + R1[4] * X1) + R1[5] * X2) + t1[1];
    const double u1 = (w.fx1 * x1c) / z1 + w.cx1;
    const double eu1 = u1 - x1, ev1 = ((w.fy1 * y1c) / z1 + w.cy1) - y1;
    double err1 = eu1 * eu1 + ev1 * ev1, lim1 = tp.chi2;
    if (stereo1) {
        const double ur = u1 - rig.bf1 * (1.0 / z1), er = ur - (double)right1;
        err1 = err1 + er * er, lim1 = sp.chi2_stereo;
    }
    if (!(err1 <= lim1 * (s1 * s1))) return ss_tri_stereo_rejected(5, mode, cosr, cs1, cs2, err1, 0.0);
    /* 6 */
    const double x2c = ((R2[0] * X0 + R2[1] * X1) + R2[2] * X2) + t2[0], y2c = ((R2[3] * X0 + R2[4] * X1) + R2[5] * X2) + t2[1];
    const double u2 = (w.fx2 * x2c) / z2 + w.cx2;
    const double eu2 = u2 - x2, ev2 = ((w.fy2 * y2c) / z2 + w.cy2) - y2;
    double err2 = eu2 * eu2 + ev2 * ev2, lim2 = tp.chi2;
    if (stereo2) {
        const double ur = u2 - rig.bf2 * (1.0 / z2), er = ur - (double)right2;
        err2 = err2 + er * er, lim2 = sp.chi2_stereo;
    }
    if (!(err2 <= lim2 * (s2 * s2))) return ss_tri_stereo_rejected(6, mode, cosr, cs1, cs2, err1, err2);
    /* 7 */
    const double n1x = X0 - w.ow1[0], n1y = X1 - w.ow1[1], n1z = X2 - w.ow1[2];
    const double n2x = X0 - w.ow2[0], n2y = X1 - w.ow2[1], n2z = X2 - w.ow2[2];
    const double d1 = sqrt((n1x * n1x + n1y * n1y) + n1z * n1z), d2 = sqrt((n2x * n2x + n2y * n2y) + n2z * n2z);
    if (!(d1 > 0.0 && d2 > 0.0)) return ss_tri_stereo_rejected(7, mode, cosr, cs1, cs2, err1, err2);
    /* 8 */
    if (tp.far_limit > 0.0 && !(d1 < tp.far_limit && d2 < tp.far_limit)) return ss_tri_stereo_rejected(8, mode, cosr, cs1, cs2, err1, err2);
    /* 9 */
    const double rd = d2 / d1, ro = s1 / s2;
    if (!(rd * tp.ratio_factor >= ro && rd <= ro * tp.ratio_factor)) return ss_tri_stereo_rejected(9, mode, cosr, cs1, cs2, err1, err2);
    ss_tri_stereo_out o = ss_tri_stereo_rejected(0, mode, cosr, cs1, cs2, err1, err2);
    const double max_dist = d1 * s1;
    o.point.x = (float)X0, o.point.y = (float)X1, o.point.z = (float)X2;
    o.point.nx = (float)((n1x / d1 + n2x / d2) / 2.0);
    o.point.ny = (float)((n1y / d1 + n2y / d2) / 2.0);
    o.point.nz = (float)((n1z / d1 + n2z / d2) / 2.0);
    o.point.max_dist = (float)max_dist;
    o.point.min_dist = (float)(max_dist / (double)scale[n_levels - 1]);
    return o;
}

#endif
