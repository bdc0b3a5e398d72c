/*
 * ss_pnp_steps.h -- the steps of the PnP RANSAC (the rule: include/sendslam_orb.h): the six draws of a
 * hypothesis, the linear six-point model in double (the 12 x 12 normal matrix of the tangent-plane residuals, its smallest
 * eigenvector by a fixed number of inverse iterations, sign, scale, the nearest rotation by Horn's quaternion), the refinement on
 * the six with the pose rule's own step, the record, one reprojection test, the selection predicate and the whole rule on the host.
 * The kernels (ss_pnp.hip), the host twins ss_pnp_host / ss_pnp_model_host / ss_pnp_check_host (ss_api_search.cpp) and
 * tests/native/pnp_steps_asan.cpp compile this text.
 *
 * Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a NaN fails it.  Compile
 * with -ffp-contract=off.  Division and square root are correctly rounded on both sides (hipcc's default).  The 12 x 12 matrix (its
 * lower triangle, packed by rows: entry (i, j), i >= j, at i (i + 1) / 2 + j) and the twelve unknowns behind it live in a work area W
 * that the caller brings: W::at(k), k < SS_PNP_WORK, is one double.  The host uses a plain array, the kernel a slice of LDS one lane
 * wide, so the factorisation and the substitutions keep their loops rolled with run-time indices and no register array is indexed
 * by a variable.  Everything else is indexed by constants once the loops are unrolled.
 */
#ifndef SS_PNP_STEPS_H
#define SS_PNP_STEPS_H

#include "ss_pose_steps.h"
#include "ss_sim3_steps.h" /* mix32 and the draws, Horn's rotation, transform and project */

#define SS_PNP_DRAWS 6
#define SS_PNP_UNKNOWNS 12
#define SS_PNP_TRI 78            /* the lower triangle of the 12 x 12 matrix */
#define SS_PNP_WORK (SS_PNP_TRI + SS_PNP_UNKNOWNS)
#define SS_PNP_INVERSE_STEPS 6   /* inverse iterations, fixed */
#define SS_PNP_SHIFT 1e-13       /* times the trace, added to the diagonal */

/* the work area of the host */
struct ss_pnp_work_host {
    double a[SS_PNP_WORK];
    double &at(int k) { return a[k]; }
};

/* the six draws of hypothesis t of problem q over 0 .. n-1 (n >= 6) */
SS_HD void ss_pnp_draw(uint32_t seed, uint32_t problem, int t, int n, int out[SS_PNP_DRAWS]) { ss_sim3_draw_k<SS_PNP_DRAWS>(seed, problem, t, n, out); }

/* what a problem's steps read of its view */
struct ss_pnp_cam {
    float fx, fy, cx, cy;
};

SS_HD ss_pnp_cam ss_pnp_cam_of(const ss_proj_view &v)
{
    ss_pnp_cam c;
    c.fx = v.fx, c.fy = v.fy, c.cx = v.cx, c.cy = v.cy;
    return c;
}

/* a hypothesis: the pose in double and rounded to float32 once; all 0 for the zero model */
struct ss_pnp_model {
    double rcw[9], tcw[3];
    float rf[9], tf[3];
};

/* the unit bearing of a keypoint: (xn, yn, 1) / sqrt((xn*xn + yn*yn) + 1) */
SS_HD void ss_pnp_bearing(float u, float v, const ss_pnp_cam &c, double b[3])
{
    const double xn = ((double)u - (double)c.cx) / (double)c.fx, yn = ((double)v - (double)c.cy) / (double)c.fy;
    const double n = sqrt((xn * xn + yn * yn) + 1.0);
    b[0] = xn / n, b[1] = yn / n, b[2] = 1.0 / n;
}

SS_HD int ss_pnp_tri(int i, int j) { return i * (i + 1) / 2 + j; }

/* Cholesky by columns over the packed lower triangle of order N, every inner sum subtracting in ascending k (ss_gn_chol_n's order).
 * False when a pivot is not > 0.  The two-view models (ss_two_view_steps.h) run it at order 9 */
template <int N, class W> SS_HD bool ss_tri_chol(W &w)
{
    bool ok = true;
    for (int j = 0; j < N; j++) {
        double s = w.at(ss_pnp_tri(j, j));
        for (int k = 0; k < j; k++) s = s - w.at(ss_pnp_tri(j, k)) * w.at(ss_pnp_tri(j, k));
        ok = ok && s > 0.0;
        const double d = sqrt(s);
        w.at(ss_pnp_tri(j, j)) = d;
        for (int i = j + 1; i < N; i++) {
            double v = w.at(ss_pnp_tri(i, j));
            for (int k = 0; k < j; k++) v = v - w.at(ss_pnp_tri(i, k)) * w.at(ss_pnp_tri(j, k));
            w.at(ss_pnp_tri(i, j)) = v / d;
        }
    }
    return ok;
}

/* one inverse iteration on the factor of order N, the vector behind the triangle: x <- L^-T L^-1 x (ss_gn_subst_n's order), then
 * x / sqrt(the sequential sum of squares) */
template <int N, class W> SS_HD void ss_tri_inverse_step(W &w)
{
    const int X = N * (N + 1) / 2;
    for (int i = 0; i < N; i++) {
        double v = w.at(X + i);
        for (int k = 0; k < i; k++) v = v - w.at(ss_pnp_tri(i, k)) * w.at(X + k);
        w.at(X + i) = v / w.at(ss_pnp_tri(i, i));
    }
    for (int i = N - 1; i >= 0; i--) {
        double v = w.at(X + i);
        for (int k = i + 1; k < N; k++) v = v - w.at(ss_pnp_tri(k, i)) * w.at(X + k);
        w.at(X + i) = v / w.at(ss_pnp_tri(i, i));
    }
    double s = w.at(X) * w.at(X);
    for (int k = 1; k < N; k++) s = s + w.at(X + k) * w.at(X + k);
    const double n = sqrt(s);
    for (int k = 0; k < N; k++) w.at(X + k) = w.at(X + k) / n;
}

template <class W> SS_HD bool ss_pnp_chol(W &w) { return ss_tri_chol<SS_PNP_UNKNOWNS>(w); }
template <class W> SS_HD void ss_pnp_inverse_step(W &w) { ss_tri_inverse_step<SS_PNP_UNKNOWNS>(w); }

/* Step 3b.  X[3i ..], uv[2i ..]: draw i.  The unknowns are the columns c1 c2 c3 of R^ and t^: unknown 3a + r is component r of
 * column a (a = 3: t^).  With d_i = (X_i - O, 1) and P_i = I - b_i b_i^T, entry (3a + r, 3b + c) of H is the sum over the draws, in
 * draw order from the first term, of (d_ia * d_ib) * P_i[r][c], P_i[r][c] = (r == c ? 1.0 : 0.0) - b_ir * b_ic.  False when the
 * Cholesky met a pivot that is not > 0 (the pose is then whatever the arithmetic gave) */
template <class W> SS_HD bool ss_pnp_linear(const float X[3 * SS_PNP_DRAWS], const float uv[2 * SS_PNP_DRAWS], const ss_pnp_cam &cam, W &w, double R[9], double t[3])
{
    double O[3];
    SS_GN_UNROLL
    for (int c = 0; c < 3; c++)
        O[c] = ((((((double)X[c] + (double)X[3 + c]) + (double)X[6 + c]) + (double)X[9 + c]) + (double)X[12 + c]) + (double)X[15 + c]) / 6.0;
    SS_GN_UNROLL
    for (int i = 0; i < SS_PNP_DRAWS; i++) {
        double d[4], b[3], P[3][3];
        SS_GN_UNROLL
        for (int c = 0; c < 3; c++) d[c] = (double)X[3 * i + c] - O[c];
        d[3] = 1.0;
        ss_pnp_bearing(uv[2 * i], uv[2 * i + 1], cam, b);
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) {
            SS_GN_UNROLL
            for (int c = 0; c < 3; c++) P[r][c] = (r == c ? 1.0 : 0.0) - b[r] * b[c];
        }
        SS_GN_UNROLL
        for (int a = 0; a < 4; a++) {
            SS_GN_UNROLL
            for (int e = 0; e <= a; e++) {
                const double dd = d[a] * d[e];
                SS_GN_UNROLL
                for (int r = 0; r < 3; r++) {
                    SS_GN_UNROLL
                    for (int c = 0; c < 3; c++) {
                        if (a == e && c > r) continue;
                        const int k = ss_pnp_tri(3 * a + r, 3 * e + c);
                        const double term = dd * P[r][c];
                        if (i == 0) w.at(k) = term;
                        else w.at(k) = w.at(k) + term;
                    }
                }
            }
        }
    }
    double trace = w.at(0);
    SS_GN_UNROLL
    for (int k = 1; k < SS_PNP_UNKNOWNS; k++) trace = trace + w.at(ss_pnp_tri(k, k));
    const double shift = SS_PNP_SHIFT * trace;
    SS_GN_UNROLL
    for (int k = 0; k < SS_PNP_UNKNOWNS; k++) w.at(ss_pnp_tri(k, k)) = w.at(ss_pnp_tri(k, k)) + shift;
    const bool ok = ss_pnp_chol(w);
    const double start = 1.0 / sqrt(12.0);
    SS_GN_UNROLL
    for (int k = 0; k < SS_PNP_UNKNOWNS; k++) w.at(SS_PNP_TRI + k) = start;
    for (int it = 0; it < SS_PNP_INVERSE_STEPS; it++) ss_pnp_inverse_step(w);
    double x[SS_PNP_UNKNOWNS];
    SS_GN_UNROLL
    for (int k = 0; k < SS_PNP_UNKNOWNS; k++) x[k] = w.at(SS_PNP_TRI + k);
    /* the sign: the points lie in front of the camera */
    double front = 0.0;
    SS_GN_UNROLL
    for (int i = 0; i < SS_PNP_DRAWS; i++) {
        double b[3];
        ss_pnp_bearing(uv[2 * i], uv[2 * i + 1], cam, b);
        const double d0 = (double)X[3 * i] - O[0], d1 = (double)X[3 * i + 1] - O[1], d2 = (double)X[3 * i + 2] - O[2];
        const double y0 = ((x[0] * d0 + x[3] * d1) + x[6] * d2) + x[9];
        const double y1 = ((x[1] * d0 + x[4] * d1) + x[7] * d2) + x[10];
        const double y2 = ((x[2] * d0 + x[5] * d1) + x[8] * d2) + x[11];
        const double dot = (b[0] * y0 + b[1] * y1) + b[2] * y2;
        front = i == 0 ? dot : front + dot;
    }
    if (front < 0.0) {
        SS_GN_UNROLL
        for (int k = 0; k < SS_PNP_UNKNOWNS; k++) x[k] = -x[k];
    }
    const double n0 = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const double n1 = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    const double n2 = sqrt((x[6] * x[6] + x[7] * x[7]) + x[8] * x[8]);
    const double s = 3.0 / ((n0 + n1) + n2);
    /* Horn with the columns of R^ as Pr1 and the unit vectors as Pr2: M[i][j] = R^[j][i], component j of column i */
    double m[3][3];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) m[i][j] = x[3 * i + j];
    }
    ss_sim3_horn(m, R);
    SS_GN_UNROLL
    for (int r = 0; r < 3; r++) t[r] = s * x[9 + r] - ((R[3 * r] * O[0] + R[3 * r + 1] * O[1]) + R[3 * r + 2] * O[2]);
    return ok;
}

/* Steps 3b - 3d of one sextuple: scale[i] the pyramid scale of draw i's keypoint, row[i] its point row */
template <class W>
SS_HD ss_pnp_model ss_pnp_model_of(const float X[3 * SS_PNP_DRAWS], const float uv[2 * SS_PNP_DRAWS], const float scale[SS_PNP_DRAWS],
                                   const int row[SS_PNP_DRAWS], const ss_pnp_cam &cam, double lambda, int refine_steps, W &w)
{
    double R[9], t[3];
    bool ok = ss_pnp_linear(X, uv, cam, w, R, t);
    SS_GN_UNROLL
    for (int i = 1; i < SS_PNP_DRAWS; i++) {
        SS_GN_UNROLL
        for (int e = 0; e < i; e++) ok = ok && row[i] != row[e];
    }
    ok = ok && ss_gn_all_finite(R, t);
    if (ok) {
        ss_pose_cam pc;
        pc.fx = (double)cam.fx, pc.fy = (double)cam.fy, pc.cx = (double)cam.cx, pc.cy = (double)cam.cy, pc.bf = 0.0;
        pc.chi2_mono = pc.chi2_stereo = pc.delta_mono = pc.delta_stereo = 0.0; /* no step here is robust */
#if defined(__HIPCC__) || defined(__clang__)
        _Pragma("unroll 1")
#endif
        for (int step = 0; step < refine_steps; step++) {
            double sum[SS_POSE_SUMS];
            SS_GN_UNROLL
            for (int k = 0; k < SS_POSE_SUMS; k++) sum[k] = 0.0;
            SS_GN_UNROLL
            for (int i = 0; i < SS_PNP_DRAWS; i++) {
                double term[SS_POSE_SUMS];
                const ss_pose_obs o = ss_pose_obs_of(X[3 * i], X[3 * i + 1], X[3 * i + 2], uv[2 * i], uv[2 * i + 1], -1.0f, scale[i]);
                if (ss_pose_terms(o, pc, R, t, false, term)) {
                    SS_GN_UNROLL
                    for (int k = 0; k < SS_POSE_SUMS; k++) sum[k] = sum[k] + term[k];
                }
            }
            double R0[9], t0[3];
            SS_GN_UNROLL
            for (int k = 0; k < 9; k++) R0[k] = R[k];
            SS_GN_UNROLL
            for (int k = 0; k < 3; k++) t0[k] = t[k];
            bool small;
            if (ss_pose_step(sum, lambda, 0.0, R, t, &small) != 0) break; /* refused: the pose is the one before the step */
            if (!ss_gn_all_finite(R, t)) {
                SS_GN_UNROLL
                for (int k = 0; k < 9; k++) R[k] = R0[k];
                SS_GN_UNROLL
                for (int k = 0; k < 3; k++) t[k] = t0[k];
                break;
            }
        }
    }
    ss_pnp_model m;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) {
        m.rcw[k] = R[k], m.rf[k] = (float)R[k];
        ok = ok && fabsf(m.rf[k]) <= 3.4028234663852886e38f;
    }
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) {
        m.tcw[k] = t[k], m.tf[k] = (float)t[k];
        ok = ok && fabsf(m.tf[k]) <= 3.4028234663852886e38f;
    }
    if (!ok) {
        SS_GN_UNROLL
        for (int k = 0; k < 9; k++) m.rcw[k] = 0.0, m.rf[k] = 0.0f;
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) m.tcw[k] = 0.0, m.tf[k] = 0.0f;
    }
    return m;
}

/* step 1 of one correspondence: its six floats; the octave inside the table: the caller has checked that */
struct ss_pnp_corr {
    float X[3], u, v, max;
};

SS_HD float ss_pnp_max(float chi2, float s) { return chi2 * (s * s); }

/* Step 3e of one correspondence under the float32 pose (r, t): 0 an inlier, 2 the depth is not > 0, 3 the error is not < max.
 * *err: the squared error, 0.0f where the depth fails */
SS_HD int ss_pnp_test(const float *r, const float *t, const ss_pnp_corr &c, const ss_pnp_cam &cam, float *err)
{
    float y[3], qu, qv;
    ss_sim3_transform(r, t, c.X[0], c.X[1], c.X[2], y);
    *err = 0.0f;
    if (!(y[2] > 0.0f)) return 2;
    ss_sim3_project(y, cam.fx, cam.fy, cam.cx, cam.cy, &qu, &qv);
    const float du = c.u - qu, dv = c.v - qv;
    *err = du * du + dv * dv;
    return *err < c.max ? 0 : 3;
}

SS_HD bool ss_pnp_inlier(const float *r, const float *t, const ss_pnp_corr &c, const ss_pnp_cam &cam)
{
    float e;
    return ss_pnp_test(r, t, c, cam, &e) == 0;
}

/* state 1 */
SS_HD bool ss_pnp_too_few(int n, int min_inliers) { return n < SS_PNP_DRAWS || n < min_inliers; }

/* The key of hypothesis t with this count: the largest key is the largest count and, among equals, the smallest t
 * (count <= SS_GUIDED_MAX_ROWS = 2^14 and t < SS_PNP_MAX_ITERATIONS = 2^10, so it fits an int) */
SS_HD int ss_pnp_key(int count, int t) { return count * SS_PNP_MAX_ITERATIONS + (SS_PNP_MAX_ITERATIONS - 1 - t); }
SS_HD int ss_pnp_key_count(int key) { return key / SS_PNP_MAX_ITERATIONS; }
SS_HD int ss_pnp_key_t(int key) { return SS_PNP_MAX_ITERATIONS - 1 - key % SS_PNP_MAX_ITERATIONS; }

/* the selection predicate on the best hypothesis' count */
SS_HD bool ss_pnp_wins(int count, int n, int min_inliers, float min_ratio) { return count >= min_inliers && (float)count >= min_ratio * (float)n; }

/* hypothesis t of a problem from its numbered correspondences (n >= 6): scale[k] and point[k] go with corr[k] */
static inline ss_pnp_model ss_pnp_hypothesis_host(const ss_pnp_corr *corr, const float *scale, const int32_t *point, int n, const ss_pnp_cam &cam,
                                                  const ss_pnp_params &p, uint32_t problem, int t)
{
    int pick[SS_PNP_DRAWS], row[SS_PNP_DRAWS];
    float X[3 * SS_PNP_DRAWS], uv[2 * SS_PNP_DRAWS], sc[SS_PNP_DRAWS];
    ss_pnp_draw(p.seed, problem, t, n, pick);
    for (int k = 0; k < SS_PNP_DRAWS; k++) {
        const ss_pnp_corr &c = corr[pick[k]];
        X[3 * k] = c.X[0], X[3 * k + 1] = c.X[1], X[3 * k + 2] = c.X[2];
        uv[2 * k] = c.u, uv[2 * k + 1] = c.v;
        sc[k] = scale[pick[k]], row[k] = point[pick[k]];
    }
    ss_pnp_work_host w;
    return ss_pnp_model_of(X, uv, sc, row, cam, p.lambda, p.refine_steps, w);
}

/* The whole problem on the host the way the kernels run it: every hypothesis, its count, the selection, the winner once more.
 * in: n bytes, 1 = inlier of the winner.  Every field of *out is written; its status is 0 */
static inline void ss_pnp_problem_host(const ss_pnp_corr *corr, const float *scale, const int32_t *point, int n, const ss_pnp_cam &cam,
                                       const ss_pnp_params &p, uint32_t problem, uint8_t *in, ss_pnp_result *out)
{
    for (int k = 0; k < 9; k++) out->rcw[k] = 0.0;
    for (int k = 0; k < 3; k++) out->tcw[k] = 0.0;
    out->state = 1, out->status = 0, out->n_corr = n, out->n_inliers = 0, out->best_inliers = 0, out->iteration = -1;
    out->reserved[0] = out->reserved[1] = 0;
    for (int k = 0; k < n; k++) in[k] = 0;
    if (ss_pnp_too_few(n, p.min_inliers)) return;
    int key = -1;
    for (int t = 0; t < p.max_iterations; t++) {
        const ss_pnp_model m = ss_pnp_hypothesis_host(corr, scale, point, n, cam, p, problem, t);
        int count = 0;
        for (int k = 0; k < n; k++) count += ss_pnp_inlier(m.rf, m.tf, corr[k], cam) ? 1 : 0;
        const int kt = ss_pnp_key(count, t);
        if (kt > key) key = kt;
    }
    out->best_inliers = ss_pnp_key_count(key);
    out->state = 2;
    if (!ss_pnp_wins(out->best_inliers, n, p.min_inliers, p.min_ratio)) return;
    const int t = ss_pnp_key_t(key);
    const ss_pnp_model m = ss_pnp_hypothesis_host(corr, scale, point, n, cam, p, problem, t);
    for (int k = 0; k < 9; k++) out->rcw[k] = m.rcw[k];
    for (int k = 0; k < 3; k++) out->tcw[k] = m.tcw[k];
    int count = 0;
    for (int k = 0; k < n; k++) count += in[k] = ss_pnp_inlier(m.rf, m.tf, corr[k], cam) ? 1 : 0;
    out->state = 0, out->n_inliers = count, out->iteration = t;
}

#endif
