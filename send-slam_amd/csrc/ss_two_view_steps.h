/*
 * ss_two_view_steps.h -- the steps of the two-view initialisation (the rule: include/sendslam_orb.h): the
 * normalisation, the eight draws of a hypothesis, the homography and the fundamental matrix of an octuple in double (the 9 x 9
 * normal matrix, its smallest eigenvector by a fixed number of inverse iterations, the rank-2 projection, the denormalisation), one
 * correspondence's score terms under either model, the model choice, the 3 x 3 singular value decomposition, the four or eight
 * motion hypotheses, CheckRT for one correspondence, the map point, the order statistic of the cosines, the acceptance and the whole
 * rule on the host.  The kernels (ss_two_view.hip), the host twins ss_two_view_host / ss_two_view_model_host / ss_two_view_check_host
 * (ss_api_search.cpp) and tests/native/two_view_steps_asan.cpp compile this text.
 *
 * All arithmetic is double on float32 inputs widened.  Every step is one IEEE operation, left to right as written; every test is in
 * its accepting form, so a NaN fails it.  Compile with -ffp-contract=off.  Division and square root are correctly rounded on both
 * sides (hipcc's default); there is no other library function.  The 9 x 9 matrix (its lower triangle packed by rows, ss_pnp_tri) and
 * the nine unknowns behind it live in a work area W that the caller brings, as in ss_pnp_steps.h; the normalised coordinates of the
 * eight draws follow them there, so the loop over the draws stays rolled.
 */
#ifndef SS_TWO_VIEW_STEPS_H
#define SS_TWO_VIEW_STEPS_H

#include <string.h>

#include "ss_epi_steps.h" /* ss_tri_null4 */
#include "ss_gn_steps.h"  /* the tree of a sum */
#include "ss_pnp_steps.h" /* ss_tri_chol, ss_tri_inverse_step */
#include "ss_sim3_steps.h" /* the draws */

#define SS_TV_DRAWS 8
#define SS_TV_ORDER 9
#define SS_TV_TRI 45 /* the lower triangle of the 9 x 9 matrix */
#define SS_TV_PTS (SS_TV_TRI + SS_TV_ORDER) /* the 32 normalised coordinates of the draws, behind the unknowns */
#define SS_TV_WORK (SS_TV_PTS + 4 * SS_TV_DRAWS)
#define SS_TV_INVERSE_STEPS 6 /* inverse iterations, fixed */
#define SS_TV_SHIFT 1e-13     /* times the trace, added to the diagonal */
#define SS_TV_SWEEPS 8        /* sweeps of cyclic Jacobi on a 3 x 3 */
#define SS_TV_CHUNK SS_GN_SLOTS /* the correspondences of one tree */
#define SS_TV_MAX_HYP 8
#define SS_TV_COS_TRI 0.99998 /* a point with a cosine not below this is good, but not triangulated */
#define SS_TV_TH2 4.0         /* 4 sigma^2, sigma = 1 */
#define SS_TV_MIN_DET 1e-300

/* the work area of the host */
struct ss_tv_work_host {
    double a[SS_TV_WORK];
    double &at(int k) { return a[k]; }
};

SS_HD void ss_tv_draw(uint32_t seed, uint32_t problem, int t, int n, int out[SS_TV_DRAWS]) { ss_sim3_draw_k<SS_TV_DRAWS>(seed, problem, t, n, out); }

/* step 2 of a problem: the mean m and the mean absolute deviation d of u1 v1 u2 v2 */
struct ss_tv_norm {
    double m[4], d[4];
};

/* a deviation that is not > 0 or not finite voids the problem */
SS_HD bool ss_tv_norm_ok(const ss_tv_norm &n)
{
    bool ok = true;
    SS_GN_UNROLL
    for (int k = 0; k < 4; k++) ok = ok && n.d[k] > 0.0 && ss_gn_is_finite(n.d[k]) && ss_gn_is_finite(n.m[k]);
    return ok;
}

/* what the steps read of a problem's camera */
struct ss_tv_cam {
    double fx, fy, cx, cy;
};
SS_HD ss_tv_cam ss_tv_cam_of(const ss_proj_view &v)
{
    ss_tv_cam c;
    c.fx = (double)v.fx, c.fy = (double)v.fy, c.cx = (double)v.cx, c.cy = (double)v.cy;
    return c;
}

/* a hypothesis: the three matrices in pixel coordinates; a zero model has ok 0 and all 0.0 */
struct ss_tv_model {
    double h21[9], h12[9], f21[9];
    int ok_h, ok_f;
};

/* c = a.b, each entry (a0*b0 + a1*b1) + a2*b2 */
SS_HD void ss_tv_mul3(const double *a, const double *b, double *c)
{
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
    }
}

SS_HD void ss_tv_t3(const double *a, double *c)
{
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * j + i];
    }
}

SS_HD double ss_tv_det3(const double *m)
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

/* the inverse by the adjugate; false when |det| is not > SS_TV_MIN_DET */
SS_HD bool ss_tv_inv3(const double *m, double *o)
{
    const double d = ss_tv_det3(m);
    const double id = 1.0 / d;
    o[0] = (m[4] * m[8] - m[5] * m[7]) * id, o[1] = (m[2] * m[7] - m[1] * m[8]) * id, o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = (m[5] * m[6] - m[3] * m[8]) * id, o[4] = (m[0] * m[8] - m[2] * m[6]) * id, o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = (m[3] * m[7] - m[4] * m[6]) * id, o[7] = (m[1] * m[6] - m[0] * m[7]) * id, o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    return fabs(d) > SS_TV_MIN_DET;
}

SS_HD bool ss_tv_finite9(const double *m)
{
    bool ok = true;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) ok = ok && ss_gn_is_finite(m[k]);
    return ok;
}

/* one Jacobi rotation on the symmetric 3 x 3 M (both triangles kept) and the vectors V: ss_tri_rotate's text at order 3 */
template <int P, int Q> SS_HD void ss_tv_rotate3(double (&M)[3][3], double (&V)[3][3])
{
    const double apq = M[P][Q];
    if (apq != 0.0) {
        const double theta = (M[Q][Q] - M[P][P]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        const int K = 3 - P - Q;
        const double akp = M[K][P], akq = M[K][Q];
        const double np = c * akp - s * akq, nq = s * akp + c * akq;
        M[K][P] = M[P][K] = np;
        M[K][Q] = M[Q][K] = nq;
        M[P][P] = M[P][P] - t * apq;
        M[Q][Q] = M[Q][Q] + t * apq;
        M[P][Q] = M[Q][P] = 0.0;
        SS_GN_UNROLL
        for (int k = 0; k < 3; k++) {
            const double vkp = V[k][P], vkq = V[k][Q];
            V[k][P] = c * vkp - s * vkq;
            V[k][Q] = s * vkp + c * vkq;
        }
    }
}

/* the eigenvalues (e, the diagonal after SS_TV_SWEEPS sweeps) and eigenvectors (the columns of V) of G = A^T A, A row-major 3 x 3;
 * G[i][j] = (A0i*A0j + A1i*A1j) + A2i*A2j, upper triangle mirrored */
SS_HD void ss_tv_eig_ata(const double *A, double e[3], double (&V)[3][3])
{
    double M[3][3];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) {
            if (j >= i) M[i][j] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    M[1][0] = M[0][1], M[2][0] = M[0][2], M[2][1] = M[1][2];
    SS_EPI_ROLLED
    for (int sweep = 0; sweep < SS_TV_SWEEPS; sweep++) {
        ss_tv_rotate3<0, 1>(M, V);
        ss_tv_rotate3<0, 2>(M, V);
        ss_tv_rotate3<1, 2>(M, V);
    }
    e[0] = M[0][0], e[1] = M[1][1], e[2] = M[2][2];
}

/* column k of V, k known at run time, without an indexed register array */
SS_HD void ss_tv_col(const double (&V)[3][3], int k, double v[3])
{
    SS_GN_UNROLL
    for (int r = 0; r < 3; r++) {
        const double a = V[r][0], b = V[r][1], c = V[r][2]; /* read first: a choice between loads becomes an indexed load */
        v[r] = k == 0 ? a : k == 1 ? b : c;
    }
}

/* Step 3, the null vector: the matrix is in the triangle of w.  trace in ascending order, the shift, the factor, the constant start
 * 1.0 / 3.0 and SS_TV_INVERSE_STEPS inverse iterations.  False when a pivot is not > 0 */
template <class W> SS_HD bool ss_tv_null9(W &w, double x[SS_TV_ORDER])
{
    double trace = w.at(0);
    SS_GN_UNROLL
    for (int k = 1; k < SS_TV_ORDER; k++) trace = trace + w.at(ss_pnp_tri(k, k));
    const double shift = SS_TV_SHIFT * trace;
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_ORDER; k++) w.at(ss_pnp_tri(k, k)) = w.at(ss_pnp_tri(k, k)) + shift;
    const bool ok = ss_tri_chol<SS_TV_ORDER>(w);
    const double start = 1.0 / 3.0;
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_ORDER; k++) w.at(SS_TV_TRI + k) = start;
    for (int it = 0; it < SS_TV_INVERSE_STEPS; it++) ss_tri_inverse_step<SS_TV_ORDER>(w);
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_ORDER; k++) x[k] = w.at(SS_TV_TRI + k);
    return ok;
}

/* Step 3 of one octuple: uv[4k ..] = u1 v1 u2 v2 of draw k, pick[k] its correspondence (two equal ones void both models) */
/* m: any record with h21, h12, f21, ok_h and ok_f (the kernel's lives in global memory: H is stored before F is begun) */
template <class W, class M> SS_HD void ss_tv_model_of(const float uv[4 * SS_TV_DRAWS], const int pick[SS_TV_DRAWS], const ss_tv_norm &nm, W &w, M &m)
{
    double s[4];
    SS_GN_UNROLL
    for (int c = 0; c < 4; c++) s[c] = 1.0 / nm.d[c];
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_DRAWS; k++) {
        SS_GN_UNROLL
        for (int c = 0; c < 4; c++) w.at(SS_TV_PTS + 4 * k + c) = ((double)uv[4 * k + c] - nm.m[c]) * s[c];
    }
    const double T1[9] = {s[0], 0.0, -nm.m[0] * s[0], 0.0, s[1], -nm.m[1] * s[1], 0.0, 0.0, 1.0};
    const double T2[9] = {s[2], 0.0, -nm.m[2] * s[2], 0.0, s[3], -nm.m[3] * s[3], 0.0, 0.0, 1.0};
    const double T2inv[9] = {nm.d[2], 0.0, nm.m[2], 0.0, nm.d[3], nm.m[3], 0.0, 0.0, 1.0};
    bool distinct = true;
    SS_GN_UNROLL
    for (int i = 1; i < SS_TV_DRAWS; i++) {
        SS_GN_UNROLL
        for (int e = 0; e < i; e++) distinct = distinct && pick[i] != pick[e];
    }
    double x[SS_TV_ORDER], tmp[9];
    /* H: the two rows of a draw, entry (i, j) of the normal matrix the sum over the draws of ra_i*ra_j + rb_i*rb_j */
    SS_EPI_ROLLED
    for (int k = 0; k < SS_TV_DRAWS; k++) {
        const double u1 = w.at(SS_TV_PTS + 4 * k), v1 = w.at(SS_TV_PTS + 4 * k + 1), u2 = w.at(SS_TV_PTS + 4 * k + 2), v2 = w.at(SS_TV_PTS + 4 * k + 3);
        const double ra[9] = {0.0, 0.0, 0.0, -u1, -v1, -1.0, v2 * u1, v2 * v1, v2};
        const double rb[9] = {u1, v1, 1.0, 0.0, 0.0, 0.0, -(u2 * u1), -(u2 * v1), -u2};
        SS_GN_UNROLL
        for (int i = 0; i < SS_TV_ORDER; i++) {
            SS_GN_UNROLL
            for (int j = 0; j <= i; j++) {
                const double term = ra[i] * ra[j] + rb[i] * rb[j];
                if (k == 0) w.at(ss_pnp_tri(i, j)) = term;
                else w.at(ss_pnp_tri(i, j)) = w.at(ss_pnp_tri(i, j)) + term;
            }
        }
    }
    bool ok = ss_tv_null9(w, x);
    {
        double h21[9], h12[9];
        ss_tv_mul3(T2inv, x, tmp);
        ss_tv_mul3(tmp, T1, h21);
        ok = ss_tv_inv3(h21, h12) && ok;
        ok = ok && distinct && ss_tv_finite9(h21) && ss_tv_finite9(h12);
        m.ok_h = ok ? 1 : 0;
        SS_GN_UNROLL
        for (int k = 0; k < 9; k++) m.h21[k] = ok ? h21[k] : 0.0, m.h12[k] = ok ? h12[k] : 0.0;
    }
    /* F: one row per draw */
    SS_EPI_ROLLED
    for (int k = 0; k < SS_TV_DRAWS; k++) {
        const double u1 = w.at(SS_TV_PTS + 4 * k), v1 = w.at(SS_TV_PTS + 4 * k + 1), u2 = w.at(SS_TV_PTS + 4 * k + 2), v2 = w.at(SS_TV_PTS + 4 * k + 3);
        const double r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
        SS_GN_UNROLL
        for (int i = 0; i < SS_TV_ORDER; i++) {
            SS_GN_UNROLL
            for (int j = 0; j <= i; j++) {
                const double term = r[i] * r[j];
                if (k == 0) w.at(ss_pnp_tri(i, j)) = term;
                else w.at(ss_pnp_tri(i, j)) = w.at(ss_pnp_tri(i, j)) + term;
            }
        }
    }
    ok = ss_tv_null9(w, x);
    {
        /* rank 2: v the eigenvector of F^T F at its smallest eigenvalue (the first among equals), F <- F - (F.v).v^T */
        double e[3], V[3][3], v[3];
        ss_tv_eig_ata(x, e, V);
        int best = 0;
        double low = e[0];
        if (e[1] < low) best = 1, low = e[1];
        if (e[2] < low) best = 2, low = e[2];
        ss_tv_col(V, best, v);
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) {
            const double fv = (x[3 * r] * v[0] + x[3 * r + 1] * v[1]) + x[3 * r + 2] * v[2];
            SS_GN_UNROLL
            for (int c = 0; c < 3; c++) x[3 * r + c] = x[3 * r + c] - fv * v[c];
        }
    }
    double T2t[9], f21[9];
    ss_tv_t3(T2, T2t);
    ss_tv_mul3(T2t, x, tmp);
    ss_tv_mul3(tmp, T1, f21);
    ok = ok && distinct && ss_tv_finite9(f21);
    m.ok_f = ok ? 1 : 0;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) m.f21[k] = ok ? f21[k] : 0.0;
}

/* Step 4 of one correspondence under a homography: its two terms added, *in its flag, chi[2] the two errors */
SS_HD double ss_tv_term_h(const double *H21, const double *H12, double u1, double v1, double u2, double v2, double th, bool *in, double chi[2])
{
    const double w21 = 1.0 / ((H12[6] * u2 + H12[7] * v2) + H12[8]);
    const double a = ((H12[0] * u2 + H12[1] * v2) + H12[2]) * w21, b = ((H12[3] * u2 + H12[4] * v2) + H12[5]) * w21;
    chi[0] = (u1 - a) * (u1 - a) + (v1 - b) * (v1 - b);
    const double w12 = 1.0 / ((H21[6] * u1 + H21[7] * v1) + H21[8]);
    const double c = ((H21[0] * u1 + H21[1] * v1) + H21[2]) * w12, d = ((H21[3] * u1 + H21[4] * v1) + H21[5]) * w12;
    chi[1] = (u2 - c) * (u2 - c) + (v2 - d) * (v2 - d);
    const bool in0 = chi[0] <= th, in1 = chi[1] <= th;
    *in = in0 && in1;
    return (in0 ? th - chi[0] : 0.0) + (in1 ? th - chi[1] : 0.0);
}

/* the same under a fundamental matrix: the inlier threshold th, the score's th_score */
SS_HD double ss_tv_term_f(const double *F, double u1, double v1, double u2, double v2, double th, double th_score, bool *in, double chi[2])
{
    const double a2 = (F[0] * u1 + F[1] * v1) + F[2], b2 = (F[3] * u1 + F[4] * v1) + F[5], c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double num2 = (a2 * u2 + b2 * v2) + c2;
    chi[0] = (num2 * num2) / (a2 * a2 + b2 * b2);
    const double a1 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7], c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const double num1 = (a1 * u1 + b1 * v1) + c1;
    chi[1] = (num1 * num1) / (a1 * a1 + b1 * b1);
    const bool in0 = chi[0] <= th, in1 = chi[1] <= th;
    *in = in0 && in1;
    return (in0 ? th_score - chi[0] : 0.0) + (in1 ? th_score - chi[1] : 0.0);
}

/* state 1 */
SS_HD bool ss_tv_too_few(int n) { return n < SS_TV_DRAWS; }

/* Step 5: does hypothesis t with this score beat the best so far (the largest score, the smallest t among equals)? */
SS_HD bool ss_tv_beats(double score, int t, double best, int best_t) { return score > best || (score == best && t < best_t); }

/* Step 6: 2 the homography, 1 the fundamental matrix, 0 neither score is > 0 */
SS_HD int ss_tv_choose(double sh, double sf, double rh_threshold)
{
    if (!(sh > 0.0) && !(sf > 0.0)) return 0;
    const double h = sh > 0.0 ? sh : 0.0, f = sf > 0.0 ? sf : 0.0;
    const double rh = h / (h + f);
    return rh > rh_threshold ? 2 : 1;
}

/* Step 7's decomposition A = U diag(s) V^T, row-major: the eigenvalues of A^T A sorted descending (among equals the smaller index
 * first), s = sqrt of each (0.0 when it is not > 0); columns 0 and 1 of U are A.v over its length, column 2 their cross product,
 * negated when its product with A.v2 is < 0 */
SS_HD void ss_tv_svd3(const double *A, double *U, double s[3], double *V)
{
    double e[3], Ve[3][3];
    ss_tv_eig_ata(A, e, Ve);
    double e0 = e[0], e1 = e[1], e2 = e[2];
    int i0 = 0, i1 = 1, i2 = 2;
    if (e1 > e0) { const double x = e0; e0 = e1, e1 = x; const int i = i0; i0 = i1, i1 = i; }
    if (e2 > e1) { const double x = e1; e1 = e2, e2 = x; const int i = i1; i1 = i2, i2 = i; }
    if (e1 > e0) { const double x = e0; e0 = e1, e1 = x; const int i = i0; i0 = i1, i1 = i; }
    s[0] = sqrt(e0 > 0.0 ? e0 : 0.0), s[1] = sqrt(e1 > 0.0 ? e1 : 0.0), s[2] = sqrt(e2 > 0.0 ? e2 : 0.0);
    double v[3][3], u[3][3];
    ss_tv_col(Ve, i0, v[0]);
    ss_tv_col(Ve, i1, v[1]);
    ss_tv_col(Ve, i2, v[2]);
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) {
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) {
            V[3 * r + k] = v[k][r];
            u[k][r] = (A[3 * r] * v[k][0] + A[3 * r + 1] * v[k][1]) + A[3 * r + 2] * v[k][2];
        }
    }
    SS_GN_UNROLL
    for (int k = 0; k < 2; k++) {
        const double n = sqrt((u[k][0] * u[k][0] + u[k][1] * u[k][1]) + u[k][2] * u[k][2]);
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) U[3 * r + k] = u[k][r] / n;
    }
    double c0 = U[3] * U[7] - U[6] * U[4], c1 = U[6] * U[1] - U[0] * U[7], c2 = U[0] * U[4] - U[3] * U[1];
    if ((c0 * u[2][0] + c1 * u[2][1]) + c2 * u[2][2] < 0.0) c0 = -c0, c1 = -c1, c2 = -c2;
    U[2] = c0, U[5] = c1, U[8] = c2;
}

/* Step 7, F: E = K^T.F.K, the four hypotheses (R1, t) (R2, t) (R1, -t) (R2, -t), each R then t as twelve doubles of hyp.  4 */
SS_HD int ss_tv_decompose_f(const double *F, const ss_tv_cam &c, double *hyp)
{
    const double K[9] = {c.fx, 0.0, c.cx, 0.0, c.fy, c.cy, 0.0, 0.0, 1.0};
    double Kt[9], tmp[9], E[9], U[9], s[3], V[9], Vt[9], R1[9], R2[9];
    ss_tv_t3(K, Kt);
    ss_tv_mul3(Kt, F, tmp);
    ss_tv_mul3(tmp, K, E);
    ss_tv_svd3(E, U, s, V);
    ss_tv_t3(V, Vt);
    const double tn = sqrt((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8]);
    const double t[3] = {U[2] / tn, U[5] / tn, U[8] / tn};
    const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    ss_tv_mul3(U, W, tmp);
    ss_tv_mul3(tmp, Vt, R1);
    ss_tv_mul3(U, Wt, tmp);
    ss_tv_mul3(tmp, Vt, R2);
    const bool n1 = ss_tv_det3(R1) < 0.0, n2 = ss_tv_det3(R2) < 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) {
        const double a = n1 ? -R1[k] : R1[k], b = n2 ? -R2[k] : R2[k];
        hyp[k] = a, hyp[12 + k] = b, hyp[24 + k] = a, hyp[36 + k] = b;
    }
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) hyp[9 + k] = t[k], hyp[21 + k] = t[k], hyp[33 + k] = -t[k], hyp[45 + k] = -t[k];
    return 4;
}

/* Step 7, H: Faugeras and Lustman's eight from A = K^-1.H.K.  8, or 0 when d1/d2 or d2/d3 is not >= 1.00001 */
SS_HD int ss_tv_decompose_h(const double *H, const ss_tv_cam &c, double *hyp)
{
    const double K[9] = {c.fx, 0.0, c.cx, 0.0, c.fy, c.cy, 0.0, 0.0, 1.0};
    const double ifx = 1.0 / c.fx, ify = 1.0 / c.fy;
    const double Kinv[9] = {ifx, 0.0, -c.cx * ifx, 0.0, ify, -c.cy * ify, 0.0, 0.0, 1.0};
    double tmp[9], A[9], U[9], w[3], V[9], Vt[9];
    ss_tv_mul3(Kinv, H, tmp);
    ss_tv_mul3(tmp, K, A);
    ss_tv_svd3(A, U, w, V);
    ss_tv_t3(V, Vt);
    const double sgn = ss_tv_det3(U) * ss_tv_det3(Vt);
    const double d1 = w[0], d2 = w[1], d3 = w[2];
    if (!(d1 / d2 >= 1.00001 && d2 / d3 >= 1.00001)) return 0;
    const double q12 = d1 * d1 - d2 * d2, q23 = d2 * d2 - d3 * d3, q13 = d1 * d1 - d3 * d3;
    const double aux1 = sqrt(q12 / q13), aux3 = sqrt(q23 / q13);
    const double root = sqrt(q12 * q23);
    const double aux_st = root / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const double aux_sp = root / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    SS_GN_UNROLL
    for (int i = 0; i < 8; i++) {
        const int j = i & 3;
        const bool pos = i < 4; /* d' = +d2, then d' = -d2 */
        const double x1 = (j < 2) ? aux1 : -aux1, x3 = (j & 1) ? -aux3 : aux3;
        const double st = (j == 0 || j == 3) ? aux_st : -aux_st, sp = (j == 0 || j == 3) ? aux_sp : -aux_sp;
        const double Rp[9] = {pos ? ct : cp, 0.0, pos ? -st : sp, 0.0, pos ? 1.0 : -1.0, 0.0, pos ? st : sp, 0.0, pos ? ct : -cp};
        double R[9];
        ss_tv_mul3(U, Rp, tmp);
        ss_tv_mul3(tmp, Vt, R);
        SS_GN_UNROLL
        for (int k = 0; k < 9; k++) hyp[12 * i + k] = sgn * R[k];
        const double scale = pos ? d1 - d3 : d1 + d3;
        const double tp0 = x1 * scale, tp2 = (pos ? -x3 : x3) * scale;
        double tt[3];
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) tt[r] = (U[3 * r] * tp0 + U[3 * r + 1] * 0.0) + U[3 * r + 2] * tp2;
        const double n = sqrt((tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2]);
        SS_GN_UNROLL
        for (int r = 0; r < 3; r++) hyp[12 * i + 9 + r] = tt[r] / n;
    }
    return 8;
}

/* the centre of camera 2 in frame 1: -R^T t, each component ((r0*t0 + r3*t1) + r6*t2) negated */
SS_HD void ss_tv_centre(const double *R, const double *t, double O[3])
{
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) O[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
}

/* the three tests of step 8 on a number: a squared reprojection error within 4 sigma^2; a cosine that exempts the point from the
 * depth tests; a cosine that counts as triangulated.  A NaN fails each */
SS_HD bool ss_tv_reprojects(double e) { return e <= SS_TV_TH2; }
SS_HD bool ss_tv_exempt(double cosp) { return cosp >= SS_TV_COS_TRI; }
SS_HD bool ss_tv_triangulated(double cosp) { return cosp < SS_TV_COS_TRI; }

/* Step 8 of one correspondence under (R, t): true when the point is good; X its position in frame 1, *cosp its parallax cosine,
 * n2 = X - O2 and d1, d2 the two distances (the map point reads them) */
struct ss_tv_point {
    double X[3], n2[3], d1, d2, cosp;
};
SS_HD bool ss_tv_check_rt(const double *R, const double *t, const ss_tv_cam &c, double u1, double v1, double u2, double v2, ss_tv_point *o)
{
    const double a1 = (u1 - c.cx) / c.fx, b1 = (v1 - c.cy) / c.fy, a2 = (u2 - c.cx) / c.fx, b2 = (v2 - c.cy) / c.fy;
    double A[4][4], v[4], O2[3];
    A[0][0] = -1.0, A[0][1] = 0.0, A[0][2] = a1, A[0][3] = 0.0;
    A[1][0] = 0.0, A[1][1] = -1.0, A[1][2] = b1, A[1][3] = 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < 4; k++) {
        const double p0 = k < 3 ? R[k] : t[0], p1 = k < 3 ? R[3 + k] : t[1], p2 = k < 3 ? R[6 + k] : t[2];
        A[2][k] = a2 * p2 - p0;
        A[3][k] = b2 * p2 - p1;
    }
    ss_tri_null4(A, v);
    o->cosp = 0.0, o->d1 = o->d2 = 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) o->X[k] = 0.0, o->n2[k] = 0.0;
    if (!(fabs(v[3]) <= 1.7976931348623157e308 && v[3] != 0.0)) return false;
    const double X0 = v[0] / v[3], X1 = v[1] / v[3], X2 = v[2] / v[3];
    if (!(ss_gn_is_finite(X0) && ss_gn_is_finite(X1) && ss_gn_is_finite(X2))) return false;
    ss_tv_centre(R, t, O2);
    const double n0 = X0 - O2[0], n1 = X1 - O2[1], n2 = X2 - O2[2];
    const double d1 = sqrt((X0 * X0 + X1 * X1) + X2 * X2), d2 = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    const double cosp = ((X0 * n0 + X1 * n1) + X2 * n2) / (d1 * d2);
    if (!ss_gn_is_finite(cosp)) return false;
    o->X[0] = X0, o->X[1] = X1, o->X[2] = X2, o->n2[0] = n0, o->n2[1] = n1, o->n2[2] = n2, o->d1 = d1, o->d2 = d2, o->cosp = cosp;
    if (!(X2 > 0.0 || ss_tv_exempt(cosp))) return false;
    const double Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0], Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    if (!(Y2 > 0.0 || ss_tv_exempt(cosp))) return false;
    const double e1x = ((c.fx * X0) / X2 + c.cx) - u1, e1y = ((c.fy * X1) / X2 + c.cy) - v1;
    if (!ss_tv_reprojects(e1x * e1x + e1y * e1y)) return false;
    const double e2x = ((c.fx * Y0) / Y2 + c.cx) - u2, e2y = ((c.fy * Y1) / Y2 + c.cy) - v2;
    if (!ss_tv_reprojects(e2x * e2x + e2y * e2y)) return false;
    return true;
}

/* the map point of a triangulated correspondence, frame 1 the world: section 18's UpdateNormalAndDepth text with O1 = 0; s1 the
 * scale of keypoint 1's octave, s_last the scale of the last level */
SS_HD ss_map_point ss_tv_map_point(const ss_tv_point &p, float s1, float s_last)
{
    ss_map_point m;
    const double max_dist = p.d1 * (double)s1;
    m.x = (float)p.X[0], m.y = (float)p.X[1], m.z = (float)p.X[2];
    m.nx = (float)((p.X[0] / p.d1 + p.n2[0] / p.d2) / 2.0);
    m.ny = (float)((p.X[1] / p.d1 + p.n2[1] / p.d2) / 2.0);
    m.nz = (float)((p.X[2] / p.d1 + p.n2[2] / p.d2) / 2.0);
    m.max_dist = (float)max_dist;
    m.min_dist = (float)(max_dist / (double)s_last);
    return m;
}

/* the key of a cosine: unsigned keys order as the doubles do (-0.0 below +0.0) */
SS_HD uint64_t ss_tv_key(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SS_HD double ss_tv_unkey(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double x;
    memcpy(&x, &b, sizeof(x));
    return x;
}
/* the index of step 8's order statistic among n_good ascending cosines, n_good >= 1 */
SS_HD int ss_tv_parallax_index(int n_good) { return n_good - 1 < 50 ? n_good - 1 : 50; }

/* Step 8's choice over the counts: the first hypothesis with the largest count, and the second largest count as upstream's loop
 * leaves it */
SS_HD void ss_tv_pick(const int *good, int n_hyp, int *best, int *best_good, int *second_good)
{
    *best = -1, *best_good = 0, *second_good = 0;
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_MAX_HYP; k++) {
        if (k >= n_hyp) continue;
        const int g = good[k];
        if (g > *best_good) *second_good = *best_good, *best_good = g, *best = k;
        else if (g > *second_good) *second_good = g;
    }
}

/* Step 9: 0 accepted, else the reason (2 too few good points, 3 ambiguous, 4 low parallax).  cosp is read only when best_good > 0 */
SS_HD int ss_tv_accept(int model, const int *good, int n_hyp, int best_good, int second_good, int n_in, double cosp, const ss_two_view_params &p)
{
    if (best_good < 1) return 2;
    if (model == 2) {
        if (!(best_good > p.min_triangulated && (double)best_good > 0.9 * (double)n_in)) return 2;
        if (!((double)second_good < 0.75 * (double)best_good)) return 3;
        if (!(cosp <= p.cos_min_parallax)) return 4;
        return 0;
    }
    int floor_n = (int)(0.9 * (double)n_in);
    if (p.min_triangulated > floor_n) floor_n = p.min_triangulated;
    if (!(best_good >= floor_n)) return 2;
    int similar = 0;
    SS_GN_UNROLL
    for (int k = 0; k < SS_TV_MAX_HYP; k++) {
        if (k < n_hyp && (double)good[k] > 0.7 * (double)best_good) similar++;
    }
    if (!(similar <= 1)) return 3;
    if (!(cosp < p.cos_min_parallax)) return 4;
    return 0;
}

SS_HD void ss_tv_result_clear(ss_two_view_result *r, int n_corr, int status)
{
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) r->r21[k] = 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) r->t21[k] = 0.0;
    r->score_h = r->score_f = r->cos_parallax = 0.0;
    r->state = 1, r->reason = 0, r->status = status, r->model = 0, r->iteration_h = r->iteration_f = -1;
    r->n_corr = n_corr, r->n_inliers = r->n_good = r->n_triangulated = 0;
    SS_GN_UNROLL
    for (int k = 0; k < 8; k++) r->reserved[k] = 0;
}

/* ---- the host's forms ---- */

/* the sum of term(0) .. term(n-1) in the rule's tree: chunks of SS_TV_CHUNK terms (absent ones +0.0), ss_gn_tree within a chunk,
 * the chunks added in ascending order from the first */
template <class F> static inline double ss_tv_tree_sum(int n, F term)
{
    double total = 0.0;
    for (int c0 = 0; c0 < n || c0 == 0; c0 += SS_TV_CHUNK) {
        double a[SS_GN_SLOTS];
        for (int s = 0; s < SS_GN_SLOTS; s++) a[s] = c0 + s < n ? term(c0 + s) : 0.0;
        const double v = ss_gn_tree(a);
        total = c0 == 0 ? v : total + v;
    }
    return total;
}

/* step 2: corr[4n ..] = u1 v1 u2 v2 */
static inline ss_tv_norm ss_tv_normalise_host(const float *corr, int n)
{
    ss_tv_norm nm;
    for (int c = 0; c < 4; c++) {
        nm.m[c] = ss_tv_tree_sum(n, [&](int k) { return (double)corr[4 * k + c]; }) / (double)n;
        const double m = nm.m[c];
        nm.d[c] = ss_tv_tree_sum(n, [&](int k) { return fabs((double)corr[4 * k + c] - m); }) / (double)n;
    }
    return nm;
}

static inline ss_tv_model ss_tv_hypothesis_host(const float *corr, int n, const ss_tv_norm &nm, uint32_t seed, uint32_t problem, int t)
{
    int pick[SS_TV_DRAWS];
    float uv[4 * SS_TV_DRAWS];
    ss_tv_draw(seed, problem, t, n, pick);
    for (int k = 0; k < SS_TV_DRAWS; k++)
        for (int c = 0; c < 4; c++) uv[4 * k + c] = corr[4 * pick[k] + c];
    ss_tv_work_host w;
    ss_tv_model m;
    ss_tv_model_of(uv, pick, nm, w, m);
    return m;
}

/* the k-th smallest (k from 0) of the n cosines by the search over the keys the kernel runs: bit by bit from the top, the smallest
 * key K with at least k + 1 keys <= K */
static inline double ss_tv_select_host(const double *cosv, int n, int k)
{
    uint64_t K = 0;
    for (int bit = 63; bit >= 0; bit--) {
        const uint64_t T = K | ((bit ? (1ull << bit) : 1ull) - 1ull);
        int count = 0;
        for (int i = 0; i < n; i++) count += ss_tv_key(cosv[i]) <= T ? 1 : 0;
        if (!(count >= k + 1)) K |= 1ull << bit;
    }
    return ss_tv_unkey(K);
}

/* The whole problem on the host the way the kernels run it.  corr: n x 4 floats; s1[n]: the scale of keypoint 1's octave; flag[n]:
 * 1 outlier of the model, 2 inlier, 3 triangulated; pts[n]: written where flag is 3.  Every field of *out is written; its status
 * is 0 */
static inline void ss_tv_problem_host(const float *corr, const float *s1, int n, const ss_tv_cam &cam, float s_last, const ss_two_view_params &p,
                                      uint32_t problem, uint8_t *flag, ss_map_point *pts, ss_two_view_result *out)
{
    ss_tv_result_clear(out, n, 0);
    for (int k = 0; k < n; k++) flag[k] = 1;
    if (ss_tv_too_few(n)) return;
    out->state = 2;
    const ss_tv_norm nm = ss_tv_normalise_host(corr, n);
    if (!ss_tv_norm_ok(nm)) return;
    double sh = -1.0, sf = -1.0;
    int th = -1, tf = -1;
    for (int t = 0; t < p.max_iterations; t++) {
        const ss_tv_model m = ss_tv_hypothesis_host(corr, n, nm, p.seed, problem, t);
        const double h = !m.ok_h ? -1.0 : ss_tv_tree_sum(n, [&](int k) {
            bool in;
            double chi[2];
            return ss_tv_term_h(m.h21, m.h12, (double)corr[4 * k], (double)corr[4 * k + 1], (double)corr[4 * k + 2], (double)corr[4 * k + 3], p.chi2_h, &in, chi);
        });
        const double f = !m.ok_f ? -1.0 : ss_tv_tree_sum(n, [&](int k) {
            bool in;
            double chi[2];
            return ss_tv_term_f(m.f21, (double)corr[4 * k], (double)corr[4 * k + 1], (double)corr[4 * k + 2], (double)corr[4 * k + 3], p.chi2_f, p.chi2_score, &in, chi);
        });
        if (th < 0 || ss_tv_beats(h, t, sh, th)) sh = h, th = t;
        if (tf < 0 || ss_tv_beats(f, t, sf, tf)) sf = f, tf = t;
    }
    out->score_h = sh, out->score_f = sf, out->iteration_h = th, out->iteration_f = tf;
    const int model = ss_tv_choose(sh, sf, p.rh_threshold);
    if (model == 0) return;
    out->model = model, out->state = 3;
    const ss_tv_model m = ss_tv_hypothesis_host(corr, n, nm, p.seed, problem, model == 2 ? th : tf);
    int n_in = 0;
    for (int k = 0; k < n; k++) {
        bool in;
        double chi[2];
        const double u1 = (double)corr[4 * k], v1 = (double)corr[4 * k + 1], u2 = (double)corr[4 * k + 2], v2 = (double)corr[4 * k + 3];
        if (model == 2) ss_tv_term_h(m.h21, m.h12, u1, v1, u2, v2, p.chi2_h, &in, chi);
        else ss_tv_term_f(m.f21, u1, v1, u2, v2, p.chi2_f, p.chi2_score, &in, chi);
        flag[k] = in ? 2 : 1;
        n_in += in ? 1 : 0;
    }
    out->n_inliers = n_in;
    double hyp[12 * SS_TV_MAX_HYP];
    for (int k = 0; k < 12 * SS_TV_MAX_HYP; k++) hyp[k] = 0.0;
    const int n_hyp = n_in < SS_TV_DRAWS ? -1 : model == 2 ? ss_tv_decompose_h(m.h21, cam, hyp) : ss_tv_decompose_f(m.f21, cam, hyp);
    int reason = 0, good[SS_TV_MAX_HYP] = {0}, best = -1, best_good = 0, second_good = 0;
    double cosp = 0.0;
    if (n_hyp < 0) reason = 2;
    else if (n_hyp == 0) reason = 1;
    else {
        for (int h = 0; h < n_hyp; h++)
            for (int k = 0; k < n; k++) {
                ss_tv_point q;
                if (flag[k] == 2 && ss_tv_check_rt(hyp + 12 * h, hyp + 12 * h + 9, cam, (double)corr[4 * k], (double)corr[4 * k + 1], (double)corr[4 * k + 2], (double)corr[4 * k + 3], &q))
                    good[h]++;
            }
        ss_tv_pick(good, n_hyp, &best, &best_good, &second_good);
    }
    if (best >= 0) {
        double *cosv = new double[(size_t)n];
        int ng = 0;
        for (int k = 0; k < n; k++) {
            ss_tv_point q;
            if (flag[k] == 2 && ss_tv_check_rt(hyp + 12 * best, hyp + 12 * best + 9, cam, (double)corr[4 * k], (double)corr[4 * k + 1], (double)corr[4 * k + 2], (double)corr[4 * k + 3], &q))
                cosv[ng++] = q.cosp;
        }
        cosp = ss_tv_select_host(cosv, ng, ss_tv_parallax_index(ng));
        delete[] cosv;
    }
    if (reason == 0) reason = ss_tv_accept(model, good, n_hyp, best_good, second_good, n_in, cosp, p);
    out->reason = reason, out->n_good = best_good, out->cos_parallax = cosp;
    if (reason != 0) {
        for (int k = 0; k < n; k++) flag[k] = 1;
        return;
    }
    out->state = 0;
    for (int k = 0; k < 9; k++) out->r21[k] = hyp[12 * best + k];
    for (int k = 0; k < 3; k++) out->t21[k] = hyp[12 * best + 9 + k];
    int n_tri = 0;
    for (int k = 0; k < n; k++) {
        ss_tv_point q;
        if (flag[k] == 2 && ss_tv_check_rt(out->r21, out->t21, cam, (double)corr[4 * k], (double)corr[4 * k + 1], (double)corr[4 * k + 2], (double)corr[4 * k + 3], &q) &&
            ss_tv_triangulated(q.cosp)) {
            flag[k] = 3, n_tri++;
            pts[k] = ss_tv_map_point(q, s1[k], s_last);
        }
    }
    out->n_triangulated = n_tri;
}

#endif
