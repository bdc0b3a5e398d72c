/*
 * ss_graph_steps.h -- the steps of the essential-graph optimisation (the rule: include/sendslam_orb.h): the two
 * new transcendentals (atan2 for y >= 0 and ln, by series), the Sim3 product and inverse, the logarithm of an edge's error, the
 * retraction, an edge's numeric Jacobian column, the incidence lists, the matrix-free product and its block-Jacobi preconditioner,
 * the map-point correction, and the whole problem on the host.  The exponentials are ss_pose_exp (ss_pose_steps.h) and
 * ss_sim3opt_exp_scale (ss_sim3opt_steps.h); the tree of a sum, the Cholesky of a run-time order and R <- dR.R are ss_gn_steps.h's;
 * lambda after a step is ss_ba_steps.h's.  The kernels (ss_graph.hip), the host twins ss_pose_graph_host and ss_pose_graph_edge_host
 * (ss_api_search.cpp) and tests/native/graph_steps_asan.cpp compile this text.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it (but for the step-size test of ss_pose_exp).  Compile with -ffp-contract=off.  Division and square root are correctly
 * rounded on both sides; there is no library function: the exponent of a double is read from its bits.
 */
#ifndef SS_GRAPH_STEPS_H
#define SS_GRAPH_STEPS_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "ss_ba_steps.h"
#include "ss_sim3opt_steps.h"

#define SS_GRAPH_SIM3 13        /* R row-major, t, s */
#define SS_GRAPH_ATAN_TERMS 24  /* |z| < 7/16: the first term left out, z^48 / 49, is below 2^-62 */
#define SS_GRAPH_LN_TERMS 13    /* |z| <= 3 - 2 sqrt 2: the first term left out, z^26 / 27, is below 2^-70 */
#define SS_GRAPH_H 0x1.12e0be826d695p-30  /* the double next to 1e-9: the step of the central differences */
#define SS_GRAPH_2H 0x1.12e0be826d695p-29 /* the double next to 2e-9 */
#define SS_GRAPH_SMALL_N 0x1.0p-26        /* below it theta / n rounds to 1 */
#define SS_GRAPH_NEAR_PI_N 0x1.0p-20      /* below it, with a negative cosine, the axis comes from the symmetric part */

/* the doubles next to 1 / (2k + 1), k = 0 .. 25 (tests/graph_ref.py forms the same table by division) */
#define SS_GRAPH_INV_ODD                                                                                                              \
    {                                                                                                                                 \
        0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4,                   \
        0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5,                  \
        0x1.8618618618618p-5, 0x1.642c8590b2164p-5, 0x1.47ae147ae147bp-5, 0x1.2f684bda12f68p-5, 0x1.1a7b9611a7b96p-5,                  \
        0x1.0842108421084p-5, 0x1.f07c1f07c1f08p-6, 0x1.d41d41d41d41dp-6, 0x1.bacf914c1bad0p-6, 0x1.a41a41a41a41ap-6,                  \
        0x1.8f9c18f9c18fap-6, 0x1.7d05f417d05f4p-6, 0x1.6c16c16c16c17p-6, 0x1.5c9882b931057p-6, 0x1.4e5e0a72f0539p-6,                  \
        0x1.4141414141414p-6                                                                                                          \
    }

/* ---- the two series ---- */
/* atan(r) for 0 <= r <= 1.  Reduction: r < 7/16: z = r; r < 11/16: z = (2r - 1) / (2 + r), plus atan(1/2); else z = (r - 1) / (r + 1),
 * plus pi/4; the constants are split into a high and a low double.  atan(z) = z + z*(mw*P), mw = -(z*z), P the Horner sum of
 * 1/3, 1/5, ... in mw from the last term */
SS_HD double ss_graph_atan01(double r)
{
    const double c[26] = SS_GRAPH_INV_ODD;
    double z = r, hi = 0.0, lo = 0.0;
    if (!(r < 0x1.cp-2)) {
        if (r < 0x1.6p-1) z = (2.0 * r - 1.0) / (2.0 + r), hi = 0x1.dac670561bb4fp-2, lo = 0x1.a2b7f222f65e2p-56;
        else z = (r - 1.0) / (r + 1.0), hi = 0x1.921fb54442d18p-1, lo = 0x1.1a62633145c07p-55;
    }
    const double mw = -(z * z);
    double P = c[SS_GRAPH_ATAN_TERMS - 1];
    SS_GN_UNROLL
    for (int k = SS_GRAPH_ATAN_TERMS - 2; k >= 1; k--) P = P * mw + c[k];
    return hi + ((z * (mw * P) + lo) + z);
}

/* atan2(y, x) for finite y >= 0 and finite x: the angle of (x, y) in 0 .. pi; (0, 0) gives 0 for x >= 0 and pi for x < 0 (a
 * negative zero counts as zero: 0).  Anything else gives NaN */
SS_HD double ss_graph_atan2(double y, double x)
{
    if (!(y >= 0.0) || !(x - x == 0.0) || !(y - y == 0.0)) {
        const double zero = (x - x) + (y - y);
        return zero / zero;
    }
    const double ax = fabs(x);
    if (y == 0.0) return x < 0.0 ? 0x1.921fb54442d18p+1 : 0.0;
    if (ax >= y) {
        const double a = ss_graph_atan01(y / ax);
        return x > 0.0 ? a : 0x1.921fb54442d18p+1 - (a - 0x1.1a62633145c07p-53);
    }
    const double a = ss_graph_atan01(ax / y);
    return x >= 0.0 ? 0x1.921fb54442d18p+0 - (a - 0x1.1a62633145c07p-54) : 0x1.921fb54442d18p+0 + (a + 0x1.1a62633145c07p-54);
}

SS_HD double ss_graph_from_bits(uint64_t b)
{
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

/* ln(s) for finite s > 0, subnormal ones included; anything else gives NaN.  s = m * 2^e with sqrt(1/2) < m <= sqrt 2 read from the
 * bits, f = m - 1 (exact), z = f / (2 + f), w = z*z, ln m = 2z + 2z*(w*P) with P the Horner sum of 1/3, 1/5, ... in w from the last
 * term; ln s = e*ln2_hi + ((2z*(w*P) + e*ln2_lo) + 2z), ln2_hi having 21 trailing zero bits so that e*ln2_hi is exact */
SS_HD double ss_graph_ln(double s)
{
    if (!(s > 0.0) || !(s - s == 0.0)) {
        const double zero = s - s;
        return zero / zero;
    }
    const double c[26] = SS_GRAPH_INV_ODD;
    int e = 0;
    if (s < 0x1.0p-1022) s = s * 0x1.0p+54, e = -54;
    uint64_t b;
    memcpy(&b, &s, sizeof b);
    e += (int)((b >> 52) & 0x7ffu) - 1023;
    double m = ss_graph_from_bits((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > 0x1.6a09e667f3bcdp+0) m = m * 0.5, e += 1;
    const double f = m - 1.0, z = f / (2.0 + f), w = z * z, z2 = 2.0 * z, de = (double)e;
    double P = c[SS_GRAPH_LN_TERMS - 1];
    SS_GN_UNROLL
    for (int k = SS_GRAPH_LN_TERMS - 2; k >= 1; k--) P = P * w + c[k];
    return de * 0x1.62e42fee00000p-1 + ((z2 * (w * P) + de * 0x1.a39ef35793c76p-33) + z2);
}

/* ---- Sim3: thirteen doubles, x -> s.R.x + t ---- */
/* o = S^-1: R^T, -(1/s).R^T.t, 1/s */
SS_HD void ss_graph_inv(const double *S, double *o)
{
    const double is = 1.0 / S[12];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) o[3 * i + j] = S[3 * j + i];
        o[9 + i] = -(is * ((S[i] * S[9] + S[3 + i] * S[10]) + S[6 + i] * S[11]));
    }
    o[12] = is;
}

/* o = A.B: RA.RB, sA.(RA.tB) + tA, sA.sB; o is neither A nor B */
SS_HD void ss_graph_mul(const double *A, const double *B, double *o)
{
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) {
        SS_GN_UNROLL
        for (int j = 0; j < 3; j++) o[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
        o[9 + i] = A[12] * ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i];
    }
    o[12] = A[12] * B[12];
}

/* every entry finite and s > 0 */
SS_HD bool ss_graph_usable(const double *S)
{
    bool ok = S[12] > 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < SS_GRAPH_SIM3; k++) ok = ok && ss_gn_is_finite(S[k]);
    return ok;
}

/* the measurement of edge (i, j): N_j . N_i^-1 */
SS_HD void ss_graph_measure(const double *Ni, const double *Nj, double *M)
{
    double inv[SS_GRAPH_SIM3];
    ss_graph_inv(Ni, inv);
    ss_graph_mul(Nj, inv, M);
}

/* e = (omega, upsilon, sigma) of a Sim3 E: the rotation logarithm, t as it stands, ln s */
SS_HD void ss_graph_log(const double *E, double e[7])
{
    const double v0 = 0.5 * (E[7] - E[5]), v1 = 0.5 * (E[2] - E[6]), v2 = 0.5 * (E[3] - E[1]);
    const double c = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
    const double n = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double th = ss_graph_atan2(n, c);
    if (c < 0.0 && n < SS_GRAPH_NEAR_PI_N) {
        /* next to pi the antisymmetric part vanishes: the axis a from B = (E + E^T) / 2 = c.I + (1 - c).a.a^T, by its largest
         * diagonal entry (the first among equals); its sign is v's, + when v gives none */
        const double d = 1.0 - c, b01 = 0.5 * (E[1] + E[3]), b02 = 0.5 * (E[2] + E[6]), b12 = 0.5 * (E[5] + E[7]);
        double a0, a1, a2;
        if (E[0] >= E[4] && E[0] >= E[8]) {
            a0 = sqrt((E[0] - c) / d);
            a1 = b01 / (d * a0), a2 = b02 / (d * a0);
        } else if (E[4] >= E[8]) {
            a1 = sqrt((E[4] - c) / d);
            a0 = b01 / (d * a1), a2 = b12 / (d * a1);
        } else {
            a2 = sqrt((E[8] - c) / d);
            a0 = b02 / (d * a2), a1 = b12 / (d * a2);
        }
        if ((a0 * v0 + a1 * v1) + a2 * v2 < 0.0) a0 = -a0, a1 = -a1, a2 = -a2;
        e[0] = a0 * th, e[1] = a1 * th, e[2] = a2 * th;
    } else if (n < SS_GRAPH_SMALL_N) {
        e[0] = v0, e[1] = v1, e[2] = v2;
    } else {
        const double f = th / n;
        e[0] = v0 * f, e[1] = v1 * f, e[2] = v2 * f;
    }
    e[3] = E[9], e[4] = E[10], e[5] = E[11];
    e[6] = ss_graph_ln(E[12]);
}

/* the error of edge (i, j) under S_i, S_j: E = (M . S_i) . S_j^-1 */
SS_HD void ss_graph_error(const double *M, const double *Si, const double *Sj, double e[7])
{
    double A[SS_GRAPH_SIM3], B[SS_GRAPH_SIM3], E[SS_GRAPH_SIM3];
    ss_graph_mul(M, Si, A);
    ss_graph_inv(Sj, B);
    ss_graph_mul(A, B, E);
    ss_graph_log(E, e);
}

SS_HD double ss_graph_dot7(const double *a, const double *b)
{
    return (((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]) + a[6] * b[6];
}

/* the retraction of the Sim3 refinement: R <- dR.R, t <- ds.(dR.t) + upsilon, s <- ds.s.  False, and S untouched, when the step is
 * too large: q > pi^2, or |delta_6| > 1 */
SS_HD bool ss_graph_retract(const double d[7], bool fix_scale, double *S)
{
    double dR[9], dt[3], tn[3];
    if (!ss_pose_exp(d, dR, dt)) return false;
    if (!fix_scale && !(fabs(d[6]) <= 1.0)) return false;
    const double ds = fix_scale ? 1.0 : ss_sim3opt_exp_scale(d[6]);
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) tn[i] = ds * ((dR[3 * i] * S[9] + dR[3 * i + 1] * S[10]) + dR[3 * i + 2] * S[11]) + d[3 + i];
    ss_gn_rotate(dR, S);
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) S[9 + k] = tn[k];
    if (!fix_scale) S[12] = ds * S[12];
    return true;
}

/* column a of the Jacobian of an edge's error by the increment of endpoint `side` (0: i, 1: j): (e(+h) - e(-h)) / 2h through the
 * retraction.  zero: the endpoint is fixed, or a is the scale under fix_scale: the column is +0.0 */
SS_HD void ss_graph_column(const double *M, const double *Si, const double *Sj, int side, int a, bool fix_scale, bool zero, double col[7])
{
    if (zero) {
        SS_GN_UNROLL
        for (int r = 0; r < 7; r++) col[r] = 0.0;
        return;
    }
    double ep[7], em[7], d[7], P[SS_GRAPH_SIM3], Pi[SS_GRAPH_SIM3], Pj[SS_GRAPH_SIM3];
    SS_GN_UNROLL
    for (int sign = 0; sign < 2; sign++) {
        SS_GN_UNROLL
        for (int k = 0; k < 7; k++) d[k] = k == a ? (sign ? -SS_GRAPH_H : SS_GRAPH_H) : 0.0;
        SS_GN_UNROLL
        for (int k = 0; k < SS_GRAPH_SIM3; k++) P[k] = side ? Sj[k] : Si[k];
        (void)ss_graph_retract(d, fix_scale, P);
        SS_GN_UNROLL
        for (int k = 0; k < SS_GRAPH_SIM3; k++) Pi[k] = side ? Si[k] : P[k], Pj[k] = side ? P[k] : Sj[k]; /* entry by entry: no pointer to choose */
        ss_graph_error(M, Pi, Pj, sign ? em : ep);
    }
    SS_GN_UNROLL
    for (int r = 0; r < 7; r++) col[r] = (ep[r] - em[r]) / SS_GRAPH_2H;
}

/* the cost term of an edge */
SS_HD double ss_graph_cost_term(const double *M, const double *Si, const double *Sj)
{
    double e[7];
    ss_graph_error(M, Si, Sj, e);
    return ss_graph_dot7(e, e);
}

/* u = J.(p_i, p_j): J is [14][7], column c at J + 7c; each entry adds its fourteen products left to right */
SS_HD void ss_graph_edge_product(const double *J, const double *pi, const double *pj, double u[7])
{
    SS_GN_UNROLL
    for (int r = 0; r < 7; r++) {
        double v = J[r] * pi[0];
        SS_GN_UNROLL
        for (int c = 1; c < 7; c++) v = v + J[7 * c + r] * pi[c];
        SS_GN_UNROLL
        for (int c = 0; c < 7; c++) v = v + J[7 * (7 + c) + r] * pj[c];
        u[r] = v;
    }
}

/* x <- S^-1(N(x)): the correction of a map point whose reference keyframe has the non-corrected N and the optimised S */
SS_HD void ss_graph_point(const double *N, const double *S, double x[3])
{
    double d[3];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) d[i] = (N[12] * ((N[3 * i] * x[0] + N[3 * i + 1] * x[1]) + N[3 * i + 2] * x[2]) + N[9 + i]) - S[9 + i];
    const double is = 1.0 / S[12];
    SS_GN_UNROLL
    for (int i = 0; i < 3; i++) x[i] = is * ((S[i] * d[0] + S[3 + i] * d[1]) + S[6 + i] * d[2]);
}

/* R and t / s: upstream's SetPose */
SS_HD void ss_graph_pose(const double *S, double pose[12])
{
    SS_GN_UNROLL
    for (int k = 0; k < 9; k++) pose[k] = S[k];
    SS_GN_UNROLL
    for (int k = 0; k < 3; k++) pose[9 + k] = S[9 + k] / S[12];
}

/* One free vertex of a step: its incident (edge, side) pairs inc[0 .. n_inc) (2 * edge + side, ascending) -> the lower triangle of
 * H_vv damped and factored in L (7 x 7, row-major; order n), the damping terms dd and the gradient g.  J [edges][14][7] and err
 * [edges][7] are the arrays of the edge numbers inc names.  False when a pivot is not > 0 */
SS_HD bool ss_graph_vertex_block(const int32_t *inc, int n_inc, const double *J, const double *err, int n, double lambda, double *L, double *dd, double *g)
{
    double H[28], gv[7];
    SS_GN_UNROLL
    for (int k = 0; k < 28; k++) H[k] = 0.0;
    SS_GN_UNROLL
    for (int k = 0; k < 7; k++) gv[k] = 0.0;
    for (int m = 0; m < n_inc; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const double *Jc = J + ((size_t)e * 14 + 7 * side) * 7, *ee = err + (size_t)e * 7;
        SS_GN_UNROLL
        for (int a = 0; a < 7; a++) {
            SS_GN_UNROLL
            for (int b = 0; b <= a; b++) H[a * (a + 1) / 2 + b] = H[a * (a + 1) / 2 + b] + ss_graph_dot7(Jc + 7 * a, Jc + 7 * b);
            gv[a] = gv[a] + ss_graph_dot7(Jc + 7 * a, ee);
        }
    }
    SS_GN_UNROLL
    for (int a = 0; a < 7; a++) {
        const double haa = H[a * (a + 1) / 2 + a];
        dd[a] = a < n ? lambda * (1.0 + haa) : 0.0;
        g[a] = a < n ? gv[a] : 0.0;
        SS_GN_UNROLL
        for (int b = 0; b <= a; b++) L[7 * a + b] = b == a ? haa + dd[a] : H[a * (a + 1) / 2 + b];
    }
    return ss_gn_chol_n(L, n, 7);
}

/* q_v = sum J_side^T.u_e over the incident pairs in order, then the damping term; entries a >= n are +0.0 */
SS_HD void ss_graph_vertex_product(const int32_t *inc, int n_inc, const double *J, const double *u, int n, const double *dd, const double *p, double *q)
{
    double acc[7];
    SS_GN_UNROLL
    for (int k = 0; k < 7; k++) acc[k] = 0.0;
    for (int m = 0; m < n_inc; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const double *Jc = J + ((size_t)e * 14 + 7 * side) * 7, *ue = u + (size_t)e * 7;
        SS_GN_UNROLL
        for (int a = 0; a < 7; a++) acc[a] = acc[a] + ss_graph_dot7(Jc + 7 * a, ue);
    }
    SS_GN_UNROLL
    for (int a = 0; a < 7; a++) q[a] = a < n ? acc[a] + dd[a] * p[a] : 0.0;
}

/* The incidence lists of n_edges edges (i, j at edges[2e], edges[2e + 1], both in 0 .. n_kf-1) over n_kf vertices: off and cnt per
 * vertex, inc [2 * n_edges] with 2 * e + side in ascending order per vertex */
static inline void ss_graph_incidence(int n_kf, int n_edges, const int32_t *edges, int32_t *off, int32_t *cnt, int32_t *inc)
{
    for (int v = 0; v < n_kf; v++) cnt[v] = 0;
    for (int e = 0; e < n_edges; e++) cnt[edges[2 * e]]++, cnt[edges[2 * e + 1]]++;
    int at = 0;
    for (int v = 0; v < n_kf; v++) off[v] = at, at += cnt[v], cnt[v] = 0;
    for (int e = 0; e < n_edges; e++)
        for (int side = 0; side < 2; side++) {
            const int v = edges[2 * e + side];
            inc[off[v] + cnt[v]++] = 2 * e + side;
        }
}

/* a dot product of the solve on the host: the tree over the 7 * n_kf entries */
static inline double ss_graph_dot_host(const double *a, const double *b, int n_kf)
{
    double slot[SS_GN_SLOTS];
    for (int s = 0; s < SS_GN_SLOTS; s++) slot[s] = 0.0;
    for (int k = 0; k < 7 * n_kf; k++) slot[k % SS_GN_SLOTS] = slot[k % SS_GN_SLOTS] + a[k] * b[k];
    return ss_gn_tree(slot);
}

/* The whole problem on the host the way the kernels run it.  nc, start: n_kf x 13 doubles; fixed: n_kf bytes; edges: n_edges pairs of
 * vertex numbers, checked by the caller; sim3: n_kf x 13 doubles out.  Every field of *out is written */
static inline void ss_graph_problem_host(int n_kf, int n_edges, const double *nc, const double *start, const uint8_t *fixed, const int32_t *edges,
                                         const ss_graph_params &p, double *sim3, ss_graph_result *out)
{
    const size_t K = (size_t)n_kf, E = (size_t)n_edges;
    const bool fix = p.fix_scale != 0;
    const int n = fix ? 6 : 7;
    bool usable = true;
    int n_free = 0;
    for (int v = 0; v < n_kf; v++) {
        usable = ss_graph_usable(nc + 13 * (size_t)v) && ss_graph_usable(start + 13 * (size_t)v) && usable;
        n_free += fixed[v] ? 0 : 1;
    }
    for (size_t k = 0; k < K * 13; k++) sim3[k] = start[k];
    int state = !usable ? 2 : (n_free == 0 || n_edges == 0) ? 1 : 0, steps = 0, accepted = 0, pcg = 0;
    double lambda = p.lambda, cost0 = 0.0, cost_before = 0.0;
    /* the workspace of the steps: a problem that does not run takes none */
    const size_t We = state == 0 ? E : 0, Wk = state == 0 ? K : 0;
    std::vector<double> M(We * 13 + 1), err(We * 7 + 1), J(We * 98 + 1), u(We * 7 + 1), L(Wk * 49 + 1), dd(Wk * 7 + 1), g(Wk * 7 + 1), x(Wk * 7 + 1),
        r(Wk * 7 + 1), z(Wk * 7 + 1), pv(Wk * 7 + 1), q(Wk * 7 + 1), trial(Wk * 13 + 1);
    std::vector<int32_t> off(Wk + 1), cnt(Wk + 1), inc(2 * We + 1);
    if (state == 0) ss_graph_incidence(n_kf, n_edges, edges, off.data(), cnt.data(), inc.data());

    auto cost_of = [&](const double *S) {
        double slot[SS_GN_SLOTS];
        for (int s = 0; s < SS_GN_SLOTS; s++) slot[s] = 0.0;
        for (int e = 0; e < n_edges; e++)
            slot[e % SS_GN_SLOTS] = slot[e % SS_GN_SLOTS] + ss_graph_cost_term(&M[13 * (size_t)e], S + 13 * (size_t)edges[2 * e], S + 13 * (size_t)edges[2 * e + 1]);
        return ss_gn_tree(slot);
    };
    auto precondition = [&]() {
        for (int v = 0; v < n_kf; v++) {
            for (int a = 0; a < 7; a++) z[7 * (size_t)v + a] = r[7 * (size_t)v + a];
            if (!fixed[v]) ss_gn_subst_n(&L[49 * (size_t)v], n, 7, &z[7 * (size_t)v]);
        }
    };

    if (state == 0) {
        for (int e = 0; e < n_edges; e++) ss_graph_measure(nc + 13 * (size_t)edges[2 * e], nc + 13 * (size_t)edges[2 * e + 1], &M[13 * (size_t)e]);
        cost0 = cost_of(sim3);
        if (!ss_gn_is_finite(cost0)) state = 2, cost0 = 0.0;
        cost_before = cost0;
    }
    for (int it = 0; state == 0 && it < p.iterations; it++) {
        /* the linearisation */
        for (int e = 0; e < n_edges; e++) {
            const int i = edges[2 * e], j = edges[2 * e + 1];
            const double *Me = &M[13 * (size_t)e], *Si = sim3 + 13 * (size_t)i, *Sj = sim3 + 13 * (size_t)j;
            ss_graph_error(Me, Si, Sj, &err[7 * (size_t)e]);
            for (int c = 0; c < 14; c++)
                ss_graph_column(Me, Si, Sj, c / 7, c % 7, fix, fixed[c < 7 ? i : j] != 0 || (fix && c % 7 == 6), &J[(14 * (size_t)e + c) * 7]);
        }
        /* the blocks */
        bool ok = true;
        for (int v = 0; v < n_kf; v++) {
            if (fixed[v]) {
                for (int a = 0; a < 7; a++) dd[7 * (size_t)v + a] = g[7 * (size_t)v + a] = 0.0;
                continue;
            }
            ok = ss_graph_vertex_block(&inc[off[v]], cnt[v], J.data(), err.data(), n, lambda, &L[49 * (size_t)v], &dd[7 * (size_t)v], &g[7 * (size_t)v]) && ok;
        }
        if (!ok) {
            state = 2;
            break;
        }
        /* the solve */
        for (size_t k = 0; k < K * 7; k++) x[k] = 0.0, r[k] = fixed[k / 7] ? 0.0 : -g[k];
        for (int v = 0; v < n_kf; v++)
            if (!fixed[v])
                for (int a = n; a < 7; a++) r[7 * (size_t)v + a] = 0.0;
        precondition();
        for (size_t k = 0; k < K * 7; k++) pv[k] = z[k];
        double rho = ss_graph_dot_host(r.data(), z.data(), n_kf);
        const double stop = (p.pcg_tol * p.pcg_tol) * rho;
        int done = 0;
        while (done < p.pcg_iterations) {
            for (int e = 0; e < n_edges; e++)
                ss_graph_edge_product(&J[98 * (size_t)e], &pv[7 * (size_t)edges[2 * e]], &pv[7 * (size_t)edges[2 * e + 1]], &u[7 * (size_t)e]);
            for (int v = 0; v < n_kf; v++) {
                if (fixed[v]) {
                    for (int a = 0; a < 7; a++) q[7 * (size_t)v + a] = 0.0;
                    continue;
                }
                ss_graph_vertex_product(&inc[off[v]], cnt[v], J.data(), u.data(), n, &dd[7 * (size_t)v], &pv[7 * (size_t)v], &q[7 * (size_t)v]);
            }
            const double pq = ss_graph_dot_host(pv.data(), q.data(), n_kf);
            if (!(pq > 0.0)) break;
            const double alpha = rho / pq;
            for (size_t k = 0; k < K * 7; k++) x[k] = x[k] + alpha * pv[k], r[k] = r[k] - alpha * q[k];
            done++;
            precondition();
            const double rho1 = ss_graph_dot_host(r.data(), z.data(), n_kf);
            if (rho1 <= stop) break;
            const double beta = rho1 / rho;
            for (size_t k = 0; k < K * 7; k++) pv[k] = z[k] + beta * pv[k];
            rho = rho1;
        }
        pcg += done;
        /* the trial state */
        bool large = false, finite = true;
        for (int v = 0; v < n_kf; v++) {
            double *T = &trial[13 * (size_t)v];
            for (int k = 0; k < 13; k++) T[k] = sim3[13 * (size_t)v + k];
            if (!fixed[v] && !ss_graph_retract(&x[7 * (size_t)v], fix, T)) large = true;
            for (int k = 0; k < 13; k++) finite = finite && ss_gn_is_finite(T[k]);
        }
        if (large) {
            state = 4;
            break;
        }
        const double cost1 = cost_of(trial.data());
        const bool accept = finite && ss_gn_is_finite(cost1) && cost1 <= cost0;
        steps++;
        lambda = ss_ba_next_lambda(lambda, accept, p.lambda_factor, p.lambda_min);
        if (!accept) continue;
        accepted++;
        cost0 = cost1;
        for (size_t k = 0; k < K * 13; k++) sim3[k] = trial[k];
    }
    out->lambda = lambda, out->cost_before = cost_before, out->cost_after = cost0;
    out->state = state, out->n_edges = n_edges, out->n_free = n_free, out->steps = steps, out->accepted = accepted, out->pcg_iterations = pcg;
}

#endif
