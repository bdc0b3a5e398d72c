/*
 * ss_gba_steps.h -- the steps of the global bundle adjustment (the rule: include/sendslam_orb.h): the sorted
 * observation table and its two incidence lists, a free keyframe's block of the reduced system and its factor, the terms of the
 * matrix-free operator q = S.p, and the whole problem on the host.  The observation's terms of V, b and W, a point's factor and its
 * triangular solves, the back-substitution, the chi-term, the trial pose and the lambda schedule are ss_ba_steps.h's, term by term;
 * the tree of a sum and the Cholesky of a run-time order are ss_gn_steps.h's.  The kernels (ss_gba.hip), the host twin
 * ss_global_ba_host (ss_api_search.cpp) and tests/native/gba_steps_asan.cpp compile this text.
 *
 * All arithmetic is double.  Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a
 * NaN fails it.  Compile with -ffp-contract=off.  Division and square root are correctly rounded on both sides; there is no other
 * library function.
 */
#ifndef SS_GBA_STEPS_H
#define SS_GBA_STEPS_H

#include <vector>

#include "ss_ba_steps.h"

#define SS_GBA_C 0                                  /* the 21 sums of C_kk = sum Y.W^T, upper triangle row by row */
#define SS_GBA_YB SS_BA_DIAG                        /* the 6 sums of Y.b */
#define SS_GBA_U (SS_BA_DIAG + 6)                   /* the 26 sums of ss_pose_terms: U's and g's */
#define SS_GBA_SUMS (SS_BA_DIAG + 6 + SS_POSE_SUMS) /* the sums of a free keyframe's block */

/* One record of the sorted table: a problem's records stand in ascending (point, kf) order; kf and point are relative to the
 * problem, orig is the record's place in the caller's table (relative to the call), valid says its octave names a pyramid level.
 * ur is what ss_pose_stored_right keeps: -1 for a monocular observation */
struct ss_gba_rec {
    int32_t kf, point;
    float u, v, ur, scale;
    int32_t orig, valid;
};

SS_HD ss_ba_meas ss_gba_meas_of(const ss_gba_rec &r)
{
    ss_ba_meas m;
    m.u = r.u, m.v = r.v, m.ur = r.ur, m.scale = r.scale;
    return m;
}

/* a_b += (W^T.p)_b: one free observation's part of a point's a_i, the six products left to right */
SS_HD void ss_gba_wt_p(const double W[SS_BA_W], const double p[6], double a[3])
{
    SS_GN_UNROLL
    for (int b = 0; b < 3; b++)
        a[b] = a[b] + (((((W[b] * p[0] + W[3 + b] * p[1]) + W[6 + b] * p[2]) + W[9 + b] * p[3]) + W[12 + b] * p[4]) + W[15 + b] * p[5]);
}

/* (U.p)_a of the damped block U (its upper triangle row by row): the six products of row a left to right */
SS_HD void ss_gba_u_p(const double U[SS_BA_DIAG], const double p[6], double out[6])
{
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) {
        double s = 0.0;
        SS_GN_UNROLL
        for (int b = 0; b < 6; b++) {
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            const double term = U[6 * lo - lo * (lo - 1) / 2 + (hi - lo)] * p[b];
            s = b == 0 ? term : s + term;
        }
        out[a] = s;
    }
}

/* The SS_GBA_SUMS terms of one linearised observation of a free keyframe: the terms of C_kk and Y.b with Y = W.V^-1 row by row
 * (only when the point is solved; otherwise they are not written), then the 26 pose terms */
SS_HD void ss_gba_block_terms(const ss_pose_obs &o, const ss_pose_cam &c, const double R[9], const double t[3], bool robust, bool solved, const double W[SS_BA_W],
                              const double L[6], const double b[3], double term[SS_GBA_SUMS])
{
    if (solved) {
        double Y[SS_BA_W];
        ss_ba_coupling(L, W, Y);
        int m = 0;
        SS_GN_UNROLL
        for (int a = 0; a < 6; a++) {
            SS_GN_UNROLL
            for (int d = a; d < 6; d++) term[m++] = ss_ba_c_term(Y, W, a, d);
        }
        SS_GN_UNROLL
        for (int a = 0; a < 6; a++) term[SS_GBA_YB + a] = ss_ba_yb_term(Y, b, a);
    }
    (void)ss_pose_terms(o, c, R, t, robust, term + SS_GBA_U);
}

/* The sums of a free keyframe -> its damped block U (upper triangle), the factor L of M = U - C_kk (6 x 6 row-major, the lower
 * triangle; the rest +0.0) and the right-hand side r = -(g - Y.b).  False when a pivot is not > 0 */
SS_HD bool ss_gba_kf_block(const double sum[SS_GBA_SUMS], double lambda, double U[SS_BA_DIAG], double L[36], double r[6])
{
    double g[6];
    ss_ba_unpack_u(sum + SS_GBA_U, lambda, U, g);
    SS_GN_UNROLL
    for (int e = 0; e < 36; e++) L[e] = 0.0;
    int m = 0;
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) {
        SS_GN_UNROLL
        for (int b = a; b < 6; b++, m++) L[6 * b + a] = U[m] - sum[SS_GBA_C + m];
    }
    SS_GN_UNROLL
    for (int a = 0; a < 6; a++) r[a] = -(g[a] - sum[SS_GBA_YB + a]);
    return ss_gn_chol_n(L, 6, 6);
}

/* The sorted table and both incidence lists of one problem of n_kf keyframes and P points from its n records in any order.  rec [n]
 * in ascending (point, kf); pt_off, pt_cnt [P]: a point's run of rec (ascending kf); kf_off, kf_cnt [n_kf]: a keyframe's run of
 * kf_list [n], the numbers of its records (ascending point).  Two stable counting passes, first by kf, then by point.  Returns 0, or
 * 1: a kf outside the problem, 2: a point outside it, 3: a (kf, point) pair twice; *bad is then the offending record's number in
 * obs.  orig = orig_base + that number */
static inline int ss_gba_tables(int n_kf, int P, const ss_gba_obs *obs, int n, const float *scale, int n_levels, bool check_right, int orig_base,
                                ss_gba_rec *rec, int32_t *pt_off, int32_t *pt_cnt, int32_t *kf_off, int32_t *kf_cnt, int32_t *kf_list, int *bad)
{
    for (int k = 0; k < n_kf; k++) kf_cnt[k] = 0;
    for (int i = 0; i < P; i++) pt_cnt[i] = 0;
    for (int m = 0; m < n; m++) {
        *bad = m;
        if (obs[m].kf < 0 || obs[m].kf >= n_kf) return 1;
        if (obs[m].point < 0 || obs[m].point >= P) return 2;
        kf_cnt[obs[m].kf]++, pt_cnt[obs[m].point]++;
    }
    int at = 0;
    for (int k = 0; k < n_kf; k++) kf_off[k] = at, at += kf_cnt[k], kf_cnt[k] = 0;
    std::vector<int32_t> by_kf((size_t)n + 1);
    for (int m = 0; m < n; m++) by_kf[(size_t)(kf_off[obs[m].kf] + kf_cnt[obs[m].kf]++)] = m;
    at = 0;
    for (int i = 0; i < P; i++) pt_off[i] = at, at += pt_cnt[i], pt_cnt[i] = 0;
    for (int j = 0; j < n; j++) {
        const int m = by_kf[(size_t)j];
        const ss_gba_obs &o = obs[m];
        ss_gba_rec &r = rec[pt_off[o.point] + pt_cnt[o.point]++];
        r.kf = o.kf, r.point = o.point, r.u = o.u, r.v = o.v;
        r.ur = ss_pose_stored_right(check_right, true, o.right);
        r.valid = (o.octave >= 0 && o.octave < n_levels) ? 1 : 0;
        r.scale = r.valid ? scale[o.octave] : 1.0f;
        r.orig = orig_base + m;
    }
    for (int k = 0; k < n_kf; k++) kf_cnt[k] = 0;
    for (int s = 0; s < n; s++) {
        if (s > 0 && rec[s].point == rec[s - 1].point && rec[s].kf == rec[s - 1].kf) {
            *bad = rec[s].orig - orig_base;
            return 3;
        }
        kf_list[kf_off[rec[s].kf] + kf_cnt[rec[s].kf]++] = s;
    }
    return 0;
}

/* a dot product of the solve on the host: the tree over the 6 * n_kf entries */
static inline double ss_gba_dot_host(const double *a, const double *b, int n_kf)
{
    double slot[SS_GN_SLOTS];
    for (int s = 0; s < SS_GN_SLOTS; s++) slot[s] = 0.0;
    for (int k = 0; k < 6 * n_kf; k++) slot[k % SS_GN_SLOTS] = slot[k % SS_GN_SLOTS] + a[k] * b[k];
    return ss_gn_tree(slot);
}

/* The whole problem on the host the way the kernels run it.  cam, start (12 doubles each) and fixed per keyframe; the tables of
 * ss_gba_tables; X [P][3] the points widened (+0.0 where pflag is 2), on return the result; pflag [P] on entry 0 = a point, 2 =
 * none; ob [n_rec] on return the rule's byte of every sorted record; poses n_kf x 12.  Every field of *out is written */
static inline void ss_gba_problem_host(int n_kf, int P, int n_rec, const ss_pose_cam *cam, const double *start, const uint8_t *fixed, const ss_gba_rec *rec,
                                       const int32_t *pt_off, const int32_t *pt_cnt, const int32_t *kf_off, const int32_t *kf_cnt, const int32_t *kf_list,
                                       const ss_gba_params &p, uint8_t *ob, double *X, uint8_t *pflag, double *poses, ss_gba_result *out)
{
    const size_t K = (size_t)n_kf, zP = (size_t)P, S = (size_t)n_rec;
    bool start_ok = true;
    int n_free = 0;
    for (int k = 0; k < n_kf; k++) {
        start_ok = ss_pose_start(start + 12 * (size_t)k, poses + 12 * (size_t)k, poses + 12 * (size_t)k + 9) && start_ok;
        n_free += fixed[k] ? 0 : 1;
    }
    /* step 1 */
    int n_obs = 0, n_stereo = 0, n_active = 0;
    for (int i = 0; i < P; i++) {
        int cnt = 0;
        for (int j = 0; j < pt_cnt[i]; j++) {
            const size_t s = (size_t)pt_off[i] + j;
            const bool good = rec[s].valid != 0 && pflag[i] == 0;
            ob[s] = good ? 0 : 2;
            if (good) cnt++, n_stereo += rec[s].ur > 0.0f ? 1 : 0;
        }
        if (pflag[i] != 0) continue;
        n_obs += cnt;
        if (cnt < p.min_point_obs) pflag[i] = 1;
        else n_active++;
    }
    int state = !start_ok ? 2 : (n_active == 0 || n_free == 0) ? 1 : 0, n_frozen_max = 0, pcg = 0;
    double lambda = p.lambda, cost0 = 0.0, cost_before = 0.0;
    for (int r = 0; r < 4; r++) out->steps[r] = out->accepted[r] = 0;

    /* the workspace of the steps: a problem that does not run takes none */
    const size_t Ws = state == 0 ? S : 0, Wp = state == 0 ? zP : 0, Wk = state == 0 ? K : 0;
    std::vector<double> Wv(Ws * SS_BA_W + 1), Lv(Wp * 6 + 1), bv(Wp * 3 + 1), cv(Wp * 3 + 1), Uv(Wk * SS_BA_DIAG + 1), Mv(Wk * 36 + 1), x(Wk * 6 + 1), r(Wk * 6 + 1),
        z(Wk * 6 + 1), pv(Wk * 6 + 1), q(Wk * 6 + 1), trial(Wk * 12 + 1), Xt(Wp * 3 + 1), cost_k(K + 1), slot((size_t)SS_GBA_SUMS * SS_GN_SLOTS);
    std::vector<uint8_t> lin(Ws + 1), solved(Wp + 1);

    auto cost_of = [&](const double *ps, const double *Xs, bool robust) {
        for (int k = 0; k < n_kf; k++) {
            for (int s = 0; s < SS_GN_SLOTS; s++) slot[(size_t)s] = 0.0;
            for (int j = 0; j < kf_cnt[k]; j++) {
                const size_t s = (size_t)kf_list[kf_off[k] + j];
                const int i = rec[s].point;
                if (pflag[i] != 0 || ob[s] != 0) continue;
                const double term = ss_ba_cost_term(ss_ba_obs_of(Xs + 3 * (size_t)i, ss_gba_meas_of(rec[s])), cam[k], ps + 12 * (size_t)k, ps + 12 * (size_t)k + 9, robust);
                slot[(size_t)(j % SS_GN_SLOTS)] = slot[(size_t)(j % SS_GN_SLOTS)] + term;
            }
            cost_k[(size_t)k] = ss_gn_tree(slot.data());
        }
        for (int s = 0; s < SS_GN_SLOTS; s++) slot[(size_t)s] = 0.0;
        for (int k = 0; k < n_kf; k++) slot[(size_t)(k % SS_GN_SLOTS)] = slot[(size_t)(k % SS_GN_SLOTS)] + cost_k[(size_t)k];
        return ss_gn_tree(slot.data());
    };
    auto precondition = [&]() {
        for (int k = 0; k < n_kf; k++) {
            for (int a = 0; a < 6; a++) z[6 * (size_t)k + a] = r[6 * (size_t)k + a];
            if (!fixed[k]) ss_gn_subst_n(&Mv[36 * (size_t)k], 6, 6, &z[6 * (size_t)k]);
        }
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
            /* steps 2 and 3: the points */
            int n_frozen = 0;
            for (int i = 0; i < P; i++) {
                solved[(size_t)i] = 0;
                for (int j = 0; j < pt_cnt[i]; j++) lin[(size_t)pt_off[i] + j] = 0;
                if (pflag[i] != 0) continue;
                double V[SS_BA_V] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                for (int j = 0; j < pt_cnt[i]; j++) {
                    const size_t s = (size_t)pt_off[i] + j;
                    if (ob[s] != 0) continue;
                    const int k = rec[s].kf;
                    double tV[SS_BA_V], tb[3], tW[SS_BA_W];
                    if (!ss_ba_lin(ss_ba_obs_of(X + 3 * (size_t)i, ss_gba_meas_of(rec[s])), cam[k], poses + 12 * (size_t)k, poses + 12 * (size_t)k + 9, robust, tV, tb, tW))
                        continue;
                    lin[s] = 1;
                    for (int e = 0; e < SS_BA_V; e++) V[e] = V[e] + tV[e];
                    for (int e = 0; e < 3; e++) b[e] = b[e] + tb[e];
                    if (!fixed[k])
                        for (int e = 0; e < SS_BA_W; e++) Wv[s * SS_BA_W + e] = tW[e];
                }
                if (!ss_ba_point_factor(V, b, lambda, &Lv[(size_t)i * 6])) {
                    n_frozen++;
                    continue;
                }
                solved[(size_t)i] = 1;
                for (int e = 0; e < 3; e++) bv[(size_t)i * 3 + e] = b[e];
            }
            n_frozen_max = n_frozen > n_frozen_max ? n_frozen : n_frozen_max;
            /* the blocks of the free keyframes */
            bool ok = true;
            for (int k = 0; k < n_kf; k++) {
                for (int a = 0; a < 6; a++) x[6 * (size_t)k + a] = 0.0, r[6 * (size_t)k + a] = 0.0;
                if (fixed[k]) continue;
                for (size_t e = 0; e < slot.size(); e++) slot[e] = 0.0;
                for (int j = 0; j < kf_cnt[k]; j++) {
                    const size_t s = (size_t)kf_list[kf_off[k] + j];
                    if (!lin[s]) continue;
                    const size_t i = (size_t)rec[s].point;
                    double term[SS_GBA_SUMS];
                    ss_gba_block_terms(ss_ba_obs_of(X + 3 * i, ss_gba_meas_of(rec[s])), cam[k], poses + 12 * (size_t)k, poses + 12 * (size_t)k + 9, robust, solved[i] != 0,
                                       &Wv[s * SS_BA_W], &Lv[i * 6], &bv[i * 3], term);
                    for (int e = solved[i] ? 0 : SS_GBA_U; e < SS_GBA_SUMS; e++) {
                        double &a = slot[(size_t)e * SS_GN_SLOTS + j % SS_GN_SLOTS];
                        a = a + term[e];
                    }
                }
                double sum[SS_GBA_SUMS];
                for (int e = 0; e < SS_GBA_SUMS; e++) sum[e] = ss_gn_tree(&slot[(size_t)e * SS_GN_SLOTS]);
                ok = ss_gba_kf_block(sum, lambda, &Uv[(size_t)k * SS_BA_DIAG], &Mv[(size_t)k * 36], &r[6 * (size_t)k]) && ok;
            }
            if (!ok) {
                state = 2;
                break;
            }
            /* the solve: S.dc = r by preconditioned conjugate gradients, S never formed */
            precondition();
            for (size_t k = 0; k < K * 6; k++) pv[k] = z[k];
            double rho = ss_gba_dot_host(r.data(), z.data(), n_kf);
            const double stop = (p.pcg_tol * p.pcg_tol) * rho;
            int done = 0;
            while (done < p.pcg_iterations) {
                for (int i = 0; i < P; i++) {
                    if (!solved[(size_t)i]) continue;
                    double a[3] = {0.0, 0.0, 0.0};
                    for (int j = 0; j < pt_cnt[i]; j++) {
                        const size_t s = (size_t)pt_off[i] + j;
                        if (lin[s] && !fixed[rec[s].kf]) ss_gba_wt_p(&Wv[s * SS_BA_W], &pv[6 * (size_t)rec[s].kf], a);
                    }
                    ss_ba_point_subst(&Lv[(size_t)i * 6], a);
                    for (int e = 0; e < 3; e++) cv[(size_t)i * 3 + e] = a[e];
                }
                for (int k = 0; k < n_kf; k++) {
                    for (int a = 0; a < 6; a++) q[6 * (size_t)k + a] = 0.0;
                    if (fixed[k]) continue;
                    for (int e = 0; e < 6 * SS_GN_SLOTS; e++) slot[(size_t)e] = 0.0;
                    for (int j = 0; j < kf_cnt[k]; j++) {
                        const size_t s = (size_t)kf_list[kf_off[k] + j], i = (size_t)rec[s].point;
                        if (!lin[s] || !solved[i]) continue;
                        for (int a = 0; a < 6; a++) {
                            double &acc = slot[(size_t)a * SS_GN_SLOTS + j % SS_GN_SLOTS];
                            acc = acc + ss_ba_yb_term(&Wv[s * SS_BA_W], &cv[i * 3], a);
                        }
                    }
                    double up[6];
                    ss_gba_u_p(&Uv[(size_t)k * SS_BA_DIAG], &pv[6 * (size_t)k], up);
                    for (int a = 0; a < 6; a++) q[6 * (size_t)k + a] = up[a] - ss_gn_tree(&slot[(size_t)a * SS_GN_SLOTS]);
                }
                const double pq = ss_gba_dot_host(pv.data(), q.data(), n_kf);
                if (!(pq > 0.0)) break;
                const double alpha = rho / pq;
                for (size_t k = 0; k < K * 6; k++) x[k] = x[k] + alpha * pv[k], r[k] = r[k] - alpha * q[k];
                done++;
                precondition();
                const double rho1 = ss_gba_dot_host(r.data(), z.data(), n_kf);
                if (rho1 <= stop) break;
                const double beta = rho1 / rho;
                for (size_t k = 0; k < K * 6; k++) pv[k] = z[k] + beta * pv[k];
                rho = rho1;
            }
            pcg += done;
            /* step 6 */
            bool small = true, finite = true, large = false;
            for (int k = 0; k < n_kf; k++) {
                double *T = &trial[12 * (size_t)k];
                for (int e = 0; e < 12; e++) T[e] = poses[12 * (size_t)k + e];
                if (fixed[k]) continue;
                bool sm = false;
                if (!ss_ba_trial_pose(&x[6 * (size_t)k], p.step_eps, T, T + 9, &sm)) large = true;
                small = small && sm;
                finite = finite && ss_gn_all_finite(T, T + 9);
            }
            if (large) {
                state = 4;
                break;
            }
            for (int i = 0; i < P; i++) {
                for (int e = 0; e < 3; e++) Xt[(size_t)i * 3 + e] = X[(size_t)i * 3 + e];
                if (pflag[i] != 0 || !solved[(size_t)i]) continue;
                double v[3] = {-bv[(size_t)i * 3], -bv[(size_t)i * 3 + 1], -bv[(size_t)i * 3 + 2]};
                for (int j = 0; j < pt_cnt[i]; j++) {
                    const size_t s = (size_t)pt_off[i] + j;
                    if (lin[s] && !fixed[rec[s].kf]) ss_ba_point_rhs(&Wv[s * SS_BA_W], &x[6 * (size_t)rec[s].kf], v);
                }
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
            for (size_t e = 0; e < K * 12; e++) poses[e] = trial[e];
            for (size_t e = 0; e < zP * 3; e++) X[e] = Xt[e];
            if (small) break;
        }
        if (state != 0) break;
        /* step 8 */
        for (int i = 0; i < P; i++) {
            if (pflag[i] != 0) continue;
            int cnt = 0;
            for (int j = 0; j < pt_cnt[i]; j++) {
                const size_t s = (size_t)pt_off[i] + j;
                if (ob[s] != 0) continue;
                const int k = rec[s].kf;
                const ss_pose_obs o = ss_ba_obs_of(X + 3 * (size_t)i, ss_gba_meas_of(rec[s]));
                if (ss_pose_inlier(o, cam[k], ss_pose_chi2(o, cam[k], poses + 12 * (size_t)k, poses + 12 * (size_t)k + 9))) cnt++;
                else ob[s] = 1;
            }
            if (cnt < p.min_point_obs) pflag[i] = 1;
        }
    }
    int n_in = 0, n_act = 0;
    for (int i = 0; i < P; i++) n_act += pflag[i] == 0 ? 1 : 0;
    for (size_t s = 0; s < S; s++) n_in += ob[s] == 0 ? 1 : 0;
    out->lambda = lambda, out->cost_before = cost_before, out->cost_after = cost0;
    out->state = state, out->status = 0;
    out->n_obs = n_obs, out->n_stereo = n_stereo, out->n_inliers = n_in, out->n_points_active = n_act, out->n_frozen_max = n_frozen_max;
    out->pcg_iterations = pcg, out->n_free = n_free, out->n_fixed = n_kf - n_free;
    out->reserved[0] = out->reserved[1] = 0;
}

#endif
