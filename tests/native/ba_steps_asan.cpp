/* The steps of the local bundle adjustment (csrc/ss_ba_steps.h, the text the kernels and the host twin compile) as a stand-alone
 * program for -fsanitize=address,undefined: the terms of an observation on random, tiny, huge, NaN and infinite inputs, the factor of
 * definite and singular V and its triangular solves, the Cholesky of a run-time order on definite, singular and non-finite S against
 * the fixed-order text, and whole problems of 0 .. 2000 points the way the kernels run them.  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ss_ba_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

static ss_proj_view view_of(float fx, float fy, float cx, float cy, float bf)
{
    ss_proj_view v = {};
    v.rcw[0] = v.rcw[4] = v.rcw[8] = 1.0f;
    v.fx = fx, v.fy = fy, v.cx = cx, v.cy = cy, v.bf = bf;
    v.max_x = 640.0f, v.max_y = 480.0f;
    return v;
}

static ss_ba_params params_of(double lambda)
{
    ss_ba_params p = {};
    p.chi2_mono = 5.991, p.chi2_stereo = 7.815, p.lambda = lambda, p.lambda_factor = 10.0, p.lambda_min = 1e-9, p.step_eps = 1e-10;
    p.n_rounds = 2, p.iterations[0] = 5, p.iterations[1] = 10, p.robust_rounds = 1, p.min_point_obs = 2;
    return p;
}

int main()
{
    long steps = 0;
    uint32_t s = 97531u;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[] = {0.0, -0.0, 1e-320, 1e300, -1e300, inf, nan, 1.0};
    const float oddf[] = {0.0f, -0.0f, 1e-40f, 3e38f, -3e38f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(), 1.0f};
    const ss_pose_cam cam = ss_pose_cam_of(view_of(300.0f, 290.0f, 160.0f, 120.0f, 30.0f), 5.991, 7.815);
    /* one observation: it takes part in both linearisations or in neither */
    for (int it = 0; it < 20000; it++) {
        double X[3] = {(unit(s) - 0.5) * 4.0, (unit(s) - 0.5) * 3.0, 2.0 + 6.0 * unit(s)};
        ss_ba_meas m = {(float)(320.0 * unit(s)), (float)(240.0 * unit(s)), it % 2 ? (float)(300.0 * unit(s)) : -1.0f, 1.0f + 0.2f * (float)(it % 8)};
        double start[12] = {1, 0.01, -0.02, -0.01, 1, 0.015, 0.02, -0.015, 1, unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5}, R[9], t[3];
        if (it % 6 == 1) X[lcg(s) % 3] = odd[lcg(s) % 8];
        if (it % 6 == 2) m.u = oddf[lcg(s) % 8];
        if (it % 6 == 3) m.scale = oddf[lcg(s) % 8];
        if (it % 6 == 4) X[2] = -X[2];
        (void)ss_pose_start(start, R, t);
        const ss_pose_obs o = ss_ba_obs_of(X, m);
        double V[SS_BA_V], b[3], W[SS_BA_W], term[SS_POSE_SUMS];
        const bool robust = it % 3 == 0;
        const bool part = ss_ba_lin(o, cam, R, t, robust, V, b, W);
        if (part != ss_pose_terms(o, cam, R, t, robust, term)) return printf("the two linearisations disagree on who takes part\n"), 1;
        if (part && it % 6 == 0) {
            /* V is positive semi-definite: its diagonal and its first 2 x 2 minor */
            if (!(V[0] >= 0.0 && V[3] >= 0.0 && V[5] >= 0.0 && V[0] * V[3] - V[1] * V[1] >= -1e-6 * V[0] * V[3])) return printf("V is not semi-definite\n"), 1;
        }
        (void)ss_ba_cost_term(o, cam, R, t, robust);
        steps++;
    }
    /* the factor of V: definite ones solve, singular ones are refused, odd ones stay defined */
    for (int it = 0; it < 20000; it++) {
        double J[4][3], V[SS_BA_V], b[3], L[6];
        const int rows = it % 5 == 1 ? 2 : 4; /* two rows: rank 2 */
        for (auto &row : J)
            for (double &v : row) v = unit(s) - 0.5;
        int k = 0;
        for (int a = 0; a < 3; a++)
            for (int c = a; c < 3; c++) {
                double h = 0.0;
                for (int r = 0; r < rows; r++) h += J[r][a] * J[r][c];
                V[k++] = h;
            }
        for (double &v : b) v = unit(s) - 0.5;
        if (it % 5 == 2) V[lcg(s) % SS_BA_V] = odd[lcg(s) % 8];
        if (it % 5 == 3) V[0] = -1.0;
        const double lambda = it % 5 == 1 || it % 5 == 3 ? 0.0 : 1e-6;
        const bool ok = ss_ba_point_factor(V, b, lambda, L);
        if (it % 5 == 3 && ok) return printf("an indefinite V was factored\n"), 1;
        if (it % 5 == 1 && ok && L[5] > 1e-4) /* the square root of what rounding leaves */ return printf("a rank-2 V has a third pivot of %g\n", L[5]), 1;
        if (ok && it % 5 == 0) {
            double v[3] = {b[0], b[1], b[2]};
            ss_ba_point_subst(L, v);
            const double r0 = ((V[0] * (1.0 + lambda) + lambda) * v[0] + V[1] * v[1]) + V[2] * v[2] - b[0];
            if (fabs(r0) > 1e-6 * (1.0 + fabs(b[0]) + fabs(v[0]) + fabs(v[1]) + fabs(v[2]))) return printf("the 3 x 3 solve leaves %g\n", r0), 1;
            double Wm[SS_BA_W], Y[SS_BA_W];
            for (double &w : Wm) w = unit(s) - 0.5;
            ss_ba_coupling(L, Wm, Y);
            (void)ss_ba_c_term(Y, Wm, 5, 5);
            (void)ss_ba_yb_term(Y, b, 5);
            double rhs[3] = {0.0, 0.0, 0.0}, dc[6] = {0.1, -0.2, 0.3, 0.0, 1e-3, -1e-3};
            ss_ba_point_rhs(Wm, dc, rhs);
        }
        steps++;
    }
    /* the Cholesky of a run-time order against the fixed-order text, and on singular and non-finite systems */
    for (int it = 0; it < 400; it++) {
        const int n = it % 4 == 0 ? 6 : 1 + (int)(lcg(s) % 192);
        std::vector<double> J((size_t)(n + 3) * n), H((size_t)n * n), g((size_t)n), delta((size_t)n);
        for (double &v : J) v = unit(s) - 0.5;
        const int rows = it % 7 == 3 && n > 1 ? n - 1 : n + 3; /* one row short: singular */
        for (int a = 0; a < n; a++)
            for (int c = a; c < n; c++) {
                double h = 0.0;
                for (int r = 0; r < rows; r++) h += J[(size_t)r * n + a] * J[(size_t)r * n + c];
                H[(size_t)a * n + c] = h;
            }
        for (double &v : g) v = unit(s) - 0.5;
        if (it % 7 == 4) H[(size_t)(lcg(s) % n) * n + n - 1] = odd[lcg(s) % 8];
        if (n == 6 && it % 7 != 4) {
            double H6[6][6], d6[6];
            for (int a = 0; a < 6; a++)
                for (int c = a; c < 6; c++) H6[a][c] = H[(size_t)a * 6 + c];
            const bool ok6 = ss_gn_solve<6>(H6, g.data(), 1e-6, d6);
            const bool okn = ss_gn_solve_n(H.data(), 6, 6, g.data(), 1e-6, delta.data());
            if (ok6 != okn || memcmp(d6, delta.data(), sizeof(d6)) != 0) return printf("the run-time order differs from the fixed one\n"), 1;
        } else {
            const bool ok = ss_gn_solve_n(H.data(), n, n, g.data(), it % 7 == 3 ? 0.0 : 1e-6, delta.data());
            if (it % 7 == 3 && n > 1 && ok) {
                /* a singular Gram matrix may pass through rounding, with a tiny last pivot */
                if (H[(size_t)(n - 1) * n + n - 1] > 1e-5) return printf("a singular S of order %d was factored with a last pivot of %g\n", n, H[(size_t)(n - 1) * n + n - 1]), 1;
            }
        }
        steps++;
    }
    /* whole problems: points under known poses, a tenth of the observations gross outliers, some points behind a camera or odd */
    const int counts[] = {0, 1, 2, 255, 256, 257, 513, 2000};
    int states[5] = {0, 0, 0, 0, 0};
    for (int P : counts) {
        for (int variant = 0; variant < 5; variant++) {
            const int n_kf = variant == 4 ? 2 : 5, n_free = variant == 4 ? 1 : 3;
            std::vector<ss_pose_cam> cams((size_t)n_kf, cam);
            std::vector<double> start((size_t)n_kf * 12), X((size_t)P * 3 + 1), poses((size_t)n_kf * 12);
            std::vector<ss_ba_meas> meas((size_t)n_kf * P + 1);
            std::vector<uint8_t> obs((size_t)n_kf * P + 1), pflag((size_t)P + 1);
            for (int k = 0; k < n_kf; k++) {
                const double st[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.3 * k, 0.0, 0.0};
                for (int e = 0; e < 12; e++) start[(size_t)12 * k + e] = st[e];
                if (k < n_free) start[(size_t)12 * k + 9] += 0.03, start[(size_t)12 * k + 1] = 0.01, start[(size_t)12 * k + 3] = -0.01;
            }
            if (variant == 3) start[4] = nan;
            for (int i = 0; i < P; i++) {
                const double z = 4.0 + 6.0 * unit(s), x = (unit(s) - 0.5) * 0.7 * z + 0.6, y = (unit(s) - 0.5) * 0.6 * z;
                X[(size_t)3 * i] = (double)(float)(x + 0.02 * (unit(s) - 0.5)), X[(size_t)3 * i + 1] = (double)(float)y, X[(size_t)3 * i + 2] = (double)(float)z;
                pflag[(size_t)i] = i % 11 == 10 ? 2 : 0;
                for (int k = 0; k < n_kf; k++) {
                    const size_t o = (size_t)k * P + i;
                    const double xc = x - 0.3 * k;
                    ss_ba_meas m = {(float)(300.0 * xc / z + 160.0 + 0.5 * (unit(s) - 0.5)), (float)(290.0 * y / z + 120.0 + 0.5 * (unit(s) - 0.5)), -1.0f, 1.0f + 0.2f * (float)(i % 4)};
                    if ((i + k) % 10 == 0) m.u += 40.0f;
                    if (variant == 1 && i % 2) m.ur = m.u - (float)(30.0 / z);
                    if (variant == 2 && i == 7 && k == 1) m.v = std::numeric_limits<float>::quiet_NaN();
                    meas[o] = m;
                    obs[o] = pflag[(size_t)i] == 2 || (i + 2 * k) % 7 == 0 ? 2 : 0;
                }
                if (variant == 2 && i % 9 == 1) X[(size_t)3 * i + 2] = -X[(size_t)3 * i + 2];
                if (pflag[(size_t)i] == 2) X[(size_t)3 * i] = X[(size_t)3 * i + 1] = X[(size_t)3 * i + 2] = 0.0;
            }
            const ss_ba_params p = params_of(variant == 4 ? 0.0 : 1e-4);
            ss_ba_result r;
            ss_ba_problem_host(n_kf, n_free, P, cams.data(), start.data(), meas.data(), p, obs.data(), X.data(), pflag.data(), poses.data(), &r);
            if (r.state < 0 || r.state > 4 || r.state == 3) return printf("a state out of range\n"), 1;
            states[r.state]++;
            for (double v : poses)
                if (!ss_gn_is_finite(v)) return printf("a pose that is not finite was returned\n"), 1;
            for (int i = 0; i < P; i++)
                for (int e = 0; e < 3; e++)
                    if (!ss_gn_is_finite(X[(size_t)3 * i + e])) return printf("a point that is not finite was returned\n"), 1;
            for (int q = 0; q < 4; q++) steps += r.steps[q];
            if (r.state == 0 && variant == 0 && P >= 255 && (fabs(poses[9]) > 0.02 || r.n_inliers < r.n_obs / 2))
                return printf("P %d: the first pose was not recovered: t %g %g %g, %d of %d inliers\n", P, poses[9], poses[10], poses[11], r.n_inliers, r.n_obs), 1;
        }
    }
    if (states[1] < 5 || states[2] < 8) return printf("unexpected states: %d %d %d %d %d\n", states[0], states[1], states[2], states[3], states[4]), 1;
    printf("ok %ld states %d %d %d %d %d\n", steps, states[0], states[1], states[2], states[3], states[4]);
    return 0;
}
