/* The steps of the Sim3 refinement (csrc/ss_sim3opt_steps.h, the text the kernels and the host twin compile) as a stand-alone program
 * for -fsanitize=address,undefined: the start on ordinary, sheared, degenerate, NaN and infinite models, the scale's series, the solve
 * on definite, singular and non-finite systems for six and seven unknowns, and whole pairs of 0 - 1000 correspondences with points
 * behind either camera, run by the very loop the host twin runs.  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_sim3opt_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

static ss_proj_view view_of(float f, float cx, float cy)
{
    ss_proj_view v = {};
    v.rcw[0] = v.rcw[4] = v.rcw[8] = 1.0f;
    v.fx = v.fy = f, v.cx = cx, v.cy = cy;
    return v;
}

static bool result_finite(const ss_sim3_opt_result &r)
{
    bool ok = ss_gn_all_finite(r.r12, r.t12) && ss_gn_is_finite(r.s12) && ss_gn_is_finite(r.cost);
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(r.model.sr12[k]) && std::isfinite(r.model.sr21[k]);
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(r.model.t12[k]) && std::isfinite(r.model.t21[k]);
    return ok && std::isfinite(r.model.s12);
}

int main()
{
    long steps = 0;
    uint32_t s = 97531u;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float odd[] = {0.0f, -0.0f, 1e-42f, 1e38f, -1e38f, inf, nan, 1.0f};
    /* the start: finite always, a rotation and the row norm for ordinary models */
    for (int it = 0; it < 20000; it++) {
        ss_sim3_result m = {};
        const double sc = 0.5 + 2.0 * unit(s);
        const double e[3] = {0.3 * (unit(s) - 0.5), 0.3 * (unit(s) - 0.5), 0.3 * (unit(s) - 0.5)};
        const double r[9] = {1, -e[2], e[1], e[2], 1, -e[0], -e[1], e[0], 1};
        for (int k = 0; k < 9; k++) m.sr12[k] = (float)(sc * r[k]);
        for (int k = 0; k < 3; k++) m.t12[k] = (float)(unit(s) - 0.5);
        if (it % 5 == 1) m.sr12[lcg(s) % 9] = odd[lcg(s) % 8];
        if (it % 5 == 2) m.t12[lcg(s) % 3] = odd[lcg(s) % 8];
        if (it % 5 == 3)
            for (int k = 0; k < 9; k++) m.sr12[k] = 0.0f;
        double R[9], t[3], sv;
        const bool ok = ss_sim3opt_start(m, it % 2 == 0, R, t, &sv);
        if (!ss_gn_all_finite(R, t) || !ss_gn_is_finite(sv) || !(sv > 0.0)) return printf("a start is not finite\n"), 1;
        if (it % 5 == 3 && ok) return printf("the zero model was accepted as a start\n"), 1;
        if (ok && it % 5 == 0) {
            const double d = (R[0] * R[3] + R[1] * R[4]) + R[2] * R[5], n = (R[6] * R[6] + R[7] * R[7]) + R[8] * R[8];
            if (fabs(d) > 1e-9 || fabs(n - 1.0) > 1e-9) return printf("a start rotation is not orthonormal: %g %g\n", d, n), 1;
            if (it % 2 == 0 && sv != 1.0) return printf("fix_scale did not give 1.0\n"), 1;
        }
        steps++;
    }
    /* the scale's series against exp */
    for (int it = 0; it < 20000; it++) {
        const double x = 2.0 * unit(s) - 1.0, v = ss_sim3opt_exp_scale(x);
        if (fabs(v - exp(x)) > 2e-15) /* Horner at x < 0 cancels: a few ulp of 1 */
            return printf("the series of the scale is off at %g: %.17g\n", x, v), 1;
        steps++;
    }
    /* the solve: singular and non-finite systems are refused or stay defined */
    const double oddd[] = {0.0, -0.0, 1e-320, 1e300, -1e300, (double)inf, (double)nan, 1.0};
    for (int it = 0; it < 6000; it++) {
        double J[9][7], sum[SS_SIM3OPT_SUMS], delta[7] = {0, 0, 0, 0, 0, 0, 0};
        for (auto &row : J)
            for (double &v : row) v = unit(s) - 0.5;
        for (int a = 0; a < 7; a++)
            for (int b = a; b < 7; b++) {
                double h = 0.0;
                for (auto &row : J) h += row[a] * row[b];
                sum[ss_sim3opt_h(a, b)] = it % 7 == 3 ? 0.0 : h;
            }
        for (int a = 0; a < 7; a++) sum[28 + a] = unit(s) - 0.5;
        if (it % 7 == 4) sum[lcg(s) % SS_SIM3OPT_SUMS] = oddd[lcg(s) % 8];
        if (it % 7 == 5) sum[0] = -1.0;
        const double lambda = it % 7 == 3 ? 0.0 : 1e-6;
        const bool ok = it % 2 ? ss_sim3opt_solve<6>(sum, lambda, delta) : ss_sim3opt_solve<7>(sum, lambda, delta);
        if ((it % 7 == 3 || it % 7 == 5) && ok) return printf("a system that is not definite was solved\n"), 1;
        if (ok && it % 7 < 3) { /* the residual of the damped system's first row */
            const int n = it % 2 ? 6 : 7;
            double r = sum[28];
            for (int b = 0; b < n; b++) r += (sum[ss_sim3opt_h(0, b)] + (b == 0 ? lambda * (1.0 + sum[0]) : 0.0)) * delta[b];
            if (fabs(r) > 1e-6) return printf("the solve leaves a residual of %g\n", r), 1;
        }
        steps++;
    }
    /* pairs: n correspondences under a known Sim3, a fifth of them gross mismatches; variants put points behind either camera, make
     * inputs non-finite, start far off or from a model that is no model */
    const ss_proj_view v1 = view_of(300.0f, 160.0f, 120.0f), v2 = view_of(320.0f, 150.0f, 130.0f);
    const int counts[] = {0, 2, 9, 10, 64, 65, 257, 1000};
    int states[5] = {0, 0, 0, 0, 0};
    ss_sim3_opt_params p = {};
    p.chi2 = 10.0, p.lambda = 1e-6, p.step_eps = 1e-10, p.iterations0 = 5, p.iterations_more = 10, p.iterations_same = 5, p.min_corr = 10, p.min_inliers = 10;
    const double s_true = 1.2, t_true[3] = {0.1, -0.05, 0.2};
    for (int n : counts) {
        for (int variant = 0; variant < 6; variant++) {
            std::vector<ss_sim3opt_corr> corr;
            for (int i = 0; i < n; i++) {
                const double z = 2.0 + 6.0 * unit(s), x = (unit(s) - 0.5) * 0.8 * z, y = (unit(s) - 0.5) * 0.6 * z;
                float x2[3] = {(float)x, (float)y, (float)z};
                float x1[3] = {(float)(s_true * x + t_true[0]), (float)(s_true * y + t_true[1]), (float)(s_true * z + t_true[2])};
                float u1 = (float)(300.0 * x1[0] / x1[2] + 160.0 + (unit(s) - 0.5)), w1 = (float)(300.0 * x1[1] / x1[2] + 120.0 + (unit(s) - 0.5));
                float u2 = (float)(320.0 * x / z + 150.0 + (unit(s) - 0.5)), w2 = (float)(320.0 * y / z + 130.0 + (unit(s) - 0.5));
                if (i % 5 == 0) u1 = (float)(320.0 * unit(s)), w2 = (float)(240.0 * unit(s));
                if (variant == 1 && i % 9 == 1) x2[2] = -x2[2];
                if (variant == 1 && i % 9 == 2) x1[2] = -x1[2];
                if (variant == 1 && i % 9 == 3) x1[2] = (float)t_true[2]; /* on the plane of camera 2 */
                if (variant == 2 && i == 7) x1[0] = nan;
                if (variant == 2 && i == 8) u2 = inf;
                if (variant == 5) x2[2] = -x2[2], x1[2] = -x1[2]; /* every correspondence behind */
                corr.push_back(ss_sim3opt_corr_of(x1, x2, u1, w1, u2, w2, 1.0f + 0.2f * (float)(i % 4), 1.0f + 0.2f * (float)(i % 3)));
            }
            ss_sim3_result start = {};
            const double s0 = variant == 3 ? 40.0 : 1.21;
            const double r0[9] = {1, 0.004, -0.003, -0.004, 1, 0.002, 0.003, -0.002, 1};
            for (int k = 0; k < 9; k++) start.sr12[k] = (float)(s0 * r0[k]);
            start.t12[0] = 0.11f, start.t12[1] = variant == 3 ? 30.0f : -0.04f, start.t12[2] = 0.19f;
            if (variant == 4) start.sr12[4] = nan;
            p.fix_scale = n % 2 == 0 && variant == 0 ? 0 : variant == 3;
            std::vector<uint8_t> active((size_t)n + 1);
            std::vector<double> slot((size_t)(SS_SIM3OPT_SUMS + 1) * SS_GN_SLOTS);
            ss_sim3_opt_result r;
            ss_sim3opt_pair_host(corr.data(), n, ss_sim3opt_cams_of(v1, v2, p.chi2), start, 0, p, active.data(), slot.data(), &r);
            steps += r.steps[0] + r.steps[1] + 1;
            if (r.state < 0 || r.state > 4) return printf("a state out of range\n"), 1;
            if (!result_finite(r)) return printf("n %d variant %d: a result is not finite\n", n, variant), 1;
            if ((r.model.state == 0) != (r.state == 0)) return printf("the embedded model's state is off\n"), 1;
            states[r.state]++;
            if (variant == 0 && n >= 64 && (r.state != 0 || fabs(r.s12 - s_true) > 0.02 || r.n_inliers < n / 2))
                return printf("n %d: the model was not recovered: state %d s %g, %d inliers\n", n, r.state, r.s12, r.n_inliers), 1;
            if (variant == 4 && r.state != 2) return printf("a NaN start did not end in state 2\n"), 1;
            if (variant == 5 && n >= 10 && r.state != 3 && r.state != 2) return printf("every correspondence behind: state %d\n", r.state), 1;
        }
    }
    if (states[0] < 4 || states[1] < 12) return printf("unexpected states: %d %d %d %d %d\n", states[0], states[1], states[2], states[3], states[4]), 1;
    printf("ok %ld states %d %d %d %d %d\n", steps, states[0], states[1], states[2], states[3], states[4]);
    return 0;
}
