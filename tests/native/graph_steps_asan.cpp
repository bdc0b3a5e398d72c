/* The steps of the essential-graph optimisation (csrc/ss_graph_steps.h, the text the kernels and the host twin compile) as a
 * stand-alone program for -fsanitize=address,undefined: both series, the logarithm, the retraction and the Jacobian columns on random,
 * tiny, huge, NaN and infinite inputs, the round trip of the logarithm through the retraction, the incidence lists, and whole problems
 * of 0 .. 300 keyframes the way the kernels run them.  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ss_graph_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

static void random_sim3(uint32_t &s, double spread, double *S)
{
    const double d[7] = {(unit(s) - 0.5) * spread, (unit(s) - 0.5) * spread, (unit(s) - 0.5) * spread, (unit(s) - 0.5) * 4.0, (unit(s) - 0.5) * 4.0,
                         (unit(s) - 0.5) * 4.0, (unit(s) - 0.5) * 0.5};
    double t[3];
    ss_gn_identity(S, t);
    S[9] = S[10] = S[11] = 0.0, S[12] = 1.0;
    (void)ss_graph_retract(d, false, S);
}

static ss_graph_params params_of(double lambda, int iterations, int pcg, bool fix)
{
    ss_graph_params p = {};
    p.lambda = lambda, p.lambda_factor = 10.0, p.lambda_min = 0.0, p.pcg_tol = 1e-3;
    p.iterations = iterations, p.pcg_iterations = pcg, p.fix_scale = fix ? 1 : 0;
    return p;
}

int main()
{
    long steps = 0;
    uint32_t s = 24680u;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[] = {0.0, -0.0, 5e-324, 1e-320, 1e300, -1e300, inf, -inf, nan, 1.0, -1.0, 1e-170};
    /* the series: every pair of odd values, then random ones against libm */
    for (double y : odd)
        for (double x : odd) {
            const double a = ss_graph_atan2(y, x);
            const bool in_range = y >= 0.0 && std::isfinite(y) && std::isfinite(x);
            if (in_range != !std::isnan(a)) return printf("atan2(%g, %g) = %g\n", y, x, a), 1;
            /* at the origin a negative zero counts as zero here: libm answers pi */
            if (in_range && !(y == 0.0 && x == 0.0) && !(std::fabs(a - std::atan2(std::fabs(y), x)) <= 4e-16 * (1.0 + a))) return printf("atan2(%g, %g) = %.17g\n", y, x, a), 1;
            steps++;
        }
    for (double x : odd) {
        const double l = ss_graph_ln(x);
        const bool in_range = x > 0.0 && std::isfinite(x);
        if (in_range != !std::isnan(l)) return printf("ln(%g) = %g\n", x, l), 1;
        if (in_range && !(std::fabs(l - std::log(x)) <= 4e-16 * (1.0 + std::fabs(l)))) return printf("ln(%g) = %.17g\n", x, l), 1;
        steps++;
    }
    for (int it = 0; it < 200000; it++) {
        const double y = unit(s) * std::pow(10.0, 16.0 * unit(s) - 8.0), x = (unit(s) - 0.5) * std::pow(10.0, 16.0 * unit(s) - 8.0);
        const double a = ss_graph_atan2(y, x), l = ss_graph_ln(y + 1e-300);
        if (!(std::fabs(a - std::atan2(y, x)) <= 1e-15 * a)) return printf("atan2(%.17g, %.17g) = %.17g\n", y, x, a), 1;
        if (!(std::fabs(l - std::log(y + 1e-300)) <= 1e-15 * std::fabs(l) + 1e-300)) return printf("ln(%.17g) = %.17g\n", y, l), 1;
        steps++;
    }
    /* the logarithm: its round trip through the retraction from the identity (rotation and scale parts), rotations next to pi
     * included; odd entries give no fault */
    for (int it = 0; it < 20000; it++) {
        double d[7], S[13], t[3], e[7];
        const double len = it % 4 == 0 ? 3.14159 : it % 4 == 1 ? 1e-9 : 2.0 * unit(s);
        double w[3] = {unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5};
        const double n = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + 1e-12;
        for (int k = 0; k < 3; k++) d[k] = w[k] / n * len, d[3 + k] = unit(s) - 0.5;
        d[6] = unit(s) - 0.5;
        ss_gn_identity(S, t);
        S[9] = S[10] = S[11] = 0.0, S[12] = 1.0;
        if (!ss_graph_retract(d, false, S)) return printf("a step below pi was refused\n"), 1;
        ss_graph_log(S, e);
        const double tol = it % 4 == 0 ? 1e-6 : 1e-12; /* next to pi the axis is ill-conditioned */
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(e[k] - d[k]) <= tol)) return printf("log(exp(omega)) differs: %g %g (length %g)\n", e[k], d[k], len), 1;
        if (!(std::fabs(e[6] - d[6]) <= 1e-15)) return printf("ln(exp(sigma)) differs\n"), 1;
        if (it % 5 == 0) {
            S[lcg(s) % 13] = odd[lcg(s) % 12];
            ss_graph_log(S, e);
        }
        steps++;
    }
    /* a rotation of exactly pi about each axis and about a diagonal: defined, of length pi */
    {
        const double R[4][9] = {{1, 0, 0, 0, -1, 0, 0, 0, -1}, {-1, 0, 0, 0, 1, 0, 0, 0, -1}, {-1, 0, 0, 0, -1, 0, 0, 0, 1}, {0, 1, 0, 1, 0, 0, 0, 0, -1}};
        for (const double *r : R) {
            double S[13] = {}, e[7];
            for (int k = 0; k < 9; k++) S[k] = r[k];
            S[12] = 1.0;
            ss_graph_log(S, e);
            const double len = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            if (!(std::fabs(len - 3.141592653589793) <= 1e-15)) return printf("log of a half turn has length %.17g\n", len), 1;
            steps++;
        }
    }
    /* the columns of an edge: finite on finite inputs, +0.0 where the rule says so, no fault on odd ones */
    for (int it = 0; it < 3000; it++) {
        double Ni[13], Nj[13], Si[13], Sj[13], M[13], col[7];
        random_sim3(s, 1.5, Ni), random_sim3(s, 1.5, Nj), random_sim3(s, 1.5, Si), random_sim3(s, 1.5, Sj);
        if (it % 3 == 1) Si[lcg(s) % 13] = odd[lcg(s) % 12];
        if (it % 3 == 2) Nj[lcg(s) % 13] = odd[lcg(s) % 12];
        ss_graph_measure(Ni, Nj, M);
        const bool fix = it % 2 == 1;
        for (int c = 0; c < 14; c++) {
            const bool zero = (fix && c % 7 == 6) || (it % 7 == 0 && c < 7);
            ss_graph_column(M, Si, Sj, c / 7, c % 7, fix, zero, col);
            for (int r = 0; r < 7; r++) {
                if (zero && !(col[r] == 0.0 && !std::signbit(col[r]))) return printf("a zero column is not +0.0\n"), 1;
                if (it % 3 == 0 && !std::isfinite(col[r])) return printf("a column of a finite edge is not finite\n"), 1;
            }
            steps++;
        }
    }
    /* whole problems: rings with chords of 0 .. 300 keyframes; a consistent one converges; odd entries end in state 2 or run through */
    const int sizes[] = {0, 1, 2, 3, 36, 37, 100, 257, 300};
    for (int n_kf : sizes) {
        for (int variant = 0; variant < 3; variant++) {
            const size_t K = (size_t)n_kf;
            std::vector<double> nc(K * 13 + 1), start(K * 13 + 1), sim3(K * 13 + 1);
            std::vector<uint8_t> fixed(K + 1, 0);
            std::vector<int32_t> edges;
            for (int v = 0; v < n_kf; v++) {
                random_sim3(s, 1.0, &nc[13 * (size_t)v]);
                memcpy(&start[13 * (size_t)v], &nc[13 * (size_t)v], 13 * sizeof(double));
                if (v > 0) {
                    const double d[7] = {0.01 * (unit(s) - 0.5), 0.01 * (unit(s) - 0.5), 0.01 * (unit(s) - 0.5), 0.02 * (unit(s) - 0.5), 0.02 * (unit(s) - 0.5),
                                         0.02 * (unit(s) - 0.5), variant == 1 ? 0.0 : 0.01 * (unit(s) - 0.5)};
                    (void)ss_graph_retract(d, variant == 1, &start[13 * (size_t)v]);
                }
            }
            if (n_kf > 0) fixed[0] = 1;
            for (int v = 0; v + 1 < n_kf; v++) edges.push_back(v), edges.push_back(v + 1);
            if (n_kf > 2) edges.push_back(n_kf - 1), edges.push_back(0);
            for (int v = 0; v + 7 < n_kf; v += 5) edges.push_back(v + 7), edges.push_back(v);
            const int n_edges = (int)edges.size() / 2;
            edges.push_back(0);
            if (variant == 2 && n_kf > 1) start[13 * (size_t)(lcg(s) % K) + lcg(s) % 13] = odd[lcg(s) % 12];
            const ss_graph_params p = params_of(variant == 0 ? 1e-16 : 1e-6, n_kf > 100 ? 3 : 8, n_kf > 100 ? 16 : 64, variant == 1);
            ss_graph_result r;
            memset(&r, 0xff, sizeof r);
            ss_graph_problem_host(n_kf, n_edges, nc.data(), start.data(), fixed.data(), edges.data(), p, sim3.data(), &r);
            if (n_kf < 2 && r.state != 1) return printf("%d keyframes: state %d\n", n_kf, r.state), 1;
            if (variant != 2 && n_kf >= 2) {
                if (r.state != 0 || r.accepted < 1 || !(r.cost_after < r.cost_before)) return printf("%d keyframes: state %d, %d accepted, cost %g -> %g\n", n_kf, r.state, r.accepted, r.cost_before, r.cost_after), 1;
                if (n_kf <= 100 && !(r.cost_after < 1e-6 * r.cost_before)) return printf("%d keyframes: the cost went %g -> %g\n", n_kf, r.cost_before, r.cost_after), 1;
            }
            if (r.state == 2 || r.state == 1)
                if (memcmp(sim3.data(), start.data(), K * 13 * sizeof(double)) != 0) return printf("a problem that did not run moved\n"), 1;
            steps += r.steps + 1;
        }
    }
    printf("ok %ld\n", steps);
    return 0;
}
