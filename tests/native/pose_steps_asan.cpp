/* The steps of the pose-only optimisation (csrc/ss_pose_steps.h, the text the kernels and the host twin compile) as a stand-alone
 * program for -fsanitize=address,undefined: the start rotation on ordinary, sheared, degenerate and non-finite poses, the series of
 * the exponential over q in 0 .. pi^2 and beyond, the solve on definite, singular and non-finite systems, the terms and chi-squares of
 * observations with odd coordinates, and whole frames the way the kernels run them (256 slot sums, the tree, every thread's solve).
 * Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_pose_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

static ss_proj_view view_of(float f, float cx, float cy, float bf)
{
    ss_proj_view v = {};
    v.rcw[0] = v.rcw[4] = v.rcw[8] = 1.0f;
    v.fx = v.fy = f, v.cx = cx, v.cy = cy, v.bf = bf;
    v.max_x = 640.0f, v.max_y = 480.0f;
    return v;
}

/* one frame through the header's host loop (ss_pose_frame_host, what ss_pose_opt_host runs); returns the state and counts the steps taken */
static int frame(const std::vector<ss_pose_obs> &obs, const ss_pose_cam &cam, const double *start, double R[9], double t[3], int *n_in, long *steps)
{
    const int n = (int)obs.size();
    ss_pose_opt_params p = {};
    p.chi2_mono = cam.chi2_mono, p.chi2_stereo = cam.chi2_stereo, p.lambda = 1e-6, p.step_eps = 1e-10;
    p.n_rounds = 4, p.iterations = 10, p.robust_rounds = 2, p.min_obs = 3;
    std::vector<uint8_t> active((size_t)n + 1);
    std::vector<double> slot((size_t)(SS_POSE_SUMS + 1) * SS_GN_SLOTS);
    ss_pose_result r;
    ss_pose_frame_host(obs.data(), n, cam, start, p, active.data(), slot.data(), &r);
    for (int k = 0; k < 9; k++) R[k] = r.rcw[k];
    for (int k = 0; k < 3; k++) t[k] = r.tcw[k];
    *n_in = r.n_inliers;
    for (int k = 0; k < 8; k++) *steps += r.steps[k];
    return r.state;
}

int main()
{
    long steps = 0;
    uint32_t s = 4321u;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    /* the start rotation: finite always, orthonormal for ordinary rows */
    const double odd[] = {0.0, -0.0, 1e-320, 1e300, -1e300, inf, nan, 1.0};
    for (int it = 0; it < 20000; it++) {
        double st[12], R[9], t[3];
        for (double &v : st) v = unit(s) * 2.0 - 1.0;
        if (it % 5 == 1) st[lcg(s) % 12] = odd[lcg(s) % 8];
        if (it % 5 == 2)
            for (int k = 0; k < 3; k++) st[3 + k] = 2.0 * st[k]; /* the second row along the first */
        const bool ok = ss_pose_start(st, R, t);
        if (!ss_gn_all_finite(R, t)) return printf("a start pose is not finite\n"), 1;
        if (ok && it % 5 != 1 && it % 5 != 2) { /* rows that are parallel, tiny or huge give a finite matrix, not a rotation */
            const double d = (R[0] * R[3] + R[1] * R[4]) + R[2] * R[5], n = (R[6] * R[6] + R[7] * R[7]) + R[8] * R[8];
            if (fabs(d) > 1e-9 || fabs(n - 1.0) > 1e-9) return printf("a start rotation is not orthonormal: %g %g\n", d, n), 1;
        }
        steps++;
    }
    /* the exponential: a rotation for q <= pi^2, refused above */
    for (int it = 0; it < 20000; it++) {
        double d[6], dR[9], dt[3];
        const double len = it % 3 == 0 ? 3.2 * unit(s) : it % 3 == 1 ? 1e-9 * unit(s) : 0.3 * unit(s);
        double a[3] = {unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5};
        const double an = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + 1e-300;
        for (int k = 0; k < 3; k++) d[k] = a[k] / an * len, d[3 + k] = unit(s) - 0.5;
        const bool ok = ss_pose_exp(d, dR, dt);
        const double q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        if (ok != !(q > SS_POSE_PI2)) return printf("the step-size test is wrong at q = %g\n", q), 1;
        if (ok) {
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    const double e = (dR[3 * i] * dR[3 * j] + dR[3 * i + 1] * dR[3 * j + 1]) + dR[3 * i + 2] * dR[3 * j + 2];
                    if (fabs(e - (i == j ? 1.0 : 0.0)) > 1e-13) return printf("exp is no rotation at q = %g: %g\n", q, e), 1;
                }
        }
        steps++;
    }
    /* the solve: the residual of a definite system; singular and non-finite ones are refused or stay defined */
    for (int it = 0; it < 5000; it++) {
        double J[8][6], sum[SS_POSE_SUMS], delta[6];
        for (auto &row : J)
            for (double &v : row) v = unit(s) - 0.5;
        int k = 0;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++) {
                if (a == 3 && b == 4) continue;
                double h = 0.0;
                for (auto &row : J) h += row[a] * row[b];
                sum[k++] = it % 7 == 3 ? 0.0 : h;
            }
        for (int a = 0; a < 6; a++) sum[20 + a] = unit(s) - 0.5;
        if (it % 7 == 4) sum[lcg(s) % SS_POSE_SUMS] = odd[lcg(s) % 8];
        if (it % 7 == 5) sum[0] = -1.0;
        const bool ok = ss_pose_solve(sum, it % 7 == 3 ? 0.0 : 1e-6, delta);
        if ((it % 7 == 3 || it % 7 == 5) && ok) return printf("a system that is not definite was solved\n"), 1;
        steps++;
    }
    /* frames: n observations of points under a known pose, a fifth of them gross outliers, some behind the camera or not finite */
    const ss_proj_view v = view_of(300.0f, 160.0f, 120.0f, 30.0f);
    const ss_pose_cam cam = ss_pose_cam_of(v, 5.991, 7.815);
    const int counts[] = {0, 2, 3, 64, 65, 257, 1000};
    int states[5] = {0, 0, 0, 0, 0};
    for (int n : counts) {
        for (int variant = 0; variant < 4; variant++) {
            std::vector<ss_pose_obs> obs;
            for (int i = 0; i < n; i++) {
                const double z = 2.0 + 6.0 * unit(s), x = (unit(s) - 0.5) * 0.9 * z, y = (unit(s) - 0.5) * 0.6 * z;
                float u = (float)(300.0 * (x + 0.05) / z + 160.0 + (unit(s) - 0.5)), w = (float)(300.0 * (y - 0.02) / z + 120.0 + (unit(s) - 0.5));
                if (i % 5 == 0) u = (float)(320.0 * unit(s)), w = (float)(240.0 * unit(s));
                float X = (float)x, Z = (float)z;
                if (variant == 1 && i % 9 == 1) Z = -Z;
                if (variant == 2 && i == 7) X = std::numeric_limits<float>::quiet_NaN();
                if (variant == 2 && i == 8) u = std::numeric_limits<float>::infinity();
                const float ur = ss_pose_stored_right(variant != 3, true, i % 2 ? u - (float)(30.0 / z) : -1.0f);
                obs.push_back(ss_pose_obs_of(X, (float)y, Z, u, w, ur, 1.0f + 0.2f * (float)(i % 4)));
            }
            const double start[12] = {1, 0.01, -0.02, -0.01, 1, 0.015, 0.02, -0.015, 1, variant == 3 ? 40.0 : 0.0, 0, variant == 3 ? -30.0 : 0.0};
            double R[9], t[3];
            int n_in = 0;
            const int st = frame(obs, cam, start, R, t, &n_in, &steps);
            if (st < 0 || st > 4) return printf("a state out of range\n"), 1;
            states[st]++;
            if (st == 0 && variant == 0 && (fabs(t[0] - 0.05) > 0.01 || fabs(t[1] + 0.02) > 0.01 || n_in < n / 2))
                return printf("n %d: the pose was not recovered: t %g %g %g, %d inliers\n", n, t[0], t[1], t[2], n_in), 1;
        }
    }
    if (states[0] < 8 || states[1] != 8) return printf("unexpected states: %d %d %d %d %d\n", states[0], states[1], states[2], states[3], states[4]), 1;
    printf("ok %ld states %d %d %d %d %d\n", steps, states[0], states[1], states[2], states[3], states[4]);
    return 0;
}
