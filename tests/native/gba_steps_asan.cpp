/* The steps of the global bundle adjustment (csrc/ss_gba_steps.h, the text the kernels and the host twin compile) as a stand-alone
 * program for -fsanitize=address,undefined: the block of a keyframe, the operator's terms and the table builder on random, tiny,
 * huge, NaN and infinite inputs, singular V and M, refused tables, and whole problems of 0 .. 300 keyframes the way the kernels run
 * them.  Prints "ok <steps evaluated>". */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ss_gba_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

static ss_gba_params params_of(double lambda, int iterations, int pcg)
{
    ss_gba_params p = {};
    p.chi2_mono = 5.991, p.chi2_stereo = 7.815, p.lambda = lambda, p.lambda_factor = 10.0, p.lambda_min = 1e-9, p.step_eps = 1e-10, p.pcg_tol = 1e-2;
    p.n_rounds = 2, p.iterations[0] = iterations, p.iterations[1] = 1, p.robust_rounds = 1, p.min_point_obs = 2, p.check_right = 1, p.pcg_iterations = pcg;
    return p;
}

/* a scene of n_kf keyframes along x looking down z and P points ahead of them; every keyframe sees a point with probability seen.
 * spoil: 0 none, 1 a NaN keypoint, 2 an infinite point, 3 a huge keypoint, 4 a NaN start, 5 a tiny depth */
static long whole_problem(uint32_t &s, int n_kf, int P, double seen, double lambda, int spoil, int pcg)
{
    const float scale[4] = {1.0f, 1.2f, 1.44f, 1.728f};
    ss_proj_view view = {};
    view.fx = 300.0f, view.fy = 300.0f, view.cx = 160.0f, view.cy = 120.0f, view.bf = 30.0f;
    std::vector<ss_proj_view> views((size_t)n_kf + 1, view);
    std::vector<double> start((size_t)n_kf * 12 + 1), poses((size_t)n_kf * 12 + 1), X((size_t)P * 3 + 1);
    std::vector<uint8_t> fixed((size_t)n_kf + 1), pflag((size_t)P + 1);
    std::vector<ss_gba_obs> obs;
    for (int k = 0; k < n_kf; k++) {
        double *st = &start[(size_t)k * 12];
        for (int e = 0; e < 9; e++) st[e] = (e % 4 == 0 ? 1.0 : 0.0) + (unit(s) - 0.5) * 0.02;
        st[9] = -0.3 * k + (unit(s) - 0.5) * 0.05, st[10] = (unit(s) - 0.5) * 0.05, st[11] = (unit(s) - 0.5) * 0.05;
        fixed[(size_t)k] = (k % 7 == 3 || (n_kf > 2 && k == n_kf - 1)) ? 1 : 0;
    }
    for (int i = 0; i < P; i++) {
        const double z = 4.0 + 6.0 * unit(s), x = (unit(s) - 0.5) * 0.6 * z + 0.15 * n_kf, y = (unit(s) - 0.5) * 0.5 * z;
        X[(size_t)i * 3] = (double)(float)x, X[(size_t)i * 3 + 1] = (double)(float)y, X[(size_t)i * 3 + 2] = (double)(float)z;
        pflag[(size_t)i] = i % 11 == 5 ? 2 : 0;
        if (pflag[(size_t)i] == 2) X[(size_t)i * 3] = X[(size_t)i * 3 + 1] = X[(size_t)i * 3 + 2] = 0.0;
        for (int k = 0; k < n_kf; k++) {
            if (!(unit(s) < seen)) continue;
            const double xc = x - 0.3 * k, u = 300.0 * xc / z + 160.0, v = 300.0 * y / z + 120.0;
            ss_gba_obs o = {k, i, (float)(u + (unit(s) - 0.5)), (float)(v + (unit(s) - 0.5)), (lcg(s) & 1u) ? (float)(u - 30.0 / z) : -1.0f, (int32_t)(lcg(s) % 6u) - 1};
            obs.push_back(o);
        }
    }
    /* any order: a rotation of the table */
    if (obs.size() > 3) std::rotate(obs.begin(), obs.begin() + (long)(obs.size() / 3), obs.end());
    if (spoil == 1 && !obs.empty()) obs[obs.size() / 2].u = std::numeric_limits<float>::quiet_NaN();
    if (spoil == 2 && P > 0) X[0] = std::numeric_limits<double>::infinity();
    if (spoil == 3 && !obs.empty()) obs[0].v = 3e38f;
    if (spoil == 4 && n_kf > 0) start[4] = std::numeric_limits<double>::quiet_NaN();
    if (spoil == 5 && P > 0) X[2] = 5e-324;
    const int n = (int)obs.size();
    std::vector<ss_gba_rec> rec((size_t)n + 1);
    std::vector<int32_t> pt_off((size_t)P + 1), pt_cnt((size_t)P + 1), kf_off((size_t)n_kf + 1), kf_cnt((size_t)n_kf + 1), kf_list((size_t)n + 1);
    int bad = -1;
    if (ss_gba_tables(n_kf, P, obs.data(), n, scale, 4, true, 0, rec.data(), pt_off.data(), pt_cnt.data(), kf_off.data(), kf_cnt.data(), kf_list.data(), &bad) != 0) {
        printf("a table of %d keyframes, %d points was refused at record %d\n", n_kf, P, bad);
        exit(1);
    }
    for (int m = 1; m < n; m++)
        if (rec[(size_t)m].point < rec[(size_t)m - 1].point || (rec[(size_t)m].point == rec[(size_t)m - 1].point && rec[(size_t)m].kf <= rec[(size_t)m - 1].kf)) {
            printf("record %d out of order\n", m);
            exit(1);
        }
    std::vector<ss_pose_cam> cam((size_t)n_kf + 1);
    for (int k = 0; k < n_kf; k++) cam[(size_t)k] = ss_pose_cam_of(views[(size_t)k], 5.991, 7.815);
    std::vector<uint8_t> ob((size_t)n + 1);
    ss_gba_result out;
    memset(&out, 0xff, sizeof out);
    const ss_gba_params p = params_of(lambda, 2, pcg);
    ss_gba_problem_host(n_kf, P, n, cam.data(), start.data(), fixed.data(), rec.data(), pt_off.data(), pt_cnt.data(), kf_off.data(), kf_cnt.data(), kf_list.data(), p,
                        ob.data(), X.data(), pflag.data(), poses.data(), &out);
    /* no NaN bits in any output, whatever went in */
    for (int e = 0; e < n_kf * 12; e++)
        if (!std::isfinite(poses[(size_t)e])) printf("pose entry %d of %d keyframes is not finite (spoil %d)\n", e, n_kf, spoil), exit(1);
    if (spoil != 2)
        for (int e = 0; e < P * 3; e++)
            if (!std::isfinite(X[(size_t)e])) printf("point entry %d is not finite (spoil %d)\n", e, spoil), exit(1);
    if (!std::isfinite(out.lambda) || !std::isfinite(out.cost_before) || !std::isfinite(out.cost_after) || out.state < 0 || out.state > 4 || out.reserved[0] != 0)
        printf("result of %d keyframes, %d points: lambda %g cost %g -> %g state %d\n", n_kf, P, out.lambda, out.cost_before, out.cost_after, out.state), exit(1);
    if (spoil == 4 && n_kf > 0 && out.state != 2) printf("a NaN start gave state %d\n", out.state), exit(1);
    return (long)out.steps[0] + out.steps[1] + out.pcg_iterations + 1;
}

int main()
{
    long steps = 0;
    uint32_t s = 13579u;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[] = {0.0, -0.0, 5e-324, 1e-320, 1e300, -1e300, inf, -inf, nan, 1.0, -1.0, 1e-170};
    /* the block of a keyframe on every kind of sum: M singular, negative, NaN */
    for (double v : odd)
        for (double lambda : {0.0, 1e-4, 1e300}) {
            double sum[SS_GBA_SUMS], U[SS_BA_DIAG], L[36], r[6], p[6], up[6];
            for (int e = 0; e < SS_GBA_SUMS; e++) sum[e] = e % 3 == 0 ? v : unit(s) - 0.5;
            const bool ok = ss_gba_kf_block(sum, lambda, U, L, r);
            if (ok)
                for (int a = 0; a < 6; a++)
                    if (!(L[7 * a] > 0.0)) return printf("a pivot %g passed\n", L[7 * a]), 1;
            for (int a = 0; a < 6; a++) p[a] = a == 2 ? v : unit(s);
            ss_gba_u_p(U, p, up);
            double a3[3] = {0.0, v, -v}, W[SS_BA_W];
            for (int e = 0; e < SS_BA_W; e++) W[e] = e == 7 ? v : unit(s) - 0.5;
            ss_gba_wt_p(W, p, a3);
            steps++;
        }
    /* all-zero sums: M = lambda on the diagonal */
    {
        double sum[SS_GBA_SUMS] = {}, U[SS_BA_DIAG], L[36], r[6];
        if (ss_gba_kf_block(sum, 0.0, U, L, r)) return printf("an empty block passed under lambda 0\n"), 1;
        if (!ss_gba_kf_block(sum, 1e-4, U, L, r) || L[0] != std::sqrt(1e-4) || L[6] != 0.0) return printf("an empty block under lambda 1e-4\n"), 1;
        steps += 2;
    }
    /* the terms of a block under odd observations; a singular V (a point seen once along its ray has rank 2) */
    for (double v : odd) {
        ss_proj_view view = {};
        view.fx = 300.0f, view.fy = 300.0f, view.cx = 160.0f, view.cy = 120.0f, view.bf = 30.0f;
        const ss_pose_cam cam = ss_pose_cam_of(view, 5.991, 7.815);
        double R[9], t[3];
        ss_gn_identity(R, t);
        const double X[3] = {0.1, v, 4.0};
        ss_ba_meas m = {160.0f, 120.0f, -1.0f, 1.0f};
        double V[SS_BA_V], b[3], W[SS_BA_W], L[6], term[SS_GBA_SUMS];
        const ss_pose_obs o = ss_ba_obs_of(X, m);
        if (!ss_ba_lin(o, cam, R, t, true, V, b, W)) { /* 0 * v is NaN for a v that is not finite: the depth is then not > 0 */
            if (std::isfinite(v)) return printf("an observation 4 m ahead took no part\n"), 1;
            continue;
        }
        const bool solved = ss_ba_point_factor(V, b, 0.0, L);
        if (solved && std::isfinite(v)) return printf("a rank-2 V was factored under lambda 0\n"), 1;
        ss_gba_block_terms(o, cam, R, t, false, ss_ba_point_factor(V, b, 1e-4, L), W, L, b, term);
        steps++;
    }
    /* refused tables */
    {
        const float scale[2] = {1.0f, 1.2f};
        ss_gba_obs obs[3] = {{0, 0, 1.0f, 1.0f, -1.0f, 0}, {1, 0, 1.0f, 1.0f, -1.0f, 0}, {0, 0, 2.0f, 2.0f, -1.0f, 1}};
        ss_gba_rec rec[3];
        int32_t pt_off[1], pt_cnt[1], kf_off[2], kf_cnt[2], kf_list[3];
        int bad = -1;
        if (ss_gba_tables(2, 1, obs, 3, scale, 2, false, 0, rec, pt_off, pt_cnt, kf_off, kf_cnt, kf_list, &bad) != 3 || bad != 2) return printf("a pair twice: record %d\n", bad), 1;
        obs[2].kf = 2;
        if (ss_gba_tables(2, 1, obs, 3, scale, 2, false, 0, rec, pt_off, pt_cnt, kf_off, kf_cnt, kf_list, &bad) != 1 || bad != 2) return printf("kf 2 of 2: record %d\n", bad), 1;
        obs[2].kf = 1, obs[1].point = -1;
        if (ss_gba_tables(2, 1, obs, 3, scale, 2, false, 0, rec, pt_off, pt_cnt, kf_off, kf_cnt, kf_list, &bad) != 2 || bad != 1) return printf("point -1: record %d\n", bad), 1;
        if (ss_gba_tables(2, 1, obs, 0, scale, 2, false, 0, rec, pt_off, pt_cnt, kf_off, kf_cnt, kf_list, &bad) != 0 || pt_cnt[0] != 0) return printf("an empty table\n"), 1;
        steps += 4;
    }
    /* whole problems: 0 .. 300 keyframes, 0 .. 600 points, every spoil, lambda 0 included */
    const int kfs[] = {0, 1, 2, 3, 7, 42, 43, 64, 65, 300};
    for (int n_kf : kfs)
        for (int P : {0, 1, 50, 600}) {
            if (n_kf == 300 && P == 600) continue;
            for (int spoil = 0; spoil < 6; spoil++)
                steps += whole_problem(s, n_kf, P, n_kf > 40 ? 6.0 / n_kf : 0.7, spoil == 3 ? 0.0 : 1e-4, spoil, n_kf > 100 ? 4 : 12);
        }
    steps += whole_problem(s, 300, 600, 0.02, 1e-4, 0, 8);
    printf("ok %ld\n", steps);
    return 0;
}
