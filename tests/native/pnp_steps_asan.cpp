/* The steps of the PnP RANSAC (csrc/ss_pnp_steps.h, the text the kernels and the host twins compile) as a stand-alone program for
 * -fsanitize=address,undefined: the draws over many counts, the model on ordinary, degenerate and non-finite sextuples at several
 * refinement counts, the test of correspondences with odd coordinates, and a whole RANSAC of 200 correspondences the way the kernels
 * run it (every hypothesis counted, the largest count, the winner once more).  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_pnp_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int main()
{
    long steps = 0;
    uint32_t s = 4321u;
    /* the draws: distinct, in range, a permutation at n = 6 */
    const int counts[] = {6, 7, 8, 9, 64, 65, 1000, 16384};
    for (int n : counts) {
        for (int t = 0; t < 1024; t++) {
            int p[SS_PNP_DRAWS];
            ss_pnp_draw(lcg(s), (uint32_t)(t & 7), t, n, p);
            for (int k = 0; k < SS_PNP_DRAWS; k++) {
                if (p[k] < 0 || p[k] >= n) return printf("draw out of range: n %d t %d\n", n, t), 1;
                for (int e = 0; e < k; e++)
                    if (p[e] == p[k]) return printf("draw repeats: n %d t %d\n", n, t), 1;
            }
            steps++;
        }
    }
    /* the model: random, coplanar, collinear, identical, repeated rows, huge, NaN and infinite sextuples */
    const ss_pnp_cam cam = {500.0f, 510.0f, 318.0f, 243.0f};
    const float scale[4] = {1.0f, 1.2f, 1.44f, 1.728f};
    const float odd[] = {0.0f, -0.0f, 1e-45f, 3e38f, -3e38f, 1e30f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    long zero_models = 0;
    for (int it = 0; it < 20000; it++) {
        float X[18], uv[12], sc[6];
        int row[6];
        for (int k = 0; k < 6; k++) {
            const float z = 3.0f + 6.0f * unit(s), x = (unit(s) - 0.5f) * z, y = (unit(s) - 0.5f) * 0.7f * z;
            X[3 * k] = x + 0.3f, X[3 * k + 1] = y - 0.2f, X[3 * k + 2] = z + 0.5f;
            uv[2 * k] = cam.fx * x / z + cam.cx + unit(s) - 0.5f, uv[2 * k + 1] = cam.fy * y / z + cam.cy + unit(s) - 0.5f;
            sc[k] = scale[lcg(s) & 3u], row[k] = k * 3;
        }
        if (it % 9 == 1)
            for (int k = 0; k < 6; k++) X[3 * k + 2] = 6.0f; /* coplanar */
        if (it % 9 == 2)
            for (int k = 1; k < 6; k++)
                for (int c = 0; c < 3; c++) X[3 * k + c] = X[c] * (1.0f + 0.1f * (float)k); /* collinear */
        if (it % 9 == 3)
            for (int k = 3; k < 18; k++) X[k] = X[k % 3]; /* identical */
        if (it % 9 == 4) row[4] = row[1];
        if (it % 9 == 5) X[lcg(s) % 18] = odd[lcg(s) % 8], uv[lcg(s) % 12] = odd[lcg(s) % 8];
        if (it % 9 == 6) X[3] = X[4] = X[5] = 0.0f; /* a point at the origin */
        if (it % 9 == 7) sc[lcg(s) % 6] = odd[lcg(s) % 8];
        ss_pnp_work_host w;
        const int refine = it % 3 == 0 ? 0 : it % 3 == 1 ? 5 : SS_PNP_MAX_REFINE;
        const ss_pnp_model m = ss_pnp_model_of(X, uv, sc, row, cam, 1e-6, refine, w);
        bool zero = true;
        for (int k = 0; k < 9; k++) {
            if (!std::isfinite(m.rcw[k]) || !std::isfinite(m.rf[k])) return printf("a model entry is not finite\n"), 1;
            zero = zero && m.rcw[k] == 0.0 && m.rf[k] == 0.0f;
        }
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(m.tcw[k]) || !std::isfinite(m.tf[k])) return printf("a model entry is not finite\n"), 1;
        }
        if (it % 9 == 4 && !zero) return printf("a repeated point row gave a model\n"), 1;
        zero_models += zero ? 1 : 0;
        steps++;
    }
    /* a problem: n correspondences under a known pose, 40 % of them gross outliers, a few with odd numbers */
    const int n = 200;
    ss_pnp_params p = {};
    p.chi2 = 5.991f, p.min_ratio = 0.5f, p.lambda = 1e-6, p.min_inliers = 10, p.max_iterations = 64, p.refine_steps = 5, p.seed = 99u;
    std::vector<ss_pnp_corr> corr;
    std::vector<float> sc;
    std::vector<int32_t> point;
    for (int i = 0; i < n; i++) {
        const float z = 3.0f + 6.0f * unit(s), x = (unit(s) - 0.5f) * z, y = (unit(s) - 0.5f) * 0.7f * z;
        ss_pnp_corr c;
        /* the world is the camera turned by 0.3 rad about y and moved */
        c.X[0] = 0.9553f * x + 0.2955f * z + 0.4f, c.X[1] = y - 0.2f, c.X[2] = -0.2955f * x + 0.9553f * z + 0.6f;
        c.u = cam.fx * x / z + cam.cx + unit(s) - 0.5f, c.v = cam.fy * y / z + cam.cy + unit(s) - 0.5f;
        if (i % 5 < 2) c.u = 640.0f * unit(s), c.v = 480.0f * unit(s);
        if (i == 5) c.X[2] = std::numeric_limits<float>::quiet_NaN();
        if (i == 7) c.u = std::numeric_limits<float>::infinity();
        if (i == 9) c.X[0] = 1e30f;
        const float sl = scale[i & 3];
        c.max = ss_pnp_max(p.chi2, sl);
        corr.push_back(c), sc.push_back(sl), point.push_back(i == 11 ? 10 : i);
        steps++;
    }
    std::vector<uint8_t> in((size_t)n);
    ss_pnp_result res;
    ss_pnp_problem_host(corr.data(), sc.data(), point.data(), n, cam, p, 3u, in.data(), &res);
    steps += (long)p.max_iterations * n;
    int flagged = 0;
    for (int i = 0; i < n; i++) flagged += in[(size_t)i];
    for (int i = 0; i < n; i++) {
        float e;
        const float r[9] = {(float)res.rcw[0], (float)res.rcw[1], (float)res.rcw[2], (float)res.rcw[3], (float)res.rcw[4],
                            (float)res.rcw[5], (float)res.rcw[6], (float)res.rcw[7], (float)res.rcw[8]};
        const float t[3] = {(float)res.tcw[0], (float)res.tcw[1], (float)res.tcw[2]};
        if ((ss_pnp_test(r, t, corr[(size_t)i], cam, &e) == 0) != (in[(size_t)i] != 0)) return printf("flag %d is not the test's\n", i), 1;
        steps++;
    }
    if (ss_pnp_too_few(n, p.min_inliers) || !ss_pnp_too_few(5, 0) || !ss_pnp_too_few(19, 20) || ss_pnp_too_few(6, 6)) return printf("too_few is wrong\n"), 1;
    if (ss_pnp_key_t(ss_pnp_key(7, 1023)) != 1023 || ss_pnp_key_count(ss_pnp_key(16384, 0)) != 16384 || ss_pnp_key(3, 5) <= ss_pnp_key(3, 6) ||
        ss_pnp_key(4, 1023) <= ss_pnp_key(3, 0))
        return printf("the key is wrong\n"), 1;
    if (!ss_pnp_wins(10, 20, 10, 0.5f) || ss_pnp_wins(9, 20, 10, 0.0f) || ss_pnp_wins(10, 21, 10, 0.5f)) return printf("wins is wrong\n"), 1;
    if (res.state != 0 || res.n_inliers != flagged || res.n_inliers != res.best_inliers || flagged < 100 || flagged > 120)
        return printf("the problem has no winner: state %d inliers %d best %d\n", res.state, res.n_inliers, res.best_inliers), 1;
    printf("ok %ld zero_models %ld winner %d inliers %d\n", steps, zero_models, res.iteration, res.n_inliers);
    return 0;
}
