/* The steps of the Sim3 RANSAC (csrc/ss_sim3_steps.h, the text the kernels and the host twins compile) as a stand-alone program for
 * -fsanitize=address,undefined: the draws over many counts, the model on ordinary, degenerate and non-finite triples, the twelve
 * floats and both errors of correspondences with odd coordinates, and a whole RANSAC on a small synthetic pair the way the kernels
 * run it (every hypothesis counted, then the first over the threshold).  Prints "ok <steps evaluated>". */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_sim3_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static ss_proj_view view_of(float f, float cx, float cy, float tz)
{
    ss_proj_view v = {};
    v.rcw[0] = v.rcw[4] = v.rcw[8] = 1.0f;
    v.tcw[2] = tz;
    v.fx = v.fy = f, v.cx = cx, v.cy = cy;
    v.max_x = 640.0f, v.max_y = 480.0f;
    return v;
}

int main()
{
    long steps = 0;
    uint32_t s = 12345u;
    /* the draws: distinct, in range, a permutation at n = 3 */
    const int counts[] = {3, 4, 5, 7, 64, 65, 1000, 16384};
    for (int n : counts) {
        for (int t = 0; t < 1024; t++) {
            int p[3];
            ss_sim3_draw(lcg(s), (uint32_t)(t & 7), t, n, p);
            for (int k = 0; k < 3; k++)
                if (p[k] < 0 || p[k] >= n) return printf("draw out of range: n %d t %d\n", n, t), 1;
            if (p[0] == p[1] || p[0] == p[2] || p[1] == p[2]) return printf("draw repeats: n %d t %d\n", n, t), 1;
            steps++;
        }
    }
    /* the model: random, collinear, identical, huge, NaN and infinite triples */
    const float odd[] = {0.0f, -0.0f, 1e-45f, 3e38f, -3e38f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(), 1.0f};
    for (int it = 0; it < 20000; it++) {
        float x1[9], x2[9];
        for (int k = 0; k < 9; k++) x1[k] = unit(s) * 8.0f - 4.0f, x2[k] = unit(s) * 8.0f - 4.0f;
        if (it % 7 == 1)
            for (int k = 0; k < 3; k++) x2[3 + k] = x2[k] * 2.0f, x2[6 + k] = x2[k] * 3.0f; /* collinear */
        if (it % 7 == 2)
            for (int k = 3; k < 9; k++) x1[k] = x1[k % 3], x2[k] = x2[k % 3]; /* identical */
        if (it % 7 == 3) x1[lcg(s) % 9] = odd[lcg(s) % 8], x2[lcg(s) % 9] = odd[lcg(s) % 8];
        const ss_sim3_model m = ss_sim3_model_of(x1, x2, it & 1);
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(m.sr12[k]) || !std::isfinite(m.sr21[k])) return printf("a model entry is not finite\n"), 1;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(m.t12[k]) || !std::isfinite(m.t21[k])) return printf("a model entry is not finite\n"), 1;
        if (!std::isfinite(m.s12)) return printf("a scale is not finite\n"), 1;
        steps++;
    }
    /* a pair: n correspondences under a known similarity, a third of them replaced by outliers */
    const int n = 200, max_it = 64, min_inliers = 40;
    const ss_proj_view v1 = view_of(500.0f, 320.0f, 240.0f, 0.25f), v2 = view_of(480.0f, 300.0f, 250.0f, -0.5f);
    const float scale[4] = {1.0f, 1.2f, 1.44f, 1.728f};
    std::vector<ss_sim3_corr> corr;
    for (int i = 0; i < n; i++) {
        const float z = 3.0f + 6.0f * unit(s), x = (unit(s) - 0.5f) * z, y = (unit(s) - 0.5f) * 0.7f * z;
        float p1[3] = {1.3f * (0.9553f * x + 0.2955f * z) + 0.4f, 1.3f * y - 0.2f, 1.3f * (-0.2955f * x + 0.9553f * z) + 0.6f};
        if (i % 3 == 0) p1[0] = (unit(s) - 0.5f) * 6.0f, p1[1] = (unit(s) - 0.5f) * 4.0f, p1[2] = 3.0f + 6.0f * unit(s);
        if (i == 5) p1[2] = -0.25f;                                           /* on the camera plane of keyframe 1: invz infinite */
        if (i == 7) p1[0] = std::numeric_limits<float>::quiet_NaN();
        corr.push_back(ss_sim3_corr_of(v1, v2, p1[0], p1[1], p1[2] - 0.25f, x, y, z + 0.5f, 9.21f, scale[i & 3], scale[(i >> 2) & 3]));
        steps++;
    }
    std::vector<int> count(max_it, 0);
    std::vector<ss_sim3_model> models(max_it);
    for (int t = 0; t < max_it; t++) {
        int p[3];
        ss_sim3_draw(99u, 0u, t, n, p);
        float x1[9], x2[9];
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < 3; i++) x1[3 * k + i] = corr[p[k]].x1[i], x2[3 * k + i] = corr[p[k]].x2[i];
        models[t] = ss_sim3_model_of(x1, x2, 0);
        for (int i = 0; i < n; i++) {
            const ss_sim3_corr &c = corr[i];
            const float e1 = ss_sim3_err(models[t].sr12, models[t].t12, c.x2, v1.fx, v1.fy, v1.cx, v1.cy, c.u1, c.v1);
            const float e2 = ss_sim3_err(models[t].sr21, models[t].t21, c.x1, v2.fx, v2.fy, v2.cx, v2.cy, c.u2, c.v2);
            count[t] += (e1 < c.max1 && e2 < c.max2) ? 1 : 0;
            steps += 2;
        }
    }
    int win = -1, best = 0;
    for (int t = max_it - 1; t >= 0; t--) {
        if (ss_sim3_wins(count[t], min_inliers)) win = t;
        if (count[t] > best) best = count[t];
    }
    if (ss_sim3_too_few(n, min_inliers) || !ss_sim3_too_few(2, 0) || !ss_sim3_too_few(19, 20)) return printf("too_few is wrong\n"), 1;
    if (win < 0 || best < 100 || best > 134) return printf("the pair has no winner: win %d best %d\n", win, best), 1;
    printf("ok %ld win %d best %d\n", steps, win, best);
    return 0;
}
