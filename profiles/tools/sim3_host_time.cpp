/* The Sim3 RANSAC rule on one host core, on the text the kernels compile (csrc/ss_sim3_steps.h): `pairs` pairs of `n`
 * correspondences (40 % gross outliers) and `iterations` hypotheses each, every hypothesis counted over every correspondence as the
 * device does, then the first over the threshold.  Prints one JSON line with the median milliseconds of `reps` runs.
 * build: g++ -O3 -std=c++17 -ffp-contract=off -I send-slam_amd/csrc -o sim3_host_time profiles/tools/sim3_host_time.cpp
 * usage: sim3_host_time [pairs] [n] [iterations] [reps] */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_sim3_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int main(int argc, char **argv)
{
    const int pairs = argc > 1 ? atoi(argv[1]) : 8, n = argc > 2 ? atoi(argv[2]) : 2000, iters = argc > 3 ? atoi(argv[3]) : 300;
    const int reps = argc > 4 ? atoi(argv[4]) : 5, min_inliers = n / 4;
    ss_proj_view v1 = {}, v2 = {};
    v1.rcw[0] = v1.rcw[4] = v1.rcw[8] = v2.rcw[0] = v2.rcw[4] = v2.rcw[8] = 1.0f;
    v1.fx = v1.fy = v2.fx = v2.fy = 500.0f, v1.cx = v2.cx = 320.0f, v1.cy = v2.cy = 240.0f;
    uint32_t s = 2024u;
    std::vector<std::vector<ss_sim3_corr>> corr(pairs);
    for (auto &c : corr)
        for (int i = 0; i < n; i++) {
            const float z = 3.0f + 6.0f * unit(s), x = (unit(s) - 0.5f) * z, y = (unit(s) - 0.5f) * 0.7f * z;
            float p1[3] = {1.3f * (0.9553365f * x + 0.2955202f * z) + 0.4f, 1.3f * y - 0.2f, 1.3f * (-0.2955202f * x + 0.9553365f * z) + 0.6f};
            if (i % 5 < 2) p1[0] = (unit(s) - 0.5f) * 6.0f, p1[1] = (unit(s) - 0.5f) * 4.0f, p1[2] = 3.0f + 6.0f * unit(s);
            c.push_back(ss_sim3_corr_of(v1, v2, p1[0], p1[1], p1[2], x, y, z, 9.21f, 1.0f, 1.0f));
        }
    std::vector<double> ms;
    long winners = 0, inliers = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < pairs; b++) {
            const std::vector<ss_sim3_corr> &c = corr[b];
            std::vector<int> count(iters, 0);
            int win = -1;
            for (int t = 0; t < iters; t++) {
                int p[3];
                ss_sim3_draw(7u, (uint32_t)b, t, n, p);
                float x1[9], x2[9];
                for (int k = 0; k < 3; k++)
                    for (int i = 0; i < 3; i++) x1[3 * k + i] = c[p[k]].x1[i], x2[3 * k + i] = c[p[k]].x2[i];
                const ss_sim3_model m = ss_sim3_model_of(x1, x2, 0);
                int cnt = 0;
                for (int i = 0; i < n; i++) {
                    const float e1 = ss_sim3_err(m.sr12, m.t12, c[i].x2, v1.fx, v1.fy, v1.cx, v1.cy, c[i].u1, c[i].v1);
                    const float e2 = ss_sim3_err(m.sr21, m.t21, c[i].x1, v2.fx, v2.fy, v2.cx, v2.cy, c[i].u2, c[i].v2);
                    cnt += (e1 < c[i].max1 && e2 < c[i].max2) ? 1 : 0;
                }
                count[t] = cnt;
            }
            for (int t = iters - 1; t >= 0; t--)
                if (ss_sim3_wins(count[t], min_inliers)) win = t;
            if (win >= 0) winners++, inliers += count[win];
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"pairs\": %d, \"correspondences\": %d, \"iterations\": %d, \"reps\": %d, \"median_ms\": %.3f, \"winners_per_run\": %ld, \"mean_inliers\": %ld}\n",
           pairs, n, iters, reps, ms[ms.size() / 2], winners / reps, winners ? inliers / winners : 0);
    return 0;
}
