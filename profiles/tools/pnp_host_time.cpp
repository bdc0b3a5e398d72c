/* The PnP RANSAC rule on one host core, on the text the kernels compile (csrc/ss_pnp_steps.h): `candidates` problems of `n`
 * correspondences (40 % gross outliers, about half a pixel of noise) and `iterations` hypotheses each with `refine` refinement steps,
 * every hypothesis counted over every correspondence as the device does, then the largest count.  Prints one JSON line with the median
 * milliseconds of `reps` runs, and the share of them spent on the models alone.
 * build: g++ -O3 -std=c++17 -ffp-contract=off -I send-slam_amd/csrc -o pnp_host_time profiles/tools/pnp_host_time.cpp
 * usage: pnp_host_time [candidates] [n] [iterations] [refine] [reps] */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_pnp_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int main(int argc, char **argv)
{
    const int cands = argc > 1 ? atoi(argv[1]) : 8, n = argc > 2 ? atoi(argv[2]) : 2000, iters = argc > 3 ? atoi(argv[3]) : 300;
    const int refine = argc > 4 ? atoi(argv[4]) : 5, reps = argc > 5 ? atoi(argv[5]) : 5;
    const ss_pnp_cam cam = {500.0f, 510.0f, 318.0f, 243.0f};
    ss_pnp_params p = {};
    p.chi2 = 5.991f, p.min_ratio = 0.5f, p.lambda = 1e-6, p.min_inliers = 10, p.max_iterations = iters, p.refine_steps = refine, p.seed = 7u;
    uint32_t s = 2026u;
    std::vector<std::vector<ss_pnp_corr>> corr(cands);
    std::vector<float> scale((size_t)n, 1.0f);
    std::vector<int32_t> point((size_t)n);
    for (int i = 0; i < n; i++) point[(size_t)i] = i;
    for (auto &c : corr)
        for (int i = 0; i < n; i++) {
            const float z = 3.0f + 6.0f * unit(s), x = (unit(s) - 0.5f) * z, y = (unit(s) - 0.5f) * 0.7f * z;
            ss_pnp_corr k;
            k.X[0] = 0.9553365f * x + 0.2955202f * z + 0.4f, k.X[1] = y - 0.2f, k.X[2] = -0.2955202f * x + 0.9553365f * z + 0.6f;
            k.u = cam.fx * x / z + cam.cx + unit(s) - 0.5f, k.v = cam.fy * y / z + cam.cy + unit(s) - 0.5f;
            if (i % 5 < 2) k.u = 640.0f * unit(s), k.v = 480.0f * unit(s);
            k.max = ss_pnp_max(p.chi2, 1.0f);
            c.push_back(k);
        }
    std::vector<double> ms, model_ms;
    std::vector<uint8_t> in((size_t)n);
    long winners = 0, inliers = 0;
    double sink = 0.0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < cands; b++) {
            ss_pnp_result res;
            ss_pnp_problem_host(corr[(size_t)b].data(), scale.data(), point.data(), n, cam, p, (uint32_t)b, in.data(), &res);
            if (res.state == 0) winners++, inliers += res.n_inliers;
        }
        const auto t1 = std::chrono::steady_clock::now();
        for (int b = 0; b < cands; b++)
            for (int t = 0; t < iters; t++) sink += ss_pnp_hypothesis_host(corr[(size_t)b].data(), scale.data(), point.data(), n, cam, p, (uint32_t)b, t).tcw[2];
        const auto t2 = std::chrono::steady_clock::now();
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        model_ms.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::sort(ms.begin(), ms.end());
    std::sort(model_ms.begin(), model_ms.end());
    printf("{\"candidates\": %d, \"correspondences\": %d, \"iterations\": %d, \"refine_steps\": %d, \"reps\": %d, \"median_ms\": %.3f, "
           "\"models_alone_median_ms\": %.3f, \"winners_per_run\": %ld, \"mean_inliers\": %ld, \"check\": %.3f}\n",
           cands, n, iters, refine, reps, ms[ms.size() / 2], model_ms[model_ms.size() / 2], winners / reps, winners ? inliers / winners : 0, sink);
    return 0;
}
