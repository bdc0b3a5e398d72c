/* The host twin of the Sim3 refinement (csrc/ss_sim3opt_steps.h, the loop ss_sim3_opt_host runs) on one host core, on the pairs
 * profiles/tools/time_sim3opt.py wrote: the same correspondences and start models the device call refines.  The file: int32 pairs,
 * int32 n; per pair one ss_sim3_result (the start), two ss_proj_view, then n x (X1 X2 u1 v1 u2 v2 s1 s2) floats.  Prints one JSON
 * line with the median milliseconds of `reps` runs over all pairs.
 * build: g++ -O3 -std=c++17 -ffp-contract=off -I send-slam_amd/csrc -o sim3opt_host_time profiles/tools/sim3opt_host_time.cpp
 * usage: sim3opt_host_time pairs.bin [reps] */
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_sim3opt_steps.h"

int main(int argc, char **argv)
{
    if (argc < 2) return fprintf(stderr, "usage: sim3opt_host_time pairs.bin [reps]\n"), 2;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    FILE *f = fopen(argv[1], "rb");
    int32_t head[2];
    if (!f || fread(head, sizeof(head), 1, f) != 1 || head[0] < 1 || head[1] < 0) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const int pairs = head[0], n = head[1];
    std::vector<ss_sim3_result> start((size_t)pairs);
    std::vector<ss_proj_view> views((size_t)pairs * 2);
    std::vector<ss_sim3opt_corr> corr((size_t)pairs * n);
    for (int b = 0; b < pairs; b++) {
        std::vector<float> rec((size_t)n * 12);
        if (fread(&start[(size_t)b], sizeof(ss_sim3_result), 1, f) != 1 || fread(&views[(size_t)b * 2], sizeof(ss_proj_view), 2, f) != 2 ||
            fread(rec.data(), sizeof(float), rec.size(), f) != rec.size())
            return fprintf(stderr, "%s is short\n", argv[1]), 2;
        for (int i = 0; i < n; i++) {
            const float *r = &rec[(size_t)i * 12];
            corr[(size_t)b * n + i] = ss_sim3opt_corr_of(r, r + 3, r[6], r[7], r[8], r[9], r[10], r[11]);
        }
    }
    fclose(f);
    ss_sim3_opt_params p = {};
    p.chi2 = 10.0, p.lambda = 1e-6, p.step_eps = 1e-10, p.iterations0 = 5, p.iterations_more = 10, p.iterations_same = 5, p.min_corr = 10, p.min_inliers = 10;
    std::vector<uint8_t> active((size_t)n + 1);
    std::vector<double> slot((size_t)(SS_SIM3OPT_SUMS + 1) * SS_GN_SLOTS);
    std::vector<double> ms;
    long inliers = 0, failed = 0, steps = 0;
    for (int r = 0; r < reps; r++) {
        inliers = failed = steps = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < pairs; b++) {
            ss_sim3_opt_result out;
            ss_sim3opt_pair_host(&corr[(size_t)b * n], n, ss_sim3opt_cams_of(views[(size_t)b * 2], views[(size_t)b * 2 + 1], p.chi2), start[(size_t)b], 0, p,
                                 active.data(), slot.data(), &out);
            if (out.state != 0) failed++;
            inliers += out.n_inliers, steps += out.steps[0] + out.steps[1];
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"pairs\": %d, \"correspondences\": %d, \"reps\": %d, \"median_ms\": %.4f, \"ms_per_pair\": %.5f, \"failed\": %ld, \"mean_inliers\": %ld, \"mean_steps\": %.2f}\n",
           pairs, n, reps, ms[ms.size() / 2], ms[ms.size() / 2] / pairs, failed, inliers / pairs, (double)steps / pairs);
    return 0;
}
