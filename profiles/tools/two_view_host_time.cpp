/* The two-view initialisation on one host core, on the text the kernels compile (csrc/ss_two_view_steps.h): `problems` problems of `n`
 * correspondences (30 % gross outliers, about half a pixel of noise) and `iterations` hypotheses each, every hypothesis scored over
 * every correspondence as the device does.  Beside it sst_two_view (csrc/ss_track.cpp, the bounded tracker's own form with its 200
 * hypotheses and its threads) on the same correspondences.  Prints one JSON line with the median milliseconds of `reps` runs.
 * build: g++ -O3 -std=c++17 -ffp-contract=off -pthread -I send-slam_amd/csrc -o two_view_host_time profiles/tools/two_view_host_time.cpp
 *        send-slam_amd/csrc/ss_track.cpp
 * usage: two_view_host_time [problems] [n] [iterations] [reps] [scene.bin]
 * scene.bin (int32 problems, int32 n, then problems x n x 4 float32: u1 v1 u2 v2) replaces the program's own scene, so that the host
 * figures are taken on the correspondences the device was timed on */
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_track.h"
#include "ss_two_view_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int main(int argc, char **argv)
{
    const int problems = argc > 1 ? atoi(argv[1]) : 8, n = argc > 2 ? atoi(argv[2]) : 2000, iters = argc > 3 ? atoi(argv[3]) : 200;
    const int reps = argc > 4 ? atoi(argv[4]) : 5;
    const ss_tv_cam cam = {500.0, 510.0, 318.0, 243.0};
    const sst_camera tcam = {500.0, 510.0, 318.0, 243.0, 0.0, 0.0, 0.0, 0.0};
    const double R[9] = {0.99870032, -0.00998734, -0.04997917, 0.00899837, 0.99976001, -0.01997367, 0.05016666, 0.01949798, 0.99855052};
    const double T[3] = {0.6, 0.1, 0.9};
    ss_two_view_params p = {};
    p.chi2_h = 5.991, p.chi2_f = 3.841, p.chi2_score = 5.991, p.rh_threshold = 0.45, p.cos_min_parallax = SS_TWO_VIEW_COS_1DEG, p.min_triangulated = 50;
    p.max_iterations = iters, p.seed = 7u;
    uint32_t s = 2026u;
    std::vector<std::vector<float>> corr((size_t)problems);
    for (auto &c : corr)
        for (int i = 0; i < n; i++) {
            const double z = 4.0 + 4.0 * unit(s), x = (unit(s) - 0.5) * 0.9 * z, y = (unit(s) - 0.5) * 0.6 * z;
            const double X2[3] = {R[0] * x + R[1] * y + R[2] * z + T[0], R[3] * x + R[4] * y + R[5] * z + T[1], R[6] * x + R[7] * y + R[8] * z + T[2]};
            float uv[4] = {(float)(cam.fx * x / z + cam.cx) + unit(s) - 0.5f, (float)(cam.fy * y / z + cam.cy) + unit(s) - 0.5f,
                           (float)(cam.fx * X2[0] / X2[2] + cam.cx) + unit(s) - 0.5f, (float)(cam.fy * X2[1] / X2[2] + cam.cy) + unit(s) - 0.5f};
            if (i % 10 < 3) uv[2] = 640.0f * unit(s), uv[3] = 480.0f * unit(s);
            c.insert(c.end(), uv, uv + 4);
        }
    if (argc > 5) {
        FILE *f = fopen(argv[5], "rb");
        int32_t head[2] = {0, 0};
        if (!f || fread(head, 4, 2, f) != 2 || head[0] != problems || head[1] != n) return fprintf(stderr, "bad scene file\n"), 1;
        for (auto &c : corr)
            if (fread(c.data(), 4, c.size(), f) != c.size()) return fprintf(stderr, "short scene file\n"), 1;
        fclose(f);
    }
    std::vector<float> s1((size_t)n, 1.0f);
    std::vector<uint8_t> flag((size_t)n);
    std::vector<ss_map_point> pts((size_t)n);
    std::vector<double> ms, track_ms;
    long maps = 0, tri = 0, track_maps = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < problems; b++) {
            ss_two_view_result res;
            ss_tv_problem_host(corr[(size_t)b].data(), s1.data(), n, cam, 3.5831816f, p, (uint32_t)b, flag.data(), pts.data(), &res);
            if (res.state == 0) maps++, tri += res.n_triangulated;
        }
        const auto t1 = std::chrono::steady_clock::now();
        for (int b = 0; b < problems; b++) {
            std::vector<double> x1((size_t)2 * n), x2((size_t)2 * n), p3;
            for (int i = 0; i < n; i++)
                x1[2 * i] = corr[(size_t)b][4 * i], x1[2 * i + 1] = corr[(size_t)b][4 * i + 1], x2[2 * i] = corr[(size_t)b][4 * i + 2], x2[2 * i + 1] = corr[(size_t)b][4 * i + 3];
            std::vector<uint8_t> tr;
            double Rt[9], tt[3];
            if (sst_two_view(tcam, n, x1.data(), x2.data(), Rt, tt, tr, p3, nullptr) > 0) track_maps++;
        }
        const auto t2 = std::chrono::steady_clock::now();
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        track_ms.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::sort(ms.begin(), ms.end());
    std::sort(track_ms.begin(), track_ms.end());
    printf("{\"problems\": %d, \"correspondences\": %d, \"iterations\": %d, \"reps\": %d, \"median_ms\": %.3f, \"maps_per_run\": %ld, \"mean_triangulated\": %ld, "
           "\"sst_two_view_median_ms\": %.3f, \"sst_two_view_iterations\": 200, \"sst_two_view_maps_per_run\": %ld}\n",
           problems, n, iters, reps, ms[ms.size() / 2], maps / reps, maps ? tri / maps : 0, track_ms[track_ms.size() / 2], track_maps / reps);
    return 0;
}
