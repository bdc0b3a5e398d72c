/* ss_track's host step sst_pose_only (csrc/ss_track.cpp) on one host core, on the frames profiles/tools/time_pose.py wrote: the same
 * observations and start poses the device call optimises.  The file: int32 frames, int32 n; per frame twelve doubles (the start pose),
 * then n x (X Y Z u v w) doubles.  Prints one JSON line with the median milliseconds of `reps` runs over all frames.
 * build: g++ -O3 -std=c++17 -ffp-contract=off -I send-slam_amd/csrc -o pose_host_time profiles/tools/pose_host_time.cpp send-slam_amd/csrc/ss_track.cpp
 * usage: pose_host_time frames.bin [reps] */
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ss_track.h"

int main(int argc, char **argv)
{
    if (argc < 2) return fprintf(stderr, "usage: pose_host_time frames.bin [reps]\n"), 2;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    FILE *f = fopen(argv[1], "rb");
    int32_t head[2];
    if (!f || fread(head, sizeof(head), 1, f) != 1 || head[0] < 1 || head[1] < 0) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    const int frames = head[0], n = head[1];
    std::vector<double> start((size_t)frames * 12), pts((size_t)frames * n * 3), obs((size_t)frames * n * 2), w((size_t)frames * n);
    for (int b = 0; b < frames; b++) {
        std::vector<double> rec((size_t)n * 6);
        if (fread(&start[(size_t)b * 12], sizeof(double), 12, f) != 12 || fread(rec.data(), sizeof(double), rec.size(), f) != rec.size())
            return fprintf(stderr, "%s is short\n", argv[1]), 2;
        for (int i = 0; i < n; i++) {
            const size_t o = (size_t)b * n + i;
            pts[3 * o] = rec[6 * (size_t)i], pts[3 * o + 1] = rec[6 * (size_t)i + 1], pts[3 * o + 2] = rec[6 * (size_t)i + 2];
            obs[2 * o] = rec[6 * (size_t)i + 3], obs[2 * o + 1] = rec[6 * (size_t)i + 4];
            w[o] = rec[6 * (size_t)i + 5];
        }
    }
    fclose(f);
    const sst_camera cam = {300.0, 300.0, 160.0, 120.0, 0, 0, 0, 0};
    std::vector<double> ms;
    long inliers = 0, failed = 0;
    for (int r = 0; r < reps; r++) {
        inliers = failed = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < frames; b++) {
            double R[9], t[3];
            for (int k = 0; k < 9; k++) R[k] = start[(size_t)b * 12 + k];
            for (int k = 0; k < 3; k++) t[k] = start[(size_t)b * 12 + 9 + k];
            std::vector<uint8_t> inl;
            const int n_in = sst_pose_only(n, &pts[(size_t)b * n * 3], &obs[(size_t)b * n * 2], &w[(size_t)b * n], cam, R, t, inl);
            if (n_in < 0) failed++;
            else inliers += n_in;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"frames\": %d, \"observations\": %d, \"reps\": %d, \"median_ms\": %.4f, \"ms_per_frame\": %.5f, \"failed\": %ld, \"mean_inliers\": %ld}\n", frames, n, reps,
           ms[ms.size() / 2], ms[ms.size() / 2] / frames, failed, inliers / frames);
    return 0;
}
