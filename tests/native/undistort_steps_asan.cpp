/*
 * undistort_steps_asan.cpp -- the steps of Frame's keypoint post-processing (csrc/ss_undistort_steps.h) under
 * -fsanitize=address,undefined: the undistortion of positions inside, outside and far outside the image, non-finite ones included,
 * under a barrel, a pincushion, a tangential and a zero camera; the bounds of each; the depth lookup on uint16 and float32 frames
 * allocated at their exact size, rows longer than the width, positions on every edge, just outside it, huge and non-finite, so that a
 * pixel index out of the frame or a float-to-int conversion out of range is caught.  Every depth row is checked against a second
 * walk that indexes with integers it has range-checked itself.  Prints "ok <points> <depth rows>" and exits 0.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ss_undistort_steps.h"

static int fails = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
        }                                                                            \
    } while (0)

static ss_camera camera(double k1, double k2, double p1, double p2)
{
    ss_camera c;
    memset(&c, 0, sizeof(c));
    c.fx = 260.0, c.fy = 257.5, c.cx = 159.0, c.cy = 121.0;
    c.k1 = k1, c.k2 = k2, c.p1 = p1, c.p2 = p2;
    c.width = 320, c.height = 240;
    return c;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const ss_camera cams[4] = {camera(-0.28, 0.07, 1e-3, -5e-4), camera(0.12, -0.03, -8e-4, 6e-4), camera(0, 0, 2e-3, -1e-3), camera(0, 0, 0, 0)};
    std::mt19937 rng(20260202u);
    std::uniform_real_distribution<float> wide(-400.0f, 800.0f);
    long points = 0, rows = 0;
    for (int k = 0; k < 4; k++) {
        const ss_undist_cam u = ss_undist_cam_of(cams[k]);
        CHECK(u.none == (k == 3) && ss_undist_cam_finite(u) && ss_undist_focal_ok(u.fx, u.fy));
        float b[4];
        ss_undist_bounds(u, 320, 240, b);
        CHECK(b[0] < b[1] && b[2] < b[3]);
        if (k == 3) CHECK(b[0] == 0.0f && b[1] == 320.0f && b[2] == 0.0f && b[3] == 240.0f);
        if (k == 0) CHECK(b[0] < -39.0f && b[1] > 361.0f && b[2] < -31.0f && b[3] > 269.0f);
        if (k == 1) CHECK(b[0] > 8.0f && b[1] < 312.0f && b[2] > 6.0f && b[3] < 235.0f);
        const float special[] = {0.0f, -0.0f, 320.0f, 1e-40f, 3e38f, -3e38f, inf, -inf, nan};
        for (float sx : special)
            for (float sy : special) {
                float x, y;
                ss_undist_point(u, sx, sy, &x, &y);
                if (k == 3) CHECK(same_bits(x, sx) && same_bits(y, sy));
                points++;
            }
        for (int i = 0; i < 4000; i++, points++) {
            const float sx = wide(rng), sy = wide(rng);
            float x, y;
            ss_undist_point(u, sx, sy, &x, &y);
            if (k == 3) CHECK(same_bits(x, sx) && same_bits(y, sy));
            /* the principal point is a fixed point of every camera */
            if (i == 0) {
                ss_undist_point(u, 159.0f, 121.0f, &x, &y);
                CHECK(x == 159.0f && y == 121.0f);
            }
        }
    }
    ss_undist_cam bad = ss_undist_cam_of(cams[0]);
    bad.k2 = nan;
    CHECK(!ss_undist_cam_finite(bad) && !ss_undist_focal_ok(0.0, 1.0) && !ss_undist_focal_ok(1.0, (double)inf) && !ss_undist_focal_ok((double)nan, 1.0));
    CHECK(ss_undist_clamp(-3, 70) == 0 && ss_undist_clamp(200, 70) == 70 && ss_undist_clamp(7, 70) == 7);

    CHECK(ss_depth_inv(0.0f) == 1.0f && ss_depth_inv(5000.0f) == 1.0f / 5000.0f && ss_depth_inv(-9e-6f) == 1.0f && ss_depth_inv(1.0f) == 1.0f);
    CHECK(!ss_depth_scales_float(1.0f) && !ss_depth_scales_float(ss_depth_inv(1.0f + 5e-6f)) && ss_depth_scales_float(ss_depth_inv(5000.0f)));
    for (int round = 0; round < 40; round++) {
        const int w = 1 + (int)(rng() % 70), h = 1 + (int)(rng() % 50), type = (int)(rng() % 2), sample = type ? 2 : 4;
        const int64_t stride = (int64_t)(w + (int)(rng() % 5)) * sample;
        /* the last row ends with its width: the frame is allocated to the byte */
        std::vector<uint8_t> frame((size_t)(stride * (h - 1) + (int64_t)w * sample));
        for (int r = 0; r < h; r++)
            for (int c = 0; c < w; c++) {
                const int pick = (int)(rng() % 10);
                if (type) {
                    const uint16_t v = pick == 0 ? 0 : (uint16_t)(rng() % 65536);
                    memcpy(&frame[(size_t)(r * stride + c * 2)], &v, 2);
                } else {
                    const float v = pick == 0 ? 0.0f : pick == 1 ? -2.0f : pick == 2 ? nan : 0.25f + (float)(rng() % 4000) / 512.0f;
                    memcpy(&frame[(size_t)(r * stride + c * 4)], &v, 4);
                }
            }
        const float factor = round % 4 == 0 ? 0.0f : round % 4 == 1 ? 1.0f + 5e-6f : round % 4 == 2 ? 5000.0f : 1.0f;
        const float inv = ss_depth_inv(factor), bf = 26.0f;
        const bool scale_float = ss_depth_scales_float(inv);
        auto along = [&](int n) { /* positions along an axis of n pixels */
            return std::vector<float>{0.0f, -0.0f, -0.5f, -0.999f, -1.0f, (float)n - 1.0f, (float)n - 0.01f, (float)n, (float)n + 0.5f, 3e38f, -3e38f, inf, -inf, nan,
                                      2147483648.0f, -2147483904.0f, 0.75f};
        };
        for (float x : along(w))
            for (float yy : along(h)) {
                float d = -7.0f, right, depth;
                const bool have = ss_depth_sample(frame.data(), w, h, stride, type, inv, scale_float, x, yy, &d);
                ss_depth_row(have, d, 100.0f, bf, &right, &depth);
                rows++;
                /* the second walk */
                bool inside = std::isfinite(x) && std::isfinite(yy) && x > -1.0f && yy > -1.0f && x < (float)w && yy < (float)h;
                float want = -1.0f;
                if (inside) {
                    const int c = (int)x, r = (int)yy;
                    CHECK(c >= 0 && c < w && r >= 0 && r < h);
                    float v;
                    if (type) {
                        uint16_t raw;
                        memcpy(&raw, &frame[(size_t)(r * stride + c * 2)], 2);
                        v = (float)raw * inv;
                    } else {
                        memcpy(&v, &frame[(size_t)(r * stride + c * 4)], 4);
                        if (scale_float) v = v * inv;
                    }
                    if (v > 0.0f) want = v;
                }
                CHECK(have == inside);
                CHECK(same_bits(depth, want));
                CHECK(want > 0.0f ? same_bits(right, 100.0f - bf / want) : right == -1.0f);
            }
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("ok %ld %ld\n", points, rows);
    return 0;
}
