/*
 * unproject_steps_asan.cpp -- the steps of the map points from depth (csrc/ss_unproject_steps.h) under -fsanitize=address,undefined:
 * frames whose keypoints, depth plane (stride 4, and stride 16 as inside ss_stereo_point, the last row ending with its four bytes)
 * and flags are allocated to the byte; depths with ties, zeros, negatives, NaNs, the largest float and infinities; octaves outside
 * the table; finite and non-finite poses.  The selection by the quota of the lowest keys is checked against upstream's sequential
 * loop over the sorted (depth, row) pairs, the map point against its own invariants.  Prints "ok <frames> <points>" and exits 0.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "ss_unproject_steps.h"

static int fails = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
        }                                                                            \
    } while (0)

static ss_unproject_view view_of(const double r[9], const double t[3])
{
    ss_unproject_view v;
    for (int k = 0; k < 9; k++) v.rcw[k] = r[k];
    for (int k = 0; k < 3; k++) {
        v.tcw[k] = t[k];
        v.ow[k] = -((r[k] * t[0] + r[3 + k] * t[1]) + r[6 + k] * t[2]);
    }
    v.fx = 317.25, v.fy = 289.5, v.cx = 171.5, v.cy = 108.25, v.invfx = 1.0 / v.fx, v.invfy = 1.0 / v.fy;
    return v;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float values[] = {0.5f, 1.0f, 1.0f, 2.0f, 3.0f, 3.0f, 3.5f, 4.0f, 4.0f, 4.0f, 3.4e38f, inf, 0.0f, -0.0f, -1.0f, nan, -inf};
    const int n_values = (int)(sizeof(values) / sizeof(values[0]));
    float scale[8];
    scale[0] = 1.0f;
    for (int k = 1; k < 8; k++) scale[k] = scale[k - 1] * 1.2f;
    /* a rotation about z by an angle whose sine and cosine are 0.6 and 0.8, then a translation */
    const double rot[9] = {0.8, -0.6, 0.0, 0.6, 0.8, 0.0, 0.0, 0.0, 1.0}, tr[3] = {0.5, -0.25, 1.0};
    const double bad_tr[3] = {0.5, (double)nan, 1.0};
    const ss_unproject_view good = view_of(rot, tr), bad = view_of(rot, bad_tr);
    std::mt19937 rng(20261021u);
    long frames = 0, points = 0;

    CHECK(ss_unproject_clamp(-3, 70) == 0 && ss_unproject_clamp(200, 70) == 70 && ss_unproject_clamp(7, 70) == 7);
    CHECK(ss_unproject_quota(SS_UNPROJECT_ALL, 5, 0, 9) == 9 && ss_unproject_quota(SS_UNPROJECT_CLOSE, 5, 0, 9) == 6 &&
          ss_unproject_quota(SS_UNPROJECT_CLOSE, 5, 7, 9) == 8 && ss_unproject_quota(SS_UNPROJECT_CLOSE, 5, 9, 9) == 9 &&
          ss_unproject_quota(SS_UNPROJECT_CLOSE, 2147483647, 3, 9) == 9 && ss_unproject_quota(SS_UNPROJECT_CLOSE, 0, 0, 0) == 0);
    CHECK(ss_unproject_key(1.0f, 3) < ss_unproject_key(1.0f, 4) && ss_unproject_key(1.0f, 16383) < ss_unproject_key(1.0000001f, 0) &&
          ss_unproject_key(3.4e38f, 5) < ss_unproject_key(inf, 0));

    for (int round = 0; round < 300; round++) {
        const int n = (int)(rng() % 90), stride = round % 2 ? 16 : 4, max_points = (int)(rng() % 12), mode = round % 5 == 0 ? SS_UNPROJECT_ALL : SS_UNPROJECT_CLOSE;
        const float close_limit = 3.0f;
        std::vector<ss_keypoint> kp((size_t)n);
        std::vector<uint8_t> plane(n ? (size_t)(n - 1) * stride + 4 : 0, 0xEE);
        for (int i = 0; i < n; i++) {
            memset(&kp[i], 0, sizeof(ss_keypoint));
            kp[i].x = (float)(rng() % 3200) / 10.0f, kp[i].y = (float)(rng() % 2400) / 10.0f;
            kp[i].octave = rng() % 20 == 0 ? (rng() % 2 ? 8 : -1) : (int)(rng() % 8);
            const float d = values[rng() % n_values];
            memcpy(&plane[(size_t)i * stride], &d, 4);
        }
        /* the library's form */
        std::vector<uint64_t> keys;
        int n_not_far = 0;
        for (int i = 0; i < n; i++) {
            const float d = ss_unproject_depth_at(plane.data(), stride, i);
            const int cls = ss_unproject_class(d, kp[i].octave, 8);
            CHECK(cls == 0 || cls == SS_UNPROJECT_NO_DEPTH || cls == SS_UNPROJECT_OCTAVE);
            CHECK((cls == SS_UNPROJECT_NO_DEPTH) == !(d > 0.0f));
            if (cls != 0) continue;
            keys.push_back(ss_unproject_key(d, i));
            n_not_far += d <= close_limit;
        }
        std::sort(keys.begin(), keys.end());
        const int quota = ss_unproject_quota(mode, max_points, n_not_far, (int)keys.size());
        CHECK(quota >= 0 && quota <= (int)keys.size());
        std::vector<char> processed((size_t)n, 0);
        for (int k = 0; k < quota; k++) processed[(size_t)(keys[(size_t)k] & 0xFFFFFFFFu)] = 1;
        /* upstream's loop */
        std::vector<std::pair<float, int>> pairs;
        for (int i = 0; i < n; i++) {
            float d;
            memcpy(&d, &plane[(size_t)i * stride], 4);
            if (d > 0.0f && kp[i].octave >= 0 && kp[i].octave < 8) pairs.push_back(std::make_pair(d, i));
        }
        std::sort(pairs.begin(), pairs.end());
        std::vector<char> visited((size_t)n, 0);
        int n_points = 0;
        for (const auto &q : pairs) {
            visited[(size_t)q.second] = 1;
            n_points++;
            if (mode == SS_UNPROJECT_CLOSE && q.first > close_limit && n_points > max_points) break;
        }
        CHECK(processed == visited);
        /* the map points */
        for (int i = 0; i < n; i++) {
            if (!processed[(size_t)i]) continue;
            const float d = ss_unproject_depth_at(plane.data(), stride, i);
            const ss_unproject_out r = ss_unproject_point(good, scale, 8, kp[i].x, kp[i].y, kp[i].octave, d);
            const ss_map_point p = r.point;
            const bool ok = r.ok;
            points++;
            CHECK(ok == std::isfinite(d));
            if (ok) {
                const double len = std::sqrt((double)p.nx * p.nx + (double)p.ny * p.ny + (double)p.nz * p.nz);
                CHECK(std::fabs(len - 1.0) < 1e-6);
                CHECK(p.max_dist > 0.0f && p.min_dist > 0.0f && (p.min_dist <= p.max_dist || !std::isfinite(p.max_dist)));
                /* back into the camera: the depth along the axis is the row's */
                const double zc = ((good.rcw[6] * p.x + good.rcw[7] * p.y) + good.rcw[8] * p.z) + good.tcw[2];
                if (d < 1e6f) CHECK(std::fabs(zc - (double)d) <= 1e-4); /* the position is float32: 2^-24 of a few metres per axis */
            } else {
                CHECK(p.x == 0.0f && p.nz == 0.0f && p.max_dist == 0.0f);
            }
            const ss_unproject_out q = ss_unproject_point(bad, scale, 8, kp[i].x, kp[i].y, kp[i].octave, d);
            CHECK(!q.ok && q.point.x == 0.0f);
        }
        frames++;
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("ok %ld %ld\n", frames, points);
    return 0;
}
