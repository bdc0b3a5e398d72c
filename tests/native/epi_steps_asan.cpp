// The steps of the epipolar search and of the triangulation (csrc/ss_epi_steps.h, the text the kernels and the host twins compile)
// under AddressSanitizer and UBSan: NaN and infinite pairs and keypoints, octaves -5 .. 1000, every level count.  The scale table is
// a heap array of exactly the entries a call may read, so an octave that leaves the table is an error the sanitizer reports.
// Build: g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I send-slam_amd/csrc.
// Prints "ok <evaluations>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_epi_steps.h"

static long evaluations = 0;

static void fail(const char *what, int state)
{
    std::fprintf(stderr, "FAIL %s: state %d\n", what, state);
    std::exit(1);
}

struct kp {
    float x, y;
    int octave;
};

static void run(const ss_epi_pair &w, const ss_tri_params &tp, const kp &a, const kp &b, int n_levels, int *states)
{
    std::vector<float> heap((size_t)n_levels); /* what the steps may read */
    float *scale = heap.data();
    scale[0] = 1.0f;
    for (int i = 1; i < n_levels; i++) scale[i] = (float)(scale[i - 1] * (double)1.2f);
    const ss_epi_line line = ss_epi_line_of(w.f12, a.x, a.y);
    for (int coarse = 0; coarse < 2; coarse++) {
        const int r = ss_epi_check(w.ex, w.ey, w.epipole_test, coarse, line, scale, n_levels, b.x, b.y, b.octave);
        evaluations++;
        if (r < 0 || r > 3) fail("check code", r);
        if ((b.octave < 0 || b.octave >= n_levels) != (r == 1)) fail("octave test", r);
        if (coarse && r == 3) fail("coarse ran the line test", r);
    }
    const ss_tri_out o = ss_tri_eval(w, tp, scale, n_levels, a.x, a.y, a.octave, b.x, b.y, b.octave);
    evaluations++;
    const int st = o.info.state;
    if (st < 0 || st > 10) fail("state", st);
    states[st]++;
    const bool outside = a.octave < 0 || a.octave >= n_levels || b.octave < 0 || b.octave >= n_levels;
    if (outside != (st == 10)) fail("octave state", st);
    const ss_map_point &p = o.point;
    if (st != 0) {
        if (p.x != 0.0f || p.y != 0.0f || p.z != 0.0f || p.nx != 0.0f || p.ny != 0.0f || p.nz != 0.0f || p.min_dist != 0.0f || p.max_dist != 0.0f) fail("rejected point", st);
        if (st == 10 && (o.info.cos_parallax != 0.0f || o.info.err1_sq != 0.0f || o.info.err2_sq != 0.0f)) fail("info of an unreached step", st);
        if (st < 5 && (o.info.err1_sq != 0.0f || o.info.err2_sq != 0.0f)) fail("info of an unreached step", st);
        return;
    }
    if (!(o.info.cos_parallax > 0.0f) || !(p.max_dist > 0.0f) || !(p.min_dist > 0.0f) || !(p.min_dist <= p.max_dist)) fail("point", st);
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double dinf = std::numeric_limits<double>::infinity(), dnan = std::numeric_limits<double>::quiet_NaN();
    /* camera 1 at the origin, camera 2 0.3 to its right, fx = 300, principal point (160, 120): F12 = [t]x up to scale */
    ss_epi_pair w = {};
    w.rcw1[0] = w.rcw1[4] = w.rcw1[8] = w.rcw2[0] = w.rcw2[4] = w.rcw2[8] = 1.0;
    w.tcw2[0] = -0.3, w.ow2[0] = 0.3;
    w.fx1 = w.fy1 = w.fx2 = w.fy2 = 300.0, w.invfx1 = w.invfy1 = w.invfx2 = w.invfy2 = 1.0 / 300.0;
    w.cx1 = w.cx2 = 160.0, w.cy1 = w.cy2 = 120.0;
    w.f12[5] = -1.0f, w.f12[7] = 1.0f, w.f12[8] = 0.0f; /* a = 0, b = 1, c = -y_i */
    w.ex = 1e9f, w.ey = 120.0f, w.epipole_test = 1;
    const ss_tri_params upstream = {0.9998, 5.991, 1.5 * 1.2, 0.0};
    std::vector<kp> pts;
    const int octaves[] = {-5, -1, 0, 1, 3, 7, 8, 15, 16, 17, 1000};
    const float odd[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-45f, 3.4e38f, -3.4e38f};
    for (int o : octaves) {
        /* a point at depth 3 seen by both: x1 = 200, x2 = 200 - 300 * 0.3 / 3 = 170; and keypoints around it */
        for (float dx : {0.0f, 0.5f, -0.5f, 30.0f, -30.0f, 40.0f})
            for (float dy : {0.0f, 0.25f, 1.9f, 2.0f, 50.0f}) pts.push_back({170.0f + dx, 100.0f + dy, o});
        for (float v : odd) {
            pts.push_back({v, 100.0f, o});
            pts.push_back({170.0f, v, o});
            pts.push_back({v, v, o});
        }
    }
    std::vector<ss_epi_pair> pairs = {w};
    for (double v : {dnan, dinf, -dinf, 0.0, 1e308}) { /* odd pairs: pose, intrinsics, camera centres, F and epipole */
        ss_epi_pair o = w;
        o.rcw1[0] = v, pairs.push_back(o);
        o = w, o.tcw2[2] = v, pairs.push_back(o);
        o = w, o.ow1[1] = v, pairs.push_back(o);
        o = w, o.invfx2 = v, o.fx2 = v, pairs.push_back(o);
        o = w, o.cx1 = v, pairs.push_back(o);
        o = w, o.f12[7] = (float)v, o.ex = (float)v, pairs.push_back(o);
        o = w, o.ex = 170.0f, o.ey = (float)v, pairs.push_back(o);
    }
    {
        ss_epi_pair o = w; /* identical poses: F is zero, the epipole test is off */
        for (float &f : o.f12) f = 0.0f;
        o.tcw2[0] = 0.0, o.ow2[0] = 0.0, o.epipole_test = 0;
        pairs.push_back(o);
    }
    const ss_tri_params params[] = {upstream, {2.0, dinf, dinf, 5.0}, {dnan, dnan, dnan, dnan}, {0.9998, 5.991, 0.0, -1.0}, {-1.0, 0.0, 1.0, 1e-300}};
    int states[11] = {};
    const kp query = {200.0f, 100.0f, 0};
    const int level_counts[] = {1, 2, 8, 15, 16};
    for (int n_levels : level_counts)
        for (const ss_epi_pair &pr : pairs)
            for (const ss_tri_params &tp : params)
                for (const kp &b : pts) {
                    run(pr, tp, query, b, n_levels, states);
                    run(pr, tp, b, query, n_levels, states);
                }
    for (int o : octaves) /* the query's own octave */
        for (const kp &b : pts) run(w, upstream, {200.0f, 100.0f, o}, b, 8, states);
    if (states[0] == 0 || states[1] == 0 || states[5] + states[6] == 0 || states[10] == 0) fail("a state that never occurred", -1);
    std::printf("ok %ld\n", evaluations);
    return 0;
}
