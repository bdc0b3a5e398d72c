// Steps 1 - 3 of the projection search (csrc/ss_proj_steps.h, the text the kernel and the host twin compile) under
// AddressSanitizer and UBSan: the boundaries of every test taken with nextafterf on both sides, NaN and infinite inputs, every
// level count.  The scale table is a heap array of exactly the entries the call may read, so a level index that leaves the
// table is an error the sanitizer reports.  Build: g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined
// -fno-sanitize-recover=all -I send-slam_amd/csrc.  Prints "ok <evaluations>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_proj_steps.h"

static long evaluations = 0;

static void fail(const char *what, const ss_proj_point &o)
{
    std::fprintf(stderr, "FAIL %s: state %d level %d radius %g\n", what, o.state, o.level, (double)o.radius);
    std::exit(1);
}

static void check(const ss_proj_view &w, const ss_map_point &p, float limit, float th, float far_limit, int n_levels)
{
    const int n_lv = n_levels < 1 ? 1 : n_levels > SS_MAX_LEVELS ? SS_MAX_LEVELS : n_levels; /* what the steps may read */
    std::vector<float> heap((size_t)n_lv);
    float *scale = heap.data();
    scale[0] = 1.0f;
    for (int i = 1; i < n_lv; i++) scale[i] = (float)(scale[i - 1] * (double)1.2f);
    const ss_proj_point o = ss_proj_eval(w, p, limit, th, far_limit, scale, n_levels);
    evaluations++;
    if (o.state < 0 || o.state > 5) fail("state", o);
    if (o.state != 0) {
        if (o.level != -1 || o.u != 0.0f || o.v != 0.0f || o.u_right != 0.0f || o.view_cos != 0.0f || o.dist != 0.0f || o.radius != 0.0f) fail("rejected point", o);
        return;
    }
    if (o.level < 0 || o.level >= n_lv) fail("level outside the table", o);
    if (!(o.radius > 0.0f)) fail("radius", o);
    if (!(o.u >= w.min_x && o.u <= w.max_x && o.v >= w.min_y && o.v <= w.max_y)) fail("projection outside the bounds", o);
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    ss_proj_view w = {};
    w.rcw[0] = w.rcw[4] = w.rcw[8] = 1.0f;
    w.fx = w.fy = 256.0f;
    w.bf = 16.0f;
    w.min_x = -160.0f, w.max_x = 160.0f, w.min_y = -120.0f, w.max_y = 120.0f;
    const ss_map_point base = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.1f, 1.0f};
    std::vector<ss_map_point> pts;
    auto around = [&](float ss_map_point::*field, float centre, ss_map_point p) {
        const float v[3] = {nextafterf(centre, -inf), centre, nextafterf(centre, inf)};
        for (float x : v) {
            p.*field = x;
            pts.push_back(p);
        }
    };
    around(&ss_map_point::z, 0.0f, base);
    around(&ss_map_point::x, -0.625f, base);
    around(&ss_map_point::x, 0.625f, base);
    around(&ss_map_point::y, -0.46875f, base);
    around(&ss_map_point::y, 0.46875f, base);
    {
        ss_map_point p = base;
        p.min_dist = 2.0f, p.max_dist = 4.0f;
        around(&ss_map_point::z, 0.8f * 2.0f, p);
        p = base, p.max_dist = 2.0f;
        around(&ss_map_point::z, 1.2f * 2.0f, p);
        p.z = 2.0f;
        around(&ss_map_point::nz, 0.5f, p);
        around(&ss_map_point::nz, 0.998f, p);
        p = base, p.max_dist = 4.0f;
        around(&ss_map_point::z, 3.0f, p);
    }
    {
        float s = 1.0f;
        for (int n = 0; n < SS_MAX_LEVELS; n++, s = (float)(s * (double)1.2f)) around(&ss_map_point::max_dist, s, base);
    }
    const float odd[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 1e-20f, 0.9f, 5.0f};
    float ss_map_point::*const fields[] = {&ss_map_point::x,  &ss_map_point::y,  &ss_map_point::z,        &ss_map_point::nx,
                                           &ss_map_point::ny, &ss_map_point::nz, &ss_map_point::min_dist, &ss_map_point::max_dist};
    for (auto f : fields)
        for (float v : odd) {
            ss_map_point p = base;
            p.*f = v;
            pts.push_back(p);
            for (auto f2 : fields) /* two odd fields at once */
                for (float v2 : {nan, inf, -inf}) {
                    ss_map_point q = p;
                    q.*f2 = v2;
                    pts.push_back(q);
                }
        }
    const int level_counts[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 0, -5, 1000};
    for (int n_levels : level_counts)
        for (const ss_map_point &p : pts) {
            check(w, p, 0.5f, 1.0f, 3.0f, n_levels);
            check(w, p, -inf, 3.0f, 0.0f, n_levels);
            check(w, p, 0.5f, 3.4e38f, nan, n_levels); /* a radius that overflows to +inf is still > 0 */
        }
    /* an odd view on every point: NaN / infinite pose and intrinsics */
    for (float v : {nan, inf, -inf}) {
        ss_proj_view o = w;
        o.tcw[2] = v;
        for (const ss_map_point &p : pts) check(o, p, 0.5f, 1.0f, 0.0f, 8);
        o = w, o.fx = v;
        for (const ss_map_point &p : pts) check(o, p, 0.5f, 1.0f, 0.0f, 8);
        o = w, o.ow[0] = v;
        for (const ss_map_point &p : pts) check(o, p, 0.5f, 1.0f, 0.0f, 8);
        o = w, o.max_x = v, o.bf = v;
        for (const ss_map_point &p : pts) check(o, p, 0.5f, 1.0f, 0.0f, 8);
    }
    std::printf("ok %ld\n", evaluations);
    return 0;
}
