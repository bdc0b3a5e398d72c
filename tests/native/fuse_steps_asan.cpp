// Steps 1 and 2 of map-point fusion (csrc/ss_fuse_steps.h, the text the kernel and the host twins compile) under
// AddressSanitizer and UBSan: the boundaries of every test of step 1 taken with nextafterf on both sides, NaN and infinite
// points and views, every level count; then every evaluated point against train rows on octaves -5 .. 1000 with odd coordinates,
// right values and flags.  The scale table is a heap array of exactly n_levels entries, and taken / right are heap arrays of one
// entry, so an index that leaves any of them is an error the sanitizer reports.  Build: g++ -std=c++17 -ffp-contract=off
// -fsanitize=address,undefined -fno-sanitize-recover=all -I send-slam_amd/csrc.  Prints "ok <evaluations>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ss_fuse_steps.h"

static long evaluations = 0;

static void fail(const char *what, const ss_fuse_point &o)
{
    std::fprintf(stderr, "FAIL %s: state %d level %d radius %g\n", what, o.state, o.level, (double)o.radius);
    std::exit(1);
}

static const float inf = std::numeric_limits<float>::infinity(), nan_ = std::numeric_limits<float>::quiet_NaN();

static void couples(const ss_fuse_point &o, const float *scale, int n_levels)
{
    float s_lo, s_hi;
    ss_fuse_scales(scale, n_levels, o.level, &s_lo, &s_hi);
    const int octaves[] = {-5, -1, 0, 1, 2, 6, 7, 8, 14, 15, 16, 17, 1000, o.level - 2, o.level - 1, o.level, o.level + 1};
    const float coords[] = {0.0f, 1.0f, -3.5f, 4.0f, nan_, inf, -inf};
    const float rights[] = {-1.0f, -0.0f, 0.0f, 1e-45f, 100.0f, nan_, inf};
    std::vector<uint8_t> taken(1);
    std::vector<float> right(1);
    for (int octave : octaves)
        for (float x : coords)
            for (float r : rights)
                for (int flag = 0; flag < 2; flag++) {
                    taken[0] = (uint8_t)(flag * 255);
                    right[0] = r;
                    const float chi2[] = {5.99f, 0.0f, nan_};
                    for (float c2 : chi2) {
                        const int got = ss_fuse_check(o, s_lo, s_hi, o.u + x, o.v, octave, 0, flag ? taken.data() : nullptr, right.data(), c2, 7.8f, 1);
                        const int mono = ss_fuse_check(o, s_lo, s_hi, o.u + x, o.v, octave, 0, taken.data(), nullptr, c2, 7.8f, 1);
                        evaluations += 2;
                        if (got < 0 || got > 4 || mono < 0 || mono > 4) fail("check result", o);
                        if (o.state != 0 && (got != 1 || mono != 1)) fail("a rejected point has a candidate", o);
                        if ((octave < 0 || octave >= n_levels || octave > o.level || octave < o.level - 1) && got != 1) fail("octave", o);
                        if (flag && got == 0) fail("a taken row is a candidate", o);
                    }
                }
}

static void check(const ss_proj_view &w, const ss_map_point &p, int skip, float limit, float th, int n_levels, bool with_couples)
{
    const int n_lv = n_levels < 1 ? 1 : n_levels > SS_MAX_LEVELS ? SS_MAX_LEVELS : n_levels; /* what the steps may read */
    std::vector<float> heap((size_t)n_lv);
    float *scale = heap.data();
    scale[0] = 1.0f;
    for (int i = 1; i < n_lv; i++) scale[i] = (float)(scale[i - 1] * (double)1.2f);
    const ss_fuse_point o = ss_fuse_eval(w, p, skip, limit, th, scale, n_levels);
    evaluations++;
    if (o.state < 0 || o.state > 5) fail("state", o);
    if ((skip != 0) != (o.state == 1)) fail("skip", o);
    if (o.state != 0) {
        if (o.level != -1 || o.u != 0.0f || o.v != 0.0f || o.u_right != 0.0f || o.dot != 0.0f || o.dist != 0.0f || o.radius != 0.0f) fail("rejected point", o);
    } else {
        if (o.level < 0 || o.level >= n_lv) fail("level outside the table", o);
        if (!(o.radius > 0.0f)) fail("radius", o);
        if (!(o.u >= w.min_x && o.u < w.max_x && o.v >= w.min_y && o.v < w.max_y)) fail("projection outside the bounds", o);
    }
    if (with_couples) couples(o, scale, n_lv);
}

int main()
{
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
    }
    {
        float s = 1.0f;
        for (int n = 0; n < SS_MAX_LEVELS; n++, s = (float)(s * (double)1.2f)) around(&ss_map_point::max_dist, s, base);
    }
    const float odd[] = {nan_, inf, -inf, 0.0f, -0.0f, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 1e-20f, 0.9f, 5.0f};
    float ss_map_point::*const fields[] = {&ss_map_point::x,  &ss_map_point::y,  &ss_map_point::z,        &ss_map_point::nx,
                                           &ss_map_point::ny, &ss_map_point::nz, &ss_map_point::min_dist, &ss_map_point::max_dist};
    const size_t n_boundary = pts.size();
    for (auto f : fields)
        for (float v : odd) {
            ss_map_point p = base;
            p.*f = v;
            pts.push_back(p);
            for (auto f2 : fields) /* two odd fields at once */
                for (float v2 : {nan_, inf, -inf}) {
                    ss_map_point q = p;
                    q.*f2 = v2;
                    pts.push_back(q);
                }
        }
    const int level_counts[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 0, -5, 1000};
    for (int n_levels : level_counts)
        for (size_t k = 0; k < pts.size(); k++) {
            const bool with_couples = k < n_boundary || k % 37 == 0; /* the couples of the boundary rows and of a sample of the odd ones */
            check(w, pts[k], 0, 0.5f, 3.0f, n_levels, with_couples);
            check(w, pts[k], 0, -inf, 4.0f, n_levels, false);
            check(w, pts[k], 0, 0.5f, 3.4e38f, n_levels, k % 37 == 0); /* a radius that overflows to +inf is still > 0 */
            check(w, pts[k], (int)(k % 3 + 1), 0.5f, 3.0f, n_levels, false);
        }
    /* an odd view on every point: NaN / infinite pose and intrinsics */
    for (float v : {nan_, inf, -inf}) {
        ss_proj_view o = w;
        o.tcw[2] = v;
        for (const ss_map_point &p : pts) check(o, p, 0, 0.5f, 3.0f, 8, false);
        o = w, o.fx = v;
        for (const ss_map_point &p : pts) check(o, p, 0, 0.5f, 3.0f, 8, false);
        o = w, o.ow[0] = v;
        for (const ss_map_point &p : pts) check(o, p, 0, 0.5f, 3.0f, 8, false);
        o = w, o.max_x = v, o.bf = v;
        for (const ss_map_point &p : pts) check(o, p, 0, 0.5f, 3.0f, 8, false);
    }
    std::printf("ok %ld\n", evaluations);
    return 0;
}
