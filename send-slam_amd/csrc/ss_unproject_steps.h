/*
 * ss_unproject_steps.h -- the steps of the map points from depth (the rule: include/sendslam_orb.h): the class
 * of a row, its selection key, the unprojection of one keypoint with a depth and its map point in double.  The kernel
 * (ss_unproject.hip), the host twin ss_unproject_host (ss_api_search.cpp) and tests/native/unproject_steps_asan.cpp compile this text.
 *
 * Every step is one IEEE operation, left to right as written; every test is in its accepting form, so a NaN fails it.  Compile
 * with -ffp-contract=off.  Division and square root are correctly rounded on both sides (hipcc's default).
 */
#ifndef SS_UNPROJECT_STEPS_H
#define SS_UNPROJECT_STEPS_H

#include "../../include/sendslam_orb.h"
#include "ss_float_steps.h" /* SS_HD, math.h */

/* the rows of a frame that count: the told count clamped to 0 .. rows */
SS_HD int ss_unproject_clamp(int n, int rows) { return n < 0 ? 0 : (n > rows ? rows : n); }

/* the depth of row i of a plane whose rows are `stride` bytes apart */
SS_HD float ss_unproject_depth_at(const uint8_t *plane, int64_t stride, int i) { return *(const float *)(plane + (int64_t)i * stride); }

SS_HD uint32_t ss_unproject_bits(float d)
{
    union { float f; uint32_t u; } v;
    v.f = d;
    return v.u;
}

/* step 1 of a row below the count: 0 ranked, else its state (SS_UNPROJECT_NO_DEPTH, SS_UNPROJECT_OCTAVE) */
SS_HD int ss_unproject_class(float depth, int octave, int n_levels)
{
    if (!(depth > 0.0f)) return SS_UNPROJECT_NO_DEPTH;
    if (!(octave >= 0 && octave < n_levels)) return SS_UNPROJECT_OCTAVE;
    return 0;
}

/* step 2: positive floats order as their bits, the row breaks ties */
SS_HD uint64_t ss_unproject_key(float depth, int i) { return (uint64_t)ss_unproject_bits(depth) << 32 | (uint32_t)i; }

/* step 3: how many of the lowest keys are processed; n_ranked when the mode takes every row */
SS_HD int ss_unproject_quota(int mode, int max_points, int n_not_far, int n_ranked)
{
    if (mode == SS_UNPROJECT_ALL) return n_ranked;
    const int r = n_not_far > max_points ? n_not_far : max_points; /* rank <= r: r + 1 rows, r < n_ranked or all of them */
    return r < n_ranked ? r + 1 : n_ranked;
}

/* the position of the keypoint (x, y) at depth z in the world: Rwc.xc + Ow.  The stereo form of the triangulation (ss_epi_steps.h)
 * calls it with the fields of a pair's side */
SS_HD void ss_unproject_xyz(const double *rcw, const double *ow, double cx, double cy, double invfx, double invfy, float x, float y, float depth,
                            double X[3])
{
    const double z = (double)depth;
    const double xc = (((double)x - cx) * z) * invfx, yc = (((double)y - cy) * z) * invfy;
    X[0] = ((rcw[0] * xc + rcw[3] * yc) + rcw[6] * z) + ow[0];
    X[1] = ((rcw[1] * xc + rcw[4] * yc) + rcw[7] * z) + ow[1];
    X[2] = ((rcw[2] * xc + rcw[5] * yc) + rcw[8] * z) + ow[2];
}
SS_HD void ss_unproject_world(const ss_unproject_view &v, float x, float y, float depth, double X[3])
{
    ss_unproject_xyz(v.rcw, v.ow, v.cx, v.cy, v.invfx, v.invfy, x, y, depth, X);
}

/* step 5: the map point of a created row (octave inside the table); ok false, with the point all 0.0f: SS_UNPROJECT_DEGENERATE */
struct ss_unproject_out {
    bool ok;
    ss_map_point point;
};
SS_HD ss_unproject_out ss_unproject_point(const ss_unproject_view &v, const float *scale, int n_levels, float x, float y, int octave, float depth)
{
    double X[3];
    ss_unproject_world(v, x, y, depth, X);
    const double n0 = X[0] - v.ow[0], n1 = X[1] - v.ow[1], n2 = X[2] - v.ow[2];
    const double d = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    ss_unproject_out o;
    o.ok = d > 0.0 && d <= 1.7976931348623157e308;
    const double max_dist = d * (double)scale[octave];
    o.point.x = o.ok ? (float)X[0] : 0.0f, o.point.y = o.ok ? (float)X[1] : 0.0f, o.point.z = o.ok ? (float)X[2] : 0.0f;
    o.point.nx = o.ok ? (float)(n0 / d) : 0.0f, o.point.ny = o.ok ? (float)(n1 / d) : 0.0f, o.point.nz = o.ok ? (float)(n2 / d) : 0.0f;
    o.point.min_dist = o.ok ? (float)(max_dist / (double)scale[n_levels - 1]) : 0.0f;
    o.point.max_dist = o.ok ? (float)max_dist : 0.0f;
    return o;
}

#endif
