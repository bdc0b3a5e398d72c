/*
 * ss_fuse_steps.h -- steps 1 and 2 of map-point fusion (the rule: include/sendslam_orb.h): the point in
 * the keyframe, and whether a train row is a candidate for it.  k_fuse_search (ss_fuse.hip), the host twins ss_fuse_points_host
 * and ss_fuse_check_host (ss_api_search.cpp) and tests/native/fuse_steps_asan.cpp compile this text.
 *
 * Every float step is one float32 IEEE operation, left to right as written; every test is in its accepting form, so a NaN
 * fails it.  Compile with -ffp-contract=off.  The division and sqrtf are correctly rounded on both sides (hipcc's default).
 */
#ifndef SS_FUSE_STEPS_H
#define SS_FUSE_STEPS_H

#include "ss_proj_steps.h" /* ss_proj_level; SS_HD, the public header */

/* what step 1 rejects: the number of the first failing test in state, floats 0.0f, level -1 */
SS_HD ss_fuse_point ss_fuse_rejected(int state)
{
    ss_fuse_point o;
    o.u = o.v = o.u_right = o.dot = o.dist = o.radius = 0.0f;
    o.level = -1;
    o.state = state;
    return o;
}

/* The scales of the two octaves a candidate of a point at `level` can have: *s_lo = scale[max(level - 1, 0)], *s_hi = scale[level].
 * The table is read at loop indices only, so no level, whatever its value, leaves it (one outside it gets scale[0]). */
SS_HD void ss_fuse_scales(const float *scale, int n_levels, int level, float *s_lo, float *s_hi)
{
    const int n_lv = n_levels < 1 ? 1 : n_levels > SS_MAX_LEVELS ? SS_MAX_LEVELS : n_levels;
    float lo = scale[0], hi = scale[0];
    for (int n = 1; n < n_lv; n++) {
        const float s = scale[n];
        if (n == level - 1) lo = s;
        if (n == level) hi = s;
    }
    *s_lo = lo;
    *s_hi = hi;
}

/* step 1 of one map point; skip: the point's skip flag, 0 where the caller has none */
SS_HD ss_fuse_point ss_fuse_eval(const ss_proj_view &w, const ss_map_point &p, int skip, float view_cos_limit, float th, const float *scale,
                                 int n_levels)
{
    /* test 1 */
    if (skip != 0) return ss_fuse_rejected(1);
    /* test 2 */
    const float pcx = ((w.rcw[0] * p.x + w.rcw[1] * p.y) + w.rcw[2] * p.z) + w.tcw[0];
    const float pcy = ((w.rcw[3] * p.x + w.rcw[4] * p.y) + w.rcw[5] * p.z) + w.tcw[1];
    const float pcz = ((w.rcw[6] * p.x + w.rcw[7] * p.y) + w.rcw[8] * p.z) + w.tcw[2];
    if (!(pcz > 0.0f)) return ss_fuse_rejected(2);
    /* test 3: KeyFrame::IsInImage, strict at the upper bounds */
    const float invz = 1.0f / pcz;
    const float u = w.fx * pcx * invz + w.cx;
    const float v = w.fy * pcy * invz + w.cy;
    if (!(u >= w.min_x && u < w.max_x && v >= w.min_y && v < w.max_y)) return ss_fuse_rejected(3);
    /* test 4 */
    const float pox = p.x - w.ow[0], poy = p.y - w.ow[1], poz = p.z - w.ow[2];
    const float dist = sqrtf((pox * pox + poy * poy) + poz * poz);
    if (!(dist >= 0.8f * p.min_dist && dist <= 1.2f * p.max_dist)) return ss_fuse_rejected(4);
    /* test 5: no division */
    const float dot = (pox * p.nx + poy * p.ny) + poz * p.nz;
    if (!(dot >= view_cos_limit * dist)) return ss_fuse_rejected(5);
    /* level, window */
    const float ratio = p.max_dist / dist;
    float s;
    ss_fuse_point o;
    o.level = ss_proj_level(ratio, scale, n_levels, &s);
    o.radius = th * s;
    o.u = u;
    o.v = v;
    o.u_right = u - w.bf * invz;
    o.dot = dot;
    o.dist = dist;
    o.state = 0;
    return o;
}

/* Step 2 of the couple (point o, train row `row` at (x, y) on `octave`): 0 if the row is a candidate, else the number 1 .. 4 of the
 * first failing test.  s_lo / s_hi: ss_fuse_scales of o.level.  taken / right: the frame's arrays, or NULL; each is read at `row`
 * only once the tests before it have passed, right only when the chi-square test uses it. */
SS_HD int ss_fuse_check(const ss_fuse_point &o, float s_lo, float s_hi, float x, float y, int octave, int row, const uint8_t *taken,
                        const float *right, float chi2_mono, float chi2_stereo, int check_right)
{
    /* test 1: the octaves level - 1 .. level of the table */
    const int olo = o.level - 1 < 0 ? 0 : o.level - 1;
    if (octave < olo || octave > o.level) return 1;
    /* test 2 */
    if (!(fabsf(x - o.u) < o.radius && fabsf(y - o.v) < o.radius)) return 2;
    /* test 3 */
    if (taken && taken[row] != 0) return 3;
    /* test 4 */
    if (chi2_mono > 0.0f) {
        const float ex = o.u - x, ey = o.v - y;
        float e2 = ex * ex + ey * ey, limit = chi2_mono;
        if (check_right && right) {
            const float ur = right[row];
            if (ur >= 0.0f) {
                const float er = o.u_right - ur;
                e2 = e2 + er * er;
                limit = chi2_stereo;
            }
        }
        const float s = octave == o.level ? s_hi : s_lo;
        if (!(e2 <= limit * (s * s))) return 4;
    }
    return 0;
}

#endif
