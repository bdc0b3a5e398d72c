/*
 * ss_proj_steps.h -- steps 1 - 3 of the map-point projection search (the rule: include/sendslam_orb.h):
 * frustum, predicted level, window.  k_proj_search (ss_proj.hip), the host twin ss_proj_points_host (ss_api_search.cpp) and
 * tests/native/proj_steps_asan.cpp compile this text.
 *
 * Every float step is one float32 IEEE operation, left to right as written; every test is in its accepting form, so a NaN
 * fails it.  Compile with -ffp-contract=off.  The division and sqrtf are correctly rounded on both sides (hipcc's default).
 */
#ifndef SS_PROJ_STEPS_H
#define SS_PROJ_STEPS_H

#include "../../include/sendslam_orb.h"
#include "ss_float_steps.h" /* SS_HD, math.h */

/* what step 1 rejects: the number of the first failing test in state, floats 0.0f, level -1 */
SS_HD ss_proj_point ss_proj_rejected(int state)
{
    ss_proj_point o;
    o.u = o.v = o.u_right = o.view_cos = o.dist = o.radius = 0.0f;
    o.level = -1;
    o.state = state;
    return o;
}

/* step 2: the smallest n in 0 .. n_levels - 1 with ratio <= scale[n], else n_levels - 1 (a NaN ratio too); *scale_n is that
 * entry.  The scan runs downwards and keeps the last hit, so the index it returns is one it has read: it cannot leave the table */
SS_HD int ss_proj_level(float ratio, const float *scale, int n_levels, float *scale_n)
{
    const int n_lv = n_levels < 1 ? 1 : n_levels > SS_MAX_LEVELS ? SS_MAX_LEVELS : n_levels;
    int level = n_lv - 1;
    float s = scale[n_lv - 1];
    for (int n = n_lv - 2; n >= 0; n--) {
        if (ratio <= scale[n]) {
            level = n;
            s = scale[n];
        }
    }
    *scale_n = s;
    return level;
}

/* steps 1 - 3 of one map point */
SS_HD ss_proj_point ss_proj_eval(const ss_proj_view &w, const ss_map_point &p, float view_cos_limit, float th, float far_limit,
                                 const float *scale, int n_levels)
{
    /* test 1 */
    const float pcx = ((w.rcw[0] * p.x + w.rcw[1] * p.y) + w.rcw[2] * p.z) + w.tcw[0];
    const float pcy = ((w.rcw[3] * p.x + w.rcw[4] * p.y) + w.rcw[5] * p.z) + w.tcw[1];
    const float pcz = ((w.rcw[6] * p.x + w.rcw[7] * p.y) + w.rcw[8] * p.z) + w.tcw[2];
    if (!(pcz > 0.0f)) return ss_proj_rejected(1);
    /* test 2 */
    const float invz = 1.0f / pcz;
    const float u = w.fx * pcx * invz + w.cx;
    const float v = w.fy * pcy * invz + w.cy;
    if (!(u >= w.min_x && u <= w.max_x && v >= w.min_y && v <= w.max_y)) return ss_proj_rejected(2);
    /* test 3 */
    const float pox = p.x - w.ow[0], poy = p.y - w.ow[1], poz = p.z - w.ow[2];
    const float dist = sqrtf((pox * pox + poy * poy) + poz * poz);
    if (!(dist >= 0.8f * p.min_dist && dist <= 1.2f * p.max_dist)) return ss_proj_rejected(3);
    /* test 4 */
    const float view_cos = ((pox * p.nx + poy * p.ny) + poz * p.nz) / dist;
    if (!(view_cos >= view_cos_limit)) return ss_proj_rejected(4);
    /* test 5 */
    if (far_limit > 0.0f && !(dist <= far_limit)) return ss_proj_rejected(5);
    /* level, window */
    const float ratio = p.max_dist / dist;
    float s;
    ss_proj_point o;
    o.level = ss_proj_level(ratio, scale, n_levels, &s);
    const float r = (view_cos > 0.998f ? 2.5f : 4.0f) * th;
    o.radius = r * s;
    o.u = u;
    o.v = v;
    o.u_right = u - w.bf * invz;
    o.view_cos = view_cos;
    o.dist = dist;
    o.state = 0;
    return o;
}

#endif
