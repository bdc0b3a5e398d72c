/*
 * ss_refresh_steps.h -- the steps of the map-point refresh (the rule: include/sendslam_orb.h): the term of one
 * observation, the 64-slot tree, the reference choice, the depth range, one pair distance, the rank select, the winner's key, and a
 * whole point row on the host.  The kernels (ss_refresh.hip), the host twin ss_refresh_host (ss_api_search.cpp) and
 * tests/native/refresh_steps_asan.cpp compile this text.
 *
 * The geometry is double from float32 inputs widened, one IEEE operation per step as written; the descriptor choice is integer and
 * order-free.  Compile with -ffp-contract=off.
 */
#ifndef SS_REFRESH_STEPS_H
#define SS_REFRESH_STEPS_H

#include <string.h>

#include <vector>

#include "../../include/sendslam_orb.h"
#include "ss_covis_steps.h"
#include "ss_gn_steps.h" /* ss_gn_is_finite */

#define SS_REFRESH_SLOTS 64 /* the partial sums of a normal's tree: slot s adds the terms s, s + 64, ... */
#define SS_REFRESH_SHORT 64 /* a point's list of at most this many records is one wave's; a longer one a workgroup's */
static_assert(sizeof(ss_refresh_params) == 32 && sizeof(ss_refresh_info) == 32 && sizeof(ss_refresh_summary) == 32, "the layouts of the header");
static_assert(SS_GBA_MAX_KF <= 1 << SS_COVIS_KF_BITS, "an observation's number fits the low 14 bits of the winner's key");

/* row i of a block is refreshed iff i < n_points (clamped), its select byte is 0 and x, y, z are finite */
SS_HD bool ss_refresh_selected(int i, int n_points, int point_rows, int select, float x, float y, float z)
{
    return i < ss_covis_clamp_rows(n_points, point_rows) && select == 0 && ss_gn_is_finite((double)x) && ss_gn_is_finite((double)y) && ss_gn_is_finite((double)z);
}

/* The term of one observation: t = (P - ow) / len.  False when len is not > 0 or not finite */
SS_HD bool ss_refresh_term(float x, float y, float z, const float *ow, double t[3], double *len)
{
    const double dx = (double)x - (double)ow[0], dy = (double)y - (double)ow[1], dz = (double)z - (double)ow[2];
    const double l = sqrt((dx * dx + dy * dy) + dz * dz);
    t[0] = dx / l, t[1] = dy / l, t[2] = dz / l;
    *len = l;
    return l > 0.0 && ss_gn_is_finite(l);
}

/* the fold of one 64-slot group of ss_gn_tree: a[l] += a[l + h], h = 32 .. 1 (the kernels: gn_wave_fold of ss_gn.h) */
SS_HD double ss_refresh_fold(double a[SS_REFRESH_SLOTS])
{
    for (int h = 32; h >= 1; h >>= 1)
        for (int l = 0; l < h; l++) a[l] = a[l] + a[l + h];
    return a[0];
}

SS_HD float ss_refresh_normal(double sum, int n) { return (float)(sum / (double)n); }

/* the reference choice: record r is the reference iff it is an observation of keyframe ref_kf; with none, observation 0 is */
SS_HD bool ss_refresh_is_ref(uint32_t r, int ref_kf) { return ss_covis_valid(r) && ss_covis_kf(r) == ref_kf; }

/* the depth range from the reference's distance and octave */
SS_HD void ss_refresh_depth(double dist, const float *scale, int level, int n_levels, float *min_dist, float *max_dist)
{
    const double mx = dist * (double)scale[level];
    const double mn = mx / (double)scale[n_levels - 1];
    *max_dist = (float)mx, *min_dist = (float)mn;
}

/* one pair distance: all 256 bits */
SS_HD int ss_refresh_dist(const uint32_t a[8], const uint32_t b[8])
{
    int d = 0;
    for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]);
    return d;
}

/* the rank of the median in a row of n distances, the self distance included (upstream: 0.5 * (N - 1), truncated) */
SS_HD int ss_refresh_rank(int n) { return (n - 1) / 2; }

/* The rank select: the smallest v in 0 .. 256 with count(v) >= need, count(v) being the number of a row's distances <= v (so
 * count(256) = n >= need), by nine halvings of 0 .. 256: the trip count is fixed */
template <class Count> SS_HD int ss_refresh_select(int need, Count count)
{
    int lo = 0, hi = 256;
    for (int it = 0; it < 9; it++) {
        const int mid = (lo + hi) >> 1;
        const bool enough = count(mid) >= need;
        hi = enough ? mid : hi, lo = enough ? lo : (mid < 256 ? mid + 1 : 256);
    }
    return lo;
}

/* the winner is the lowest key: the lowest median, then the lowest observation number */
SS_HD uint32_t ss_refresh_key(int median, int a) { return ((uint32_t)median << SS_COVIS_KF_BITS) | (uint32_t)a; }
SS_HD int ss_refresh_key_median(uint32_t key) { return (int)(key >> SS_COVIS_KF_BITS); }
SS_HD int ss_refresh_key_obs(uint32_t key) { return (int)(key & SS_COVIS_KF_MASK); }

SS_HD ss_refresh_info ss_refresh_info_none(int state, int n_obs, int count) { return ss_refresh_info{state, n_obs, count, -1, -1, -1, -1, 0}; }

/* what a refresh reads besides the map's tables, on the host */
struct ss_refresh_host_in {
    const int32_t *pt_row = nullptr;  /* [records], in the order of pt_item; NULL without descriptor */
    const int32_t *n_points = nullptr; /* [n_blocks] */
    const int32_t *ref_kf = nullptr;   /* [n_blocks][point_rows] or NULL */
    const uint8_t *select = nullptr;   /* [n_blocks][point_rows] or NULL */
    const uint8_t *desc = nullptr;     /* [n_kf][rows_per_frame][32] */
    int rows_per_frame = 0;
    const float *ow = nullptr;         /* [n_kf][3] */
    const float *scale = nullptr;
    int n_levels = 0, geometry = 1, descriptor = 1;
};

/* One point row on the host: row i of block b of the map m.  Writes the info, and the point's fields and descriptor on state 0 */
static inline void ss_refresh_row_host(const ss_covis_tab &m, const ss_refresh_host_in &in, int b, int i, ss_map_point *points, uint8_t *point_desc, ss_refresh_info *info)
{
    const size_t gp = (size_t)b * m.point_rows + i;
    const int q = m.blk_prob[b];
    ss_map_point &P = points[gp];
    if (q < 0 || !ss_refresh_selected(i, in.n_points[b], m.point_rows, in.select ? in.select[gp] : 0, P.x, P.y, P.z)) {
        info[gp] = ss_refresh_info_none(-1, 0, 0);
        return;
    }
    const int first_kf = m.prob[q].first_kf, off = m.pt_off[gp], cnt = m.pt_cnt[gp];
    std::vector<int> at; /* the observations' places in the run */
    int count = 0, ref_a = 0;
    for (int e = 0; e < cnt; e++) {
        const uint32_t r = m.pt_item[off + e];
        if (!ss_covis_valid(r)) continue;
        if (in.ref_kf && ss_refresh_is_ref(r, in.ref_kf[gp])) ref_a = (int)at.size();
        count += 1 + ss_covis_stereo(r);
        at.push_back(off + e);
    }
    const int n = (int)at.size();
    if (n == 0) {
        info[gp] = ss_refresh_info_none(1, 0, 0);
        return;
    }
    ss_refresh_info out = ss_refresh_info_none(0, n, count);
    float geo[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (in.geometry) {
        double slot[3][SS_REFRESH_SLOTS], dist = 0.0;
        for (int c = 0; c < 3; c++)
            for (int s = 0; s < SS_REFRESH_SLOTS; s++) slot[c][s] = 0.0;
        bool ok = true;
        for (int a = 0; a < n; a++) {
            double t[3], len;
            ok = ss_refresh_term(P.x, P.y, P.z, in.ow + 3 * (size_t)(first_kf + ss_covis_kf(m.pt_item[at[(size_t)a]])), t, &len) && ok;
            for (int c = 0; c < 3; c++) slot[c][a % SS_REFRESH_SLOTS] = slot[c][a % SS_REFRESH_SLOTS] + t[c];
            if (a == ref_a) dist = len;
        }
        if (!ok) {
            info[gp] = ss_refresh_info_none(2, n, count);
            return;
        }
        for (int c = 0; c < 3; c++) geo[c] = ss_refresh_normal(ss_refresh_fold(slot[c]), n);
        const uint32_t ref = m.pt_item[at[(size_t)ref_a]];
        out.ref_kf = ss_covis_kf(ref), out.level = ss_covis_octave(ref);
        ss_refresh_depth(dist, in.scale, out.level, in.n_levels, &geo[3], &geo[4]);
    }
    if (in.descriptor) {
        std::vector<uint32_t> w((size_t)n * 8);
        for (int a = 0; a < n; a++) {
            const int s = at[(size_t)a];
            memcpy(&w[(size_t)a * 8], in.desc + ((size_t)(first_kf + ss_covis_kf(m.pt_item[s])) * in.rows_per_frame + in.pt_row[s]) * 32, 32);
        }
        uint32_t best = 0xffffffffu;
        const int need = ss_refresh_rank(n) + 1;
        for (int a = 0; a < n; a++) {
            int cum[257];
            for (int v = 0; v <= 256; v++) cum[v] = 0;
            for (int o = 0; o < n; o++) cum[ss_refresh_dist(&w[(size_t)a * 8], &w[(size_t)o * 8])]++;
            for (int v = 1; v <= 256; v++) cum[v] += cum[v - 1];
            const uint32_t key = ss_refresh_key(ss_refresh_select(need, [&](int v) { return cum[v]; }), a);
            best = key < best ? key : best;
        }
        const int a = ss_refresh_key_obs(best);
        out.best_kf = ss_covis_kf(m.pt_item[at[(size_t)a]]), out.best_median = ss_refresh_key_median(best);
        memcpy(point_desc + gp * 32, &w[(size_t)a * 8], 32);
    }
    if (in.geometry) P.nx = geo[0], P.ny = geo[1], P.nz = geo[2], P.min_dist = geo[3], P.max_dist = geo[4];
    info[gp] = out;
}

/* the summary of block b from its rows' infos */
static inline void ss_refresh_summary_host(const ss_covis_tab &m, int b, int n_points, const ss_refresh_info *info, ss_refresh_summary *out)
{
    ss_refresh_summary s = {SS_OK, m.blk_prob[b] >= 0 ? ss_covis_clamp_rows(n_points, m.point_rows) : 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < m.point_rows; i++) {
        const ss_refresh_info &r = info[(size_t)b * m.point_rows + i];
        if (r.state < 0) continue;
        s.n_selected++;
        s.n_refreshed += r.state == 0, s.n_no_obs += r.state == 1, s.n_degenerate += r.state == 2;
        s.max_obs = r.n_obs > s.max_obs ? r.n_obs : s.max_obs;
    }
    *out = s;
}

#endif
