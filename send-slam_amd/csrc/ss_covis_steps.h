/*
 * ss_covis_steps.h -- the steps of the covisibility family (the rule: include/sendslam_orb.h): the compact
 * incidence lists of a map, a record's packed form, the visit of one record of a point's list from a row, the closing of an item's
 * culling terms, the sort key of a neighbour, the redundancy verdict, and a whole row on the host.  The kernels (ss_covis.hip), the
 * host twins ss_covis_kf_host / ss_covis_frames_host (ss_api_search.cpp) and tests/native/covis_steps_asan.cpp compile this text.
 *
 * All of it is integer, except ss_covis_redundant: one float multiply and one compare.  Compile with -ffp-contract=off.
 */
#ifndef SS_COVIS_STEPS_H
#define SS_COVIS_STEPS_H

#include <algorithm>
#include <vector>

#include "../../include/sendslam_orb.h"
#include "ss_float_steps.h" /* SS_HD */

/* One record of a point's list in 32 bits: kf in bits 0 .. 13, the octave in bits 14 .. 21 (an observation's only), bit 29: the
 * record is an observation, bit 30: it is stereo, bit 31: its skip byte is set */
#define SS_COVIS_KF_BITS 14
#define SS_COVIS_KF_MASK 16383u
static_assert(SS_GBA_MAX_KF == 1 << SS_COVIS_KF_BITS, "a keyframe number fits the low bits of a record and of a sort key");
static_assert(SS_MAX_LEVELS <= 256, "an octave fits eight bits");
static_assert(((uint64_t)SS_COVIS_MAX_ROW_ITEMS << SS_COVIS_KF_BITS | SS_COVIS_KF_MASK) <= 0xffffffffull && SS_GUIDED_MAX_ROWS <= SS_COVIS_MAX_ROW_ITEMS,
              "a weight and a keyframe number are one 32-bit key, for a keyframe row and a frame row");

SS_HD uint32_t ss_covis_pack(int kf, int octave, int n_levels, bool stereo, bool skip)
{
    const bool valid = octave >= 0 && octave < n_levels;
    return (uint32_t)kf | (valid ? ((uint32_t)octave << SS_COVIS_KF_BITS) | (1u << 29) : 0u) | (stereo ? 1u << 30 : 0u) | (skip ? 1u << 31 : 0u);
}
SS_HD int ss_covis_kf(uint32_t r) { return (int)(r & SS_COVIS_KF_MASK); }
SS_HD int ss_covis_octave(uint32_t r) { return (int)((r >> SS_COVIS_KF_BITS) & 255u); }
SS_HD bool ss_covis_valid(uint32_t r) { return ((r >> 29) & 1u) != 0; }
SS_HD int ss_covis_stereo(uint32_t r) { return (int)((r >> 30) & 1u); }
SS_HD bool ss_covis_skip(uint32_t r) { return (r >> 31) != 0; }

/* One record r of a point's list seen from a row (self: the row's keyframe relative to its problem, -1 for a frame row; own_oct: the
 * octave of the row's own record of the point).  Returns the keyframe the record votes for, or -1; adds the record's part to the
 * point's count(i) and near */
SS_HD int ss_covis_visit(uint32_t r, int self, int own_oct, int slack, int *count, int *near)
{
    if (!ss_covis_valid(r)) return -1;
    *count += 1 + ss_covis_stereo(r);
    const int kf = ss_covis_kf(r);
    if (kf == self) return -1;
    if (ss_covis_octave(r) <= own_oct + slack) *near += 1;
    return kf;
}

/* the culling terms of a keyframe row's item once its point's list has been visited; own is the row's own record of the point */
SS_HD void ss_covis_close(uint32_t own, int count, int near, int cull_obs, int *n_mps, int *n_redundant)
{
    if (ss_covis_skip(own)) return;
    *n_mps += 1;
    if (count > cull_obs && near > cull_obs) *n_redundant += 1;
}

/* weight descending, then kf ascending, is key descending */
SS_HD uint32_t ss_covis_key(int weight, int kf) { return ((uint32_t)weight << SS_COVIS_KF_BITS) | (SS_COVIS_KF_MASK - (uint32_t)kf); }
SS_HD int ss_covis_key_weight(uint32_t key) { return (int)(key >> SS_COVIS_KF_BITS); }
SS_HD int ss_covis_key_kf(uint32_t key) { return (int)(SS_COVIS_KF_MASK - (key & SS_COVIS_KF_MASK)); }

SS_HD int ss_covis_redundant(int n_redundant, int n_mps, float th)
{
    const float bound = th * (float)n_mps;
    return (float)n_redundant > bound ? 1 : 0;
}

/* The hits of a frame row: row i of the block counts iff i < n and idx >= 0 */
SS_HD int ss_covis_clamp_rows(int n_points, int point_rows) { return n_points < 0 ? 0 : (n_points > point_rows ? point_rows : n_points); }

/* a problem of the map as the tables hold it */
struct ss_covis_prob {
    int32_t first_kf, n_kf, first_block, n_blocks;
};

/* The map's tables, on the host or on the device.  Keyframe and block numbers index the call's arrays; a point's number is block *
 * point_rows + row of the call; pt_off / kf_off index pt_item / kf_item of the whole map (the problems' records one after the
 * other); what pt_item holds (kf) is relative to the problem */
struct ss_covis_tab {
    int n_kf = 0, n_blocks = 0, point_rows = 0, n_problems = 0, max_kf = 0;
    const ss_covis_prob *prob = nullptr;                /* [n_problems] */
    const int32_t *kf_prob = nullptr, *blk_prob = nullptr; /* [n_kf], [n_blocks]: the problem, or -1 */
    const int32_t *kf_off = nullptr, *kf_cnt = nullptr; /* [n_kf]: the keyframe's run of kf_item */
    const int32_t *pt_off = nullptr, *pt_cnt = nullptr; /* [n_blocks * point_rows]: the point's run of pt_item */
    const uint32_t *pt_item = nullptr;                  /* [records]: ss_covis_pack, a point's run in ascending kf */
    const int32_t *kf_item = nullptr;                   /* [records][2]: the point, the record's place in the point's run */
};

/* The lists of one problem of n_kf keyframes and P points from its n records in any order (skip: one byte per record, or NULL).
 * pt_off, pt_cnt [P], kf_off, kf_cnt [n_kf], pt_item [n], kf_item [n][2]; the offsets stored start at item_base, the points at
 * point_base.  Two stable counting passes, first by kf, then by point, as ss_gba_tables.  Returns 0, or 1: a kf outside the problem,
 * 2: a point outside it, 3: a (kf, point) pair twice, 4: a keyframe with more than SS_COVIS_MAX_ROW_ITEMS records; *bad is then the
 * offending record's number in obs.  from (NULL: not wanted) [n]: the record of obs that stands at each place of pt_item */
static inline int ss_covis_tables(int n_kf, int P, const ss_gba_obs *obs, const uint8_t *skip, int n, int n_levels, bool check_right, int item_base, int point_base,
                                  int32_t *pt_off, int32_t *pt_cnt, int32_t *kf_off, int32_t *kf_cnt, uint32_t *pt_item, int32_t *kf_item, int *bad,
                                  int32_t *from = nullptr)
{
    for (int k = 0; k < n_kf; k++) kf_cnt[k] = 0;
    for (int i = 0; i < P; i++) pt_cnt[i] = 0;
    for (int m = 0; m < n; m++) {
        *bad = m;
        if (obs[m].kf < 0 || obs[m].kf >= n_kf) return 1;
        if (obs[m].point < 0 || obs[m].point >= P) return 2;
        if (kf_cnt[obs[m].kf] >= SS_COVIS_MAX_ROW_ITEMS) return 4;
        kf_cnt[obs[m].kf]++, pt_cnt[obs[m].point]++;
    }
    int at = 0;
    for (int k = 0; k < n_kf; k++) kf_off[k] = at, at += kf_cnt[k], kf_cnt[k] = 0;
    std::vector<int32_t> by_kf((size_t)n + 1), orig((size_t)n + 1);
    for (int m = 0; m < n; m++) by_kf[(size_t)(kf_off[obs[m].kf] + kf_cnt[obs[m].kf]++)] = m;
    at = 0;
    for (int i = 0; i < P; i++) pt_off[i] = at, at += pt_cnt[i], pt_cnt[i] = 0;
    for (int j = 0; j < n; j++) {
        const int m = by_kf[(size_t)j];
        const ss_gba_obs &o = obs[m];
        const int s = pt_off[o.point] + pt_cnt[o.point]++;
        pt_item[s] = ss_covis_pack(o.kf, o.octave, n_levels, check_right && o.right > 0.0f, skip && skip[m] != 0);
        orig[(size_t)s] = m;
        if (from) from[s] = m;
    }
    for (int k = 0; k < n_kf; k++) kf_cnt[k] = 0;
    for (int i = 0; i < P; i++)
        for (int e = 0; e < pt_cnt[i]; e++) {
            const int s = pt_off[i] + e, k = ss_covis_kf(pt_item[s]);
            if (e > 0 && k == ss_covis_kf(pt_item[s - 1])) {
                *bad = orig[(size_t)s];
                return 3;
            }
            int32_t *item = kf_item + 2 * (size_t)(kf_off[k] + kf_cnt[k]++);
            item[0] = point_base + i, item[1] = e;
        }
    for (int k = 0; k < n_kf; k++) kf_off[k] += item_base;
    for (int i = 0; i < P; i++) pt_off[i] += item_base;
    return 0;
}

/* One row on the host.  kf: the call's keyframe number of a keyframe row, or -1: a frame row on block `block` with the hits of idx
 * [point_rows] under n_points of the block.  nb [cap][2], out: the row.  w is scratch of max_kf counters */
static inline void ss_covis_row_host(const ss_covis_tab &m, int kf, int block, const int32_t *idx, int n_points, const ss_covis_params &p, int cap, int32_t *nb,
                                     ss_covis_row *out, std::vector<int32_t> &w)
{
    const int q = kf >= 0 ? m.kf_prob[kf] : m.blk_prob[block];
    const int n_kf = q >= 0 ? m.prob[q].n_kf : 0;
    w.assign((size_t)n_kf + 1, 0);
    int n_mps = 0, n_red = 0;
    if (q >= 0 && kf >= 0) {
        const int self = kf - m.prob[q].first_kf;
        for (int t = 0; t < m.kf_cnt[kf]; t++) {
            const int32_t *item = m.kf_item + 2 * (size_t)(m.kf_off[kf] + t);
            const int off = m.pt_off[item[0]], cnt = m.pt_cnt[item[0]];
            const uint32_t own = m.pt_item[off + item[1]];
            if (!ss_covis_valid(own)) continue;
            int count = 0, near = 0;
            for (int e = 0; e < cnt; e++) {
                const int j = ss_covis_visit(m.pt_item[off + e], self, ss_covis_octave(own), p.cull_slack, &count, &near);
                if (j >= 0) w[(size_t)j]++;
            }
            ss_covis_close(own, count, near, p.cull_obs, &n_mps, &n_red);
        }
    } else if (q >= 0) {
        const int n = ss_covis_clamp_rows(n_points, m.point_rows);
        for (int i = 0; i < n; i++) {
            if (idx[i] < 0) continue;
            const size_t gp = (size_t)block * m.point_rows + i;
            int count = 0, near = 0;
            for (int e = 0; e < m.pt_cnt[gp]; e++) {
                const int j = ss_covis_visit(m.pt_item[m.pt_off[gp] + e], -1, 0, 0, &count, &near);
                if (j >= 0) w[(size_t)j]++;
            }
        }
    }
    std::vector<uint32_t> keys;
    uint32_t best = 0;
    int n_shared = 0;
    for (int j = 0; j < n_kf; j++) {
        if (w[(size_t)j] <= 0) continue;
        n_shared++;
        best = std::max(best, ss_covis_key(w[(size_t)j], j));
        if (w[(size_t)j] >= p.min_weight) keys.push_back(ss_covis_key(w[(size_t)j], j));
    }
    if (keys.empty() && p.fallback != 0 && best != 0) keys.push_back(best);
    std::sort(keys.begin(), keys.end(), [](uint32_t a, uint32_t b) { return a > b; });
    const int n_listed = (int)keys.size(), n_written = std::min(n_listed, cap);
    for (int e = 0; e < cap; e++) {
        nb[2 * e] = e < n_written ? ss_covis_key_kf(keys[(size_t)e]) : -1;
        nb[2 * e + 1] = e < n_written ? ss_covis_key_weight(keys[(size_t)e]) : 0;
    }
    out->n_shared = n_shared, out->max_weight = best ? ss_covis_key_weight(best) : 0, out->max_kf = best ? ss_covis_key_kf(best) : -1;
    out->n_listed = n_listed, out->n_written = n_written;
    out->n_mps = n_mps, out->n_redundant = n_red, out->redundant = ss_covis_redundant(n_red, n_mps, p.redundant_th);
}

#endif
