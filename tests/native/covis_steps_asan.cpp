/* The steps of the covisibility family (csrc/ss_covis_steps.h, the text the kernels and the host twins compile) as a stand-alone
 * program for -fsanitize=address,undefined: the table builder and whole rows on random, empty and refused tables, octaves at
 * INT32_MIN / INT32_MAX, both ends of the record's and the key's packing, and a keyframe at the row-item limit and one past it.
 * Every row is held to a direct count on the records.  Prints "ok <rows evaluated>". */
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "ss_covis_steps.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("failed %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

struct built {
    std::vector<ss_covis_prob> prob;
    std::vector<int32_t> kf_prob, blk_prob, pt_off, pt_cnt, kf_off, kf_cnt, kf_item;
    std::vector<uint32_t> pt_item;
    ss_covis_tab m;
};

/* one problem of n_kf keyframes and P points in one block of max(P, 1) rows; the vectors are sized exactly, so a stray index is a
 * sanitizer report */
static int build(built &b, int n_kf, int P, const std::vector<ss_gba_obs> &obs, const std::vector<uint8_t> &skip, int n_levels, bool check_right, int *bad)
{
    const int n = (int)obs.size();
    b.prob.assign(1, ss_covis_prob{0, n_kf, 0, 1});
    b.kf_prob.assign((size_t)n_kf, 0), b.blk_prob.assign(1, 0);
    b.pt_off.assign((size_t)std::max(P, 1), 0), b.pt_cnt.assign((size_t)std::max(P, 1), 0), b.kf_off.assign((size_t)n_kf, 0), b.kf_cnt.assign((size_t)n_kf, 0);
    b.pt_item.assign((size_t)n, 0u), b.kf_item.assign(2 * (size_t)n, 0);
    const int why = ss_covis_tables(n_kf, P, obs.data(), skip.empty() ? nullptr : skip.data(), n, n_levels, check_right, 0, 0, b.pt_off.data(), b.pt_cnt.data(),
                                    b.kf_off.data(), b.kf_cnt.data(), b.pt_item.data(), b.kf_item.data(), bad);
    b.m = ss_covis_tab();
    b.m.n_kf = n_kf, b.m.n_blocks = 1, b.m.point_rows = std::max(P, 1), b.m.n_problems = 1, b.m.max_kf = n_kf;
    b.m.prob = b.prob.data(), b.m.kf_prob = b.kf_prob.data(), b.m.blk_prob = b.blk_prob.data();
    b.m.kf_off = b.kf_off.data(), b.m.kf_cnt = b.kf_cnt.data(), b.m.pt_off = b.pt_off.data(), b.m.pt_cnt = b.pt_cnt.data();
    b.m.pt_item = b.pt_item.data(), b.m.kf_item = b.kf_item.data();
    return why;
}

/* the weights of keyframe row k counted directly on the records */
static std::map<int, int> direct_weights(const std::vector<ss_gba_obs> &obs, int n_levels, int k)
{
    std::map<int, std::vector<int>> seen;
    for (const ss_gba_obs &o : obs)
        if (o.octave >= 0 && o.octave < n_levels) seen[o.point].push_back(o.kf);
    std::map<int, int> w;
    for (const auto &pt : seen)
        if (std::find(pt.second.begin(), pt.second.end(), k) != pt.second.end())
            for (int j : pt.second)
                if (j != k) w[j]++;
    return w;
}

static long random_maps(uint32_t &s)
{
    long rows = 0;
    for (int round = 0; round < 60; round++) {
        const int n_kf = 1 + (int)(lcg(s) % 40u), P = (int)(lcg(s) % 90u), n_levels = 1 + (int)(lcg(s) % 16u);
        std::vector<ss_gba_obs> obs;
        std::vector<uint8_t> skip;
        for (int i = 0; i < P; i++)
            for (int k = 0; k < n_kf; k++) {
                if (lcg(s) % 5u != 0u) continue;
                const uint32_t pick = lcg(s) % 12u;
                const int32_t octave = pick == 0 ? INT32_MIN : pick == 1 ? INT32_MAX : pick == 2 ? -1 : pick == 3 ? n_levels : (int32_t)(lcg(s) % (uint32_t)n_levels);
                obs.push_back(ss_gba_obs{k, i, 0.0f, 0.0f, (lcg(s) & 1u) ? 3.0f : -1.0f, octave});
                skip.push_back((uint8_t)(lcg(s) % 7u == 0u ? 1 : 0));
            }
        for (size_t a = obs.size(); a > 1; a--) { /* any order */
            const size_t c = lcg(s) % a;
            std::swap(obs[a - 1], obs[c]), std::swap(skip[a - 1], skip[c]);
        }
        built b;
        int bad = -1;
        CHECK(build(b, n_kf, P, obs, skip, n_levels, (round & 1) != 0, &bad) == 0);
        ss_covis_params p = {1 + (int)(lcg(s) % 4u), (int)(lcg(s) & 1u), (int)(lcg(s) % 4u), (int)(lcg(s) % 3u), 0.5f, {0, 0, 0}};
        const int cap = 1 + (int)(lcg(s) % 12u);
        std::vector<int32_t> nb((size_t)cap * 2), w;
        for (int k = 0; k < n_kf; k++, rows++) {
            ss_covis_row r;
            ss_covis_row_host(b.m, k, 0, nullptr, 0, p, cap, nb.data(), &r, w);
            const std::map<int, int> want = direct_weights(obs, n_levels, k);
            int listed = 0, best_w = 0, best_j = -1;
            for (const auto &jw : want) {
                listed += jw.second >= p.min_weight ? 1 : 0;
                if (jw.second > best_w) best_w = jw.second, best_j = jw.first;
            }
            if (listed == 0 && p.fallback && best_j >= 0) listed = 1;
            CHECK(r.n_shared == (int)want.size() && r.max_weight == best_w && r.max_kf == best_j && r.n_listed == listed && r.n_written == std::min(listed, cap));
            for (int e = 0; e < cap; e++) {
                if (e >= r.n_written) {
                    CHECK(nb[2 * e] == -1 && nb[2 * e + 1] == 0);
                    continue;
                }
                CHECK(want.at(nb[2 * e]) == nb[2 * e + 1]);
                CHECK(e == 0 || nb[2 * e - 1] > nb[2 * e + 1] || (nb[2 * e - 1] == nb[2 * e + 1] && nb[2 * e - 2] < nb[2 * e]));
            }
            CHECK(r.n_redundant <= r.n_mps && r.n_mps <= b.kf_cnt[(size_t)k] && (r.redundant == 0 || r.redundant == 1));
        }
        /* frame rows on the same map: every row a hit, every other row, none; counts past the block and below 0 */
        std::vector<int32_t> idx((size_t)std::max(P, 1));
        for (int form = 0; form < 4; form++, rows++) {
            for (size_t i = 0; i < idx.size(); i++) idx[i] = form == 0 ? INT32_MAX : form == 1 ? ((i & 1) ? 0 : -1) : form == 2 ? INT32_MIN : 7;
            ss_covis_row r;
            ss_covis_row_host(b.m, -1, 0, idx.data(), form == 3 ? -5 : P + 100, p, cap, nb.data(), &r, w);
            CHECK(r.n_mps == 0 && r.n_redundant == 0 && r.redundant == 0 && r.n_written <= cap);
            if (form >= 2) CHECK(r.n_shared == 0 && r.max_kf == -1);
        }
    }
    return rows;
}

static long refused_and_empty()
{
    built b;
    int bad = -1;
    std::vector<uint8_t> none;
    CHECK(build(b, 3, 0, {}, none, 8, false, &bad) == 0); /* no point, no record */
    ss_covis_params p = {15, 1, 3, 1, 0.9f, {0, 0, 0}};
    std::vector<int32_t> nb(8), w;
    ss_covis_row r;
    ss_covis_row_host(b.m, 2, 0, nullptr, 0, p, 4, nb.data(), &r, w);
    CHECK(r.n_shared == 0 && r.max_kf == -1 && r.n_listed == 0 && nb[0] == -1 && nb[7] == 0);
    const ss_gba_obs a = {0, 0, 0, 0, -1, 0}, k_out = {3, 0, 0, 0, -1, 0}, k_neg = {-1, 0, 0, 0, -1, 0}, p_out = {0, 2, 0, 0, -1, 0}, p_neg = {0, INT32_MIN, 0, 0, -1, 0};
    CHECK(build(b, 3, 2, {a, k_out}, none, 8, false, &bad) == 1 && bad == 1);
    CHECK(build(b, 3, 2, {k_neg}, none, 8, false, &bad) == 1 && bad == 0);
    CHECK(build(b, 3, 2, {a, a, p_out}, none, 8, false, &bad) == 2 && bad == 2);
    CHECK(build(b, 3, 2, {p_neg}, none, 8, false, &bad) == 2 && bad == 0);
    const ss_gba_obs other = {1, 0, 0, 0, -1, 0}, twice = {0, 0, 0, 0, 5.0f, INT32_MAX};
    CHECK(build(b, 3, 2, {a, other, twice}, none, 8, false, &bad) == 3 && (bad == 2 || bad == 0));
    return 6;
}

static long packing_ends()
{
    const uint32_t r = ss_covis_pack(16383, 15, 16, true, true), q = ss_covis_pack(16383, INT32_MAX, 16, false, false), z = ss_covis_pack(0, INT32_MIN, 16, false, true);
    CHECK(ss_covis_kf(r) == 16383 && ss_covis_octave(r) == 15 && ss_covis_valid(r) && ss_covis_stereo(r) == 1 && ss_covis_skip(r));
    CHECK(ss_covis_kf(q) == 16383 && !ss_covis_valid(q) && ss_covis_stereo(q) == 0 && !ss_covis_skip(q));
    CHECK(ss_covis_kf(z) == 0 && !ss_covis_valid(z) && ss_covis_skip(z));
    const uint32_t top = ss_covis_key(SS_COVIS_MAX_ROW_ITEMS, 0), low = ss_covis_key(1, 16383);
    CHECK(top == 0xffffffffu && ss_covis_key_weight(top) == SS_COVIS_MAX_ROW_ITEMS && ss_covis_key_kf(top) == 0);
    CHECK(low == 1u << 14 && ss_covis_key_weight(low) == 1 && ss_covis_key_kf(low) == 16383);
    CHECK(ss_covis_key(5, 3) > ss_covis_key(5, 4) && ss_covis_key(6, 9) > ss_covis_key(5, 0));
    CHECK(ss_covis_redundant(9, 10, 0.9f) == 0 && ss_covis_redundant(10, 10, 0.9f) == 1 && ss_covis_redundant(0, 0, 0.0f) == 0 && ss_covis_redundant(INT32_MAX, INT32_MAX, 1.0f) == 0);
    CHECK(ss_covis_clamp_rows(INT32_MIN, 5) == 0 && ss_covis_clamp_rows(INT32_MAX, 5) == 5 && ss_covis_clamp_rows(3, 5) == 3);
    int count = 0, near = 0;
    CHECK(ss_covis_visit(r, -1, 0, 16, &count, &near) == 16383 && count == 2 && near == 1);
    CHECK(ss_covis_visit(r, 16383, 255, 16, &count, &near) == -1 && count == 4 && near == 1);
    CHECK(ss_covis_visit(q, 0, 0, 0, &count, &near) == -1 && count == 4);
    return 5;
}

/* keyframe 0 with exactly SS_COVIS_MAX_ROW_ITEMS records, every one shared with keyframe 16 383: the largest weight and the largest kf
 * in one key; then one record more */
static long item_limit()
{
    const int n = SS_COVIS_MAX_ROW_ITEMS;
    std::vector<ss_gba_obs> obs;
    obs.reserve(2 * (size_t)n + 2);
    for (int i = 0; i < n; i++) obs.push_back(ss_gba_obs{0, i, 0, 0, -1, 0}), obs.push_back(ss_gba_obs{16383, i, 0, 0, -1, 1});
    built b;
    int bad = -1;
    std::vector<uint8_t> none;
    CHECK(build(b, 16384, n + 1, obs, none, 8, false, &bad) == 0);
    ss_covis_params p = {15, 0, 3, 1, 0.9f, {0, 0, 0}};
    std::vector<int32_t> nb(4), w;
    ss_covis_row r;
    ss_covis_row_host(b.m, 0, 0, nullptr, 0, p, 2, nb.data(), &r, w);
    CHECK(r.n_shared == 1 && r.max_weight == n && r.max_kf == 16383 && r.n_listed == 1 && nb[0] == 16383 && nb[1] == n && nb[2] == -1 && r.n_mps == n && r.n_redundant == 0);
    obs.push_back(ss_gba_obs{0, n, 0, 0, -1, 0});
    CHECK(build(b, 16384, n + 1, obs, none, 8, false, &bad) == 4 && bad == 2 * n);
    return 2;
}

int main()
{
    uint32_t s = 12345u;
    long rows = random_maps(s);
    rows += refused_and_empty();
    rows += packing_ends();
    rows += item_limit();
    printf("ok %ld\n", rows);
    return 0;
}
