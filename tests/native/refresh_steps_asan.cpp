/* The steps of the map-point refresh (csrc/ss_refresh_steps.h) under -fsanitize=address,undefined, with a main of its own: random
 * maps built by ss_covis_tables with rows, every row of ss_refresh_row_host held to a direct O(n^2 log n) restatement (a sorted row
 * of distances per observation, a sequential walk for the reference and the count), empty lists, and the steps alone on a list of
 * 16 384 observations.  Prints "ok <rows checked>" and exits 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "ss_refresh_steps.h"

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (fails++ < 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

struct host_map {
    std::vector<ss_covis_prob> prob;
    std::vector<int32_t> kf_prob, blk_prob, pt_off, pt_cnt, kf_off, kf_cnt, kf_item, pt_row;
    std::vector<uint32_t> pt_item;
    ss_covis_tab tab;
};

static int popcount_direct(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int k = 0; k < 32; k++)
        for (int bit = 0; bit < 8; bit++) d += ((a[k] ^ b[k]) >> bit) & 1;
    return d;
}

static long check_map(std::mt19937 &rng, int n_kf, int P, int max_len, int n_levels, int rpf, bool geometry, bool descriptor)
{
    std::vector<ss_gba_obs> obs;
    std::vector<int32_t> rows;
    for (int i = 0; i < P; i++) {
        std::vector<int> kfs((size_t)n_kf);
        for (int k = 0; k < n_kf; k++) kfs[(size_t)k] = k;
        std::shuffle(kfs.begin(), kfs.end(), rng);
        const int len = max_len > 0 ? (int)(rng() % (unsigned)(std::min(max_len, n_kf) + 1)) : 0;
        for (int e = 0; e < len; e++) {
            const int octave = rng() % 5 == 0 ? (int)(rng() % (unsigned)(n_levels + 2)) - 1 : (int)(rng() % (unsigned)n_levels);
            obs.push_back(ss_gba_obs{kfs[(size_t)e], i, 0.0f, 0.0f, rng() % 3 == 0 ? 4.0f : -1.0f, octave});
            rows.push_back((int32_t)(rng() % (unsigned)rpf));
        }
    }
    std::vector<size_t> perm(obs.size());
    for (size_t m = 0; m < perm.size(); m++) perm[m] = m;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<ss_gba_obs> so(obs.size() + 1);
    std::vector<int32_t> sr(obs.size() + 1);
    for (size_t m = 0; m < perm.size(); m++) so[m] = obs[perm[m]], sr[m] = rows[perm[m]];
    const int n = (int)obs.size();
    host_map h;
    h.prob = {ss_covis_prob{0, n_kf, 0, 1}};
    h.kf_prob.assign((size_t)n_kf, 0), h.blk_prob.assign(1, 0);
    h.pt_off.assign((size_t)P + 1, 0), h.pt_cnt.assign((size_t)P + 1, 0), h.kf_off.assign((size_t)n_kf + 1, 0), h.kf_cnt.assign((size_t)n_kf + 1, 0);
    h.pt_item.assign((size_t)n + 1, 0u), h.kf_item.assign(2 * (size_t)n + 2, 0), h.pt_row.assign((size_t)n + 1, 0);
    std::vector<int32_t> from((size_t)n + 1);
    int bad = 0;
    CHECK(ss_covis_tables(n_kf, P, so.data(), nullptr, n, n_levels, true, 0, 0, h.pt_off.data(), h.pt_cnt.data(), h.kf_off.data(), h.kf_cnt.data(), h.pt_item.data(),
                          h.kf_item.data(), &bad, from.data()) == 0);
    for (int s = 0; s < n; s++) h.pt_row[(size_t)s] = sr[(size_t)from[(size_t)s]];
    ss_covis_tab &m = h.tab;
    m.n_kf = n_kf, m.n_blocks = 1, m.point_rows = P, m.n_problems = 1, m.max_kf = n_kf;
    m.prob = h.prob.data(), m.kf_prob = h.kf_prob.data(), m.blk_prob = h.blk_prob.data(), m.kf_off = h.kf_off.data(), m.kf_cnt = h.kf_cnt.data();
    m.pt_off = h.pt_off.data(), m.pt_cnt = h.pt_cnt.data(), m.pt_item = h.pt_item.data(), m.kf_item = h.kf_item.data();

    std::vector<float> ow((size_t)n_kf * 3), scale((size_t)n_levels);
    for (auto &v : ow) v = (float)((int)(rng() % 2001) - 1000) / 64.0f;
    scale[0] = 1.0f;
    for (int l = 1; l < n_levels; l++) scale[(size_t)l] = (float)(scale[(size_t)l - 1] * (double)1.2f);
    std::vector<uint8_t> desc((size_t)n_kf * rpf * 32), pdesc((size_t)P * 32, 0xC3), select((size_t)P);
    for (auto &v : desc) v = (uint8_t)(rng() % 4 == 0 ? rng() : 0x55); /* few distinct bytes: many ties */
    std::vector<ss_map_point> pts((size_t)P);
    std::vector<int32_t> ref((size_t)P);
    for (int i = 0; i < P; i++) {
        pts[(size_t)i] = ss_map_point{(float)((int)(rng() % 2001) - 1000) / 64.0f, (float)(rng() % 100), (float)(rng() % 7), -77.0f, -77.0f, -77.0f, -77.0f, -77.0f};
        if (rng() % 17 == 0) pts[(size_t)i].y = NAN;
        ref[(size_t)i] = (int32_t)(rng() % (unsigned)(n_kf + 1)) - 1;
        select[(size_t)i] = (uint8_t)(rng() % 9 == 0 ? 1 + rng() % 2 : 0);
    }
    if (P > 0 && n_kf > 0) pts[0].x = ow[0], pts[0].y = ow[1], pts[0].z = ow[2]; /* on keyframe 0's centre */
    const int32_t n_points = P - (P > 3 ? 1 : 0);
    ss_refresh_host_in in;
    in.pt_row = h.pt_row.data(), in.n_points = &n_points, in.ref_kf = ref.data(), in.select = select.data(), in.desc = desc.data(), in.rows_per_frame = rpf;
    in.ow = ow.data(), in.scale = scale.data(), in.n_levels = n_levels, in.geometry = geometry, in.descriptor = descriptor;
    std::vector<ss_refresh_info> info((size_t)P + 1);
    const std::vector<ss_map_point> before = pts;
    for (int i = 0; i < P; i++) ss_refresh_row_host(m, in, 0, i, pts.data(), pdesc.data(), info.data());
    ss_refresh_summary sum;
    ss_refresh_summary_host(m, 0, n_points, info.data(), &sum);

    int n_sel = 0, n_ok = 0;
    for (int i = 0; i < P; i++) {
        const ss_refresh_info &r = info[(size_t)i];
        const ss_map_point &b = before[(size_t)i], &a = pts[(size_t)i];
        CHECK(a.x == b.x || (a.x != a.x && b.x != b.x));
        CHECK(a.z == b.z && r.reserved == 0);
        const bool sel = i < n_points && select[(size_t)i] == 0 && isfinite(b.x) && isfinite(b.y) && isfinite(b.z);
        CHECK((r.state >= 0) == sel);
        /* the observations by a direct walk over the caller's records */
        std::vector<std::pair<int, int>> lst; /* (kf, record) */
        int count = 0;
        for (int k = 0; k < n; k++)
            if (so[(size_t)k].point == i && so[(size_t)k].octave >= 0 && so[(size_t)k].octave < n_levels) lst.push_back({so[(size_t)k].kf, k}), count += 1 + (so[(size_t)k].right > 0.0f);
        std::sort(lst.begin(), lst.end());
        const int L = (int)lst.size();
        if (!sel) {
            CHECK(r.n_obs == 0 && r.count == 0 && r.ref_kf == -1 && r.level == -1 && r.best_kf == -1 && r.best_median == -1);
            CHECK(a.nx == -77.0f && a.max_dist == -77.0f && pdesc[(size_t)i * 32] == 0xC3);
            continue;
        }
        n_sel++;
        CHECK(r.n_obs == L && r.count == count);
        if (L == 0) {
            CHECK(r.state == 1 && a.nx == -77.0f && pdesc[(size_t)i * 32 + 31] == 0xC3);
            continue;
        }
        bool centre = false;
        for (auto &o : lst) centre = centre || (geometry && ow[(size_t)o.first * 3] == b.x && ow[(size_t)o.first * 3 + 1] == b.y && ow[(size_t)o.first * 3 + 2] == b.z);
        CHECK(r.state == (centre ? 2 : 0));
        if (centre) {
            CHECK(a.nx == -77.0f && pdesc[(size_t)i * 32] == 0xC3 && r.ref_kf == -1 && r.best_kf == -1);
            continue;
        }
        n_ok++;
        if (geometry) {
            int at = 0;
            for (int e = 0; e < L; e++)
                if (lst[(size_t)e].first == ref[(size_t)i]) at = e;
            CHECK(r.ref_kf == lst[(size_t)at].first && r.level == so[(size_t)lst[(size_t)at].second].octave);
            const float *c = &ow[(size_t)r.ref_kf * 3];
            const double dx = (double)b.x - c[0], dy = (double)b.y - c[1], dz = (double)b.z - c[2], mx = sqrt((dx * dx + dy * dy) + dz * dz) * (double)scale[(size_t)r.level];
            CHECK(a.max_dist == (float)mx && a.min_dist == (float)(mx / (double)scale[(size_t)n_levels - 1]));
            CHECK(fabs((double)a.nx) <= 1.0 && fabs((double)a.ny) <= 1.0 && fabs((double)a.nz) <= 1.0);
        } else {
            CHECK(r.ref_kf == -1 && r.level == -1 && a.nx == -77.0f && a.min_dist == -77.0f);
        }
        if (descriptor) {
            long best_med = 1 << 20;
            int best = -1;
            for (int e = 0; e < L; e++) {
                std::vector<int> row;
                const uint8_t *de = &desc[((size_t)lst[(size_t)e].first * rpf + sr[(size_t)lst[(size_t)e].second]) * 32];
                for (int f = 0; f < L; f++) row.push_back(popcount_direct(de, &desc[((size_t)lst[(size_t)f].first * rpf + sr[(size_t)lst[(size_t)f].second]) * 32]));
                std::sort(row.begin(), row.end());
                if (row[(size_t)((L - 1) / 2)] < best_med) best_med = row[(size_t)((L - 1) / 2)], best = e;
            }
            CHECK(r.best_kf == lst[(size_t)best].first && r.best_median == best_med);
            CHECK(memcmp(&pdesc[(size_t)i * 32], &desc[((size_t)lst[(size_t)best].first * rpf + sr[(size_t)lst[(size_t)best].second]) * 32], 32) == 0);
        } else {
            CHECK(r.best_kf == -1 && r.best_median == -1 && pdesc[(size_t)i * 32] == 0xC3);
        }
    }
    CHECK(sum.status == SS_OK && sum.n_rows == n_points && sum.n_selected == n_sel && sum.n_refreshed == n_ok && sum.reserved == 0);
    CHECK(sum.n_selected == sum.n_refreshed + sum.n_no_obs + sum.n_degenerate);
    return P;
}

/* the steps alone on the longest list the rule allows: the tree against a long double sum, the select against a sorted row */
static void check_longest(std::mt19937 &rng)
{
    const int n = SS_GBA_MAX_KF;
    std::vector<double> term((size_t)n);
    double slot[SS_REFRESH_SLOTS];
    for (int s = 0; s < SS_REFRESH_SLOTS; s++) slot[s] = 0.0;
    long double exact = 0.0L;
    for (int a = 0; a < n; a++) {
        term[(size_t)a] = (double)((int)(rng() % 2001) - 1000) / 1000.0;
        slot[a % SS_REFRESH_SLOTS] = slot[a % SS_REFRESH_SLOTS] + term[(size_t)a];
        exact += term[(size_t)a];
    }
    CHECK(fabsl((long double)ss_refresh_fold(slot) - exact) < 1e-9L);
    std::vector<uint32_t> w((size_t)n * 8);
    for (auto &v : w) v = rng();
    std::vector<int> row((size_t)n);
    int cum[257] = {0};
    for (int b = 0; b < n; b++) row[(size_t)b] = ss_refresh_dist(&w[0], &w[(size_t)b * 8]), cum[row[(size_t)b]]++;
    for (int v = 1; v <= 256; v++) cum[v] += cum[v - 1];
    std::sort(row.begin(), row.end());
    CHECK(row[0] == 0 && ss_refresh_rank(n) == 8191);
    for (int rank : {0, 1, 8190, 8191, 8192, n - 1}) CHECK(ss_refresh_select(rank + 1, [&](int v) { return cum[v]; }) == row[(size_t)rank]);
    CHECK(ss_refresh_key_obs(ss_refresh_key(256, n - 1)) == n - 1 && ss_refresh_key_median(ss_refresh_key(256, n - 1)) == 256);
    CHECK(ss_refresh_key(5, n - 1) < ss_refresh_key(6, 0) && ss_refresh_key(5, 3) < ss_refresh_key(5, 4));
    uint32_t zero[8] = {0}, ones[8];
    for (int k = 0; k < 8; k++) ones[k] = 0xffffffffu;
    CHECK(ss_refresh_dist(zero, ones) == 256 && ss_refresh_dist(ones, ones) == 0);
    CHECK(ss_refresh_select(1, [](int v) { return v >= 256 ? 1 : 0; }) == 256 && ss_refresh_select(1, [](int) { return 1; }) == 0);
}

int main()
{
    std::mt19937 rng(20261020u);
    long rows = 0;
    rows += check_map(rng, 1, 4, 0, 8, 1, true, true); /* empty lists */
    rows += check_map(rng, 1, 5, 1, 1, 1, true, true);
    for (int round = 0; round < 6; round++) {
        rows += check_map(rng, 9, 60, 9, 8, 5, true, true);
        rows += check_map(rng, 70, 25, 70, 8, 3, round % 2 == 0, round % 2 == 1);
        rows += check_map(rng, 140, 12, 140, 16, 2, true, true);
    }
    rows += check_map(rng, 300, 4, 300, 8, 2, true, true);
    check_longest(rng);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok %ld\n", rows);
    return 0;
}
