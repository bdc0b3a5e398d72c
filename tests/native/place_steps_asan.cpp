/*
 * place_steps_asan.cpp -- the steps of the place recognition (csrc/ss_place_steps.h, csrc/ss_bow_merge.h) under
 * -fsanitize=address,undefined: random databases with skipped rows, rows of no problem, out-of-range words, counts past the stride and
 * below 0, covisibility rows that name keyframes outside their problem and neighbour rows with early end markers go through the
 * inverted file and the whole query, every array allocated at its exact size so that a step out of bounds is caught.  Each query is
 * checked against a second walk that uses no inverted file (the votes by direct intersection), and the order key against the float
 * comparison it stands for.  Prints "ok <queries> <candidates>" and exits 0.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ss_place_steps.h"

static int fails = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
        }                                                                            \
    } while (0)

static void keys()
{
    const float v[] = {-3.5f, -1.0f, -0.0f, 0.0f, 1e-30f, 0.75f, 1.0f, 3.0f};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int a = 0; a < n; a++) {
        CHECK(ss_place_key(v[a]) != 0u);
        float back = ss_place_unkey(ss_place_key(v[a]));
        CHECK(memcmp(&back, &v[a], 4) == 0);
        for (int b = a + 1; b < n; b++) CHECK(ss_place_key(v[a]) < ss_place_key(v[b]));
    }
    CHECK(ss_place_min_common(5, 0.8f) == 4 && ss_place_min_common(4, 0.8f) == 3 && ss_place_min_common(0, 0.8f) == 0);
    CHECK(!ss_place_retained(0.75f, 1.0f, 0.75f) && ss_place_retained(0.75000006f, 1.0f, 0.75f) && !ss_place_retained(-0.0f, -0.0f, 0.75f));
    CHECK(ss_place_order(ss_place_key(1.0f), 3) > ss_place_order(ss_place_key(1.0f), 4) && ss_place_order_row(ss_place_order(7u, 123456)) == 123456);
}

int main()
{
    keys();
    std::mt19937 rng(20260101u);
    auto below = [&](int n) { return (int)(rng() % (uint32_t)n); };
    long queries = 0, candidates = 0;
    for (int round = 0; round < 60; round++) {
        const int n_db = 1 + below(40), stride = 1 + below(9), q_stride = 1 + below(9), n_words = 1 + below(24), nb_cap = 1 + below(4), q_cap = 1 + below(4);
        const int n_problems = 1 + below(3), cand_cap = 1 + below(5), n_q = 1 + below(4);
        std::vector<int32_t> db_word((size_t)n_db * stride), db_count((size_t)n_db), nb((size_t)n_db * nb_cap * 2);
        std::vector<double> db_value((size_t)n_db * stride);
        std::vector<uint8_t> skip((size_t)n_db);
        auto fill = [&](int32_t *w, double *v, int cap) { /* ascending distinct words from -2 .. n_words + 1 */
            int32_t at = -2 - below(2);
            for (int j = 0; j < cap; j++) {
                at += 1 + below(3);
                w[j] = at, v[j] = (double)below(17) / 64.0;
            }
        };
        for (int r = 0; r < n_db; r++) {
            fill(&db_word[(size_t)r * stride], &db_value[(size_t)r * stride], stride);
            db_count[(size_t)r] = below(stride + 4) - 1;
            skip[(size_t)r] = below(8) == 0;
            for (int e = 0; e < nb_cap; e++) nb[((size_t)r * nb_cap + e) * 2] = below(n_db + 3) - 2, nb[((size_t)r * nb_cap + e) * 2 + 1] = 15 + e;
        }
        ss_place_host_db h;
        ss_place_db &db = h.view;
        /* the problems: consecutive ranges, the last rows in none */
        h.row_prob.assign((size_t)n_db, -1), h.prob.assign((size_t)n_problems * 2, 0);
        int first = 0, made = 0;
        for (int q = 0; q < n_problems && first < n_db; q++, made++) {
            const int n = 1 + below(n_db - first);
            h.prob[(size_t)q * 2] = first, h.prob[(size_t)q * 2 + 1] = n;
            for (int k = first; k < first + n; k++) h.row_prob[(size_t)k] = q;
            first += n + below(2);
        }
        h.prob.resize((size_t)made * 2);
        db.word = db_word.data(), db.value = db_value.data(), db.count = db_count.data(), db.skip = below(4) ? skip.data() : nullptr;
        db.n_db = n_db, db.stride = stride, db.n_words = n_words, db.n_problems = made;
        db.row_prob = h.row_prob.data(), db.prob = h.prob.data();
        ss_place_build_host(h);
        CHECK(h.off.size() == (size_t)n_words + 1 && h.off[0] == 0);
        for (int q = 0; q < n_q; q++, queries++) {
            std::vector<int32_t> q_word((size_t)q_stride), conn((size_t)q_cap * 2), words((size_t)n_db);
            std::vector<double> q_value((size_t)q_stride);
            std::vector<float> score((size_t)n_db);
            std::vector<ss_place_cand> cand((size_t)cand_cap);
            fill(q_word.data(), q_value.data(), q_stride);
            const int nq = ss_place_clamp(below(q_stride + 3) - 1, q_stride);
            const int q_kf = below(3) ? below(n_db) : -1;
            const int q_problem = q_kf >= 0 && h.row_prob[(size_t)q_kf] >= 0 ? h.row_prob[(size_t)q_kf] : below(made);
            for (int e = 0; e < q_cap; e++) conn[(size_t)e * 2] = below(n_db + 2) - 1, conn[(size_t)e * 2 + 1] = 20;
            const bool has_conn = below(3) != 0;
            const int n_conn = has_conn ? ss_place_clamp(below(q_cap + 3) - 1, q_cap) : 0;
            ss_place_params p = {below(2), (float)below(9) / 64.0f, below(3) ? 0 : 1 + below(3), below(2), 0.8f, 0.75f, {0, 0}};
            ss_place_summary s;
            ss_place_query_one_host(db, q_word.data(), q_value.data(), nq, q_kf, q_problem, has_conn ? conn.data() : nullptr, n_conn, nb.data(), nb_cap, p, cand_cap,
                                    cand.data(), &s, words.data(), score.data());
            /* the votes again, without the lists */
            int sharing = 0, max_common = 0;
            for (int r = 0; r < n_db; r++) {
                bool excluded = (db.skip && db.skip[r]) || h.row_prob[(size_t)r] < 0 || r == q_kf;
                for (int e = 0; e < n_conn; e++) excluded = excluded || ss_place_row_of(db, q_problem, conn[(size_t)e * 2]) == r;
                int common = 0;
                const int nd = ss_place_clamp(db_count[(size_t)r], stride);
                for (int t = 0; t < nq && !excluded; t++)
                    for (int j = 0; j < nd; j++) common += q_word[(size_t)t] == db_word[(size_t)r * stride + j] && ss_place_word_ok(q_word[(size_t)t], n_words);
                CHECK(words[(size_t)r] == common);
                sharing += common > 0, max_common = common > max_common ? common : max_common;
            }
            CHECK(s.n_sharing == sharing && s.max_common == max_common && s.n_survivors <= sharing && s.n_seeds <= s.n_survivors);
            CHECK(s.n_written == (s.n_candidates < cand_cap ? s.n_candidates : cand_cap) && s.status == SS_OK);
            for (int e = 0; e < cand_cap; e++) {
                const ss_place_cand &c = cand[(size_t)e];
                if (e >= s.n_written) {
                    CHECK(c.kf == -1 && c.problem == -1 && c.words == 0);
                    continue;
                }
                candidates++;
                CHECK(c.kf >= 0 && c.kf < n_db && c.problem == h.row_prob[(size_t)c.kf] && c.words == words[(size_t)c.kf] && c.words > s.min_common);
                CHECK(c.cls == (c.problem != q_problem) && (p.scope == 1 || c.cls == 0));
                CHECK(p.n_best > 0 || ss_place_retained(c.acc, s.best_acc, p.retain_ratio));
                if (e > 0) CHECK(ss_place_order(ss_place_key(cand[(size_t)e - 1].acc), cand[(size_t)e - 1].kf) > ss_place_order(ss_place_key(c.acc), c.kf));
            }
        }
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("ok %ld %ld\n", queries, candidates);
    return 0;
}
