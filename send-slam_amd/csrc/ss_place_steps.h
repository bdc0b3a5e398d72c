/*
 * ss_place_steps.h -- the steps of the place recognition (the rule: include/sendslam_orb.h): the exclusion
 * flags of a row, the word threshold, the float rounding of a score, the group walk of one seed, the total order of the accumulated
 * scores, the cut, the candidate order, and a whole query on the host.  The kernels (ss_place.hip), the host twin
 * ss_place_query_host (ss_api_search.cpp) and tests/native/place_steps_asan.cpp compile this text.
 *
 * Every float step is one IEEE float32 operation.  Compile with -ffp-contract=off.
 */
#ifndef SS_PLACE_STEPS_H
#define SS_PLACE_STEPS_H

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/sendslam_orb.h"
#include "ss_bow_merge.h"
#include "ss_float_steps.h" /* SS_HD */

/* why a row takes no part in a query: any bit excludes it */
#define SS_PLACE_F_SKIP 1u      /* its skip byte is set */
#define SS_PLACE_F_NO_PROBLEM 2u
#define SS_PLACE_F_SELF 4u      /* it is the query's own row */
#define SS_PLACE_F_CONNECTED 8u /* the query's covisibility row lists it */

/* a database and its inverted file, on the host or on the device */
struct ss_place_db {
    const int32_t *word = nullptr; /* [n_db][stride] */
    const double *value = nullptr;
    const int32_t *count = nullptr; /* [n_db] */
    const uint8_t *skip = nullptr;  /* [n_db] or NULL */
    int n_db = 0, stride = 0, n_words = 0, n_problems = 0;
    const int32_t *row_prob = nullptr; /* [n_db]: the row's problem or -1 */
    const int32_t *prob = nullptr;     /* [n_problems][2]: first_kf, n_kf */
    const int32_t *off = nullptr;      /* [n_words + 1]: where a word's list starts */
    const int32_t *list = nullptr;     /* the rows of every list */
};

SS_HD int ss_place_clamp(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

/* the flags of row r for a query whose own row is q_kf, before its covisibility row is read */
SS_HD uint32_t ss_place_base_flags(const ss_place_db &db, int r, int q_kf)
{
    return ((db.skip && db.skip[r]) ? SS_PLACE_F_SKIP : 0u) | (db.row_prob[r] < 0 ? SS_PLACE_F_NO_PROBLEM : 0u) | (r == q_kf ? SS_PLACE_F_SELF : 0u);
}

/* the call row of entry kf of a covisibility row of problem q, or -1 if the entry names no keyframe of it */
SS_HD int ss_place_row_of(const ss_place_db &db, int q, int kf)
{
    if (q < 0 || q >= db.n_problems || kf < 0 || kf >= db.prob[2 * q + 1]) return -1;
    return db.prob[2 * q] + kf;
}

/* whether entry j of a row's word list is one the inverted file holds */
SS_HD bool ss_place_word_ok(int32_t w, int n_words) { return w >= 0 && w < n_words; }

/* minCommonWords: one float multiply, then truncation */
SS_HD int ss_place_min_common(int max_common, float ratio) { return (int)((float)max_common * ratio); }

/* the score as upstream stores it */
SS_HD float ss_place_round(double s) { return (float)s; }

SS_HD bool ss_place_survivor(uint8_t flag, int words, int min_common) { return flag == 0 && words > min_common; }

/* The group of seed i (its score s_i; nb: its row of d_nb, (kf, weight) pairs relative to problem q of the seed).  flags, words and
 * score are the query's rows of those tables. */
SS_HD void ss_place_group(const ss_place_db &db, int i, float s_i, const int32_t *nb, int nb_cap, const uint8_t *flags, const int32_t *words, const float *score,
                          int min_common, float *acc_out, int *best_out)
{
    float acc = s_i, best_s = s_i;
    int best = i;
    const int q = db.row_prob[i];
    for (int e = 0; e < nb_cap; e++) {
        const int kf = nb[2 * e];
        if (kf < 0) break;
        const int j = ss_place_row_of(db, q, kf);
        if (j < 0 || !ss_place_survivor(flags[j], words[j], min_common)) continue;
        const float sj = score[j];
        acc = acc + sj;
        if (sj > best_s) best = j, best_s = sj;
    }
    *acc_out = acc, *best_out = best;
}

/* The accumulated scores are compared through their place in the IEEE total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf <
 * NaN, a 32-bit key that grows with it.  So a maximum folded over keys with integer atomics is the same whatever the schedule, for
 * every bit pattern: -0.0 loses to +0.0 and a NaN has a fixed place.  0 is kept for "no value": the one pattern that would map to
 * it (a negative NaN whose payload is all ones) shares key 1 with its neighbour. */
SS_HD uint32_t ss_place_key(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return k ? k : 1u;
}
SS_HD float ss_place_unkey(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

/* the 0.75 cut: one float multiply and a strict compare */
SS_HD bool ss_place_retained(float acc, float best_acc, float ratio) { return acc > ratio * best_acc; }

/* the candidate order, acc* descending then row ascending, is this key descending */
SS_HD uint64_t ss_place_order(uint32_t key, int row) { return ((uint64_t)key << 32) | (uint64_t)(0xffffffffu - (uint32_t)row); }
SS_HD int ss_place_order_row(uint64_t o) { return (int)(0xffffffffu - (uint32_t)(o & 0xffffffffu)); }

/* whether the walk over the order takes a row of class cls (0 own map, 1 another) whose key is `key`; taken: how many of each class
 * it has taken so far */
SS_HD bool ss_place_wanted(const ss_place_params &p, uint32_t key, float best_acc, int cls, const int *taken)
{
    if (cls == 1 && p.scope == 0) return false;
    if (p.n_best > 0) return taken[cls] < p.n_best;
    return ss_place_retained(ss_place_unkey(key), best_acc, p.retain_ratio);
}

SS_HD ss_place_cand ss_place_cand_of(const ss_place_db &db, int row, int q_problem, const int32_t *words, const float *score, uint32_t key)
{
    ss_place_cand c;
    c.kf = row, c.problem = db.row_prob[row], c.words = words[row], c.cls = db.row_prob[row] != q_problem ? 1 : 0;
    c.score = score[row], c.acc = ss_place_unkey(key);
    return c;
}
SS_HD ss_place_cand ss_place_no_cand()
{
    ss_place_cand c;
    c.kf = -1, c.problem = -1, c.words = 0, c.cls = 0, c.score = 0.0f, c.acc = 0.0f;
    return c;
}

/* ---- the host: the inverted file and a whole query ---- */
struct ss_place_host_db {
    std::vector<int32_t> row_prob, prob, off, list;
    ss_place_db view;
};

/* count, exclusive scan, fill: the three passes of the device build.  db holds the caller's arrays and the problems' ranges */
static inline void ss_place_build_host(ss_place_host_db &h)
{
    ss_place_db &db = h.view;
    h.off.assign((size_t)db.n_words + 1, 0);
    for (int r = 0; r < db.n_db; r++) {
        const int n = ss_place_clamp(db.count[r], db.stride);
        for (int j = 0; j < n; j++) {
            const int32_t w = db.word[(size_t)r * db.stride + j];
            if (ss_place_word_ok(w, db.n_words)) h.off[(size_t)w]++;
        }
    }
    int32_t run = 0;
    for (size_t w = 0; w <= (size_t)db.n_words; w++) {
        const int32_t c = h.off[w];
        h.off[w] = run;
        run += c;
    }
    h.list.assign((size_t)run + 1, 0);
    std::vector<int32_t> cursor(h.off.begin(), h.off.end() - 1);
    for (int r = 0; r < db.n_db; r++) {
        const int n = ss_place_clamp(db.count[r], db.stride);
        for (int j = 0; j < n; j++) {
            const int32_t w = db.word[(size_t)r * db.stride + j];
            if (ss_place_word_ok(w, db.n_words)) h.list[(size_t)cursor[(size_t)w]++] = r;
        }
    }
    db.off = h.off.data(), db.list = h.list.data();
}

/* One query.  q_word / q_value: its vector, n_q_words its clamped count; conn: its covisibility row ((kf, weight) pairs) or NULL,
 * n_conn its clamped n_written; nb: d_nb.  words_out [n_db] and score_out [n_db] are written in full; cand [cand_cap]; summary. */
static inline void ss_place_query_one_host(const ss_place_db &db, const int32_t *q_word, const double *q_value, int n_q_words, int q_kf, int q_problem,
                                           const int32_t *conn, int n_conn, const int32_t *nb, int nb_cap, const ss_place_params &p, int cand_cap, ss_place_cand *cand,
                                           ss_place_summary *summary, int32_t *words, float *score)
{
    const size_t N = (size_t)db.n_db;
    std::vector<uint8_t> flags(N);
    std::vector<uint32_t> star(N, 0u);
    for (int r = 0; r < db.n_db; r++) flags[(size_t)r] = (uint8_t)ss_place_base_flags(db, r, q_kf), words[r] = 0, score[r] = -1.0f;
    for (int e = 0; e < n_conn; e++) {
        const int j = ss_place_row_of(db, q_problem, conn[2 * e]);
        if (j >= 0) flags[(size_t)j] |= (uint8_t)SS_PLACE_F_CONNECTED;
    }
    /* 1. the votes */
    for (int t = 0; t < n_q_words; t++) {
        const int32_t w = q_word[t];
        if (!ss_place_word_ok(w, db.n_words)) continue;
        for (int32_t at = db.off[w]; at < db.off[w + 1]; at++) {
            const int r = db.list[at];
            if (flags[(size_t)r] == 0) words[r]++;
        }
    }
    ss_place_summary s;
    memset(&s, 0, sizeof(s));
    for (int r = 0; r < db.n_db; r++)
        if (words[r] > 0) s.n_sharing++, s.max_common = std::max(s.max_common, words[r]);
    /* 2. the threshold */
    s.min_common = ss_place_min_common(s.max_common, p.common_ratio);
    std::vector<int32_t> surv;
    for (int r = 0; r < db.n_db; r++)
        if (ss_place_survivor(flags[(size_t)r], words[r], s.min_common)) surv.push_back(r);
    s.n_survivors = (int32_t)surv.size();
    /* 3. the scores */
    auto score_of = [&](int r) {
        return ss_place_round(ss_bow_score_seq(q_word, q_value, n_q_words, db.word + (size_t)r * db.stride, db.value + (size_t)r * db.stride,
                                               ss_place_clamp(db.count[r], db.stride)));
    };
    for (int r : surv) score[r] = score_of(r);
    s.min_score = p.min_score;
    if (p.min_score_mode == 1) {
        s.min_score = 1.0f;
        for (int e = 0; e < n_conn; e++) {
            const int j = ss_place_row_of(db, q_problem, conn[2 * e]);
            if (j < 0 || (flags[(size_t)j] & SS_PLACE_F_SKIP)) continue;
            score[j] = score_of(j);
            if (score[j] < s.min_score) s.min_score = score[j];
        }
    }
    /* 4. the groups */
    for (int i : surv) {
        if (!(score[i] >= s.min_score)) continue;
        s.n_seeds++;
        float acc;
        int best;
        ss_place_group(db, i, score[i], nb + (size_t)i * nb_cap * 2, nb_cap, flags.data(), words, score, s.min_common, &acc, &best);
        star[(size_t)best] = std::max(star[(size_t)best], ss_place_key(acc));
    }
    /* 5. the candidates */
    std::vector<uint64_t> order;
    uint32_t top = 0u;
    for (int r : surv)
        if (star[(size_t)r]) order.push_back(ss_place_order(star[(size_t)r], r)), top = std::max(top, star[(size_t)r]);
    std::sort(order.begin(), order.end(), [](uint64_t a, uint64_t b) { return a > b; });
    s.best_acc = top ? ss_place_unkey(top) : 0.0f;
    int taken[2] = {0, 0};
    for (uint64_t o : order) {
        const int r = ss_place_order_row(o), cls = db.row_prob[r] != q_problem ? 1 : 0;
        const uint32_t key = (uint32_t)(o >> 32);
        if (!ss_place_wanted(p, key, s.best_acc, cls, taken)) continue;
        taken[cls]++;
        if (s.n_candidates < cand_cap) cand[s.n_candidates] = ss_place_cand_of(db, r, q_problem, words, score, key);
        s.n_candidates++;
    }
    s.n_written = std::min(s.n_candidates, cand_cap);
    for (int e = s.n_written; e < cand_cap; e++) cand[e] = ss_place_no_cand();
    *summary = s;
}

#endif
