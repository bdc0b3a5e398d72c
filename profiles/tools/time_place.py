"""Times of the place recognition, one context alone on the chip.  Databases of 100, 2 000 and 16 384 keyframes of about 1 000 words
each, drawn from 10^6 words with a Zipf-like skew (word = floor(10^6 u^3): the lowest ids sit in most vectors, so some lists are as long
as the database) and grouped in places of eight keyframes that share a pool of words; a keyframe's covisibility row is its five
neighbours on either side.  1 and 16 queries, each a keyframe of the database.  For each: ss_place_set_database from the call to
synchronize and its stage by HIP events, ss_place_query_device per stage by HIP events and from the call to synchronize, and, in the
same run, the two things it is compared with: ss_bow_score_device over the whole database plus the download of the scores, once per
query (what a caller does without this family; the filter, the groups and the cut are then still to do on the host), and
ss_place_query_host on one core (its inverted file included, and separately a call with no query: the build alone).
usage: python profiles/tools/time_place.py [reps] [out.json] [quick]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
quick = len(sys.argv) > 3
SIZES = (100, 2000) if quick else (100, 2000, 16384)
N_WORDS, STRIDE, CAP, CAND = 1000000, 1024, 10, 16
STAGES = ("place_flags", "place_vote", "place_reduce", "place_score", "place_seeds", "place_final")
ctx = binding.OrbContext(0, n_features=500)
rows = []


def zipf(rng, n):
    return np.floor(N_WORDS * rng.random(n) ** 3).astype(np.int64)


def database(seed, n_db):
    rng = np.random.default_rng(seed)
    word, value, count = np.full((n_db, STRIDE), -1, np.int32), np.zeros((n_db, STRIDE)), np.zeros(n_db, np.int32)
    pool = None
    for r in range(n_db):
        if r % 8 == 0:
            pool = np.unique(zipf(rng, 1500))
        w = np.unique(np.concatenate([rng.choice(pool, min(len(pool), 800), replace=False), zipf(rng, 300)]))[:STRIDE]
        v = rng.integers(1, 9, len(w)).astype(np.float64)
        word[r, :len(w)], value[r, :len(w)], count[r] = w, v / v.sum(), len(w)
    nb = np.zeros((n_db, CAP, 2), np.int32)
    nb[:, :, 0] = -1
    for r in range(n_db):
        near = [j for d in range(1, 6) for j in (r - d, r + d) if 0 <= j < n_db][:CAP]
        nb[r, :len(near), 0], nb[r, :len(near), 1] = near, 100
    row = np.zeros(n_db, binding.COVIS_ROW_DTYPE)
    row["n_written"] = (nb[:, :, 0] >= 0).sum(axis=1)
    return word, value, count, nb, row


def median_ms(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def staged(fn, n, names):
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(n):
        fn()
        ctx.synchronize()
    ctx.profile(False)
    return {s["name"]: round(s["total_ms"] / n, 5) for s in ctx.stats() if s["name"] in names and s["launches"]}


for n_db in SIZES:
    word, value, count, nb, row = database(3300 + n_db, n_db)
    problems = np.array([(0, n_db, 0, 0, 0, 0, (0, 0))], binding.GBA_PROBLEM_DTYPE)
    d_word, d_value, d_count, d_nb = (torch.from_numpy(a).cuda() for a in (word, value, count, nb))
    d_row = torch.from_numpy(row.view(np.uint8).reshape(n_db, -1)).cuda()
    params = binding.place_params()
    torch.cuda.synchronize()

    def set_database():
        ctx.place_set_database(d_word.data_ptr(), d_value.data_ptr(), d_count.data_ptr(), n_db, STRIDE, N_WORDS, problems)
        ctx.synchronize()

    set_database(), set_database()
    n = reps if n_db <= 2000 else max(reps // 2, 5)
    entry = {"n_db": n_db, "mean_words": round(float(count.mean()), 1), "reps": n, "set_database_wall_ms": median_ms(set_database, max(n // 2, 3)),
             "set_database_stage_ms": staged(set_database, 3, ("place_build",)), "queries": []}
    entry["host_inverted_file_ms"] = median_ms(lambda: binding.place_query_host(word, value, count, N_WORDS, problems, word[:0], value[:0], count[:0], [], [], nb, params, CAND), 3)
    for n_q in (1, 16):
        q_kf = (np.arange(n_q) * max(n_db // n_q, 1) + n_db // 3) % n_db
        idx = torch.from_numpy(q_kf).cuda()
        q_word, q_value, q_count, q_nb, q_row = (t[idx].contiguous() for t in (d_word, d_value, d_count, d_nb, d_row))
        d_cand = torch.empty((n_q, CAND * 24), dtype=torch.uint8, device="cuda")
        d_sum = torch.empty((n_q, 48), dtype=torch.uint8, device="cuda")
        d_score = torch.empty(n_db, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def query():
            ctx.place_query_device(q_word.data_ptr(), q_value.data_ptr(), q_count.data_ptr(), STRIDE, q_kf, np.zeros(n_q, np.int32), d_nb.data_ptr(), CAP, params, CAND,
                                   d_cand.data_ptr(), d_sum.data_ptr(), d_q_nb=q_nb.data_ptr(), d_q_row=q_row.data_ptr(), q_cap=CAP)
            ctx.synchronize()

        def whole_database():
            for q in range(n_q):
                ctx.bow_score_device(q_word[q].data_ptr(), q_value[q].data_ptr(), q_count[q:].data_ptr(), STRIDE, d_word.data_ptr(), d_value.data_ptr(), d_count.data_ptr(),
                                     n_db, STRIDE, d_score.data_ptr())
                ctx.synchronize()
                d_score.cpu()

        query(), query(), whole_database()
        call_ms, whole_ms = median_ms(query, n), median_ms(whole_database, n)
        stages = staged(query, n, STAGES)
        score_stage = staged(whole_database, max(n // 4, 2), ("bow_score",))
        twin = lambda: binding.place_query_host(word, value, count, N_WORDS, problems, word[q_kf], value[q_kf], count[q_kf], q_kf, np.zeros(n_q, np.int32), nb, params,  # noqa: E731
                                                CAND, q_nb=nb[q_kf], q_row=row[q_kf])
        host, host_ms = twin(), median_ms(twin, 3)
        cand = d_cand.cpu().numpy().view(binding.PLACE_CAND_DTYPE).reshape(n_q, CAND)
        summary = d_sum.cpu().numpy().view(binding.PLACE_SUMMARY_DTYPE).reshape(n_q)
        assert cand.tobytes() == host[0].tobytes() and summary.tobytes() == host[1].tobytes(), "the device and the host twin differ"
        entry["queries"].append({"n_q": n_q, "stages_ms": stages, "stages_sum_ms": round(sum(stages.values()), 5), "query_wall_ms": call_ms,
                                 "whole_database_score_and_download_wall_ms": whole_ms, "whole_database_score_stage_ms": score_stage.get("bow_score"),
                                 "ratio_whole_database_over_query": round(whole_ms / call_ms, 2), "host_twin_one_core_ms": round(host_ms, 2),
                                 "host_twin_queries_only_ms": round(host_ms - entry["host_inverted_file_ms"], 2),
                                 "mean_sharing": float(summary["n_sharing"].mean()), "mean_survivors": float(summary["n_survivors"].mean()),
                                 "mean_seeds": float(summary["n_seeds"].mean()), "mean_candidates": float(summary["n_candidates"].mean())})
    rows.append(entry)
    print(json.dumps(entry), flush=True)
    del d_word, d_value, d_count, d_nb, d_row
    torch.cuda.empty_cache()

NOTE = ("stages: HIP events around each stage's launches with profiling on, per call; *_wall_ms: the median of one unprofiled call to synchronize (the whole-database "
        "figures: n_q calls of ss_bow_score_device, each synchronised and its n_db doubles downloaded; its stage is the n_q launches alone); host_inverted_file_ms: ss_place_query_host with no query, one core")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps({"device": torch.cuda.get_device_name(0), "note": NOTE, "rows": rows}, indent=1) + "\n")
