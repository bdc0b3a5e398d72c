"""Scenes for the place recognition (tests/place_ref.py is the rule).  Vectors are synthesised directly as word ids and dyadic values
(k / 64), so every score is exact: for positive values it is the sum of min(v, w) over the common words, and the thresholds can be hit
exactly.  A case is a dictionary of the arrays ss_place takes; `expect` (hand-derived) is the candidate rows of each query in order."""
import numpy as np

import place_ref as PR

U = 1.0 / 64.0


def vec(words, value=4):
    """{word: value * U} for the words"""
    return {int(w): value * U for w in words}


def _pack(vectors, stride, counts=None):
    word, value = np.full((len(vectors), stride), -1, np.int32), np.zeros((len(vectors), stride), np.float64)
    count = np.zeros(len(vectors), np.int32)
    for r, v in enumerate(vectors):
        ws = sorted(v)
        word[r, :len(ws)], value[r, :len(ws)], count[r] = ws, [v[w] for w in ws], len(ws)
    if counts is not None:
        for r, c in counts.items():
            count[r] = c
    return word, value, count


def case(rows, queries, n_words=64, problems=None, nb=None, nb_cap=3, params=None, cand_cap=8, skip=None, stride=None, q_stride=None, counts=None,
         q_counts=None, q_cap=4, expect=None):
    """rows: one {word: value} per database row; queries: dicts of vec, kf (-1), problem (0) and conn (None: no covisibility arrays in
    the call; else a list of (kf relative to the problem, weight), or (list, n_written)); nb: {row: [kf relative, ...]}"""
    n_db = len(rows)
    stride = stride or max([len(v) for v in rows] + [1])
    q_stride = q_stride or max([len(q.get("vec", {})) for q in queries] + [1])
    db_word, db_value, db_count = _pack(rows, stride, counts)
    q_word, q_value, q_count = _pack([q.get("vec", {}) for q in queries], q_stride, q_counts)
    nbr = np.zeros((n_db, nb_cap, 2), np.int32)
    nbr[:, :, 0] = -1
    for r, lst in (nb or {}).items():
        for e, kf in enumerate(lst):
            nbr[r, e] = (kf, 20 - e)
    q_nb = q_row = None
    if any(q.get("conn") is not None for q in queries):
        q_nb, q_row = np.zeros((len(queries), q_cap, 2), np.int32), np.zeros(len(queries), PR.ROW_DTYPE)
        q_nb[:, :, 0] = -1
        for i, q in enumerate(queries):
            conn = q.get("conn") or []
            lst, n_written = conn if isinstance(conn, tuple) else (conn, len(conn))
            for e, (kf, w) in enumerate(lst):
                q_nb[i, e] = (kf, w)
            q_row[i]["n_written"] = q_row[i]["n_listed"] = n_written
    return dict(db_word=db_word, db_value=db_value, db_count=db_count, db_skip=None if skip is None else np.asarray(skip, np.uint8), n_words=n_words,
                problems=PR.problems_table(problems if problems is not None else [(0, n_db)]), q_word=q_word, q_value=q_value, q_count=q_count,
                q_kf=np.array([q.get("kf", -1) for q in queries], np.int32), q_problem=np.array([q.get("problem", 0) for q in queries], np.int32),
                q_nb=q_nb, q_row=q_row, nb=nbr, params=dict({"min_score_mode": 0, "min_score": 0.0}, **(params or {})), cand_cap=cand_cap, expect=expect)


def shared_cases():
    """name -> case: the scenes of the issue, small enough to derive by hand"""
    c = {}
    q12, q123, q1234, q12345 = (dict(vec=vec(range(1, n), 8)) for n in (3, 4, 5, 6))
    c["empty_query"] = case([vec([1, 2]), vec([2, 3])], [dict(vec={})], expect=[[]])
    c["shares_nothing"] = case([vec([1, 2]), vec([2, 3])], [dict(vec=vec([10, 11], 8))], expect=[[]])
    c["n_db_1"] = case([vec([1, 2])], [q12], expect=[[0]])
    c["own_only_sharer"] = case([vec([1, 2]), vec([5])], [dict(q12, kf=0)], expect=[[]])
    win = [vec([1, 2, 3, 4]), vec([1, 2, 3]), vec([1, 2, 3], 2)]
    c["connected_would_win"] = case(win, [dict(q1234, conn=[(0, 20)])], expect=[[1]])
    c["skipped"] = case(win, [q1234], skip=[1, 0, 0], expect=[[1]])
    c["no_problem"] = case(win, [q1234], problems=[(1, 2)], expect=[[1]])
    # words -1 and 20 lie outside 0 .. 15: in no list, but the score's merge still meets them; counts 7 and -2 clamp to 3 and 0
    c["out_of_range"] = case([{-1: 4 * U, 3: 4 * U, 20: 4 * U}, vec([3, 4, 5], 1), vec([3, 4, 5])], [dict(vec={-1: 8 * U, 3: 8 * U, 20: 8 * U})], n_words=16,
                             counts={1: 7, 2: -2}, q_counts={0: 9}, expect=[[0]])
    # max_common 5 -> min_common 4: the row with 4 words is out, the one with 5 in.  max_common 4 -> 3 (3.2 truncated): 3 words out, 4 in
    c["max_common_5"] = case([vec(range(1, 6)), vec(range(1, 5)), vec(range(1, 4))], [q12345], expect=[[0]])
    c["max_common_4"] = case([vec(range(1, 5)), vec(range(1, 4)), vec(range(1, 5), 2)], [q1234], expect=[[0]])
    for name, floor in (("floor_equal", np.float32(0.125)), ("floor_one_ulp_above", np.nextafter(np.float32(0.125), np.float32(1))),
                        ("floor_one_ulp_below", np.nextafter(np.float32(0.125), np.float32(0)))):
        c[name] = case([vec([1, 2])], [q12], params=dict(min_score=float(floor)), expect=[[] if "above" in name else [0]])
    m1 = [vec([1, 2]), vec([1]), vec([1, 2], 2), vec([1], 2), vec([1])]
    c["mode1_no_connected"] = case(m1, [dict(q12, conn=([(1, 20), (3, 18)], 0))], params=dict(min_score_mode=1), expect=[[]])
    c["mode1_all_skipped"] = case(m1, [dict(q12, conn=[(1, 20), (3, 18)])], skip=[0, 1, 0, 1, 0], params=dict(min_score_mode=1), expect=[[]])
    c["mode1_minimum_twice"] = case(m1, [dict(q12, conn=[(1, 20), (4, 18)])], params=dict(min_score_mode=1), expect=[[0]])
    # a group's best is never a non-seed: s(j) > best_s >= s(i) >= min_score makes j a seed.  What a non-seed survivor can do is add to acc
    c["non_seed_adds"] = case([vec([1, 2, 3]), vec([1, 2, 3], 1)], [q123], nb={0: [1]}, params=dict(min_score=0.1), expect=[[0]])
    c["marked_not_survivor"] = case([vec(range(1, 6)), vec([1, 2])], [q12345], nb={0: [1]}, expect=[[0]])
    c["two_seeds_one_best"] = case([vec([1, 2, 3]), vec([1, 2, 3], 2), vec([1, 2, 3], 8)], [q123], nb={0: [2], 1: [2]}, expect=[[2]])
    one = dict(vec={1: 1.0})
    c["cut_exact"] = case([{1: 1.0}, {1: 0.75}], [one], expect=[[0]])
    c["cut_one_ulp_above"] = case([{1: 1.0}, {1: 0.75 + 2.0 ** -24}], [one], expect=[[0, 1]])
    tie = [vec([1, 2], 4), vec([1, 2], 8), vec([1, 2], 8)]
    q_big = dict(vec=vec([1, 2], 16))
    c["equal_acc"] = case(tie, [q_big], expect=[[1, 2]])
    c["cand_cap_small"] = case(tie, [q_big], cand_cap=1, expect=[[1, 2]])
    maps = [vec([1, 2], v) for v in (1, 2, 3, 4, 5, 6, 7, 8, 6.5)]
    three = [(0, 3), (3, 3), (6, 3)]
    c["n_best_1"] = case(maps, [dict(q_big, problem=1)], problems=three, params=dict(n_best=1), expect=[[7, 5]])
    c["n_best_3"] = case(maps, [dict(q_big, problem=1)], problems=three, params=dict(n_best=3), expect=[[7, 6, 8, 5, 4, 3]])
    c["scope_0_after_merge"] = case([vec(range(1, 5)), vec(range(1, 4)), vec(range(1, 6))], [q12345], problems=[(0, 2), (2, 1)], params=dict(scope=0), expect=[[]])
    c["nb_end_marker_first"] = case([vec([1, 2]), vec([1, 2], 2)], [q12], nb={0: [-1, 1]}, expect=[[0]])
    c["nb_cap_1"] = case([vec([1, 2]), vec([1, 2], 2)], [q12], nb={0: [1]}, nb_cap=1, expect=[[0]])
    # a stored value of 0.0 on the only common word: the term is 0, s = 0.0 and the score -0.0 / 2 = -0.0f, a survivor and a seed
    # (-0.0 >= 0.0); the cut is strict, so the threshold form keeps nothing, the N-best form keeps it
    c["zero_score"] = case([{1: 0.0}], [dict(vec={1: 8 * U})], expect=[[]])
    c["zero_score_n_best"] = case([{1: 0.0}], [dict(vec={1: 8 * U})], params=dict(n_best=1), expect=[[0]])
    return c


def random_case(seed, n_db, n_q, n_words=97, stride=12, q_stride=9, nb_cap=3, q_cap=4, n_problems=2, cand_cap=6, mode=1, n_best=0, scope=1, empty=(), conn=True,
                fill=None):
    """a random database of n_db rows over n_problems maps (the last rows belong to none) and n_q queries, some of them database rows;
    words cluster on a few popular ids so that rows share several; values are k / 64"""
    rng = np.random.default_rng(seed)
    popular = rng.choice(n_words, min(14, n_words), replace=False)

    def draw(limit):
        n = int(rng.integers(1, limit + 1)) if fill is None else min(fill, limit)
        pool = np.concatenate([popular, rng.choice(n_words, 4)])
        return {int(w): int(rng.integers(1, 17)) * U for w in rng.choice(pool, min(n, len(pool)), replace=False)}

    owned = n_db if n_db < 4 else n_db - 1
    n_problems = max(1, min(n_problems, owned))
    cuts = [owned * q // n_problems for q in range(n_problems + 1)]
    problems = [(cuts[q], cuts[q + 1] - cuts[q]) for q in range(n_problems)]
    rows = [draw(stride) for _ in range(n_db)]
    skip = (rng.random(n_db) < 0.1).astype(np.uint8)
    nb = {}
    for q, (first, n) in enumerate(problems):
        for r in range(first, first + n):
            nb[r] = [int(x) for x in rng.choice(n, min(n, int(rng.integers(0, nb_cap + 1))), replace=False) if x != r - first]
    queries = []
    for i in range(n_q):
        kf = int(rng.integers(0, owned)) if i % 2 == 0 else -1
        problem = next(q for q, (first, n) in enumerate(problems) if first <= kf < first + n) if kf >= 0 else int(rng.integers(0, n_problems))
        v = {} if i in empty else (dict(rows[kf]) if kf >= 0 and i % 4 == 0 else draw(q_stride))
        v = dict(list(v.items())[:q_stride])
        lst = [(int(x), int(20 - e)) for e, x in enumerate(rng.choice(problems[problem][1], min(problems[problem][1], int(rng.integers(0, q_cap + 1))), replace=False))]
        queries.append(dict(vec=v, kf=kf, problem=problem, conn=lst if conn else None))
    return case(rows, queries, n_words=n_words, problems=problems, nb=nb, nb_cap=nb_cap, params=dict(min_score_mode=mode, min_score=2 * U, n_best=n_best, scope=scope),
                cand_cap=cand_cap, skip=skip, stride=stride, q_stride=q_stride, q_cap=q_cap)
