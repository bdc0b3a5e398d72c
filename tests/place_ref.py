"""The place-recognition rule of include/sendslam_orb.h restated in plain Python and numpy: its normative statement.  Every float step goes
through np.float32.  Written from the rule, not from the library's text: it builds no offset table and no flag byte, only a dictionary of
sets per word and sets of rows per query.

Below it, `upstream` is a second, literal restatement of KeyFrameDatabase's sequential loops (marks and counters on keyframe objects,
std::list pushes, GetBestCovisibilityKeyFrames, a set for the duplicates).  The two give the same candidate SET wherever no two acc* are
equal and no marked neighbour is unscored (tests/test_place_ref.py shows it); their ORDER differs by design (ours: acc* descending, then
row; upstream's: list position)."""
import math

import numpy as np

PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_kf", "n_kf", "first_block", "n_blocks", "first_obs", "n_obs")] + [("reserved", "<i4", (2,))])
ROW_DTYPE = np.dtype([(n, "<i4") for n in ("n_shared", "max_weight", "max_kf", "n_listed", "n_written", "n_mps", "n_redundant", "redundant")])
CAND_DTYPE = np.dtype([("kf", "<i4"), ("problem", "<i4"), ("words", "<i4"), ("class", "<i4"), ("score", "<f4"), ("acc", "<f4")])
SUMMARY_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common", "<i4"), ("min_common", "<i4"), ("n_survivors", "<i4"), ("n_seeds", "<i4"),
                          ("min_score", "<f4"), ("best_acc", "<f4"), ("n_candidates", "<i4"), ("n_written", "<i4"), ("status", "<i4"),
                          ("reserved", "<i4", (2,))])
DEFAULTS = dict(min_score_mode=1, min_score=0.0, n_best=0, scope=1, common_ratio=0.8, retain_ratio=0.75)
MAX_DB, MAX_QUERIES, MAX_CANDIDATES, MAX_NEIGHBOURS = 262144, 256, 256, 1024
F32 = np.float32


def problems_table(ranges):
    """[(first_kf, n_kf), ...] -> PROBLEM_DTYPE rows (only those two fields are read)"""
    out = np.zeros(len(ranges), PROBLEM_DTYPE)
    for q, (first, n) in enumerate(ranges):
        out[q]["first_kf"], out[q]["n_kf"] = first, n
    return out


def l1_score(qw, qv, dw, dv) -> float:
    """ss_bow_score_device's double: both ascending lists walked, the terms of the common words added in ascending order"""
    if len(qw) == 0 or len(dw) == 0:
        return 0.0
    s, i, j = 0.0, 0, 0
    while i < len(qw) and j < len(dw):
        if qw[i] == dw[j]:
            v, w = float(qv[i]), float(dv[j])
            t = math.fabs(v - w)
            t = t - math.fabs(v)
            t = t - math.fabs(w)
            s += t
            i, j = i + 1, j + 1
        elif qw[i] < dw[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0


def total_key(x) -> int:
    """the place of a float32 in the IEEE total order, as an integer that grows with it; never 0"""
    u = int(np.array(x, F32).view(np.uint32))
    k = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return k or 1


def min_common_of(max_common: int, ratio=0.8) -> int:
    return int(F32(max_common) * F32(ratio))


class Database:
    """word int32 / value float64 [n_db][stride], count [n_db], problems PROBLEM_DTYPE, skip uint8 [n_db] or None"""

    def __init__(self, word, value, count, n_words, problems, skip=None):
        self.word, self.value = np.asarray(word, np.int32), np.asarray(value, np.float64)
        self.n_db, self.stride = self.word.shape
        self.count = np.clip(np.asarray(count, np.int64), 0, self.stride)
        self.n_words = n_words
        self.problems = np.asarray(problems, PROBLEM_DTYPE).reshape(-1)
        self.skip = np.zeros(self.n_db, bool) if skip is None else np.asarray(skip).astype(bool)
        self.problem = np.full(self.n_db, -1)
        for q, pr in enumerate(self.problems):
            self.problem[pr["first_kf"]:pr["first_kf"] + pr["n_kf"]] = q
        self.lists = {}
        for r in range(self.n_db):
            for w in self.word[r, :self.count[r]]:
                if 0 <= w < n_words:
                    self.lists.setdefault(int(w), []).append(r)

    def vector(self, r):
        return self.word[r, :self.count[r]], self.value[r, :self.count[r]]

    def row_of(self, q, kf):
        """the call row of keyframe kf of problem q, or None"""
        if not 0 <= q < len(self.problems) or not 0 <= kf < self.problems[q]["n_kf"]:
            return None
        return int(self.problems[q]["first_kf"]) + int(kf)


def connected_rows(db, q_problem, q_nb, q_row):
    """the connected entries of a covisibility row, in list order, as call rows (None for an entry that names no keyframe)"""
    if q_nb is None:
        return []
    n = min(max(int(q_row["n_written"]), 0), len(q_nb))
    return [db.row_of(q_problem, int(q_nb[e][0])) for e in range(n)]


def query(db, qw, qv, q_kf, q_problem, nb, params, cand_cap, q_nb=None, q_row=None):
    """one query -> (cand CAND_DTYPE [cand_cap], summary SUMMARY_DTYPE scalar, words int32 [n_db], score float32 [n_db])"""
    p = dict(DEFAULTS, **params)
    conn = connected_rows(db, q_problem, q_nb, q_row)
    connected = {j for j in conn if j is not None}
    excluded = {r for r in range(db.n_db) if db.skip[r] or db.problem[r] < 0 or r == q_kf or r in connected}
    # 1
    words = np.zeros(db.n_db, np.int32)
    for w in qw:
        if 0 <= w < db.n_words:
            for r in db.lists.get(int(w), []):
                if r not in excluded:
                    words[r] += 1
    sharing = [r for r in range(db.n_db) if words[r] > 0]
    s = np.zeros((), SUMMARY_DTYPE)
    s["n_sharing"] = len(sharing)
    s["max_common"] = max([int(words[r]) for r in sharing], default=0)
    # 2
    s["min_common"] = min_common_of(int(s["max_common"]), p["common_ratio"])
    survivors = [r for r in sharing if words[r] > s["min_common"]]
    s["n_survivors"] = len(survivors)
    # 3
    score = np.full(db.n_db, -1.0, F32)
    for r in survivors:
        score[r] = F32(l1_score(qw, qv, *db.vector(r)))
    floor = F32(p["min_score"])
    if p["min_score_mode"] == 1:
        floor = F32(1.0)
        for j in conn:
            if j is None or db.skip[j]:
                continue
            score[j] = F32(l1_score(qw, qv, *db.vector(j)))
            if score[j] < floor:
                floor = score[j]
    s["min_score"] = floor
    seeds = [r for r in survivors if score[r] >= floor]
    s["n_seeds"] = len(seeds)
    # 4
    star = {}
    alive = set(survivors)
    for i in seeds:
        acc, best, best_s = score[i], i, score[i]
        for kf, _weight in nb[i]:
            if kf < 0:
                break
            j = db.row_of(db.problem[i], int(kf))
            if j is None or j not in alive:
                continue
            acc = F32(acc + score[j])
            if score[j] > best_s:
                best, best_s = j, score[j]
        if best not in star or total_key(acc) > total_key(star[best]):
            star[best] = acc
    # 5
    order = sorted(star, key=lambda b: (-total_key(star[b]), b))
    s["best_acc"] = star[order[0]] if order else F32(0.0)
    cut = F32(F32(p["retain_ratio"]) * s["best_acc"])
    chosen, taken = [], [0, 0]
    for b in order:
        cls = int(db.problem[b] != q_problem)
        if cls == 1 and p["scope"] == 0:
            continue
        if p["n_best"] > 0:
            if taken[cls] >= p["n_best"]:
                continue
        elif not star[b] > cut:
            continue
        taken[cls] += 1
        chosen.append((b, cls))
    s["n_candidates"], s["n_written"] = len(chosen), min(len(chosen), cand_cap)
    cand = np.zeros(cand_cap, CAND_DTYPE)
    cand["kf"], cand["problem"] = -1, -1
    for e, (b, cls) in enumerate(chosen[:cand_cap]):
        cand[e] = (b, db.problem[b], words[b], cls, score[b], star[b])
    return cand, s, words, score


def run(case, **over):
    """every query of a case (tests/place_cases.py) -> (cand [n_q][cand_cap], summary [n_q], words [n_q][n_db], score [n_q][n_db])"""
    k = dict(case, **over)
    db = Database(k["db_word"], k["db_value"], k["db_count"], k["n_words"], k["problems"], k["db_skip"])
    q_word, q_value = np.asarray(k["q_word"], np.int32), np.asarray(k["q_value"], np.float64)
    n_q, q_stride = q_word.shape
    out = []
    for q in range(n_q):
        n = min(max(int(k["q_count"][q]), 0), q_stride)
        q_nb = None if k["q_nb"] is None else np.asarray(k["q_nb"])[q]
        q_row = None if k["q_nb"] is None else np.asarray(k["q_row"], ROW_DTYPE)[q]
        out.append(query(db, q_word[q, :n], q_value[q, :n], int(k["q_kf"][q]), int(k["q_problem"][q]), np.asarray(k["nb"]), k["params"], k["cand_cap"], q_nb, q_row))
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], SUMMARY_DTYPE), np.stack([o[2] for o in out]), np.stack([o[3] for o in out]))


# ---- upstream's loops, literally ----
class KeyFrame:
    def __init__(self, row, problem):
        self.row, self.map = row, problem
        self.query, self.words, self.score = None, 0, F32(0.0)  # mnLoopQuery / mnPlaceRecognitionQuery, ...Words, ...Score
        self.best_covisibles = []


def upstream(case, q, **over):
    """KeyFrameDatabase::DetectLoopCandidates (n_best == 0) or DetectNBestCandidates (n_best > 0) for query q of a case: the set of call
    rows it returns (loop and merge candidates together), scope applied at the end"""
    k = dict(case, **over)
    p = dict(DEFAULTS, **k["params"])
    db = Database(k["db_word"], k["db_value"], k["db_count"], k["n_words"], k["problems"], k["db_skip"])
    q_kf, q_problem = int(k["q_kf"][q]), int(k["q_problem"][q])
    n = min(max(int(k["q_count"][q]), 0), np.asarray(k["q_word"]).shape[1])
    qw, qv = np.asarray(k["q_word"], np.int32)[q, :n], np.asarray(k["q_value"], np.float64)[q, :n]
    nb = np.asarray(k["nb"])
    kfs = {r: KeyFrame(r, int(db.problem[r])) for r in range(db.n_db)}
    for r, kf in kfs.items():
        for e in nb[r]:
            if e[0] < 0:
                break
            j = db.row_of(kf.map, int(e[0]))
            if j is not None:
                kf.best_covisibles.append(kfs[j])
    # add() was called for every keyframe but the query; erase() for the bad ones; a keyframe of no map was never added
    inverted = {w: [kfs[r] for r in rows if r != q_kf and not db.skip[r] and db.problem[r] >= 0] for w, rows in db.lists.items()}
    q_nb = None if k["q_nb"] is None else np.asarray(k["q_nb"])[q]
    q_row = None if k["q_nb"] is None else np.asarray(k["q_row"], ROW_DTYPE)[q]
    connected = [kfs[j] for j in connected_rows(db, q_problem, q_nb, q_row) if j is not None]
    sp_connected = set(connected)
    query_id = object()
    sharing = []  # lKFsSharingWords
    for w in qw:
        for kf in inverted.get(int(w), []):
            if kf.query is not query_id:
                kf.words = 0
                if kf not in sp_connected:
                    kf.query = query_id
                    sharing.append(kf)
            kf.words += 1
    if not sharing:
        return set()
    max_common = 0
    for kf in sharing:
        if kf.words > max_common:
            max_common = kf.words
    min_common = int(F32(max_common) * F32(p["common_ratio"]))
    min_score = F32(p["min_score"])
    if p["min_score_mode"] == 1:  # LoopClosing::DetectLoop
        min_score = F32(1.0)
        for kf in connected:
            if db.skip[kf.row]:
                continue
            sc = F32(l1_score(qw, qv, *db.vector(kf.row)))
            if sc < min_score:
                min_score = sc
    score_and_match = []
    for kf in sharing:
        if kf.words > min_common:
            kf.score = F32(l1_score(qw, qv, *db.vector(kf.row)))
            if kf.score >= min_score:
                score_and_match.append((kf.score, kf))
    if not score_and_match:
        return set()
    acc_and_match, best_acc = [], F32(min_score)
    for sc, kf in score_and_match:
        best_score, acc, best = sc, sc, kf
        for kf2 in kf.best_covisibles[:k["nb"].shape[1]]:
            if kf2.query is query_id and kf2.words > min_common:  # DetectNBestCandidates tests the mark alone: the deviation
                acc = F32(acc + kf2.score)
                if kf2.score > best_score:
                    best, best_score = kf2, kf2.score
        acc_and_match.append((acc, best))
        if acc > best_acc:
            best_acc = acc
    out, already = [], set()
    if p["n_best"] == 0:
        retain = F32(F32(p["retain_ratio"]) * best_acc)
        for acc, kf in acc_and_match:
            if acc > retain and kf not in already:
                out.append(kf)
                already.add(kf)
    else:
        acc_and_match.sort(key=lambda t: -float(t[0]))  # list::sort(compFirst) is stable
        loops = merges = 0
        for acc, kf in acc_and_match:
            if kf in already:
                continue
            if kf.map == q_problem and loops < p["n_best"]:
                out.append(kf)
                loops += 1
            elif kf.map != q_problem and merges < p["n_best"]:
                out.append(kf)
                merges += 1
            else:
                continue
            already.add(kf)
    return {kf.row for kf in out if p["scope"] == 1 or kf.map == q_problem}
