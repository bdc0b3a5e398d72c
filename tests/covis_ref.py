"""The covisibility rule of include/sendslam_orb.h restated in numpy and plain Python: its normative statement.  Integer counting on
the map's observation records; one float32 multiply and compare closes the culling vote.  Written from the rule, not from the
library's text: it builds no sorted table and no incidence list of the library's shape, only a dictionary per point."""
import numpy as np

OBS_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("right", "<f4"), ("octave", "<i4")])
PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_kf", "n_kf", "first_block", "n_blocks", "first_obs", "n_obs")] + [("reserved", "<i4", (2,))])
ROW_DTYPE = np.dtype([(n, "<i4") for n in ("n_shared", "max_weight", "max_kf", "n_listed", "n_written", "n_mps", "n_redundant", "redundant")])
DEFAULTS = dict(min_weight=15, fallback=1, cull_obs=3, cull_slack=1, redundant_th=0.9)
MAX_ROW_ITEMS, MAX_NEIGHBOURS = 262143, 1024


def obs_records(kf, point, octave=0, right=-1.0):
    """records from arrays (or scalars) of kf, point, octave and right"""
    kf = np.atleast_1d(np.asarray(kf, np.int32))
    out = np.zeros(len(kf), OBS_DTYPE)
    out["kf"], out["point"], out["octave"], out["right"] = kf, point, octave, right
    return out


class Map:
    """problems: rows of PROBLEM_DTYPE (or tuples in its order); obs: OBS_DTYPE of the call; skip: one byte per record or None.
    Per problem q: points[q][i] = {kf: (octave, stereo, skip)} of the observations only, seen[q][k] = {i: (octave, skip)}"""

    def __init__(self, problems, n_kf, n_blocks, point_rows, obs, n_levels, skip=None, check_right=False):
        self.problems = np.array(problems, PROBLEM_DTYPE).reshape(-1)
        self.n_kf, self.n_blocks, self.point_rows = n_kf, n_blocks, point_rows
        self.kf_prob, self.blk_prob = np.full(n_kf, -1), np.full(n_blocks, -1)
        self.points, self.seen = [], []
        obs = np.asarray(obs, OBS_DTYPE)
        for q, pr in enumerate(self.problems):
            self.kf_prob[pr["first_kf"]:pr["first_kf"] + pr["n_kf"]] = q
            self.blk_prob[pr["first_block"]:pr["first_block"] + pr["n_blocks"]] = q
            points, seen = {}, {}
            for m in range(pr["first_obs"], pr["first_obs"] + pr["n_obs"]):
                o = obs[m]
                k, i, octave = int(o["kf"]), int(o["point"]), int(o["octave"])
                assert 0 <= k < pr["n_kf"] and 0 <= i < pr["n_blocks"] * point_rows
                if not 0 <= octave < n_levels:
                    continue  # not an observation: it neither votes nor counts
                assert k not in points.get(i, {}), "a (kf, point) pair twice"
                sk = bool(skip is not None and skip[m])
                points.setdefault(i, {})[k] = (octave, bool(check_right and o["right"] > 0), sk)
                seen.setdefault(k, {})[i] = (octave, sk)
            self.points.append(points)
            self.seen.append(seen)


def weights_kf(m, kf):
    """w(j) of the keyframe row `kf` (a call keyframe number) -> (problem or -1, {j: w})"""
    q = int(m.kf_prob[kf])
    w = {}
    if q >= 0:
        k = kf - int(m.problems[q]["first_kf"])
        for i in m.seen[q].get(k, {}):
            for j in m.points[q][i]:
                if j != k:
                    w[j] = w.get(j, 0) + 1
    return q, w


def weights_frame(m, idx_row, n_points, block):
    q = int(m.blk_prob[block])
    w = {}
    if q >= 0:
        n = min(max(int(n_points), 0), m.point_rows)
        base = (block - int(m.problems[q]["first_block"])) * m.point_rows
        for i in np.flatnonzero(np.asarray(idx_row[:n]) >= 0):
            for j in m.points[q].get(base + int(i), {}):
                w[j] = w.get(j, 0) + 1
    return q, w


def point_count(m, q, i):
    """count(i): the observations of point i of problem q plus its stereo ones once more (MapPoint::Observations())"""
    return sum(2 if stereo else 1 for (_, stereo, _) in m.points[q].get(i, {}).values())


def point_near(m, q, i, k, slack):
    """near: the observations (j, i), j != k, with octave_j <= octave_k + slack"""
    obs = m.points[q][i]
    return sum(1 for j, (oj, _, _) in obs.items() if j != k and oj <= obs[k][0] + slack)


def culling(m, kf, p):
    """(n_mps, n_redundant) of the keyframe row"""
    q = int(m.kf_prob[kf])
    n_mps = n_red = 0
    if q >= 0:
        k = kf - int(m.problems[q]["first_kf"])
        for i, (octave, skip) in m.seen[q].get(k, {}).items():
            if skip:
                continue
            n_mps += 1
            if point_count(m, q, i) > p["cull_obs"] and point_near(m, q, i, k, p["cull_slack"]) > p["cull_obs"]:
                n_red += 1
    return n_mps, n_red


def finish(w, p, cap, n_mps=0, n_red=0):
    """the summary and the neighbour list of one row from its weights"""
    nb, row = np.zeros((cap, 2), np.int32), np.zeros((), ROW_DTYPE)
    nb[:] = (-1, 0)
    shared = sorted((j for j in w if w[j] > 0), key=lambda j: (-w[j], j))
    row["n_shared"] = len(shared)
    row["max_weight"], row["max_kf"] = (w[shared[0]], shared[0]) if shared else (0, -1)
    listed = [j for j in shared if w[j] >= p["min_weight"]]
    if not listed and p["fallback"] and shared:
        listed = [shared[0]]
    row["n_listed"], row["n_written"] = len(listed), min(len(listed), cap)
    for e, j in enumerate(listed[:cap]):
        nb[e] = (j, w[j])
    row["n_mps"], row["n_redundant"] = n_mps, n_red
    row["redundant"] = int(np.float32(n_red) > np.float32(p["redundant_th"]) * np.float32(n_mps))
    return nb, row


def kf_rows(m, rows, params, cap):
    """-> (nb int32 [n_rows][cap][2], ROW_DTYPE [n_rows]); rows None: every keyframe of the map"""
    p = dict(DEFAULTS, **params)
    rows = range(m.n_kf) if rows is None else rows
    out = [finish(weights_kf(m, int(k))[1], p, cap, *culling(m, int(k), p)) for k in rows]
    return np.array([o[0] for o in out], np.int32).reshape(-1, cap, 2), np.array([o[1] for o in out], ROW_DTYPE).reshape(-1)


def frame_rows(m, idx, n_points, point_src, params, cap):
    p = dict(DEFAULTS, **params)
    out = [finish(weights_frame(m, idx[b], n_points[blk], int(blk))[1], p, cap) for b, blk in enumerate(point_src)]
    return np.array([o[0] for o in out], np.int32).reshape(-1, cap, 2), np.array([o[1] for o in out], ROW_DTYPE).reshape(-1)


def edges(nb, row, row_kf, min_weight):
    """the pairs (k, j), j > k, of weight >= min_weight, in ascending row and then list order"""
    out = []
    for r in range(len(row)):
        for e in range(int(row[r]["n_written"])):
            j, w = int(nb[r][e][0]), int(nb[r][e][1])
            if j > int(row_kf[r]) and w >= min_weight:
                out.append((int(row_kf[r]), j))
    return np.array(out, np.int32).reshape(-1, 2)
