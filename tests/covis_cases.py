"""Cases of the covisibility tests: combinatorial incidence tables, no geometry.  A case is one problem: n_kf keyframes, n_points
points, its records (relative to the problem), optional skip bytes, check_right, the parameters, the cap and the rows to query (None:
every keyframe).  tests/test_covis_ref.py holds the host twin to the reference on them and asserts that each exercises the branch it is
named for; tests/test_covis.py holds the device to the reference (shared cases) or to the host twin (ladders)."""
import numpy as np

import covis_ref as CR

N_LEVELS = 8  # the pyramid of the tests' context


def case(n_kf, n_points, recs, skip=None, check_right=False, params=None, cap=64, rows=None):
    obs = np.concatenate([np.asarray(r, CR.OBS_DTYPE).reshape(-1) for r in recs]) if len(recs) else np.zeros(0, CR.OBS_DTYPE)
    return dict(n_kf=n_kf, n_points=n_points, obs=obs, skip=None if skip is None else np.asarray(skip, np.uint8), check_right=check_right,
                params=dict(params or {}), cap=cap, rows=rows)


def _seen_by(point, kfs, octave=0, right=-1.0):
    kfs = np.asarray(kfs, np.int32)
    return CR.obs_records(kfs, np.full(len(kfs), point, np.int32), octave, right)


def planted(**params):
    """keyframe 0 shares exactly j points with keyframe j, j = 1 .. 40"""
    recs, i = [], 0
    for j in range(1, 41):
        for _ in range(j):
            recs.append(_seen_by(i, [0, j]))
            i += 1
    return case(41, i, recs, params=params)


def lonely():
    """keyframe 0 and 2 see points nobody else sees, keyframe 1 has no record"""
    return case(3, 6, [_seen_by(i, [0]) for i in range(5)] + [_seen_by(5, [2])])


def ties(cap=64):
    """keyframe 0: thirty neighbours (3 .. 32) at weight 16, two (1 and 2) at the maximum of 20"""
    recs, i = [], 0
    for j, w in [(1, 20), (2, 20)] + [(j, 16) for j in range(3, 33)]:
        for _ in range(w):
            recs.append(_seen_by(i, [0, j]))
            i += 1
    return case(33, i, recs, cap=cap, rows=[0])


def many_listed(cap=1024):
    """keyframe 0 against 1500 neighbours of weight 1 .. 3 under min_weight 1: more listed than the largest cap"""
    recs, i = [], 0
    for j in range(1, 1501):
        for _ in range(1 + j % 3):
            recs.append(_seen_by(i, [0, j]))
            i += 1
    return case(1501, i, recs, cap=cap, rows=[0], params=dict(min_weight=1))


def culling():
    """keyframe 0 sees every point at octave 2; see the comments for what each point checks.  n_mps 8, n_redundant 2"""
    lv = N_LEVELS
    recs = [
        _seen_by(0, [0], 2), _seen_by(0, [1, 2]),                       # count 3, near 2: no
        _seen_by(1, [0], 2), _seen_by(1, [1, 2, 3]),                    # count 4, near 3: no (near > 3 fails)
        _seen_by(2, [0], 2), _seen_by(2, [1, 2, 3, 4]),                 # count 5, near 4: redundant
        _seen_by(3, [0], 2), _seen_by(3, [1, 2, 3, 4], 3),              # an octave above: near 4, redundant
        _seen_by(4, [0], 2), _seen_by(4, [1, 2, 3, 4], 4),              # two octaves above: near 0
        _seen_by(5, [0], 2), _seen_by(5, [1, 2, 3], 3), _seen_by(5, [4], 4),  # near 3
        _seen_by(6, [0], 2, 5.0), _seen_by(6, [1], 0, 7.0), _seen_by(6, [2]),  # two stereo records: count 5 under check_right, 3 without
        _seen_by(7, [0], 2), _seen_by(7, [1, 2, 3, 4]),                 # keyframe 0's record carries a skip byte: not examined
        _seen_by(8, [0], 2), _seen_by(8, [1, 2, 3]), _seen_by(8, [4], -1), _seen_by(8, [5], lv),  # octaves -1 and n_levels: near 3
        _seen_by(9, [0], -1), _seen_by(9, [1, 2, 3, 4]),                # keyframe 0's own record is no observation: no item
    ]
    obs = np.concatenate(recs)
    skip = np.zeros(len(obs), np.uint8)
    skip[(obs["point"] == 7) & (obs["kf"] == 0)] = 1
    skip[(obs["point"] == 2) & (obs["kf"] == 3)] = 1  # another keyframe's skip byte changes nothing in row 0
    return case(6, 10, [obs], skip=skip, check_right=True, params=dict(min_weight=1))


def ten_items(n_redundant):
    """keyframe 0 sees ten points; n_redundant of them are seen by four more keyframes, the rest by two"""
    recs = []
    for i in range(10):
        recs += [_seen_by(i, [0]), _seen_by(i, [1, 2, 3, 4] if i < n_redundant else [1, 2])]
    return case(5, 10, recs, rows=[0])


def shared_cases():
    return {"planted": planted(), "planted_no_fallback": planted(fallback=0), "planted_min1": planted(min_weight=1), "lonely": lonely(), "ties": ties(),
            "cap_1": ties(1), "cap_listed": ties(32), "cap_listed_less_1": ties(31), "cap_1024_of_1500": many_listed(), "culling": culling(),
            "culling_mono": dict(culling(), check_right=False), "ten_9": ten_items(9), "ten_10": ten_items(10)}


# ---- ladders ----
KF_LADDER = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 16384)
ITEM_LADDER = (0, 1, 255, 256, 257, 513)
LIST_LADDER = (1, 2, 63, 64, 65, 300)


def random_map(n_kf, seed, n_points=None, rows=None, params=None, cap=48):
    """every point seen by 1 .. 6 keyframes, the first and the last keyframe more often than the rest; octaves -1 .. N_LEVELS, some stereo,
    some skipped"""
    rng = np.random.default_rng(seed)
    P = n_points if n_points is not None else max(8, min(2 * n_kf, 1500))
    recs = []
    for i in range(P):
        kfs = set(rng.choice(n_kf, size=min(n_kf, int(rng.integers(1, 7))), replace=False).tolist())
        if rng.random() < 0.4:
            kfs.add(0)
        if rng.random() < 0.4:
            kfs.add(n_kf - 1)
        kfs = np.array(sorted(kfs), np.int32)
        recs.append(CR.obs_records(kfs, np.full(len(kfs), i, np.int32), rng.integers(-1, N_LEVELS + 1, len(kfs)), np.where(rng.random(len(kfs)) < 0.3, 9.0, -1.0)))
    obs = np.concatenate(recs)
    obs = obs[rng.permutation(len(obs))]
    return case(n_kf, P, [obs], skip=(rng.random(len(obs)) < 0.1), check_right=True, params=dict(dict(min_weight=2), **(params or {})), cap=cap, rows=rows)


def kf_ladder(n_kf):
    return random_map(n_kf, 100 + n_kf, rows=[0, n_kf - 1] if n_kf > 2000 else None)


def item_ladder(n_items):
    """keyframe 0 has exactly n_items records"""
    rng = np.random.default_rng(200 + n_items)
    recs = []
    for i in range(max(n_items, 1) + 3):
        others = (1 + np.flatnonzero(rng.random(5) < 0.6)).astype(np.int32)
        kfs = np.concatenate([[0] if i < n_items else [], others]).astype(np.int32)
        if len(kfs):
            recs.append(CR.obs_records(kfs, np.full(len(kfs), i, np.int32), rng.integers(0, 4, len(kfs))))
    return case(6, max(n_items, 1) + 3, recs, params=dict(min_weight=1), rows=[0, 1])


def list_ladder(n_seen):
    """three points seen by exactly n_seen keyframes each (0 among them), and one seen by keyframe 0 alone"""
    n_kf = 301
    rng = np.random.default_rng(300 + n_seen)
    recs = [_seen_by(3, [0])]
    for i in range(3):
        kfs = np.sort(np.concatenate([[0], 1 + rng.choice(n_kf - 1, size=n_seen - 1, replace=False)])).astype(np.int32)
        recs.append(CR.obs_records(kfs, np.full(len(kfs), i, np.int32), rng.integers(0, 3, len(kfs))))
    return case(n_kf, 4, recs, params=dict(min_weight=2), cap=512, rows=[0, 300, 17])


def key_ends():
    """both ends of the sort key: keyframe 0 shares 16 383 points with keyframe 16 383, and three with keyframe 5"""
    pts = np.arange(16383, dtype=np.int32)
    recs = [CR.obs_records(np.zeros(16383, np.int32), pts), CR.obs_records(np.full(16383, 16383, np.int32), pts), CR.obs_records(np.full(3, 5, np.int32), pts[:3])]
    return case(16384, 16383, recs, params=dict(min_weight=1), cap=4, rows=[0, 16383, 5])


def ladder_cases():
    out = {f"kf_{n}": kf_ladder(n) for n in KF_LADDER}
    out.update({f"items_{n}": item_ladder(n) for n in ITEM_LADDER})
    out.update({f"list_{n}": list_ladder(n) for n in LIST_LADDER})
    out["key_ends"] = key_ends()
    return out


# ---- calls ----
def stack(cases, point_rows, lead=0, gap=0, order=None, shuffle_seed=None):
    """the problems of one map, each with blocks of point_rows rows of its own: keyframes, blocks and records one problem after the other in
    the order `order`, after `lead` keyframes, blocks and records of no problem and with `gap` of each between two problems; the records of
    no problem hold junk -> a dict: table (in the cases' order), n_kf, n_blocks, point_rows, obs, skip, check_right"""
    order = list(range(len(cases))) if order is None else order
    at_kf = at_blk = at_obs = lead
    table = [None] * len(cases)
    for q in order:
        c = cases[q]
        nb = -(-c["n_points"] // point_rows)
        table[q] = (at_kf, c["n_kf"], at_blk, nb, at_obs, len(c["obs"]), (0, 0))
        at_kf, at_blk, at_obs = at_kf + c["n_kf"] + gap, at_blk + nb + gap, at_obs + len(c["obs"]) + gap
    obs = np.zeros(at_obs, CR.OBS_DTYPE)
    obs["kf"], obs["point"], obs["octave"] = -3, 1 << 30, 1
    skip = np.ones(at_obs, np.uint8)
    for q, c in enumerate(cases):
        s0, ns = table[q][4], table[q][5]
        seg = c["obs"].copy()
        sk = np.zeros(ns, np.uint8) if c["skip"] is None else c["skip"].astype(np.uint8).copy()
        if shuffle_seed is not None:
            perm = np.random.default_rng(shuffle_seed + q).permutation(ns)
            seg, sk = seg[perm], sk[perm]
        obs[s0:s0 + ns], skip[s0:s0 + ns] = seg, sk
    assert len({c["check_right"] for c in cases}) == 1
    return dict(table=np.array(table, CR.PROBLEM_DTYPE), n_kf=at_kf, n_blocks=at_blk, point_rows=point_rows, obs=obs, skip=skip, check_right=cases[0]["check_right"])


def single(c, point_rows=None):
    return stack([c], point_rows or max(1, min(c["n_points"], 16384)))


def ref_map(call):
    return CR.Map(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], N_LEVELS, call["skip"], call["check_right"])


def frames_case():
    """a map of two problems and the frame rows of the issue: idx of -1, 0 and large values, hits past n_points, n_points beyond point_rows
    and below 0, two frames on one block, a frame on a block of no problem -> (call, idx, n_points, point_src)"""
    rows = 96
    a, b = random_map(40, 7, n_points=2 * rows), random_map(9, 8, n_points=rows - 5)
    call = stack([dict(a, check_right=True), b], rows, lead=1, gap=1, shuffle_seed=3)
    rng = np.random.default_rng(11)
    # blocks: 0 lead (no problem), 1 2 problem 0, 3 gap, 4 problem 1, 5 gap
    point_src = np.array([1, 2, 2, 0, 4, 4, 3, 1], np.int32)
    idx = rng.choice(np.array([-1, -1, 0, 5, 2 ** 31 - 1, 123456, -7], np.int64), size=(len(point_src), rows)).astype(np.int32)
    idx[7] = -1  # a frame without a hit
    n_points = np.array([rows, rows, rows - 10, rows, rows + 500, -4], np.int32)  # block 4 beyond point_rows, block 5 below 0
    return call, idx, n_points, point_src
