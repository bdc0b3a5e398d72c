"""Cases of the map-point refresh tests.  A case is one problem: n_kf keyframes with a camera centre and rows_per_frame descriptors
each, n_points points, and per point its list of records (kf, octave, right); every record gets a keypoint row.  single() lays a case
out as a call of one block, stack() several cases as the problems of one call with gaps between their keyframes, blocks and records.
tests/test_refresh_ref.py holds the host twin to the reference on them and asserts that the cases are live; tests/test_refresh.py
holds the device to the reference (shared cases) or to the host twin (ladders)."""
import numpy as np

import refresh_ref as RR

N_LEVELS = 8  # the pyramid of the tests' context
LADDER = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
VIEW_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))] + [(n, "<f4") for n in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y")])


def case(n_kf, lists, seed, rows_per_frame=8, ow=None, xyz=None, desc=None, ref_kf=None, select=None, check_right=False, n_points=None, rows=None):
    """lists: per point a list of (kf, octave) or (kf, octave, right) in any order"""
    rng = np.random.default_rng(seed)
    P = len(lists)
    recs = [(k[0], i, k[1], k[2] if len(k) > 2 else -1.0) for i, lst in enumerate(lists) for k in lst]
    obs = np.zeros(len(recs), RR.OBS_DTYPE)
    for m, (kf, i, octave, right) in enumerate(recs):
        obs[m]["kf"], obs[m]["point"], obs[m]["octave"], obs[m]["right"] = kf, i, octave, right
    obs["u"], obs["v"] = rng.random(len(recs)) * 600, rng.random(len(recs)) * 400
    points = np.zeros(P, RR.MAP_POINT_DTYPE)
    pos = rng.normal(0, 4, (P, 3)).astype(np.float32) if xyz is None else np.asarray(xyz, np.float32)
    points["x"], points["y"], points["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    for name in ("nx", "ny", "nz", "min_dist", "max_dist"):
        points[name] = -77.0  # what a refresh never leaves
    return dict(n_kf=n_kf, n_points=P, count=P if n_points is None else n_points, obs=obs,
                obs_row=rng.integers(0, rows_per_frame, len(recs)).astype(np.int32) if rows is None else np.asarray(rows, np.int32),
                points=points, point_desc=np.full((P, 32), 0xC3, np.uint8), rows_per_frame=rows_per_frame,
                ow=(rng.normal(0, 9, (n_kf, 3)).astype(np.float32) if ow is None else np.asarray(ow, np.float32)),
                desc=rng.integers(0, 256, (n_kf, rows_per_frame, 32)).astype(np.uint8) if desc is None else np.asarray(desc, np.uint8),
                ref_kf=None if ref_kf is None else np.asarray(ref_kf, np.int32), select=None if select is None else np.asarray(select, np.uint8), check_right=check_right)


def views_of(ow):
    v = np.zeros(len(ow), VIEW_DTYPE)
    v["ow"] = ow
    v["rcw"][:, [0, 4, 8]] = 1
    v["tcw"] = -np.asarray(ow)
    return v


def stack(cases, point_rows, lead=0, gap=0, order=None, shuffle_seed=None):
    """the cases as the problems of one call: `lead` keyframes, blocks and junk records ahead of the first, `gap` between two; order:
    the problems' order in the table; the records of each problem shuffled under shuffle_seed.  Every case takes the blocks it needs"""
    order = list(range(len(cases))) if order is None else order
    rpf = max(c["rows_per_frame"] for c in cases)
    table, obs, rows, kf0, blk0, obs0 = [None] * len(cases), [], [], lead, lead, lead
    junk = np.zeros(1, RR.OBS_DTYPE)
    junk["kf"], junk["point"] = 99999, 99999
    obs += [junk] * lead
    rows += [np.full(1, -5, np.int32)] * lead  # a junk record's row is never read
    parts = []
    for q, c in enumerate(cases):
        nb = max(1, -(-c["n_points"] // point_rows))
        o, r = c["obs"].copy(), c["obs_row"].copy()
        if shuffle_seed is not None:
            perm = np.random.default_rng(shuffle_seed + q).permutation(len(o))
            o, r = o[perm], r[perm]
        table[order.index(q)] = (kf0, c["n_kf"], blk0, nb, obs0, len(o), (0, 0))
        parts.append((c, kf0, blk0, nb))
        obs += [o] + [junk] * gap
        rows += [r] + [np.full(1, -5, np.int32)] * gap
        kf0, blk0, obs0 = kf0 + c["n_kf"] + gap, blk0 + nb + gap, obs0 + len(o) + gap
    n_kf, n_blocks = kf0, blk0
    points, pdesc = np.zeros((n_blocks, point_rows), RR.MAP_POINT_DTYPE), np.full((n_blocks, point_rows, 32), 0xC3, np.uint8)
    for name in RR.MAP_POINT_DTYPE.names:
        points[name] = 3.5  # the rows of no problem are finite points nobody refreshes
    n_points = np.full(n_blocks, point_rows, np.int32)
    any_ref, any_sel = any(c["ref_kf"] is not None for c in cases), any(c["select"] is not None for c in cases)
    ref_kf, select = (np.full((n_blocks, point_rows), -1, np.int32) if any_ref else None), (np.zeros((n_blocks, point_rows), np.uint8) if any_sel else None)
    ow = np.full((n_kf, 3), 1e3, np.float32)
    desc = np.random.default_rng(77).integers(0, 256, (n_kf, rpf, 32)).astype(np.uint8)
    for c, k0, b0, nb in parts:
        P = c["n_points"]
        flat = slice(b0 * point_rows, b0 * point_rows + P)
        points.reshape(-1)[flat], pdesc.reshape(-1, 32)[flat] = c["points"], c["point_desc"]
        for b in range(nb):
            n_points[b0 + b] = c["count"] - b * point_rows if c["count"] != P else min(P - b * point_rows, point_rows)  # a count given: as it is, unclamped
        if c["ref_kf"] is not None:
            ref_kf.reshape(-1)[flat] = c["ref_kf"]
        if c["select"] is not None:
            select.reshape(-1)[flat] = c["select"]
        ow[k0:k0 + c["n_kf"]] = c["ow"]
        desc[k0:k0 + c["n_kf"], :c["rows_per_frame"]] = c["desc"]
    return dict(table=np.array(table, RR.PROBLEM_DTYPE), n_kf=n_kf, n_blocks=n_blocks, point_rows=point_rows, obs=np.concatenate(obs) if obs else np.zeros(0, RR.OBS_DTYPE),
                obs_row=np.concatenate(rows) if rows else np.zeros(0, np.int32), points=points, point_desc=pdesc, n_points=n_points, ref_kf=ref_kf, select=select,
                desc=desc, rows_per_frame=rpf, views=views_of(ow), check_right=any(c["check_right"] for c in cases))


def single(c, point_rows=None):
    return stack([c], point_rows or max(c["n_points"], 1))


def random_case(seed, n_kf=12, n_points=40, max_len=None, pool=None, rows_per_frame=8):
    """lists of 0 .. max_len records, octaves -1 .. N_LEVELS, some stereo; a reference keyframe table with every kind of entry and a
    select table with 0, 1 and 2; pool: the descriptors are drawn from so few that medians tie"""
    rng = np.random.default_rng(seed)
    max_len = n_kf if max_len is None else max_len
    lists = []
    for _ in range(n_points):
        kfs = rng.choice(n_kf, size=int(rng.integers(0, max_len + 1)), replace=False)
        lists.append([(int(k), int(rng.integers(-1, N_LEVELS + 1)) if rng.random() < 0.2 else int(rng.integers(0, N_LEVELS)), 5.0 if rng.random() < 0.3 else -1.0) for k in kfs])
    desc = None
    if pool:
        base = rng.integers(0, 256, (pool, 32)).astype(np.uint8)
        desc = base[rng.integers(0, pool, (n_kf, rows_per_frame))]
        flip = rng.random((n_kf, rows_per_frame)) < 0.5
        desc[flip, 0] ^= 1
    ref = rng.integers(-1, n_kf, n_points)
    sel = np.where(rng.random(n_points) < 0.15, rng.integers(1, 3, n_points), 0)
    xyz = rng.normal(0, 4, (n_points, 3)).astype(np.float32)
    xyz[rng.random(n_points) < 0.05, 0] = np.nan
    return case(n_kf, lists, seed + 1000, rows_per_frame=rows_per_frame, desc=desc, ref_kf=ref, select=sel, check_right=True, xyz=xyz)


def ladder_case(length, seed=3):
    """one point seen by `length` keyframes, one whose list of `length` records holds records that are no observation, one seen once"""
    rng = np.random.default_rng(seed + length)
    n_kf = max(length, 2)
    full = [(k, int(rng.integers(0, N_LEVELS))) for k in range(length)]
    holes = [(k, -1 if rng.random() < 0.3 else int(rng.integers(0, N_LEVELS)), 2.0) for k in range(length)]
    return case(n_kf, [full, holes, [(n_kf - 1, 3)]], seed + length, rows_per_frame=3, ref_kf=[length // 2, 0, -1], check_right=True)


def shared_cases():
    return {"random_12": random_case(1), "random_70": random_case(2, n_kf=70, n_points=30), "ties_pool_3": random_case(3, n_kf=20, n_points=60, pool=3),
            "ties_pool_2": random_case(4, n_kf=9, n_points=60, pool=2), "one_row_frames": random_case(5, n_kf=6, n_points=20, rows_per_frame=1)}


def ladder_cases(extra=()):
    return {f"len_{n}": ladder_case(n) for n in LADDER + tuple(extra)}
