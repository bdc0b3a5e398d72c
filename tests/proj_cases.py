"""The scenes, crafted tables and cached references the projection-search tests share (test infrastructure, plain module).

    scenes()           map points = a frame's oracle keypoints back-projected at varied depths, seen under a pose a few pixels away
                       from identity, searched in a train frame of guided_cases (320 x 240, 500 features)
    boundary_table()   identity pose, exact products: every boundary of steps 1 - 3 taken with np.nextafter on both sides
    ratio_frames()     the level-aware acceptance test, a taken row and a right-eye rejection that change the winner
    capacity_frames()  two frames of SS_GUIDED_MAX_ROWS points and train rows
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import guided_cases as G
import proj_ref as P

f32 = np.float32
FX = FY = 300.0
CX, CY = 160.0, 120.0
BF = 30.0
SCENES = [("synth_t0", "synth_t0"), ("synth_t0", "synth_t1"), ("checker", "checker_shift")]

# ratio on / off x one_to_one x th x check_right x the taken mask
COMBOS = [dict(ratio=r, one_to_one=bool(o), th=t, check_right=bool(c), taken=bool(k))
          for r, o, t, c, k in itertools.product(((8, 10), (0, 0)), (0, 1), (1.0, 3.0), (0, 1), (0, 1))]


def combo_name(c) -> str:
    return f"r{c['ratio'][0]}_{c['ratio'][1]}_u{int(c['one_to_one'])}_th{int(c['th'])}_right{int(c['check_right'])}_taken{int(c['taken'])}"


def scale():
    """the pyramid table of the default parameters (1.2, 8 levels); it does not depend on the image size"""
    return G.scales()


def rot(ax: float, ay: float, az: float = 0.0) -> np.ndarray:
    def r(i, j, a):
        m = np.eye(3)
        c, s = np.cos(a), np.sin(a)
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return r(1, 2, ax) @ r(2, 0, ay) @ r(0, 1, az)


POSES = [(rot(0.003, -0.004, 0.002), (0.02, -0.01, 0.03)), (rot(-0.002, 0.005), (-0.03, 0.02, -0.02)), (rot(0.004, 0.003, -0.003), (0.01, 0.03, 0.05))]


def desc_near(rng, desc, max_bits: int = 5) -> np.ndarray:
    """the descriptors with 0 .. max_bits random bits flipped each"""
    d = np.ascontiguousarray(desc, np.uint8).copy()
    for i in range(len(d)):
        for bit in rng.integers(0, 256, rng.integers(0, max_bits + 1)):
            d[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def back_project(rng, kp, sc, fx=FX, fy=FY, cx=CX, cy=CY, depth=None):
    """keypoints -> MAP_POINT_DTYPE rows in the frame of an identity camera, and their depths.  Depths 2 .. 8; the viewing
    direction exact, tilted by about 20 degrees or by about 70 (below the 0.5 limit); max_dist puts the predicted level on the
    keypoint's octave, one above (still a candidate) or one below (none); a few points are too near, behind the camera or
    outside the image"""
    n = len(kp)
    z = 2.0 + 6.0 * rng.random(n) if depth is None else np.asarray(depth, np.float64)
    what = rng.random(n)
    z = np.where((what > 0.90) & (what <= 0.93), -z, z)
    x = (kp["x"].astype(np.float64) - cx) / fx * z
    y = (kp["y"].astype(np.float64) - cy) / fy * z
    x = np.where((what > 0.93) & (what <= 0.96), x + 3.0 * z, x)
    dist = np.sqrt(x * x + y * y + z * z)
    nrm = np.stack([x, y, z], 1) / dist[:, None]
    tilt = rng.choice([0.0, 0.35, 1.2], n, p=[0.6, 0.3, 0.1])
    for i in range(n):
        nrm[i] = rot(tilt[i], 0.0) @ nrm[i]
    factor = rng.choice([0.95, 1.1, 0.8], n, p=[0.6, 0.3, 0.1])
    scl = np.array([float(s) for s in sc])
    pts = np.zeros(n, P.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = x, y, z
    pts["nx"], pts["ny"], pts["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    pts["max_dist"] = dist * scl[np.clip(kp["octave"], 0, len(scl) - 1)] * factor
    pts["min_dist"] = np.where((what > 0.96) & (what <= 0.99), 2.0 * dist, 0.3 * dist)
    return pts, z


@functools.lru_cache(maxsize=None)
def scenes():
    """-> list of dicts view points p_desc t_kp t_desc right taken, one per SCENES entry"""
    out = []
    for k, (src, train) in enumerate(SCENES):
        rng = np.random.Generator(np.random.PCG64(0x9E0 + k))
        kp, desc = G.features(src)
        tk, td = G.features(train)
        pts, z = back_project(rng, kp, scale())
        view = P.view_init(FX, FY, CX, CY, G.W, G.H, POSES[k][0], POSES[k][1], BF)
        # right coordinates: a stereo match at the row's depth (the map point's depth where both frames are the same, else a random
        # one), -1 for a monocular row, a wrong one for some; taken: one row in five
        depth = np.resize(np.abs(z), len(tk))
        right = (tk["x"].astype(np.float64) - BF / depth + rng.normal(0, 0.5, len(tk))).astype(np.float32)
        kind = rng.random(len(tk))
        right = np.where(kind < 0.15, f32(-1), np.where(kind < 0.30, right - f32(40), right)).astype(np.float32)
        taken = (rng.random(len(tk)) < 0.2).astype(np.uint8)
        out.append({"view": view, "points": pts, "p_desc": desc_near(rng, desc), "t_kp": tk, "t_desc": td, "right": right, "taken": taken})
    return out


@functools.lru_cache(maxsize=None)
def scene_proj(k: int, th: float):
    s = scenes()[k]
    return P.eval_points(s["view"], s["points"], 0.5, th, 0.0, scale())


@functools.lru_cache(maxsize=None)
def scene_found(k: int, th: float, check_right: bool, taken: bool):
    s = scenes()[k]
    return P.search(scene_proj(k, th), s["p_desc"], s["t_kp"], s["t_desc"], check_right, s["right"], s["taken"] if taken else None)


def scene_reference(k: int, combo):
    """-> (idx, d1, d2, proj, summary, cands) of scene k under a COMBOS entry; the search is computed once per (th, right, taken)"""
    s = scenes()[k]
    proj = scene_proj(k, combo["th"])
    idx, d1, d2, summ, cands = P.finish(scene_found(k, combo["th"], combo["check_right"], combo["taken"]), proj, s["t_kp"], 100,
                                        combo["ratio"][0], combo["ratio"][1], combo["one_to_one"])
    return idx, d1, d2, proj, summ, cands


def combo_params(binding, combo, **kw):
    return binding.proj_params(view_cos_limit=0.5, th=combo["th"], far_limit=0.0, th_high=100, ratio_num=combo["ratio"][0],
                               ratio_den=combo["ratio"][1], one_to_one=combo["one_to_one"], check_right=combo["check_right"], **kw)


# ---- the boundary table -------------------------------------------------------------------------------------------------------
B_FX = 256.0                      # a power of two: fx * x is exact
B_LIMITS = dict(view_cos_limit=0.5, th=1.0, far_limit=3.0)


def _point(x=0.0, y=0.0, z=1.0, nx=0.0, ny=0.0, nz=1.0, min_dist=0.1, max_dist=1.0):
    p = np.zeros((), P.MAP_POINT_DTYPE)
    p["x"], p["y"], p["z"], p["nx"], p["ny"], p["nz"], p["min_dist"], p["max_dist"] = x, y, z, nx, ny, nz, min_dist, max_dist
    return p


def around(v):
    """the float32 below, the value, the float32 above"""
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


@functools.lru_cache(maxsize=None)
def boundary_table():
    """-> (view, points, groups, train keypoints).  Identity pose, principal point 0, image bounds -160 .. 160 x -120 .. 120: with
    x = y = 0 the distance is z and the cosine nz, with z = 1 the projection is 256 * x and the ratio max_dist, all exactly.
    groups: (name, first row, live): three consecutive rows below / on / above a boundary; live False = a boundary the rule makes
    moot (ratio on the last table entry: both sides give the last level)."""
    sc = scale()
    view = P.view_init(B_FX, B_FX, 0.0, 0.0, 0, 0, np.eye(3), (0.0, 0.0, 0.0), 16.0)
    view["min_x"], view["max_x"], view["min_y"], view["max_y"] = -160, 160, -120, 120
    rows, groups = [], []

    def group(name, field, centre, live=True, **base):
        groups.append((name, len(rows), live))
        for v in around(centre):
            rows.append(_point(**dict(base, **{field: v})))

    group("z at 0", "z", 0.0)
    group("u on min_x", "x", -160.0 / B_FX)
    group("u on max_x", "x", 160.0 / B_FX)
    group("v on min_y", "y", -120.0 / B_FX)
    group("v on max_y", "y", 120.0 / B_FX)
    group("dist on 0.8f * min_dist", "z", f32(0.8) * f32(2.0), min_dist=2.0, max_dist=4.0)
    group("dist on 1.2f * max_dist", "z", f32(1.2) * f32(2.0), max_dist=2.0)
    group("view_cos on the limit", "nz", 0.5, z=2.0, max_dist=2.0)
    group("view_cos on 0.998", "nz", f32(0.998), z=2.0, max_dist=2.0)
    group("dist on far_limit", "z", 3.0, max_dist=4.0)
    for n in range(len(sc)):
        group(f"ratio on scale[{n}]", "max_dist", sc[n], live=n < len(sc) - 1)
    singles = [_point(max_dist=0.9), _point(max_dist=0.84), _point(max_dist=5.0), _point(max_dist=np.inf), _point(x=np.nan), _point(y=np.inf),
               _point(x=-np.inf), _point(z=np.inf), _point(z=np.inf, max_dist=np.inf), _point(z=np.nan), _point(nx=np.nan),
               _point(nz=np.inf), _point(min_dist=np.nan), _point(max_dist=np.nan), _point(min_dist=np.inf), _point(z=-1.0)]
    points = np.array(rows + singles, P.MAP_POINT_DTYPE)
    # a handful of train rows: every octave at the principal point, two octaves on each image bound
    x = [0.0] * 8 + [-160.0, -160.0, 160.0, 160.0, 0.0, 0.0, 0.0, 0.0]
    y = [0.0] * 8 + [0.0, 0.0, 0.0, 0.0, -120.0, -120.0, 120.0, 120.0]
    tk = G.kp_rows(x, y, octave=list(range(8)) + [0, 1] * 4)
    rng = np.random.Generator(np.random.PCG64(0xB0DE))
    td = rng.integers(0, 256, (len(tk), 32), dtype=np.uint8)
    pd = rng.integers(0, 256, (len(points), 32), dtype=np.uint8)
    return view, points, groups, tk, td, pd


# ---- the level-aware acceptance test ---------------------------------------------------------------------------------------------
def bits(k: int) -> np.ndarray:
    """a descriptor at Hamming distance k from the all-zero one"""
    d = np.zeros(32, np.uint8)
    for b in range(k):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


R_U, R_V = 160.0, 120.0  # where the point (0, 0, 1) lands: u_right = 160 - 30 = 130
# name: (max_dist -> predicted level, [(octave, distance, right, taken)], expected idx under 8 / 10, check_right on)
RATIO_CASES = {
    # d1 * 10 > d2 * 8 rejects: 8 against 9 (80 > 72) is rejected, 8 against 10 (80 > 80 is false) and 8 against 11 accepted
    "same_level_8_9": (1.3, [(2, 8, -1, 0), (2, 9, -1, 0)], -1),
    "same_level_8_10": (1.3, [(2, 8, -1, 0), (2, 10, -1, 0)], 0),
    "same_level_8_11": (1.3, [(2, 8, -1, 0), (2, 11, -1, 0)], 0),
    "other_level_8_9": (1.3, [(2, 8, -1, 0), (1, 9, -1, 0)], 0),
    "other_level_8_11": (1.3, [(1, 11, -1, 0), (2, 8, -1, 0)], 1),
    "equal_distances": (1.3, [(2, 8, -1, 0), (2, 8, -1, 0)], -1),
    "single": (1.3, [(2, 8, -1, 0), (3, 1, -1, 0), (0, 1, -1, 0)], 0),
    "level_0": (1.0, [(1, 2, -1, 0), (0, 12, -1, 0), (-1, 8, -1, 0)], 2),
    "level_0_single_below": (1.0, [(-1, 8, -1, 0)], 0),
    "taken_row": (1.3, [(2, 8, -1, 1), (2, 30, -1, 0)], 1),
    "right_eye": (1.3, [(2, 8, 100.0, 0), (2, 30, 131.0, 0), (1, 9, 140.0, 0)], 1),
    # level 0, view_cos 1: the radius is 2.5 * 1.0; |130 - 132.5| <= 2.5 holds, the float32 above 132.5 is outside
    "right_eye_on_the_radius": (1.0, [(0, 8, float(np.nextafter(f32(132.5), f32(np.inf))), 0), (0, 30, 132.5, 0)], 1),
}


@functools.lru_cache(maxsize=None)
def ratio_frames():
    """-> (view, list of dicts name points p_desc t_kp t_desc right taken expect)"""
    view = P.view_init(B_FX, B_FX, R_U, R_V, G.W, G.H, np.eye(3), (0.0, 0.0, 0.0), BF)
    frames = []
    for name, (max_dist, rows, expect) in RATIO_CASES.items():
        tk = G.kp_rows([R_U + 0.25 * j for j in range(len(rows))], [R_V] * len(rows), octave=[r[0] for r in rows])
        frames.append({"name": name, "points": np.array([_point(max_dist=max_dist)], P.MAP_POINT_DTYPE), "p_desc": np.zeros((1, 32), np.uint8),
                       "t_kp": tk, "t_desc": np.stack([bits(r[1]) for r in rows]), "right": np.array([r[2] for r in rows], np.float32),
                       "taken": np.array([r[3] for r in rows], np.uint8), "expect": expect})
    return view, frames


RATIO_PARAMS = dict(view_cos_limit=0.5, th=1.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10, one_to_one=False, check_right=True)


# ---- full capacity ---------------------------------------------------------------------------------------------------------------
CAP_ROWS = 16384
CAP_W, CAP_H = 3840, 2160
CAP_F, CAP_CX, CAP_CY = 1000.0, 1920.0, 1080.0
CAP_PARAMS = dict(view_cos_limit=0.5, th=3.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10, one_to_one=True, check_right=True)


@functools.lru_cache(maxsize=None)
def capacity_frames():
    """Two frames of CAP_ROWS points and CAP_ROWS train rows each, dense over 3840 x 2160.  Every point is the back-projection of a
    train row drawn WITH replacement (frame 1: from the upper half only), its descriptor that row's with a few bits flipped: many
    rows are wanted by several points, on both sides of the 8192-row pass of the conflict table."""
    frames = []
    for b in range(2):
        rng = np.random.Generator(np.random.PCG64(0xCA9 + b))
        proto = rng.integers(0, 256, size=(48, 32), dtype=np.uint8)
        tk = G.kp_rows(rng.integers(0, CAP_W * 4, CAP_ROWS).astype(np.float32) / f32(4), rng.integers(0, CAP_H * 4, CAP_ROWS).astype(np.float32) / f32(4),
                       octave=rng.integers(0, 8, CAP_ROWS))
        td = G.near(rng, proto, CAP_ROWS)
        want = rng.integers(8192 if b else 0, CAP_ROWS, CAP_ROWS)
        depth = 2.0 + 6.0 * rng.random(CAP_ROWS)  # of the train rows: their right coordinates and their map points agree on it
        pts, _ = back_project(rng, tk[want], scale(), CAP_F, CAP_F, CAP_CX, CAP_CY, depth[want])
        right = (tk["x"].astype(np.float64) - BF / depth).astype(np.float32)
        right[rng.random(CAP_ROWS) < 0.2] = -1
        taken = (rng.random(CAP_ROWS) < 0.1).astype(np.uint8)
        view = P.view_init(CAP_F, CAP_F, CAP_CX, CAP_CY, CAP_W, CAP_H, POSES[b][0], POSES[b][1], BF)
        frames.append({"view": view, "points": pts, "p_desc": desc_near(rng, td[want], 3), "t_kp": tk, "t_desc": td, "right": right, "taken": taken})
    return frames


@functools.lru_cache(maxsize=None)
def capacity_found(b: int):
    """the projections and the search of capacity frame b, once"""
    f, c = capacity_frames()[b], CAP_PARAMS
    proj = P.eval_points(f["view"], f["points"], c["view_cos_limit"], c["th"], c["far_limit"], scale())
    return proj, P.search(proj, f["p_desc"], f["t_kp"], f["t_desc"], c["check_right"], f["right"], f["taken"])


def capacity_reference(b: int, one_to_one: bool = True):
    """-> (idx, d1, d2, proj, summary, cands)"""
    f, c = capacity_frames()[b], CAP_PARAMS
    proj, found = capacity_found(b)
    idx, d1, d2, summ, cands = P.finish(found, proj, f["t_kp"], c["th_high"], c["ratio_num"], c["ratio_den"], one_to_one)
    return idx, d1, d2, proj, summ, cands
