"""The scenes, crafted tables and cached references the projection-search tests share (test infrastructure, plain module).

    scenes()           map points = a frame's oracle keypoints back-projected at varied depths, seen under a pose a few pixels away
                       from identity, searched in a train frame of guided_cases (320 x 240, 500 features)
    boundary_table()   identity pose, exact products: every boundary of steps 1 - 3 taken with np.nextafter on both sides; over any
                       pyramid table (PYRAMIDS)
    edge_table()       projections on and next to the image bounds, windows that reach beyond it, train rows in the border cells
    count_frames()     point and train counts at 0, 1, 63, 64, 65 and above their row counts, live rows past them
    ratio_frames()     the level-aware acceptance test, a taken row and a right-eye rejection that change the winner
    capacity_frames()  two frames of SS_GUIDED_MAX_ROWS points and train rows
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import camera_cases as CC
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
def scenes(cams=None):
    """-> list of dicts view points p_desc t_kp t_desc right taken, one per SCENES entry.  cams: one camera (fx, fy, cx, cy, bf)
    per scene (a tuple of tuples; None: the square camera for all): the points are back-projected and seen under it, the right
    coordinates made with its bf"""
    out = []
    for k, (src, train) in enumerate(SCENES):
        rng = np.random.Generator(np.random.PCG64(0x9E0 + k))
        kp, desc = G.features(src)
        tk, td = G.features(train)
        fx, fy, cx, cy, bf = (FX, FY, CX, CY, BF) if cams is None else cams[k]
        pts, z = back_project(rng, kp, scale(), fx, fy, cx, cy)
        view = P.view_init(fx, fy, cx, cy, G.W, G.H, POSES[k][0], POSES[k][1], bf)
        # right coordinates: a stereo match at the row's depth (the map point's depth where both frames are the same, else a random
        # one), -1 for a monocular row, a wrong one for some; taken: one row in five
        depth = np.resize(np.abs(z), len(tk))
        right = (tk["x"].astype(np.float64) - bf / depth + rng.normal(0, 0.5, len(tk))).astype(np.float32)
        kind = rng.random(len(tk))
        right = np.where(kind < 0.15, f32(-1), np.where(kind < 0.30, right - f32(40), right)).astype(np.float32)
        taken = (rng.random(len(tk)) < 0.2).astype(np.uint8)
        out.append({"view": view, "points": pts, "p_desc": desc_near(rng, desc), "t_kp": tk, "t_desc": td, "right": right, "taken": taken})
    return out


# ---- odd cameras: the three scenes, one camera each (CC.FRAME_CAMERAS) ------------------------------------------------------------------
CAMERA_COMBO = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=True, taken=True)  # check_right: each frame's bf reaches u_right


def camera_scenes():
    return scenes(CC.FRAME_CAMERAS)


def camera_view(k: int, cam):
    """the view of scene k under another camera"""
    return P.view_init(*cam[:4], G.W, G.H, POSES[k][0], POSES[k][1], cam[4])


@functools.lru_cache(maxsize=None)
def camera_reference(k: int, shared: bool, cam=None):
    """frame k of the camera scenes on its own block of points, or on block 0 (point_src [0, 0, 0]); cam: the camera a confused
    kernel would see frame k through (None: its own)"""
    s, c = camera_scenes(), CAMERA_COMBO
    b = s[0] if shared else s[k]
    view = s[k]["view"] if cam is None else camera_view(k, cam)
    return P.match(view, b["points"], b["p_desc"], s[k]["t_kp"], s[k]["t_desc"], scale(), th=c["th"], ratio_num=c["ratio"][0], ratio_den=c["ratio"][1],
                   one_to_one=c["one_to_one"], check_right=c["check_right"], right=s[k]["right"], taken=s[k]["taken"])


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


# the pyramid tables a context can hold besides the default: name -> (scale_factor, n_levels).  ss_create accepts all of them
# (its geometry check on a nominal 640 x 480 image refuses invalid parameters only)
PYRAMIDS = {"one_level": (1.2, 1), "two_levels": (1.2, 2), "factor_2": (2.0, 4), "sixteen_levels": (1.1, 16)}


def scale_table(scale_factor: float, n_levels: int):
    """the context's table as include/sendslam_orb.h states it: scale[0] = 1, scale[i] = (float)(scale[i - 1] * (double)factor)"""
    sc = [f32(1)]
    for _ in range(1, n_levels):
        sc.append(f32(float(sc[-1]) * float(f32(scale_factor))))
    return tuple(sc)


@functools.lru_cache(maxsize=None)
def boundary_table(sc=None):
    """-> (view, points, groups, train keypoints).  Identity pose, principal point 0, image bounds -160 .. 160 x -120 .. 120: with
    x = y = 0 the distance is z and the cosine nz, with z = 1 the projection is 256 * x and the ratio max_dist, all exactly.
    groups: (name, first row, live): three consecutive rows below / on / above a boundary; live False = a boundary the rule makes
    moot (ratio on the last table entry: both sides give the last level).  sc: the pyramid table (None: the default one)."""
    sc = scale() if sc is None else sc
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
               _point(nz=np.inf), _point(min_dist=np.nan), _point(max_dist=np.nan), _point(min_dist=np.inf), _point(z=-1.0),
               _point(max_dist=2.0 * float(sc[-1]))]  # ratios below scale[0] = 1 and above the last entry, whatever the table
    points = np.array(rows + singles, P.MAP_POINT_DTYPE)
    # a handful of train rows: every octave (and one below / above the table) at the principal point, two octaves on each image bound
    octs = list(range(-1, len(sc) + 1))
    x = [0.0] * len(octs) + [-160.0, -160.0, 160.0, 160.0, 0.0, 0.0, 0.0, 0.0]
    y = [0.0] * len(octs) + [0.0, 0.0, 0.0, 0.0, -120.0, -120.0, 120.0, 120.0]
    tk = G.kp_rows(x, y, octave=octs + [0, min(1, len(sc) - 1)] * 4)
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


# ---- other grids --------------------------------------------------------------------------------------------------------------
# the index follows the extent, the answer does not: 256 px cells; 4096 x 1 cells beyond 2^24; a 2 x 2 grid; 157 x 2 cells; one cell;
# an extent smaller than the keypoints' spread (train rows outside it share the border cells)
EXTENTS = list(G.CAP_EXTENTS) + [(5000, 37), (1, 1), (100, 80)]
EXTENT_COMBOS = [dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=True, taken=True), dict(ratio=(0, 0), one_to_one=False, th=1.0, check_right=False, taken=False)]


# ---- windows at the image's edge and beyond -----------------------------------------------------------------------------------
E_W, E_H = 320, 240
E_THS = (1.0, 20.0, 300.0, 1e30)  # radii of 4 .. 14 px, 80 .. 290 px, beyond the image on all sides, and as large as th can make them


@functools.lru_cache(maxsize=None)
def edge_table():
    """-> (view, points, p_desc, train keypoints, t_desc).  Identity pose, fx = fy = 256, principal point (160, 120), z = 1: the
    projection is 256 * x + 160 exactly.  Points on each image bound and in each corner, one float32 step of x / y inside and
    outside it (of x / y at the lower bounds, of u / v at the upper ones), at levels 0, 3 and 7; train rows in the first and the last cell of rows and columns, on pixel 0, on the last pixel
    (319, 239), on the bound (320, 240) and outside the extent on every side, at every octave."""
    view = P.view_init(B_FX, B_FX, E_W / 2, E_H / 2, E_W, E_H, np.eye(3), (0.0, 0.0, 0.0), BF)
    sc = scale()
    # the lower bounds: the float32 steps of x around -160 / 256 (u = -2^-16, 0, 2^-16); the upper bounds: the x that lands on the
    # float32 steps of u around 320 (a step of x there is half a step of u, and would round onto the bound)
    xs = around(-160.0 / B_FX) + [f32((float(u) - E_W / 2) / B_FX) for u in around(E_W)] + [f32(0)]
    ys = around(-120.0 / B_FX) + [f32((float(v) - E_H / 2) / B_FX) for v in around(E_H)] + [f32(0)]
    rows = []
    for x in xs:
        for y in ys:
            dist = float(np.sqrt(np.float64(x) ** 2 + np.float64(y) ** 2 + 1.0))
            for level in (0, 3, 7):
                rows.append(_point(x=x, y=y, max_dist=dist * float(sc[level]) * 0.97, min_dist=0.1))
    points = np.array(rows, P.MAP_POINT_DTYPE)
    rng = np.random.Generator(np.random.PCG64(0xED6E))
    ex = [0.0, 31.0, 32.0, 319.0, 319.0, 0.0, 320.0, 320.0, 319.5, 5.0, 315.0, 160.0, 160.0, 288.0, 0.0, -3.0, 330.0, 160.0, 160.0, 1000.0]
    ey = [0.0, 0.0, 0.0, 0.0, 239.0, 239.0, 240.0, 120.0, 239.5, 120.0, 120.0, 3.0, 236.0, 224.0, 208.0, 120.0, 120.0, -2.0, 250.0, 1000.0]
    n_rand = 140
    tk = G.kp_rows(np.concatenate([np.repeat(ex, 2), rng.integers(-40, (E_W + 40) * 4, n_rand) / 4.0]).astype(np.float32),
                   np.concatenate([np.repeat(ey, 2), rng.integers(-40, (E_H + 40) * 4, n_rand) / 4.0]).astype(np.float32),
                   octave=np.concatenate([np.tile([0, 3], len(ex)), rng.integers(-1, 9, n_rand)]))
    td = rng.integers(0, 256, (len(tk), 32), dtype=np.uint8)
    pd = rng.integers(0, 256, (len(points), 32), dtype=np.uint8)
    return view, points, pd, tk, td


E_PARAMS = dict(view_cos_limit=0.5, far_limit=0.0, th_high=256, ratio_num=0, ratio_den=0, one_to_one=False, check_right=False)


@functools.lru_cache(maxsize=None)
def edge_reference(th: float):
    view, points, pd, tk, td = edge_table()
    return P.match(view, points, pd, tk, td, scale(), **dict(E_PARAMS, th=th))


# ---- a distance of 256 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_descriptor_frame():
    """one point whose only candidate holds the complement of its descriptor"""
    view = P.view_init(B_FX, B_FX, R_U, R_V, G.W, G.H, np.eye(3), (0.0, 0.0, 0.0), BF)
    pd = np.random.Generator(np.random.PCG64(0xD256)).integers(0, 256, (1, 32), dtype=np.uint8)
    return {"view": view, "points": np.array([_point(max_dist=1.3)], P.MAP_POINT_DTYPE), "p_desc": pd, "t_kp": G.kp_rows([R_U + 0.5], [R_V - 0.25], octave=2),
            "t_desc": np.bitwise_xor(pd, np.uint8(255))}


# ---- counts -------------------------------------------------------------------------------------------------------------------
COUNT_ROWS = 65  # point_rows and rows_per_frame: one past the 64 points of a workgroup
COUNTS = [(0, 65), (1, 65), (63, 65), (64, 65), (65, 65), (65, 0), (65, 1), (65, 63), (65, 64), (0, 0), (1, 1), (70, 65), (65, 1000), (-3, 65), (65, -1),
          (1 << 30, 1 << 30)]


def count_frames():
    """-> (scene 0 cut to COUNT_ROWS points and train rows, COUNTS): every frame of the call holds ALL the rows, live, whatever its
    counts say"""
    s = scenes()[0]
    n = COUNT_ROWS
    return {"view": s["view"], "points": s["points"][:n], "p_desc": s["p_desc"][:n], "t_kp": s["t_kp"][:n], "t_desc": s["t_desc"][:n],
            "right": s["right"][:n], "taken": s["taken"][:n]}, COUNTS


COUNT_PARAMS = dict(view_cos_limit=0.5, th=3.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10, one_to_one=True, check_right=True)


@functools.lru_cache(maxsize=None)
def count_reference(n_points: int, n_train: int):
    f, _ = count_frames()
    k, nt = min(max(n_points, 0), COUNT_ROWS), min(max(n_train, 0), COUNT_ROWS)
    return P.match(f["view"], f["points"][:k], f["p_desc"][:k], f["t_kp"][:nt], f["t_desc"][:nt], scale(), right=f["right"][:nt], taken=f["taken"][:nt],
                   **COUNT_PARAMS)
