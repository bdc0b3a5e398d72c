"""The scenes, crafted tables and cached references the map-point fusion tests share (test infrastructure, plain module).  It
reuses what proj_cases has: scenes(), back_project, around, _point, PYRAMIDS, bits.

    boundary_table()    identity pose, exact products: every boundary of step 1 taken with np.nextafter on both sides
    candidate_cases()   one point at a known (u, v, u_right, level) and crafted train rows: every boundary of steps 2 and 3
    outcome_frames()    three points on one row, free and occupied; ids of 0, -1 and INT32_MIN; no ids at all
    scene(), PARAM_SETS the three proj_cases scenes with seeded skip and id masks under upstream's parameters and the Sim3 forms
    count_frames()      point and train counts at 0, 1, 63, 64, 65 and above their row counts, live rows past them
    capacity_frames()   two frames of SS_GUIDED_MAX_ROWS points and train rows, about half of the rows occupied
"""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import fuse_ref as F
import guided_cases as G
import proj_cases as PC
import proj_ref as P

f32 = np.float32
INT32_MIN = -(1 << 31)


# ---- the boundary table of step 1 ---------------------------------------------------------------------------------------------
B_LIMITS = dict(view_cos_limit=0.5, th=3.0)


@functools.lru_cache(maxsize=None)
def boundary_table(sc=None):
    """-> (view, points, skip, groups, train keypoints, t_desc, p_desc).  proj_cases.boundary_table's frame: identity pose,
    fx = 256, principal point 0, image bounds -160 .. 160 x -120 .. 120: with x = y = 0 the distance is z and dot is z * nz, with
    z = 1 the projection is 256 * x and the ratio max_dist, all exactly.  groups: (name, first row, live): three consecutive rows
    below / on / above a boundary."""
    sc = PC.scale() if sc is None else sc
    view = P.view_init(PC.B_FX, PC.B_FX, 0.0, 0.0, 0, 0, np.eye(3), (0.0, 0.0, 0.0), 16.0)
    view["min_x"], view["max_x"], view["min_y"], view["max_y"] = -160, 160, -120, 120
    rows, groups = [], []

    def group(name, field, centre, live=True, **base):
        groups.append((name, len(rows), live))
        for v in PC.around(centre):
            rows.append(PC._point(**dict(base, **{field: v})))

    group("z at 0", "z", 0.0)
    group("u on min_x", "x", -160.0 / PC.B_FX)
    group("u on max_x", "x", 160.0 / PC.B_FX)
    group("v on min_y", "y", -120.0 / PC.B_FX)
    group("v on max_y", "y", 120.0 / PC.B_FX)
    group("dist on 0.8f * min_dist", "z", f32(0.8) * f32(2.0), min_dist=2.0, max_dist=4.0)
    group("dist on 1.2f * max_dist", "z", f32(1.2) * f32(2.0), max_dist=2.0)
    group("dot on view_cos_limit * dist", "nz", 0.5, z=2.0, max_dist=2.0)  # dot = 2 * nz against 0.5 * 2
    for n in range(len(sc)):
        group(f"ratio on scale[{n}]", "max_dist", sc[n], live=n < len(sc) - 1)
    pt = PC._point
    singles = [pt(max_dist=0.9), pt(max_dist=0.84), pt(max_dist=5.0), pt(max_dist=np.inf), pt(x=np.nan), pt(y=np.inf), pt(x=-np.inf), pt(z=np.inf),
               pt(z=np.inf, max_dist=np.inf), pt(z=np.nan), pt(nx=np.nan), pt(nz=np.inf), pt(min_dist=np.nan), pt(max_dist=np.nan),
               pt(min_dist=np.inf), pt(z=-1.0), pt(max_dist=2.0 * float(sc[-1]))]
    n_skipped = 3  # live points behind a skip flag: 1, 255 and, for contrast, 0
    points = np.array(rows + singles + [pt()] * n_skipped, P.MAP_POINT_DTYPE)
    skip = np.zeros(len(points), np.uint8)
    skip[-3], skip[-2] = 1, 255
    octs = list(range(-1, len(sc) + 1))
    x = [0.0] * len(octs) + [-160.0, -160.0, 160.0, 160.0, 0.0, 0.0, 0.0, 0.0]
    y = [0.0] * len(octs) + [0.0, 0.0, 0.0, 0.0, -120.0, -120.0, 120.0, 120.0]
    tk = G.kp_rows(x, y, octave=octs + [0, min(1, len(sc) - 1)] * 4)
    rng = np.random.Generator(np.random.PCG64(0xF05E))
    td = rng.integers(0, 256, (len(tk), 32), dtype=np.uint8)
    pd = rng.integers(0, 256, (len(points), 32), dtype=np.uint8)
    return view, points, skip, tuple(groups), tk, td, pd


def boundary_reference(sc=None):
    sc = PC.scale() if sc is None else sc
    view, points, skip, groups, tk, td, pd = boundary_table(sc)
    return F.match(view, points, pd, tk, td, sc, chi2_mono=0.0, th_low=256, skip=skip, **B_LIMITS)


# ---- the candidate table: steps 2 and 3 -------------------------------------------------------------------------------------
C_U, C_V, C_BF = 160.0, 120.0, 30.0  # where the point (0, 0, 1) lands; u_right = 130
C_BASE = dict(view_cos_limit=0.5, th=3.0, chi2_mono=5.99, chi2_stereo=7.8, th_low=50, check_right=False)


def candidate_view():
    return P.view_init(PC.B_FX, PC.B_FX, C_U, C_V, G.W, G.H, np.eye(3), (0.0, 0.0, 0.0), C_BF)


def _last_accepted(accepts, start, towards):
    """walks float32 steps from `start` (accepted) `towards` a value until the next step is rejected -> the last accepted value"""
    v = f32(start)
    assert accepts(v)
    for _ in range(1 << 20):
        nxt = np.nextafter(v, f32(towards))
        if not accepts(nxt):
            return v
        v = nxt
    raise AssertionError("no boundary found")


@functools.lru_cache(maxsize=None)
def candidate_cases(sc=None):
    """-> list of dicts name params level scale points p_desc t_kp t_desc right taken train_point expect cands: one point at
    u = 160, v = 120, u_right = 130 on level T = min(2, the last level) of the table sc (None: the default one, T = 2, max_dist 1.3,
    radius 3 * 1.44) or on level 0 (max_dist 1.0); its descriptor is all zero, so a row's distance is the number of bits set in it.
    expect: the idx the rule must give; cands: the rows it must count.  Both are asserted on the reference by
    tests/test_fuse_ref.py."""
    sc = PC.scale() if sc is None else sc
    top = min(2, len(sc) - 1)
    top_dist = 1.0 if top == 0 else (1.3 if sc == PC.scale() else (float(sc[top - 1]) + float(sc[top])) / 2)
    u, v, ur = f32(C_U), f32(C_V), f32(C_U - C_BF)
    radius = f32(f32(3.0) * sc[top])
    sigma2 = f32(sc[top] * sc[top])
    cases = []

    def case(name, rows, level=top, expect=None, cands=None, p_desc=None, **params):
        """rows: (x, y, octave, distance or a descriptor, right, taken, id)"""
        tk = G.kp_rows([r[0] for r in rows], [r[1] for r in rows], octave=[r[2] for r in rows])
        td = np.stack([PC.bits(r[3]) if np.isscalar(r[3]) else np.asarray(r[3], np.uint8) for r in rows])
        c = {"name": name, "params": dict(C_BASE, **params), "level": level, "scale": sc,
             "points": np.array([PC._point(max_dist=top_dist if level == top else 1.0)], P.MAP_POINT_DTYPE),
             "p_desc": np.zeros((1, 32), np.uint8) if p_desc is None else p_desc, "t_kp": tk, "t_desc": td,
             "right": np.array([r[4] for r in rows], np.float32), "taken": np.array([r[5] for r in rows], np.uint8),
             "train_point": np.array([r[6] for r in rows], np.int32), "expect": expect, "cands": cands}
        cases.append(c)

    row = lambda x=u, y=v, o=top, d=8, right=-1.0, taken=0, pid=-1: (x, y, o, d, right, taken, pid)  # noqa: E731
    # octaves level - 2 .. level + 1: only max(level - 1, 0) .. level are candidates, whatever the distances say (the default table:
    # rows 1 and 2, of which row 1 is the closer)
    octs, dists = [top - 2, top - 1, top, top + 1], [1, 5, 7, 0]
    inside = [k for k, o in enumerate(octs) if max(top - 1, 0) <= o <= top]
    case("octaves around the level", [row(o=o, d=d) for o, d in zip(octs, dists)], expect=inside[0], cands=inside)
    # level 0: the octaves max(-1, 0) .. 0; the projection search accepts octave -1 there
    case("octave -1 at level 0", [row(o=-1, d=1), row(o=0, d=9), row(o=1, d=0)], level=0, expect=1, cands=[1])
    # |x - u| and |y - v| on the radius, from both sides (no chi-square test: the window binds)
    xs = PC.around(u + radius) + PC.around(u - radius)
    case("x on the radius", [row(x=x, d=3 + k) for k, x in enumerate(xs)], chi2_mono=0.0)
    ys = PC.around(v + radius) + PC.around(v - radius)
    case("y on the radius", [row(y=y, d=3 + k) for k, y in enumerate(ys)], chi2_mono=0.0)
    # e2 on chi2_mono * sigma2: the walk starts a quarter pixel inside the limit, on an offset that float32 holds exactly, and ends
    # on the last x below u whose e2 = (u - x)^2 is accepted (160 - x is exact: both are multiples of 2^-16)
    inside_of = lambda limit: f32(np.floor(np.sqrt(float(limit)) * 4.0) / 4.0)  # noqa: E731
    lim_m = f32(f32(5.99) * sigma2)
    e2_of = lambda x: f32(f32(u - f32(x)) * f32(u - f32(x)))  # noqa: E731
    xm = _last_accepted(lambda x: e2_of(x) <= lim_m, u - inside_of(lim_m), 0.0)
    case("e2 on chi2_mono * sigma2", [row(x=x, d=3 + k) for k, x in enumerate(PC.around(xm))], cands=[1, 2])
    # ... and on chi2_stereo * sigma2: x = u, e2 = (u_right - right)^2
    lim_s = f32(f32(7.8) * sigma2)
    er2 = lambda r: f32(f32(ur - f32(r)) * f32(ur - f32(r)))  # noqa: E731
    rs = _last_accepted(lambda r: er2(r) <= lim_s, ur - inside_of(lim_s), 0.0)
    case("e2 on chi2_stereo * sigma2", [row(right=r, d=3 + k) for k, r in enumerate(PC.around(rs))], cands=[1, 2], check_right=True)
    # a right coordinate of -1 is monocular; -0.0, 0.0 and the float32 above are stereo and 130 px off
    tiny = np.nextafter(f32(0), f32(1))
    case("right of -1, -0.0, 0.0 and just above", [row(right=-0.0, d=1), row(right=0.0, d=2), row(right=tiny, d=3), row(right=-1.0, d=9)], expect=3, cands=[3],
         check_right=True)
    case("right coordinates unread without check_right", [row(right=-0.0, d=1), row(right=0.0, d=2)], expect=0, cands=[0, 1])
    # chi2_mono of 0, negative and NaN switch the test off: a row 0.9 radii away, inside the window, whose e2 of 7.3 sigma2 is above
    # 5.99 sigma2 (the default table: 4 px in a window of 4.32 px)
    away = f32(np.round(0.9 * float(radius) * 4.0) / 4.0)
    off = [row(x=u + away, d=2), row(d=9)]
    case("chi2_mono 5.99 rejects 0.9 radii", off, expect=1, cands=[1])
    for name, c2 in (("0", 0.0), ("negative", -1.0), ("NaN", float("nan"))):
        case(f"chi2_mono {name} is no test", off, expect=0, cands=[0, 1], chi2_mono=c2)
    case("a taken row changes the winner", [row(d=8, taken=1), row(d=30)], expect=1, cands=[1])
    case("d1 on th_low", [row(d=50)], expect=0, cands=[0])
    case("d1 one above th_low", [row(d=50)], expect=-1, cands=[0], th_low=49)
    pd = np.random.Generator(np.random.PCG64(0xD256)).integers(0, 256, (1, 32), dtype=np.uint8)
    far = [row(d=np.bitwise_xor(pd[0], np.uint8(255)))]
    case("a distance of 256 at th_low 256", far, expect=0, cands=[0], p_desc=pd, th_low=256)
    case("a distance of 256 at th_low 255", far, expect=-1, cands=[0], p_desc=pd, th_low=255)
    case("equal distances: the lower row wins", [row(d=20), row(x=u + f32(0.5), d=8), row(x=u - f32(0.5), d=8), row(d=9)], expect=1, cands=[0, 1, 2, 3])
    return cases


def case_reference(c):
    return F.match(candidate_view(), c["points"], c["p_desc"], c["t_kp"], c["t_desc"], c["scale"], right=c["right"], taken=c["taken"],
                   train_point=c["train_point"], **c["params"])


# ---- outcome frames ----------------------------------------------------------------------------------------------------------
def _three_on_one_row(ids):
    """three points at (0, 0, 1) whose descriptors are 9, 8 and 8 bits from the one train row's; ids: train_point, or None"""
    d8b = np.zeros(32, np.uint8)
    d8b[31] = 0xFF
    return {"points": np.array([PC._point(max_dist=1.3)] * 3, P.MAP_POINT_DTYPE), "p_desc": np.stack([PC.bits(9), PC.bits(8), d8b]),
            "t_kp": G.kp_rows([C_U, C_U + 1.0], [C_V, C_V], octave=[2, 5]), "t_desc": np.zeros((2, 32), np.uint8),
            "train_point": None if ids is None else np.array(ids, np.int32)}


# name: (ids of the two train rows or None, the (action, other) of the three points)
OUTCOMES = {
    "free row, distances 9 8 8": ([-1, -1], [(3, 1), (1, -1), (3, 1)]),
    "no ids at all": (None, [(3, 1), (1, -1), (3, 1)]),
    "occupied row": ([77, -1], [(2, 77)] * 3),
    "id 0 is a map point": ([0, -1], [(2, 0)] * 3),
    "INT32_MIN is free": ([INT32_MIN, 5], [(3, 1), (1, -1), (3, 1)]),
}


def outcome_frames():
    return [dict(_three_on_one_row(ids), name=name, expect=expect) for name, (ids, expect) in OUTCOMES.items()]


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def _set(name, **kw):
    return dict(name=name, taken=kw.pop("taken", False), params=dict(F.LOCAL_MAPPING, **kw))


# upstream's local-mapping call with and without the right coordinates; th 1 and 2, where the window and not the chi-square test
# binds; the Sim3 forms (no chi-square test) at th 4 and 8, with and without the taken mask, at th_low 50 and 37
PARAM_SETS = [_set("local_mapping"), _set("local_mapping_right", check_right=True), _set("th1", th=1.0), _set("th2", th=2.0)] + \
             [_set(f"sim3_th{int(th)}_taken{int(tk)}_low{low}", th=th, chi2_mono=0.0, chi2_stereo=0.0, th_low=low, taken=tk)
              for th in (4.0, 8.0) for tk in (False, True) for low in (50, 37)]
SET_NAMES = [s["name"] for s in PARAM_SETS]


@functools.lru_cache(maxsize=None)
def scenes(cams=None):
    """proj_cases.scenes(cams) with a seeded 10 % skip mask over the points and ids on a seeded 40 % of the train rows"""
    out = []
    for k, s in enumerate(PC.scenes(cams)):
        rng = np.random.Generator(np.random.PCG64(0xF5E0 + k))
        skip = (rng.random(len(s["points"])) < 0.1).astype(np.uint8)
        nt = len(s["t_kp"])
        ids = np.where(rng.random(nt) < 0.4, 1000 + np.arange(nt), -1).astype(np.int32)
        out.append(dict(s, skip=skip, train_point=ids))
    return out


# ---- odd cameras: the three scenes, one camera each (CC.FRAME_CAMERAS) ------------------------------------------------------------------
# Fuse as local mapping calls it, with the right coordinates (each frame's bf reaches u_right and the stereo chi-square test), and the
# Sim3 projection search of the candidate check under views made from Scw = [s.R | s.t]
CAMERA_SETS = {"fuse": dict(F.LOCAL_MAPPING, check_right=True), "sim3_search": dict(F.CANDIDATE_CHECK)}
SIM3_SCALE = 1.25


def camera_scenes():
    return scenes(CC.FRAME_CAMERAS)


def scw(k: int):
    """the Sim3 of scene k's pose at the scale SIM3_SCALE: (s.R, s.t)"""
    r, t = PC.POSES[k]
    return SIM3_SCALE * np.asarray(r, np.float64), SIM3_SCALE * np.asarray(t, np.float64)


def camera_view(k: int, which: str, cam):
    """the view of scene k under a camera: the plain one, or the one ss_fuse_view_sim3 makes from scw(k)"""
    if which == "fuse":
        return PC.camera_view(k, cam)
    return F.view_sim3(*cam[:4], G.W, G.H, *scw(k), cam[4])


def library_view(binding, k: int, which: str):
    """the same view from the library's own view makers: ss_proj_view_init for Fuse; for the Sim3 search ss_fuse_view_sim3 on scw(k),
    and for the last scene ss_sim3_to_view on a Sim3 result of the scale alone (s12 = SIM3_SCALE, R12 = I, t12 = 0) and the scene's pose"""
    fx, fy, cx, cy, bf = CC.FRAME_CAMERAS[k]
    cam = binding.Camera(fx=fx, fy=fy, cx=cx, cy=cy, width=G.W, height=G.H)
    if which == "fuse":
        return binding.proj_view(cam, *PC.POSES[k], bf)
    if k < 2:
        return binding.fuse_view_sim3(cam, *scw(k), bf)
    res = np.zeros((), binding.SIM3_RESULT_DTYPE)
    res["sr12"], res["s12"] = (SIM3_SCALE * np.eye(3)).reshape(9), SIM3_SCALE
    res["sr21"], res["iteration"] = (np.eye(3) / SIM3_SCALE).reshape(9), 0
    return binding.sim3_to_view(cam, res, *PC.POSES[k], bf)[0]


def camera_skip(k: int, shared: bool):
    """the skip flags of frame k over its own block, or over block 0: the flags are the frame's, not the block's"""
    s = camera_scenes()
    skip = np.zeros(len(s[0 if shared else k]["points"]), np.uint8)
    m = min(len(skip), len(s[k]["skip"]))
    skip[:m] = s[k]["skip"][:m]
    return skip


@functools.lru_cache(maxsize=None)
def camera_reference(k: int, which: str, shared: bool, cam=None):
    """frame k of the camera scenes on its own block of points, or on block 0 (point_src [0, 0, 0]), under CAMERA_SETS[which]; cam:
    the camera a confused kernel would see frame k through (None: its own)"""
    s = camera_scenes()
    b = s[0] if shared else s[k]
    view = camera_view(k, which, CC.FRAME_CAMERAS[k] if cam is None else cam)
    return F.match(view, b["points"], b["p_desc"], s[k]["t_kp"], s[k]["t_desc"], PC.scale(), skip=camera_skip(k, shared), right=s[k]["right"],
                   taken=s[k]["taken"], train_point=s[k]["train_point"], **CAMERA_SETS[which])


@functools.lru_cache(maxsize=None)
def scene_points(k: int, th: float):
    s = scenes()[k]
    return F.eval_points(s["view"], s["points"], s["skip"], 0.5, th, PC.scale())


@functools.lru_cache(maxsize=None)
def scene_found(k: int, th: float, chi2_mono: float, chi2_stereo: float, check_right: bool, taken: bool):
    s = scenes()[k]
    return F.search(scene_points(k, th), s["p_desc"], s["t_kp"], s["t_desc"], PC.scale(), chi2_mono, chi2_stereo, check_right, s["right"],
                    s["taken"] if taken else None)


def scene_reference(k: int, pset):
    """-> (idx, d1, actions, points, summary, found) of scene k under a PARAM_SETS entry; the search is computed once per distinct
    (th, chi-square, right, taken)"""
    s, p = scenes()[k], pset["params"]
    pts = scene_points(k, p["th"])
    found = scene_found(k, p["th"], p["chi2_mono"], p["chi2_stereo"], p["check_right"], pset["taken"])
    idx, d1, act, summ = F.finish(found, pts, len(s["t_kp"]), p["th_low"], s["train_point"])
    return idx, d1, act, pts, summ, found


def set_params(binding, pset, **kw):
    return binding.fuse_params(**dict(pset["params"], **kw))


EXTENT_SETS = [PARAM_SETS[1], PARAM_SETS[-1]]

# ---- counts -------------------------------------------------------------------------------------------------------------------
COUNT_ROWS = PC.COUNT_ROWS
COUNTS = PC.COUNTS
COUNT_SET = dict(name="counts", taken=True, params=dict(F.LOCAL_MAPPING, th=4.0, chi2_mono=0.0, check_right=True))


def count_frames():
    """-> (scene 0 cut to COUNT_ROWS points and train rows, COUNTS): every frame of the call holds ALL the rows, live, whatever its
    counts say"""
    s = scenes()[0]
    n = COUNT_ROWS
    return {k: (v[:n] if k != "view" else v) for k, v in s.items()}, COUNTS


@functools.lru_cache(maxsize=None)
def count_reference(n_points: int, n_train: int):
    f, _ = count_frames()
    k, nt = min(max(n_points, 0), COUNT_ROWS), min(max(n_train, 0), COUNT_ROWS)
    return F.match(f["view"], f["points"][:k], f["p_desc"][:k], f["t_kp"][:nt], f["t_desc"][:nt], PC.scale(), skip=f["skip"][:k], right=f["right"][:nt],
                   taken=f["taken"][:nt], train_point=f["train_point"][:nt], **COUNT_SET["params"])


# ---- full capacity ------------------------------------------------------------------------------------------------------------
CAP_ROWS = PC.CAP_ROWS
CAP_PARAMS = dict(F.LOCAL_MAPPING, check_right=True)


@functools.lru_cache(maxsize=None)
def capacity_frames():
    """proj_cases.capacity_frames(): every point is the back-projection of a train row drawn WITH replacement (frame 1: from the
    upper half only), so free rows are contested on both sides of row 8192; about half of the rows carry an id, one point in ten is
    skipped"""
    out = []
    for b, f in enumerate(PC.capacity_frames()):
        rng = np.random.Generator(np.random.PCG64(0xFCA9 + b))
        ids = np.where(rng.random(CAP_ROWS) < 0.5, rng.integers(0, 1 << 30, CAP_ROWS), -1).astype(np.int32)
        out.append(dict(f, skip=(rng.random(CAP_ROWS) < 0.1).astype(np.uint8), train_point=ids))
    return out


@functools.lru_cache(maxsize=None)
def capacity_reference(b: int):
    f = capacity_frames()[b]
    return F.match(f["view"], f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), skip=f["skip"], right=f["right"], taken=f["taken"],
                   train_point=f["train_point"], **CAP_PARAMS)


# ---- end to end: epipolar search -> triangulation -> fusion into a third keyframe -----------------------------------------------------
END_TO_END = dict(F.LOCAL_MAPPING)
END_TO_END_COMBO = dict(coarse=False, one_to_one=True, orientation=1, taken=True)


@functools.lru_cache(maxsize=None)
def end_to_end_thirds():
    """the third keyframe of every epi_cases scene: the world points behind the scene's query keypoints seen from a third pose; its
    row i carries a map point (id 5000 + i) iff the first two keyframes matched query row i.  epi_cases keeps no depths, so the world
    points come from its own second_view() on the scene's seed, and the replay is checked: it must give back the scene's train
    keypoints (all but the few rows the scene moved onto the epipole afterwards)"""
    import epi_cases as EC
    out = []
    for k, s in enumerate(EC.scenes()):
        k2, xw = EC.second_view(np.random.Generator(np.random.PCG64(0xE91 + k)), s["q_kp"], *s["poses"])
        back = s["t_kp"][s["truth"]]
        same = sum(k2[i].tobytes() == back[i].tobytes() for i in range(len(k2)))
        assert same >= len(k2) - 8, f"scene {k}: second_view() on the scene's seed gives back {same} of {len(k2)} train keypoints"
        rng = np.random.Generator(np.random.PCG64(0xF3D + k))
        r3, t3 = EC.pose((k + 2) % 3)
        pc = xw @ np.asarray(r3).T + np.asarray(t3)
        k3 = s["q_kp"].copy()
        k3["x"] = EC.CAM[0] * pc[:, 0] / pc[:, 2] + EC.CAM[2] + rng.normal(0, 0.3, len(k3))
        k3["y"] = EC.CAM[1] * pc[:, 1] / pc[:, 2] + EC.CAM[3] + rng.normal(0, 0.3, len(k3))
        matched = EC.scene_reference(k, END_TO_END_COMBO)[0] >= 0
        out.append({"view": P.view_init(*EC.CAM, G.W, G.H, r3, t3, PC.BF), "points": np.zeros(0, P.MAP_POINT_DTYPE), "p_desc": np.zeros((0, 32), np.uint8),
                    "t_kp": k3, "t_desc": PC.desc_near(rng, s["q_desc"]),
                    "train_point": np.where(matched, 5000 + np.arange(len(k3)), -1).astype(np.int32)})
    return out


@functools.lru_cache(maxsize=None)
def end_to_end_reference(k: int):
    """-> (epi_ref's triangulation of scene k's matches, fuse_ref.match of its block into the third keyframe)"""
    import epi_cases as EC
    import epi_ref as E
    s, third = EC.scenes()[k], end_to_end_thirds()[k]
    tri = E.triangulate_rows(s["pair"], EC.TRI, EC.scale(), s["q_kp"], s["q_desc"], s["t_kp"], EC.scene_reference(k, END_TO_END_COMBO)[0])
    return tri, F.match(third["view"], tri[1], tri[2], third["t_kp"], third["t_desc"], EC.scale(), train_point=third["train_point"], **END_TO_END)
