"""The scenes and shared cases of the local bundle adjustment tests (test infrastructure, plain module): float32 map points seen from a
row of keyframes with known poses, keypoints with pixel noise by octave, planted gross outliers, free keyframes that start a degree and
a few centimetres off, points that start a few centimetres off, right coordinates on some rows."""
from __future__ import annotations

import functools

import numpy as np

import ba_ref as BR
import camera_cases as CC
import guided_cases as G
import pose_cases as PO
import proj_cases as PC

f32 = np.float32
W, H = 320, 240
DEG = np.pi / 180.0


def true_pose(k: int):
    """keyframe k of the row: a step sideways and a small turn each"""
    return PC.rot(0.01 * ((k * 7) % 5 - 2), 0.012 * ((k * 3) % 7 - 3), 0.008 * ((k * 5) % 3 - 1)), np.array([-0.3 * k, 0.05 * ((k * 2) % 5 - 2), 0.04 * (k % 4)])


def make_problem(seed: int, n_kf: int, n_free: int, n_points: int, p_obs: float = 0.7, n_out: int = 0, stereo_every: int = 0, noise: float = 0.5,
                 point_noise: float = 0.03, pose_off=(1.0 * DEG, 0.05), cams=None, rows: int | None = None, skip_every: int = 0, min_obs: int = 2, scale=None,
                 octave_edits: int = 0):
    """n_points map points, each seen by a keyframe with probability p_obs (and by min_obs at the least); the first n_out observations
    drawn, of points that three keyframes see, are gross outliers; every stereo_every-th keypoint row has a right coordinate; every skip_every-th point row carries a skip
    byte.  cams: one (fx, fy, cx, cy, bf) per keyframe (None: the square camera).  The free keyframes (the first n_free) start pose_off
    = (angle, distance) away from the truth, the fixed ones at it.  -> a dict: views, start [n_kf][12], n_free, points, kp [n_kf][rows],
    idx [n_kf][n_points], right [n_kf][rows], skip, n_kp, truth (poses [n_kf][12], xyz [n_points][3] in double), planted (bool
    [n_kf][n_points]: the gross outliers).  scale: the pyramid table the octaves and the noise are drawn against (None: the default
    one, PC.scale()).  octave_edits: after everything is drawn, that many observations (spread over the keyframes, none a planted
    outlier) get the octaves -1, n_levels and n_levels - 1 in turn -> edited: a list of (keyframe, point row, octave)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = rows or max(n_points, 1)
    sc = np.asarray(PC.scale() if scale is None else scale, f32)
    cams = [CC.SQUARE] * n_kf if cams is None else [cams[k % len(cams)] for k in range(n_kf)]
    xyz = np.empty((n_points, 3))
    xyz[:, 2] = rng.uniform(4.0, 10.0, n_points)
    xyz[:, 0] = rng.uniform(-0.35, 0.35, n_points) * xyz[:, 2] + 0.15 * n_kf
    xyz[:, 1] = rng.uniform(-0.3, 0.3, n_points) * xyz[:, 2]
    seen = rng.uniform(0, 1, (n_kf, n_points)) < p_obs
    for i in range(n_points):  # every point in min_obs keyframes at the least
        while seen[:, i].sum() < min(min_obs, n_kf):
            seen[rng.integers(0, n_kf), i] = True
    kp = np.zeros((n_kf, rows), G.kp_rows([0.0], [0.0]).dtype)
    right = np.full((n_kf, rows), -1.0, f32)
    idx = np.full((n_kf, n_points), -1, np.int32)
    planted = np.zeros((n_kf, n_points), bool)
    truth, start, views = np.empty((n_kf, 12)), np.empty((n_kf, 12)), []
    left = n_out
    for k in range(n_kf):
        R, t = true_pose(k)
        truth[k] = PO.start_of(R, t)
        if k < n_free:
            axis = rng.normal(0, 1, 3)
            axis *= pose_off[0] / np.linalg.norm(axis)
            shift = rng.normal(0, 1, 3)
            shift *= pose_off[1] / np.linalg.norm(shift)
            dR = PC.rot(*axis)
            start[k] = PO.start_of(dR @ R, dR @ t + shift)
        else:
            start[k] = truth[k]
        views.append(PO.view(cam=cams[k]))
        kp[k] = G.kp_rows(rng.uniform(0, W, rows).astype(f32), rng.uniform(0, H, rows).astype(f32), rng.integers(0, len(sc), rows))
        pts = np.flatnonzero(seen[k])
        pts = pts[np.argsort(seen[:, pts].sum(axis=0) < 3, kind="stable")]  # those in three keyframes or more first: an outlier there can be told
        krow = rng.permutation(rows)[:len(pts)]
        u, v, ur = PO.project(xyz[pts].astype(f32), R, t, cam=cams[k])
        octave = rng.integers(0, len(sc), len(pts))
        s = sc[octave].astype(np.float64)
        u, v, ur = u + rng.normal(0, noise, len(pts)) * s, v + rng.normal(0, noise, len(pts)) * s, ur + rng.normal(0, noise, len(pts)) * s
        bad = min(left, int((seen[:, pts].sum(axis=0) >= 3).sum()) // 8)
        left -= bad
        u[:bad], v[:bad] = u[:bad] + rng.choice([-1, 1], bad) * rng.uniform(25, 60, bad), v[:bad] + rng.choice([-1, 1], bad) * rng.uniform(25, 60, bad)
        planted[k, pts[:bad]] = True
        kp["x"][k, krow], kp["y"][k, krow], kp["octave"][k, krow] = u.astype(f32), v.astype(f32), octave
        if stereo_every:
            has = krow % stereo_every == 0
            right[k, krow[has]] = ur[has].astype(f32)
        idx[k, pts] = krow
    assert left == 0, "too few observations to plant the outliers in"
    moved = (xyz.astype(f32).astype(np.float64) + rng.normal(0, point_noise, (n_points, 3))).astype(f32)
    skip = None
    if skip_every:
        skip = (np.arange(n_points) % skip_every == 1).astype(np.uint8)
    edited = []
    if octave_edits:
        where = np.argwhere((idx >= 0) & ~planted)
        for j, (k, i) in enumerate(where[np.linspace(0, len(where) - 1, octave_edits).astype(int)]):
            edited.append((int(k), int(i), (-1, len(sc), len(sc) - 1)[j % 3]))
            kp["octave"][k, idx[k, i]] = edited[-1][2]
    pr = {"views": np.array(views), "start": start, "n_free": n_free, "points": PO.points_of(moved), "kp": kp, "idx": idx, "right": right if stereo_every else None,
          "skip": skip, "n_kp": np.full(n_kf, rows, np.int32), "truth": (truth, xyz.astype(f32).astype(np.float64)), "planted": planted}
    if octave_edits:
        pr["edited"] = edited
    return pr


def _case(name, problem_kw, **params):
    return {"name": name, "problem": problem_kw, "params": dict(BR.DEFAULTS, **params)}


# Every case with planted gross outliers removes them in round 0; tests/test_ba_ref.py asserts what else the cases are there for
CASES = [
    _case("mono_8kf_300", dict(seed=1, n_kf=8, n_free=4, n_points=300, n_out=40)),
    _case("stereo_mixed_6kf_257", dict(seed=2, n_kf=6, n_free=3, n_points=257, n_out=30, stereo_every=2, cams=CC.FRAME_CAMERAS), check_right=True),
    _case("far_start", dict(seed=3, n_kf=5, n_free=3, n_points=120, n_out=12, pose_off=(3.0 * DEG, 0.2), point_noise=0.1)),
    _case("one_round_of_ten", dict(seed=4, n_kf=4, n_free=2, n_points=200, n_out=20, skip_every=7), n_rounds=1, iterations=(10, 0, 0, 0)),
    _case("noise_free", dict(seed=5, n_kf=6, n_free=3, n_points=150, noise=0.0, point_noise=0.02), step_eps=1e-6),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_problem(k: int):
    return make_problem(**CASES[k]["problem"])


def solve(pr, params, status: int = 0, trace=None, scale=None):
    """ba_ref on one problem dict"""
    return BR.optimise(pr["views"], pr["start"], pr["n_free"], PC.scale() if scale is None else scale, pr["points"], pr["kp"], pr["idx"],
                       dict(BR.DEFAULTS, **params), pr["n_kp"], pr.get("skip"), pr.get("right"), status, trace)


@functools.lru_cache(maxsize=None)
def reference(k: int):
    """(poses, xyz, point flags, observation flags, result, trace) of case k"""
    trace = []
    return solve(case_problem(k), CASES[k]["params"], trace=trace) + (trace,)


@functools.lru_cache(maxsize=None)
def frozen_problem():
    """three keyframes, the first free; point 0 is seen by the fixed keyframes 1 and 2 only, which stand on one line with it, so
    that both rays coincide: V has rank 2, and under lambda 0 its third pivot is not > 0.  The other points are ordinary"""
    pr = make_problem(seed=6, n_kf=3, n_free=1, n_points=40, p_obs=1.0, noise=0.0, point_noise=0.0, pose_off=(0.2 * DEG, 0.01))
    pr = dict(pr, start=pr["start"].copy(), points=pr["points"].copy(), kp=pr["kp"].copy(), idx=pr["idx"].copy())
    eye = PO.start_of(np.eye(3), np.zeros(3))
    pr["start"][1], pr["start"][2] = eye, PO.start_of(np.eye(3), np.array([0.0, 0.0, -1.0]))  # both look along z; the second stands 1 ahead
    pr["points"]["x"][0], pr["points"]["y"][0], pr["points"]["z"][0] = 0.0, 0.0, 4.0  # on the common optical axis
    pr["idx"][0, 0] = -1
    for k in (1, 2):
        row = pr["idx"][k, 0]
        pr["kp"]["x"][k, row], pr["kp"]["y"][k, row], pr["kp"]["octave"][k, row] = CC.SQUARE[2], CC.SQUARE[3], 0
    for k in (1, 2):  # the other points' keypoints under the new poses, exactly
        R, t = pr["start"][k][:9].reshape(3, 3), pr["start"][k][9:]
        xyz = np.stack([pr["points"][n].astype(np.float64) for n in "xyz"], 1)
        u, v, _ = PO.project(xyz.astype(f32), R, t, cam=CC.SQUARE)
        rows = pr["idx"][k, 1:]
        pr["kp"]["x"][k, rows], pr["kp"]["y"][k, rows] = u[1:].astype(f32), v[1:].astype(f32)
    return pr


FROZEN_PARAMS = dict(BR.DEFAULTS, lambda_=0.0, lambda_min=0.0)


# ---- rotated camera rows, other pyramid tables, row counts, a free keyframe nobody sees -------------------------------------------------
CAMERA_PARAMS = dict(BR.DEFAULTS, n_rounds=2, iterations=(2, 1, 0, 0), check_right=True)


@functools.lru_cache(maxsize=None)
def camera_problems():
    """three problems of four keyframes for one call: keyframe k of problem q has camera (k + q) % 3 of camera_cases.FRAME_CAMERAS, so
    with first frames 0, 4 and 8 no two problems share a camera row, and views[k] for views[first_frame + k] gives problems 1 and 2
    other cameras"""
    return [make_problem(seed=800 + q, n_kf=4, n_free=2, n_points=60, n_out=6, stereo_every=2, cams=[CC.FRAME_CAMERAS[(k + q) % 3] for k in range(4)])
            for q in range(3)]


def with_cameras(problems, cams):
    """the problems of a call under the cameras `cams`, one per frame of the call (a mix-up's: what a wrong kernel would read)"""
    out, f0 = [], 0
    for pr in problems:
        n_kf = len(pr["views"])
        out.append(dict(pr, views=np.array([PO.view(cam=c) for c in cams[f0:f0 + n_kf]])))
        f0 += n_kf
    return out


def call_cameras(problems):
    """(fx, fy, cx, cy, bf) of every frame of a call"""
    return [tuple(float(v[n]) for n in ("fx", "fy", "cx", "cy", "bf")) for pr in problems for v in pr["views"]]


PYRAMID_NAMES = ("one_level", "factor_2", "sixteen_levels")
PYRAMID_PARAMS = dict(BR.DEFAULTS, n_rounds=2, iterations=(2, 1, 0, 0))


@functools.lru_cache(maxsize=None)
def pyramid_problem(name: str):
    """-> (problem, table): octaves and noise drawn against PC.PYRAMIDS[name]; nine observations carry the octaves -1, n_levels and
    n_levels - 1, three each (pr["edited"])"""
    table = PC.scale_table(*PC.PYRAMIDS[name])
    return make_problem(seed=820 + PYRAMID_NAMES.index(name), n_kf=4, n_free=2, n_points=80, n_out=6, scale=table, octave_edits=9), table


ROW_COUNTS = (100, 91, 0, 64, 100)
ROW_COUNT_PARAMS = dict(BR.DEFAULTS, n_rounds=2, iterations=(2, 1, 0, 0))


@functools.lru_cache(maxsize=None)
def row_count_problem():
    """five keyframes of 100 keypoint rows, told ROW_COUNTS: keyframe 2 (fixed) has none, keyframes 1 and 3 lose the observations whose
    keypoint row lies at or past their count.  Four points that keep two good observations besides carry junk in one more keyframe's
    idx: n_kp[k], n_kp[k] + 5, 1 << 30 and -7 (pr["junk"]: a list of (keyframe, point row, entry))"""
    pr = make_problem(seed=840, n_kf=5, n_free=2, n_points=90, n_out=6, rows=100)
    pr = dict(pr, idx=pr["idx"].copy(), n_kp=np.array(ROW_COUNTS, np.int32))
    good = (pr["idx"] >= 0) & (pr["idx"] < pr["n_kp"][:, None])
    junk = []
    for i in np.flatnonzero(good.sum(axis=0) >= 3):
        k = (1, 3, 0, 4)[len(junk)]
        if good[k, i]:
            junk.append((k, int(i), (int(pr["n_kp"][k]), int(pr["n_kp"][k]) + 5, 1 << 30, -7)[len(junk)]))
            pr["idx"][k, i] = junk[-1][2]
            if len(junk) == 4:
                break
    assert len(junk) == 4
    pr["junk"] = junk
    return pr


def without_junk(pr):
    """the row-count problem with -1 where the rule sees no observation: an entry at or past n_kp[k], or below -1"""
    idx = np.where((pr["idx"] >= 0) & (pr["idx"] < np.clip(pr["n_kp"], 0, pr["kp"].shape[1])[:, None]), pr["idx"], -1).astype(np.int32)
    return dict(pr, idx=idx)


@functools.lru_cache(maxsize=None)
def unobserved_free_problem():
    """camera_problems()[0] with no observation in keyframe 0, which is free: its diagonal block is lambda alone"""
    pr = camera_problems()[0]
    idx = pr["idx"].copy()
    idx[0] = -1
    return dict(pr, idx=idx)


UNOBSERVED_PARAMS = (dict(CAMERA_PARAMS), dict(CAMERA_PARAMS, lambda_=0.0, lambda_min=0.0))
