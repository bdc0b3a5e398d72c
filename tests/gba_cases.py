"""The scenes and shared cases of the global bundle adjustment tests (test infrastructure, plain module): the scenes of
tests/ba_cases.py (float32 map points seen from a row of keyframes, pixel noise by octave, planted gross outliers, starts a degree and
a few centimetres off) with their dense observation table turned into records, and a fixed byte per keyframe in the place of "the
first n_free"."""
from __future__ import annotations

import functools

import numpy as np

import ba_cases as BC
import camera_cases as CC
import gba_ref as GR
import proj_cases as PC

f32 = np.float32


def make_problem(seed: int, n_kf: int, n_free: int, n_points: int, fixed=None, shuffle: int = 0, **kw):
    """BC.make_problem's scene as a global problem -> a dict: views, start [n_kf][12], fixed uint8 [n_kf] (None: the keyframes from
    n_free on, which start at the truth), points, obs (GR.OBS_DTYPE records in ascending (point, kf) order, or shuffled by the seed
    `shuffle`), skip, truth, planted (bool per record), dense (the problem of BC.make_problem, for ss_local_ba_*)"""
    pr = BC.make_problem(seed=seed, n_kf=n_kf, n_free=n_free, n_points=n_points, **kw)
    obs = GR.obs_from_idx(pr["kp"], pr["idx"], pr["n_kp"], pr["right"])
    planted = pr["planted"][obs["kf"], obs["point"]] if len(obs) else np.zeros(0, bool)
    if shuffle:
        order = np.random.Generator(np.random.PCG64(shuffle)).permutation(len(obs))
        obs, planted = obs[order], planted[order]
    fx = (np.arange(n_kf) >= n_free).astype(np.uint8) if fixed is None else np.asarray(fixed, np.uint8)
    return {"views": pr["views"], "start": pr["start"], "fixed": fx, "points": pr["points"], "obs": obs, "skip": pr["skip"], "truth": pr["truth"],
            "planted": planted, "dense": pr}


SHORT = dict(n_rounds=2, iterations=(3, 2, 0, 0), pcg_iterations=16)


def _case(name, problem_kw, **params):
    return {"name": name, "problem": problem_kw, "params": dict(GR.DEFAULTS, **params)}


# tests/test_gba_ref.py asserts what the cases are there for.  noise_free runs the default schedule (upstream's: one robust round
# of ten), the others a short one
CASES = [
    _case("noise_free", dict(seed=11, n_kf=6, n_free=4, n_points=150, noise=0.0, point_noise=0.02), step_eps=1e-7),
    _case("noisy_outliers", dict(seed=12, n_kf=8, n_free=6, n_points=300, n_out=40), **SHORT),
    _case("stereo_mixed", dict(seed=13, n_kf=6, n_free=4, n_points=257, n_out=30, stereo_every=2, cams=CC.FRAME_CAMERAS), check_right=True, **SHORT),
    _case("two_fixed_disagree", dict(seed=14, n_kf=6, n_free=4, n_points=160, n_out=16), **SHORT),
    _case("no_fixed", dict(seed=15, n_kf=5, n_free=5, n_points=140, n_out=12), **SHORT),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_problem(k: int):
    pr = make_problem(**CASES[k]["problem"])
    if CASES[k]["name"] == "two_fixed_disagree":  # the last keyframe is fixed two degrees and 10 cm away from where the other fixed one wants it
        start = pr["start"].copy()
        R = PC.rot(0.02, -0.03, 0.01) @ start[5][:9].reshape(3, 3)
        start[5] = np.concatenate([R.reshape(-1), start[5][9:] + np.array([0.1, 0.0, -0.05])])
        pr = dict(pr, start=start)
    return pr


def solve(pr, params, trace=None, scale=None):
    """gba_ref on one problem dict"""
    return GR.optimise(pr["views"], pr["start"], pr["fixed"], PC.scale() if scale is None else scale, pr["points"], pr["obs"], dict(GR.DEFAULTS, **params),
                       pr.get("skip"), trace)


@functools.lru_cache(maxsize=None)
def reference(k: int):
    """(poses, xyz, point flags, observation flags, result, trace) of case k"""
    trace = []
    return solve(case_problem(k), CASES[k]["params"], trace=trace) + (trace,)


# ---- the ladders: one schedule, short ---------------------------------------------------------------------------------------------
LADDER = dict(n_rounds=2, iterations=(2, 1, 0, 0), pcg_iterations=8, check_right=True)
KF_LADDER = (2, 3, 42, 43, 44, 257)        # free keyframes; 6 n_kf crosses the 256 slots of a dot product between 42 and 43
POINT_LADDER = (0, 1, 2, 255, 256, 257, 513)
LIST_LADDER = (1, 255, 256, 257, 513)      # the length of every keyframe's list


@functools.lru_cache(maxsize=None)
def kf_ladder_problem(n_free: int):
    """n_free free keyframes and one fixed; with many keyframes every point is seen by a few of them"""
    n_kf = n_free + 1
    return make_problem(seed=1000 + n_free, n_kf=n_kf, n_free=n_free, n_points=60 if n_free < 100 else 300, p_obs=0.9 if n_kf <= 8 else 4.0 / n_kf, n_out=4 if n_free > 2 else 0,
                        stereo_every=3, shuffle=7)


@functools.lru_cache(maxsize=None)
def point_ladder_problem(n_points: int):
    return make_problem(seed=1100 + n_points, n_kf=4, n_free=3, n_points=n_points, rows=max(n_points, 3) + 5, n_out=min(n_points // 16, 8), shuffle=8)


@functools.lru_cache(maxsize=None)
def list_ladder_problem(length: int):
    """three keyframes that each see every point: every keyframe's list has `length` items"""
    return make_problem(seed=1200 + length, n_kf=3, n_free=2, n_points=length, p_obs=1.0, min_obs=3, n_out=min(length // 32, 6), stereo_every=2, shuffle=9)


@functools.lru_cache(maxsize=None)
def seen_by_problem():
    """66 keyframes, 65 free, every point drawn in every keyframe, then records dropped: point 0 keeps one (inactive), point 1 two,
    point 2 sixty-five; the others keep three spread over the row and one in twelve of the rest"""
    pr = make_problem(seed=1300, n_kf=66, n_free=65, n_points=120, p_obs=1.0)
    obs = pr["obs"]
    k, i = obs["kf"].astype(np.int64), obs["point"].astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(1301))
    keep = (rng.uniform(0, 1, len(obs)) < 1.0 / 12) | (k == i % 66) | (k == (i + 1) % 66) | (k == (7 * i + 5) % 66)
    keep = np.where(i == 0, k == 0, np.where(i == 1, k < 2, np.where(i == 2, k < 65, keep)))
    obs = obs[keep]
    return dict(pr, obs=obs, planted=np.zeros(len(obs), bool))


@functools.lru_cache(maxsize=None)
def beyond_local_problem():
    """65 keyframes, 33 free: one more of each than ss_local_ba_host takes"""
    return make_problem(seed=1400, n_kf=65, n_free=33, n_points=200, p_obs=0.1, n_out=6)


@functools.lru_cache(maxsize=None)
def lonely_problem():
    """keyframe 0 is free and has no record; keyframe 1 is free and sees only points nobody else sees (inactive ones)"""
    pr = make_problem(seed=1500, n_kf=6, n_free=4, n_points=90, p_obs=0.8, n_out=4)
    obs = pr["obs"]
    keep = (obs["kf"] != 0) & ~((obs["kf"] == 1) & (obs["point"] >= 10))
    obs = obs[keep]
    obs = obs[~((obs["kf"] != 1) & (obs["point"] < 10))]
    return dict(pr, obs=obs, planted=np.zeros(len(obs), bool))
