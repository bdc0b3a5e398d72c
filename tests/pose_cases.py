"""The scenes and shared cases of the pose-only optimisation tests (test infrastructure, plain module): float32-representable map
points seen from a known pose, keypoints with pixel noise by octave, planted gross outliers and borderline observations, a start pose
a few degrees and centimetres off, in both idx directions and with right coordinates."""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import guided_cases as G
import pose_ref as PR
import proj_cases as PC
import proj_ref as P

f32 = np.float32
W, H = 320, 240
R_TRUE = PC.rot(0.05, -0.03, 0.02)
T_TRUE = np.array([0.1, -0.05, 0.2])
START_OFF = (PC.rot(0.02, -0.015, 0.01), np.array([0.05, -0.03, 0.04]))


CAM = (PC.FX, PC.FY, PC.CX, PC.CY, PC.BF)


def view(bf: float | None = None, cam=None) -> np.ndarray:
    """the camera of the scenes: cam = (fx, fy, cx, cy, bf), None: the square camera; bf, where given, replaces the camera's.  The
    view's own pose is not read by the optimisation"""
    fx, fy, cx, cy, cbf = CAM if cam is None else cam
    return P.view_init(fx, fy, cx, cy, W, H, np.eye(3), np.zeros(3), cbf if bf is None else bf)


def start_of(R, t) -> np.ndarray:
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def points_of(xyz) -> np.ndarray:
    p = np.zeros(len(xyz), P.MAP_POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["nz"], p["min_dist"], p["max_dist"] = 1.0, 0.1, 100.0
    return p


def project(xyz, R=R_TRUE, t=T_TRUE, bf: float | None = None, cam=None):
    """double projections (u, v, ur) of float32 points under (R, t) by the camera cam (None: the square one)"""
    fx, fy, cx, cy, cbf = CAM if cam is None else cam
    pc = np.asarray(xyz, np.float64) @ np.asarray(R).T + np.asarray(t)
    u = fx * pc[:, 0] / pc[:, 2] + cx
    v = fy * pc[:, 1] / pc[:, 2] + cy
    return u, v, u - (cbf if bf is None else bf) / pc[:, 2]


def make_frame(seed: int, n: int, n_out: int = 0, n_border: int = 0, stereo_every: int = 0, by_row: bool = False, n_points: int | None = None,
               n_kp: int | None = None, noise: float = 0.6, start_off=START_OFF, cam=None, octaves=None):
    """n observations among n_points map points and n_kp keypoint rows (both default n), the rows of either side permuted; the first
    n_out observations are gross outliers, the next n_border lie near the chi-square threshold; every stereo_every-th keypoint row has
    a right coordinate.  cam: the camera that sees the scene, (fx, fy, cx, cy, bf) (None: the square one); octaves: the octaves the
    keypoints are drawn from (None: those of the default pyramid table; an octave outside it has that table's last scale as its
    noise).  -> a dict: view, start, points, kp, idx, right, truth and the observations' slots (obs_slots) in observation
    order, the gross outliers first"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_points, n_kp = n_points or n, n_kp or n
    sc = np.asarray(PC.scale(), f32)
    pc = np.empty((n_points, 3))
    pc[:, 2] = rng.uniform(2.0, 8.0, n_points)
    pc[:, 0] = rng.uniform(-0.45, 0.45, n_points) * pc[:, 2]
    pc[:, 1] = rng.uniform(-0.33, 0.33, n_points) * pc[:, 2]
    xyz = ((pc - T_TRUE) @ R_TRUE).astype(f32)  # world = R^T (pc - t), then float32
    prow = rng.permutation(n_points)[:n]
    krow = rng.permutation(n_kp)[:n]
    u, v, ur = project(xyz[prow], cam=cam)
    octave = rng.integers(0, len(sc), n) if octaves is None else rng.choice(octaves, n)
    s = sc[np.clip(octave, 0, len(sc) - 1)].astype(np.float64)
    du, dv, dr = (rng.normal(0.0, noise, n) * s for _ in range(3))
    border = slice(n_out, n_out + n_border)
    ang = rng.uniform(0, 2 * np.pi, n_border)
    mag = np.sqrt(rng.uniform(5.0, 7.0, n_border)) * s[border]
    du[border], dv[border], dr[border] = mag * np.cos(ang), mag * np.sin(ang), 0.0
    u, v, ur = u + du, v + dv, ur + dr
    u[:n_out], v[:n_out] = rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)
    kp = G.kp_rows(rng.uniform(0, W, n_kp).astype(f32), rng.uniform(0, H, n_kp).astype(f32), rng.integers(0, len(sc), n_kp))
    kp["x"][krow], kp["y"][krow], kp["octave"][krow] = u.astype(f32), v.astype(f32), octave
    right = np.full(n_kp, -1.0, f32)
    if stereo_every:
        has = krow % stereo_every == 0
        right[krow[has]] = ur[has].astype(f32)
    if by_row:
        idx = np.full(n_kp, -1, np.int32)
        idx[krow] = prow
        slots = krow
    else:
        idx = np.full(n_points, -1, np.int32)
        idx[prow] = krow
        slots = prow
    return {"view": view(cam=cam), "start": start_of(start_off[0] @ R_TRUE, start_off[0] @ T_TRUE + start_off[1]), "points": points_of(xyz), "kp": kp,
            "idx": idx, "right": right, "skip": None, "truth": (R_TRUE, T_TRUE), "obs_slots": slots, "n_out": n_out, "by_row": by_row}


def _case(name, frame_kw, early=True, **params):
    return {"name": name, "frame": frame_kw, "early": early, "params": dict(PR.UPSTREAM, **params)}


# every case removes its gross outliers in round 0 and re-admits an observation later; all but "every_step" end a round early
CASES = [
    _case("mono_300", dict(seed=1, n=300, n_out=40, n_border=40)),
    _case("stereo_mixed_257", dict(seed=2, n=257, n_out=30, n_border=40, stereo_every=2), check_right=True),
    _case("by_row_513", dict(seed=3, n=513, n_out=60, n_border=60, by_row=True, n_points=600, n_kp=700), idx_by_row=True),
    _case("by_row_stereo_129", dict(seed=4, n=129, n_out=20, n_border=30, by_row=True, stereo_every=3, n_points=140), idx_by_row=True, check_right=True),
    _case("every_step", dict(seed=5, n=65, n_out=8, n_border=20), early=False, step_eps=0.0),
    _case("three_robust_rounds_of_five", dict(seed=6, n=200, n_out=30, n_border=40, n_points=256), n_rounds=5, iterations=5, robust_rounds=3),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_frame(k: int):
    return make_frame(**CASES[k]["frame"])


def solve_frame(fr, params, status: int = 0, trace=None, scale=None):
    """pose_ref on one frame dict"""
    p = dict(PR.UPSTREAM, **params)
    return PR.optimise(fr["view"], fr["start"], PC.scale() if scale is None else scale, fr["points"], fr["kp"], fr["idx"], p, fr.get("skip"),
                       fr.get("right"), status, trace)


@functools.lru_cache(maxsize=None)
def reference(k: int):
    """(result, flags, the inlier mask after every round) of case k"""
    trace = []
    res, flags = solve_frame(case_frame(k), CASES[k]["params"], trace=trace)
    return res, flags, trace


@functools.lru_cache(maxsize=None)
def failure_frames():
    """name -> (frame, the state it ends in): observations on and behind the camera plane, starts that are turned away, sheared, far
    off or not finite, NaN coordinates of a keypoint and of a point"""
    base = make_frame(80, 120, n_out=10, n_border=20)
    behind_some = dict(base, points=base["points"].copy())
    rows = base["obs_slots"][10:30]
    pc = -np.abs(np.stack([behind_some["points"][n][rows].astype(np.float64) for n in "xyz"], 1) @ R_TRUE.T + T_TRUE)  # z < 0 under the truth
    back = ((pc - T_TRUE) @ R_TRUE).astype(np.float32)
    behind_some["points"]["x"][rows], behind_some["points"]["y"][rows], behind_some["points"]["z"][rows] = back[:, 0], back[:, 1], back[:, 2]
    on_plane = base["obs_slots"][30]
    behind_some["points"]["x"][on_plane], behind_some["points"]["y"][on_plane], behind_some["points"]["z"][on_plane] = ((np.zeros(3) - T_TRUE) @ R_TRUE).astype(np.float32)
    turned = PC.rot(0.0, np.pi, 0.0)  # looking the other way: every point behind the camera
    behind_all = dict(base, start=start_of(turned @ R_TRUE, turned @ T_TRUE))
    nan = dict(base, kp=base["kp"].copy())
    nan["kp"]["y"][base["idx"][base["obs_slots"][50]]] = np.nan  # the residual is NaN, and so is every sum
    nan_point = dict(base, points=base["points"].copy())
    nan_point["points"]["y"][base["obs_slots"][50]] = np.nan  # z is NaN: not > 0, the observation takes no part
    shear = np.eye(3) + 1e-3 * np.array([[0.0, 1.0, -0.5], [0.3, 0.2, 0.7], [-0.4, 0.1, 0.0]])
    sheared = dict(base, start=start_of((START_OFF[0] @ R_TRUE) @ shear, base["start"][9:]))
    far = dict(base, start=start_of(PC.rot(0.0, 0.0, 3.0) @ R_TRUE, T_TRUE))  # rolled by 172 degrees: the third step is above pi
    nan_start = dict(base, start=np.where(np.arange(12) == 4, np.nan, base["start"]))
    zero_row = dict(base, start=np.where(np.arange(12) < 3, 0.0, base["start"]))
    inf_t = dict(base, start=np.where(np.arange(12) == 10, np.inf, base["start"]))
    return {"z <= 0 for some": (behind_some, 0), "every point behind": (behind_all, 3), "a NaN coordinate": (nan, 2), "a sheared start": (sheared, 0),
            "a step above pi": (far, 4), "a NaN start": (nan_start, 2), "a start row of zeros": (zero_row, 2), "an infinite start": (inf_t, 2), "a NaN point": (nan_point, 0)}


# ---- odd cameras: three frames per call under CC.FRAME_CAMERAS ---------------------------------------------------------------------------
# kind -> (make_frame keywords, parameters, one seed per frame).  The seeds are the first at which the reference removes the gross
# outliers in round 0, re-admits an observation later and ends a round early (tests/test_pose_ref.py asserts it)
CAMERA_KINDS = {
    "monocular": (dict(), dict(), (7, 8, 9)),
    "every_third_row_stereo": (dict(stereo_every=3), dict(check_right=True), (20, 23, 24)),
    "by_keypoint_row": (dict(by_row=True, stereo_every=3), dict(idx_by_row=True, check_right=True), (43, 44, 48)),
}
CAMERA_FRAME = dict(n=130, n_out=15, n_border=20, n_points=150, n_kp=140)


def camera_params(kind: str):
    return dict(PR.UPSTREAM, **CAMERA_KINDS[kind][1])


@functools.lru_cache(maxsize=None)
def camera_frames(kind: str, cams=CC.FRAME_CAMERAS):
    """one frame per camera of cams, each its own scene seen by that camera"""
    kw, _, seeds = CAMERA_KINDS[kind]
    return [make_frame(seed, cam=cam, **CAMERA_FRAME, **kw) for seed, cam in zip(seeds, cams)]


@functools.lru_cache(maxsize=None)
def camera_reference(kind: str):
    """[(result, flags, the inlier mask after every round)] of camera_frames(kind)"""
    out = []
    for fr in camera_frames(kind):
        trace = []
        res, flags = solve_frame(fr, camera_params(kind), trace=trace)
        out.append((res, flags, trace))
    return out


@functools.lru_cache(maxsize=None)
def no_baseline_frame():
    """a frame with right coordinates on every third row whose view has bf = 0: the right coordinate of a point is its left one"""
    return make_frame(25, cam=CC.A[:4] + (0.0,), stereo_every=3, **CAMERA_FRAME)


# ---- parameter limits, a singular system, other pyramid tables ----------------------------------------------------------------------------
LIMIT_FRAME = dict(seed=5, n=65, n_out=8, n_border=20)  # the frame of "every_step"
# name: (parameters, the states the frame may end in)
LIMITS = {
    "eight rounds of 32 steps": (dict(n_rounds=8, iterations=32, step_eps=0.0), (0,)),
    "no robust round": (dict(robust_rounds=0), (0,)),
    "eight robust rounds": (dict(n_rounds=8, robust_rounds=8), (0,)),
    "lambda 0": (dict(lambda_=0.0), (0,)),
    "min_obs at n_obs": (dict(min_obs=65), (0, 3)),
    "min_obs above n_obs": (dict(min_obs=66), (1,)),
}


@functools.lru_cache(maxsize=None)
def singular_frame():
    """every keypoint row is matched to ONE map point, which lies on the optical axis of the start pose: the three Jacobian rows of
    every observation are the same and none has an entry in column 2, so H22 is a sum of zeros and, under lambda = 0, the third pivot
    of the Cholesky factorisation is 0 - 0 - 0: not > 0, with every sum finite"""
    n = 40
    rng = np.random.Generator(np.random.PCG64(0x51A6))
    R, t = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.25, -0.125, 0.5])  # a quarter turn: exact
    xyz = np.array([[0.125, 0.25, 3.5]], f32)  # (0, 0, 4) in the camera of the start pose, exactly
    kp = G.kp_rows((CC.A[2] + rng.normal(0, 1.0, n)).astype(f32), (CC.A[3] + rng.normal(0, 1.0, n)).astype(f32), rng.integers(0, 8, n))
    return {"view": view(cam=CC.A), "start": start_of(R, t), "points": points_of(xyz), "kp": kp, "idx": np.zeros(n, np.int32), "right": None, "skip": None}


SINGULAR_PARAMS = dict(PR.UPSTREAM, lambda_=0.0, idx_by_row=True)


def pyramid_frame(n_levels: int):
    """keypoints on octaves 0, 1, n_levels - 1 and n_levels: the last is outside a table of n_levels entries (and, in a table of one
    level, octave 1 is too)"""
    return make_frame(300 + n_levels, 120, n_out=12, n_border=20, n_points=140, n_kp=130, cam=CC.B, octaves=(0, 1, n_levels - 1, n_levels))
