"""The scenes and shared cases of the pose-only optimisation tests (test infrastructure, plain module): float32-representable map
points seen from a known pose, keypoints with pixel noise by octave, planted gross outliers and borderline observations, a start pose
a few degrees and centimetres off, in both idx directions and with right coordinates."""
from __future__ import annotations

import functools

import numpy as np

import guided_cases as G
import pose_ref as PR
import proj_cases as PC
import proj_ref as P

f32 = np.float32
W, H = 320, 240
R_TRUE = PC.rot(0.05, -0.03, 0.02)
T_TRUE = np.array([0.1, -0.05, 0.2])
START_OFF = (PC.rot(0.02, -0.015, 0.01), np.array([0.05, -0.03, 0.04]))


def view(bf: float = PC.BF) -> np.ndarray:
    """the camera of the scenes; the view's own pose is not read by the optimisation"""
    return P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, W, H, np.eye(3), np.zeros(3), bf)


def start_of(R, t) -> np.ndarray:
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def points_of(xyz) -> np.ndarray:
    p = np.zeros(len(xyz), P.MAP_POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["nz"], p["min_dist"], p["max_dist"] = 1.0, 0.1, 100.0
    return p


def project(xyz, R=R_TRUE, t=T_TRUE, bf: float = PC.BF):
    """double projections (u, v, ur) of float32 points under (R, t)"""
    pc = np.asarray(xyz, np.float64) @ np.asarray(R).T + np.asarray(t)
    u = PC.FX * pc[:, 0] / pc[:, 2] + PC.CX
    v = PC.FY * pc[:, 1] / pc[:, 2] + PC.CY
    return u, v, u - bf / pc[:, 2]


def make_frame(seed: int, n: int, n_out: int = 0, n_border: int = 0, stereo_every: int = 0, by_row: bool = False, n_points: int | None = None,
               n_kp: int | None = None, noise: float = 0.6, start_off=START_OFF):
    """n observations among n_points map points and n_kp keypoint rows (both default n), the rows of either side permuted; the first
    n_out observations are gross outliers, the next n_border lie near the chi-square threshold; every stereo_every-th keypoint row has
    a right coordinate.  -> a dict: view, start, points, kp, idx, right, truth and the observations' slots (obs_slots) in observation
    order, the gross outliers first"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_points, n_kp = n_points or n, n_kp or n
    sc = np.asarray(PC.scale(), f32)
    cam = np.empty((n_points, 3))
    cam[:, 2] = rng.uniform(2.0, 8.0, n_points)
    cam[:, 0] = rng.uniform(-0.45, 0.45, n_points) * cam[:, 2]
    cam[:, 1] = rng.uniform(-0.33, 0.33, n_points) * cam[:, 2]
    xyz = ((cam - T_TRUE) @ R_TRUE).astype(f32)  # world = R^T (pc - t), then float32
    prow = rng.permutation(n_points)[:n]
    krow = rng.permutation(n_kp)[:n]
    u, v, ur = project(xyz[prow])
    octave = rng.integers(0, len(sc), n)
    s = sc[octave].astype(np.float64)
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
    return {"view": view(), "start": start_of(start_off[0] @ R_TRUE, start_off[0] @ T_TRUE + start_off[1]), "points": points_of(xyz), "kp": kp,
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
