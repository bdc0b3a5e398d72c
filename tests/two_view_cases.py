"""The synthetic scenes and the case table the two-view initialisation tests share (test infrastructure, plain module).

    make_scene()    points in front of camera 1 (a general cloud, an oblique plane, or degenerate sets), seen by camera 2 under a planted
                    motion X2 = R.X1 + t; keypoints on both projections rounded to float32 (plus Gaussian noise on request); gross
                    outliers on request: their second keypoint sits anywhere in the image; the correspondences scattered over the rows
                    of frame 1, the rows of frame 2 permuted
    CASES           the states and reasons of the rule (tests/test_two_view_ref.py asserts on the host twin that each is what its name
                    says)
    host()          ss_two_view_host of a scene, cached per case
    restatement()   two_view_ref.solve of a case as problem number `problem` of a call, cached
"""
from __future__ import annotations

import functools

import numpy as np

import guided_cases as G
import proj_cases as PC
import proj_ref as P
import two_view_ref as R

f32 = np.float32
FX, FY, CX, CY, W, H = 500.0, 510.0, 318.0, 243.0, 640, 480
CAM = (FX, FY, CX, CY)
MOTION = (PC.rot(0.02, -0.05, 0.01), (0.5, 0.05, 0.1))  # about 4 degrees of parallax at the scenes' depth
ROWS = 400  # rows of the pairs form the cases run through


def view(cam=CAM):
    """the view of the camera; the rule reads fx fy cx cy only"""
    return P.view_init(*cam, W, H, np.eye(3), (0.0, 0.0, 0.0), 0.0)


def project(xc, cam=CAM):
    xc = np.asarray(xc, np.float64)
    return np.stack([cam[0] * xc[:, 0] / xc[:, 2] + cam[2], cam[1] * xc[:, 1] / xc[:, 2] + cam[3]], axis=1)


def unit(t):
    t = np.asarray(t, np.float64)
    return t / np.linalg.norm(t)


def camera_points(rng, n, shape="general"):
    z = rng.uniform(4.0, 8.0, n)
    xc = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], axis=1)
    if shape == "planar":  # a plane oblique to the optical axis
        xc[:, 2] = 6.0 + 0.3 * xc[:, 0] - 0.2 * xc[:, 1]
    elif shape == "same_point":
        xc[:] = xc[0]
    elif shape == "collinear":
        s = rng.uniform(-1.0, 1.0, n)
        xc = np.array([0.2, -0.1, 6.0]) + s[:, None] * np.array([1.0, 0.5, 0.8])
    return xc


def make_scene(rng_seed: int, n: int, n_out: int = 0, n1: int | None = None, n2: int | None = None, noise: float = 0.0, shape: str = "general",
               cam=CAM, motion=MOTION, octaves=(0, 1, 2, 3), scatter: bool = True):
    """n correspondences of which n_out are gross outliers, over n1 rows of frame 1 and n2 rows of frame 2 -> dict view kp1 kp2 idx
    (int32 [n1]) rows (the rows of frame 1 that carry a correspondence, ascending) inlier_rows motion"""
    rng = np.random.Generator(np.random.PCG64(0x7E0000 + rng_seed))
    n1 = n if n1 is None else n1
    n2 = n if n2 is None else n2
    assert n1 >= n and n2 >= n
    x1 = camera_points(rng, n, shape)
    x2 = x1 @ np.asarray(motion[0]).T + np.asarray(motion[1])
    uv1, uv2 = project(x1, cam), project(x2, cam)
    if noise:
        uv1, uv2 = uv1 + rng.normal(0.0, noise, (n, 2)), uv2 + rng.normal(0.0, noise, (n, 2))
    out = np.zeros(n, bool)
    if n_out:
        out[rng.choice(n, n_out, replace=False)] = True
        uv2[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], axis=1)
    rows = np.sort(rng.choice(n1, n, replace=False)) if scatter else np.arange(n)
    cols = rng.permutation(n2)[:n] if scatter else np.arange(n)
    kp1 = G.kp_rows(rng.uniform(0, W, n1).astype(f32), rng.uniform(0, H, n1).astype(f32), octave=rng.choice(octaves, n1))
    kp2 = G.kp_rows(rng.uniform(0, W, n2).astype(f32), rng.uniform(0, H, n2).astype(f32), octave=rng.choice(octaves, n2))
    kp1["x"][rows], kp1["y"][rows] = uv1[:, 0], uv1[:, 1]
    kp2["x"][cols], kp2["y"][cols] = uv2[:, 0], uv2[:, 1]
    idx = np.full(n1, -1, np.int32)
    idx[rows] = cols
    return dict(view=view(cam), kp1=kp1, kp2=kp2, idx=idx, rows=rows, inlier_rows=rows[~out], motion=motion, xyz=x1, out=out)


def _case(name, expect, scene_kw, **params):
    """expect: (state, reason, model)"""
    p = dict(max_iterations=48, seed=0)
    p.update(params)
    return dict(name=name, expect=expect, scene_kw=scene_kw, params=p)


FORWARD = (PC.rot(0.02, -0.05, 0.01), (0.6, 0.1, 0.9))
WIDE = (PC.rot(0.03, -0.12, 0.02), (1.2, 0.1, 0.2))
PLANAR_MOTION = (PC.rot(0.05, -0.2, 0.03), (1.5, 0.1, 0.2))  # wide enough that the second Faugeras solution loses its points: found on the CPU
SMALL_T = (PC.rot(0.02, -0.05, 0.01), (0.08, 0.008, 0.016))
PURE_ROTATION = (PC.rot(0.02, -0.05, 0.01), (0.0, 0.0, 0.0))
PLANE = dict(n=200, n1=256, n2=256, shape="planar")
EXACT = dict(rng_seed=3, n=120, n1=128, n2=130)
# expect = (state, reason, model); None: whatever the rule gives (the degenerate sets), held bit for bit only
CASES = [
    _case("state 0, F: 300 correspondences of a cloud, 90 gross outliers, 0.5 px noise", (0, 0, 1),
          dict(rng_seed=24, n=300, n_out=90, n1=380, n2=400, noise=0.5, motion=FORWARD), seed=24, max_iterations=200),
    _case("state 0, H: 200 exact correspondences of a plane", (0, 0, 2), dict(rng_seed=2, motion=PLANAR_MOTION, **PLANE), seed=2),
    _case("state 0, H: a plane, 40 gross outliers, 0.3 px noise", (0, 0, 2), dict(rng_seed=2, n_out=40, noise=0.3, motion=PLANAR_MOTION, **PLANE), seed=2, max_iterations=100),
    _case("state 0, F: 120 exact correspondences", (0, 0, 1), dict(**EXACT), seed=3, max_iterations=12),
    _case("state 3, low parallax: a cloud under a translation of 8 cm", (3, 4, 1), dict(rng_seed=4, n=200, n1=256, n2=256, motion=SMALL_T), seed=4),
    _case("state 3, singular values: pure rotation", (3, 1, 2), dict(rng_seed=4, n=200, n1=256, n2=256, motion=PURE_ROTATION), seed=4),
    _case("state 3, ambiguous: a plane under a narrow baseline", (3, 3, 2), dict(rng_seed=2, **PLANE), seed=2),
    _case("state 3, too few good points: min_triangulated above the inliers", (3, 2, 1), dict(**EXACT), seed=3, max_iterations=12, min_triangulated=121),
    _case("state 1: 7 correspondences", (1, 0, 0), dict(rng_seed=5, n=7, n1=12, n2=9)),
    _case("smallest: 8 exact correspondences, min_triangulated 0", (0, 0, 1), dict(rng_seed=6, n=8, n1=9, n2=8), min_triangulated=0, max_iterations=4),
    _case("all matches are gross outliers", (3, 2, None), dict(rng_seed=7, n=100, n_out=100, n1=128, n2=128), seed=7),
    _case("state 2: every correspondence is one point", (2, 0, 0), dict(rng_seed=8, n=40, n1=64, n2=64, shape="same_point"), max_iterations=8),
    _case("collinear points", (None, None, None), dict(rng_seed=9, n=60, n1=64, n2=64, shape="collinear"), max_iterations=16),
    _case("rh_threshold 0.5 hands the plane to F", (None, None, 1), dict(rng_seed=2, motion=PLANAR_MOTION, **PLANE), seed=2, rh_threshold=0.5),
]
# four scenes of 300 correspondences, 30 % gross outliers, 0.5 px noise for which the rule flags at least 90 % of the planted inliers:
# (motion, scene and draw seed), found on the CPU.  A minimal-set F under that noise often decomposes into a motion whose triangulated
# points miss the 2 px reprojection bound, so many seeds end in state 3, as upstream's initialiser does; the cap stays, the seeds move
RECOVERY = [(WIDE, 15), (WIDE, 41), (FORWARD, 15), (FORWARD, 24)]


def recovery_scene(k: int):
    motion, seed = RECOVERY[k]
    return make_scene(seed, 300, 90, 380, 400, noise=0.5, motion=motion), dict(max_iterations=200, seed=seed)


CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_scene(k: int):
    return make_scene(**CASES[k]["scene_kw"])


def host(sc, params, problem: int = 0, scale=None):
    """ss_two_view_host of the scene -> (flags, points, point rows, result record)"""
    from send_slam_amd import binding
    return binding.two_view_host(sc["view"], PC.scale() if scale is None else scale, sc["kp1"], sc["kp2"], sc["idx"], binding.two_view_params(**params),
                                 problem)


@functools.lru_cache(maxsize=None)
def reference(k: int, problem: int = 0):
    return host(case_scene(k), CASES[k]["params"], problem)


def motion_error(res, motion):
    """(the angle of r21 . R^T, the angle between t21 and t) in radians"""
    r = np.asarray(res["r21"]).reshape(3, 3) @ np.asarray(motion[0]).T
    c = np.clip((np.trace(r) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.arccos(c)), float(np.arccos(np.clip(np.dot(res["t21"], unit(motion[1])), -1.0, 1.0)))


def solve_scene(sc, params, problem: int = 0, scale=None, status: int = 0):
    """two_view_ref.solve of the scene -> (flags, points, point rows, result record, the scores of every hypothesis)"""
    return R.solve(sc["view"], sc["kp1"], sc["kp2"], sc["idx"], PC.scale() if scale is None else scale, problem=problem, status=status, **params)


@functools.lru_cache(maxsize=None)
def restatement(k: int, problem: int = 0):
    return solve_scene(case_scene(k), CASES[k]["params"], problem)


# every match a gross outlier and thresholds so tight that no term of any model is accepted: every real model scores exactly 0.0, so
# the winners are decided by the tie rule alone
TIE_SCENE = dict(rng_seed=7, n=100, n_out=100, n1=128, n2=128)
TIE_PARAMS = dict(chi2_h=1e-300, chi2_f=1e-300, chi2_score=1e-300, seed=7)


# ---- the chain: SearchForInitialization -> Reconstruct -> the 20-iteration adjustment -> the first projection search ----
CHAIN_ROWS = 128
CHAIN_GUIDED = dict(th=50, ratio_num=9, ratio_den=10, one_to_one=True)
CHAIN_TWO_VIEW = dict(max_iterations=24, seed=5)
CHAIN_PROJ = dict(th=3.0, ratio_num=8, ratio_den=10, one_to_one=True)
CHAIN_GBA = dict(n_rounds=1, iterations=(5, 0, 0, 0), pcg_iterations=16)
# the adjusted pose against the planted one, up to scale (rotation angle, angle of the translation direction; radians): section 29's
# bound of a noise-free adjustment against the ground truth, TRUTH_BOUND_POSE = 2.3e-6 of tests/test_gba_ref.py, on both angles (an
# angle moves no pose entry by more than itself).  Seen on the references: 2.1e-8 and 2.1e-7
CHAIN_POSE_BOUND = (2.3e-6, 2.3e-6)


@functools.lru_cache(maxsize=None)
def chain_scene():
    """the exact scene of 120 correspondences with descriptors: a matched pair shares one up to a flipped bit, every other row has a
    random one (about 128 bits away from any other); windows of 80 px around the reference keypoints, every octave"""
    import guided_ref as GRf
    sc = dict(make_scene(3, 120, 0, CHAIN_ROWS, CHAIN_ROWS))
    rng = np.random.Generator(np.random.PCG64(0xC4A1))
    d1 = rng.integers(0, 256, (CHAIN_ROWS, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (CHAIN_ROWS, 32), dtype=np.uint8)
    d2[sc["idx"][sc["rows"]]] = d1[sc["rows"]]
    d2[sc["idx"][sc["rows"]], rng.integers(0, 32, len(sc["rows"]))] ^= 1
    sc.update(desc1=d1, desc2=d2, windows=GRf.make_windows(sc["kp1"]["x"], sc["kp1"]["y"], 80.0, 0, 7))
    return sc


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the chain on the references -> (guided match, two-view restatement, obs records, start poses, global BA, refined block,
    the view of frame 2, projection search)"""
    import gba_ref as GBR
    import guided_ref as GRf
    import pose_cases as PO
    sc = chain_scene()
    guided = GRf.match(sc["kp1"], sc["desc1"], sc["kp2"], sc["desc2"], sc["windows"], **CHAIN_GUIDED)
    tv = solve_scene(dict(sc, idx=guided[0]), CHAIN_TWO_VIEW)
    flag, pts, rows, res = tv[:4]
    k = len(pts)
    kp = np.stack([sc["kp1"], sc["kp2"]])
    obs = GBR.obs_from_idx(kp, rows.T.copy(), np.array([CHAIN_ROWS, CHAIN_ROWS], np.int32))
    start = np.stack([PO.start_of(np.eye(3), np.zeros(3)), PO.start_of(res["r21"], res["t21"])])
    gviews = np.array([PO.view(cam=CAM + (0.0,))] * 2)
    gba = GBR.optimise(gviews, start, np.array([1, 0], np.uint8), PC.scale(), pts, obs, dict(GBR.DEFAULTS, **CHAIN_GBA))
    refined = pts.copy()
    for e, name in enumerate("xyz"):
        refined[name] = np.where(gba[2] == 2, pts[name], gba[1][:, e].astype(f32))
    wview = P.view_init(*CAM, W, H, gba[0][1][:9], gba[0][1][9:], 0.0)
    proj = P.match(wview, refined, sc["desc1"][rows[:, 0]], sc["kp2"], sc["desc2"], PC.scale(), **CHAIN_PROJ)
    return guided, tv, obs, start, gba, refined, wview, proj

