"""The synthetic scenes and cached references the PnP RANSAC tests share (test infrastructure, plain module).

    make_scene()    map points at depth 3 - 9 in a camera of known pose, taken to world coordinates and rounded to float32; keypoints on
                    their projections (plus Gaussian noise on request); gross outliers on request: their keypoints sit anywhere in the
                    image; the correspondences scattered over the keypoint rows, the point rows permuted
    CASES           the states and boundaries of the rule (tests/test_pnp_ref.py asserts on the reference that each is what its name
                    says)
    reference()     pnp_ref.solve of a case as problem number `problem` of a call, cached
    host()          ss_pnp_host of a scene: the twin that tests/test_pnp_ref.py holds to the restatement bit for bit on every case, and
                    that the GPU tests use where the restatement (20 ms per hypothesis) would take minutes
    sextuples       well-spread ones with exact projections, random noisy ones, and the degenerate sets of the issue
"""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import guided_cases as G
import pnp_ref as N
import proj_cases as PC
import proj_ref as P

f32 = np.float32
FX, FY, CX, CY, W, H = 500.0, 510.0, 318.0, 243.0, 640, 480
POSE = (PC.rot(0.3, -0.2, 0.1), (0.3, -0.2, 0.5))
ROWS = 64  # rows of the pairs form the cases run through
CAM = (FX, FY, CX, CY)


def view(cam=CAM):
    """the view of the camera; the rule reads fx fy cx cy only, so its pose is left at a value that is not the scene's"""
    return P.view_init(*cam, W, H, np.eye(3), (0.0, 0.0, 0.0), 0.0)


def points_of(xyz) -> np.ndarray:
    xyz = np.asarray(xyz)
    pts = np.zeros(len(xyz), P.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["nz"], pts["min_dist"], pts["max_dist"] = 1.0, 0.1, 100.0
    return pts


def to_world(xc, pose=POSE):
    """camera coordinates -> world coordinates under pose = (rcw, tcw): R^T (X - t), row vectors"""
    return (np.asarray(xc, np.float64) - np.asarray(pose[1])) @ np.asarray(pose[0])


def project(xc, cam=CAM):
    xc = np.asarray(xc, np.float64)
    return np.stack([cam[0] * xc[:, 0] / xc[:, 2] + cam[2], cam[1] * xc[:, 1] / xc[:, 2] + cam[3]], axis=1)


def camera_points(rng, n, shape="spread"):
    z = rng.uniform(3.0, 9.0, n)
    xc = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], axis=1)
    if shape == "same_point":
        xc[:] = xc[0]
    elif shape == "coplanar":  # a plane oblique to the optical axis
        xc[:, 2] = 6.0 + 0.3 * xc[:, 0] - 0.2 * xc[:, 1]
    elif shape == "collinear":
        s = rng.uniform(-1.0, 1.0, n)
        xc = np.array([0.2, -0.1, 6.0]) + s[:, None] * np.array([1.0, 0.5, 0.8])
    return xc


def make_scene(rng_seed: int, n: int, n_out: int = 0, n_kp: int | None = None, n_points: int | None = None, octaves=(0, 1, 2, 3),
               noise: float = 0.0, scatter: bool = True, shape: str = "spread", cam=CAM, pose=POSE):
    """n correspondences of which n_out are gross outliers, over n_kp keypoint rows and n_points point rows -> dict view points kp idx
    (int32 [n_kp]) skip rows (the keypoint rows of the correspondences, ascending) inlier_rows pose"""
    rng = np.random.Generator(np.random.PCG64(0x9A90000 + rng_seed))
    n_kp = n if n_kp is None else n_kp
    n_points = n if n_points is None else n_points
    assert n_kp >= n and n_points >= n
    xc = camera_points(rng, n, shape)
    uv = project(xc, cam) + (rng.normal(0.0, noise, (n, 2)) if noise else 0.0)
    out = np.zeros(n, bool)
    if n_out:
        out[rng.choice(n, n_out, replace=False)] = True
        uv[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], axis=1)
    rows = np.sort(rng.choice(n_kp, n, replace=False)) if scatter else np.arange(n)
    cols = rng.permutation(n_points)[:n] if scatter else np.arange(n)
    points = points_of(rng.uniform(-5, 5, (n_points, 3)) + [0, 0, 8.0])
    points[cols] = points_of(to_world(xc, pose))
    kp = G.kp_rows(rng.uniform(0, W, n_kp).astype(f32), rng.uniform(0, H, n_kp).astype(f32), octave=rng.choice(octaves, n_kp))
    kp["x"][rows], kp["y"][rows] = uv[:, 0], uv[:, 1]
    idx = np.full(n_kp, -1, np.int32)
    idx[rows] = cols
    return dict(view=view(cam), points=points, kp=kp, idx=idx, skip=None, rows=rows, inlier_rows=rows[~out], pose=pose)


def _case(name, expect_state, scene_kw, **params):
    p = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=40, refine_steps=5, seed=0)
    p.update(params)
    return dict(name=name, expect_state=expect_state, scene_kw=scene_kw, params=p)


# The table of the issue; every case fits ROWS rows.  BEST_30: scenes of 40 correspondences with 10 gross outliers and no noise, whose
# best hypothesis counts exactly the 30 planted inliers (asserted on the reference), so that min_inliers and min_ratio are met from
# both sides with literal numbers
BEST_30 = dict(n=40, n_out=10, n_kp=64, n_points=50)
CASES = [
    _case("state 0: 60 correspondences, 24 gross outliers, 0.5 px noise", 0, dict(rng_seed=1, n=60, n_out=24, n_kp=64, n_points=64, noise=0.5), seed=1),
    _case("ties: 30 exact correspondences, the smallest t wins", 0, dict(rng_seed=2, n=30, n_kp=40, n_points=30), seed=2, max_iterations=12),
    _case("min_inliers met: 30 of 30", 0, dict(rng_seed=3, **BEST_30), seed=3, min_inliers=30, min_ratio=0.0),
    _case("min_inliers missed: 30 of 31", 2, dict(rng_seed=3, **BEST_30), seed=3, min_inliers=31, min_ratio=0.0),
    _case("min_ratio met: 30 >= 0.75 * 40", 0, dict(rng_seed=3, **BEST_30), seed=3, min_ratio=0.75),
    _case("min_ratio missed: 30 < 0.76 * 40", 2, dict(rng_seed=3, **BEST_30), seed=3, min_ratio=0.76),
    _case("min_ratio off: 14 inliers of 30", 0, dict(rng_seed=4, n=30, n_out=16, n_kp=64, n_points=64), seed=22, min_ratio=0.0, max_iterations=16),
    _case("min_ratio on: 14 < 0.5 * 30", 2, dict(rng_seed=4, n=30, n_out=16, n_kp=64, n_points=64), seed=22, max_iterations=16),
    _case("state 2: 40 correspondences, 28 outliers, 4 iterations", 2, dict(rng_seed=5, n=40, n_out=28, n_kp=64, n_points=50), seed=5, max_iterations=4),
    _case("smallest: 6 correspondences, min_inliers 6", 0, dict(rng_seed=6, n=6, n_kp=9, n_points=7), seed=6, min_inliers=6, max_iterations=3),
    _case("state 1: 19 correspondences under min_inliers 20", 1, dict(rng_seed=7, n=19, n_kp=33, n_points=64), min_inliers=20),
    _case("state 1: 5 correspondences, min_inliers 0", 1, dict(rng_seed=8, n=5, n_kp=8, n_points=8), min_inliers=0),
    _case("degenerate: every correspondence is one point, and any pose through it counts them all", 0, dict(rng_seed=9, n=30, n_kp=64, n_points=64, shape="same_point"), min_inliers=5, max_iterations=8),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_scene(k: int):
    return make_scene(**CASES[k]["scene_kw"])


def solve_scene(sc, params, problem: int = 0, scale=None, status: int = 0):
    return N.solve(sc["view"], sc["points"], sc["kp"], sc["skip"], sc["idx"], PC.scale() if scale is None else scale, problem=problem,
                   status=status, **params)


@functools.lru_cache(maxsize=None)
def reference(k: int, problem: int = 0):
    """-> (result record, flags, counts) of case k run as problem number `problem` of a call"""
    return solve_scene(case_scene(k), CASES[k]["params"], problem)


def host(sc, params, problem: int = 0, scale=None):
    """ss_pnp_host of the scene -> (result record, flags)"""
    from send_slam_amd import binding
    flags, res = binding.pnp_host(sc["view"], PC.scale() if scale is None else scale, sc["points"], sc["kp"], sc["idx"], binding.pnp_params(**params),
                                  skip=sc["skip"], problem=problem)
    return res, flags


def corr_of(sc, chi2=5.991, scale=None):
    return N.correspondences(sc["points"], sc["kp"], sc["skip"], sc["idx"], PC.scale() if scale is None else scale, chi2)


# ---- sextuples ------------------------------------------------------------------------------------------------------------------------
def spread_of(xyz, pose=POSE) -> float:
    """the smallest singular value of the six centred points over the largest: 0 for a planar set"""
    x = np.asarray(xyz, np.float64).reshape(6, 3)
    s = np.linalg.svd(x - x.mean(axis=0), compute_uv=False)
    return float(s[2] / s[0])


def exact_sextuples(rng, n: int, min_spread: float = 0.25):
    """n well-spread sextuples with exact projections: world points that ARE float32 numbers and keypoints computed from them in
    double, so the only error in the data is the rounding of u, v to float32 -> (xyz [n, 6, 3] float32, uv [n, 6, 2] float32)"""
    xyz, uv = [], []
    while len(xyz) < n:
        xw = to_world(camera_points(rng, 6)).astype(f32)
        if spread_of(xw) < min_spread:
            continue
        xc = xw.astype(np.float64) @ np.asarray(POSE[0]).T + np.asarray(POSE[1])
        xyz.append(xw)
        uv.append(project(xc).astype(f32))
    return np.array(xyz), np.array(uv)


def noisy_sextuples(rng, n: int, noise: float = 1.0):
    xc = np.array([camera_points(rng, 6) for _ in range(n)])
    uv = np.array([project(x) for x in xc]) + rng.normal(0.0, noise, (n, 6, 2))
    return np.array([to_world(x) for x in xc]).astype(f32), uv.astype(f32)


def degenerate_sextuples():
    """-> list of (name, xyz [6, 3], uv [6, 2], point rows [6]): the sets of the issue"""
    rng = np.random.Generator(np.random.PCG64(0xDE6))
    out = []

    def one(name, xc, rows=np.arange(6), edit=None):
        xw, uv = to_world(xc).astype(f32), project(xc).astype(f32)
        if edit:
            edit(xw, uv)
        out.append((name, xw, uv, np.asarray(rows, np.int32)))

    one("coplanar", camera_points(rng, 6, "coplanar"))
    one("collinear", camera_points(rng, 6, "collinear"))
    xc = camera_points(rng, 6)
    xc[4] = xc[1]
    one("two identical points", xc)
    one("a repeated point row", camera_points(rng, 6), rows=[0, 1, 2, 3, 1, 5])
    one("every point the same", camera_points(rng, 6, "same_point"))
    xc = camera_points(rng, 6)
    xc[2] = [0.0, 0.0, 1e-9]  # the keypoint of a point at the centre is anywhere: the principal point here
    one("a point at the camera centre", xc, edit=lambda xw, uv: xw.__setitem__(2, to_world(np.zeros((1, 3)))[0].astype(f32)))
    for name, v in (("1e30", 1e30), ("infinite", np.inf), ("NaN", np.nan)):
        one(name + " in a point", camera_points(rng, 6), edit=lambda xw, uv, v=v: xw.__setitem__((3, 1), v))
        one(name + " in a keypoint", camera_points(rng, 6), edit=lambda xw, uv, v=v: uv.__setitem__((5, 0), v))
    return out


def degenerate_scenes():
    """scenes every hypothesis of which is degenerate, and a good scene with broken rows among its correspondences"""
    scenes = [("coplanar", make_scene(20, 30, 0, 40, 40, shape="coplanar")), ("collinear", make_scene(21, 30, 0, 40, 40, shape="collinear")),
              ("one point", make_scene(22, 30, 0, 40, 40, shape="same_point"))]
    sc = dict(make_scene(23, 40, 8, 48, 48, noise=0.5))
    sc["points"], sc["kp"] = sc["points"].copy(), sc["kp"].copy()
    cols = sc["idx"][sc["rows"]]
    sc["points"]["x"][cols[0]], sc["points"]["y"][cols[1]], sc["points"]["z"][cols[2]] = 1e30, np.inf, np.nan
    sc["kp"]["x"][sc["rows"][3]], sc["kp"]["y"][sc["rows"][4]] = np.nan, np.inf
    sc["idx"] = sc["idx"].copy()
    sc["idx"][sc["rows"][6]] = sc["idx"][sc["rows"][5]]  # two keypoints on one point row
    scenes.append(("broken rows among good ones", sc))
    return scenes


# ---- a camera per problem, strides that differ, counts told wrong ----------------------------------------------------------------------
CAMERA_POSES = (POSE, (PC.rot(-0.2, 0.25, -0.15), (-0.4, 0.1, 0.8)), (PC.rot(0.1, 0.1, 0.3), (0.2, 0.3, -0.2)))
CAMERA_PARAMS = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=24, refine_steps=5, seed=7)
CAMERA_INLIERS, CAMERA_WINNERS = 36, (3, 3, 6)  # of every scene as problem b of one call (asserted on the restatement)


def camera_scenes(cams=CC.SIM3_FRAME_CAMERAS):
    """scene b under camera b of camera_cases.SIM3_FRAME_CAMERAS (P, Q, the square one) and pose b, to be run as problem b of one call:
    48 correspondences, 12 gross outliers, 0.5 px noise, over 64 keypoint rows and 80 point rows.  cams: the cameras the views are
    built from (a mix-up's, where a test shows what a wrong kernel would compute); the keypoints are always the true cameras'"""
    scenes = [make_scene(300 + b, 48, 12, 64, 80, noise=0.5, cam=CC.intrinsics(CC.SIM3_FRAME_CAMERAS[b]), pose=CAMERA_POSES[b]) for b in range(3)]
    return [dict(sc, view=view(CC.intrinsics(c))) for sc, c in zip(scenes, cams)]


def cut(sc):
    """what a call may read of sc: the rows under the counts it is told (the keys n_points and n_kp, where they are not the lengths of
    the arrays), clamped to 0 .. the rows there are, as the rule clamps them"""
    n_p = min(max(sc.get("n_points", len(sc["points"])), 0), len(sc["points"]))
    n_k = min(max(sc.get("n_kp", len(sc["kp"])), 0), len(sc["kp"]))
    return dict(sc, points=sc["points"][:n_p], kp=sc["kp"][:n_k], idx=sc["idx"][:n_k], skip=None if sc["skip"] is None else sc["skip"][:n_p])


# (point_rows, rows_per_frame, the n_points and the n_kp told for each scene): no count reaches either row figure, so whichever of the
# two a stride or a clamp is taken from, only the stride shows
STRIDE_LAYOUTS = {"more point rows than keypoint rows": (83, 67, (66, 60, 63), (61, 64, 58)),
                  "fewer point rows than keypoint rows": (51, 69, (48, 48, 48), (50, 47, 49))}
STRIDE_PARAMS = dict(chi2=5.991, min_ratio=0.3, lambda_=1e-6, min_inliers=10, max_iterations=16, refine_steps=5, seed=3)


@functools.lru_cache(maxsize=None)
def stride_scenes(layout: str):
    """-> (three scenes, point_rows, rows_per_frame): 40 correspondences each (6 gross outliers, 0.5 px noise) under the counts told,
    skip bytes on five matched points, and rows that look live past the counts: the keypoint rows past n_kp repeat matched rows with
    their matches, the point rows past n_points repeat matched points, and three unmatched keypoint rows name them"""
    point_rows, rows, n_points, n_kp = STRIDE_LAYOUTS[layout]
    scenes = []
    for b in range(3):
        sc = dict(make_scene(310 + 3 * list(STRIDE_LAYOUTS).index(layout) + b, 40, 6, n_kp[b], n_points[b], noise=0.5))
        more_k, more_p = sc["rows"][np.arange(rows - n_kp[b]) % 40], sc["idx"][sc["rows"]][np.arange(point_rows - n_points[b]) % 40]
        sc["kp"], sc["points"] = np.concatenate([sc["kp"], sc["kp"][more_k]]), np.concatenate([sc["points"], sc["points"][more_p]])
        sc["idx"] = np.concatenate([sc["idx"], sc["idx"][more_k]])
        sc["idx"][np.flatnonzero(sc["idx"][:n_kp[b]] < 0)[:3]] = n_points[b] + np.arange(3) % (point_rows - n_points[b])
        sc["skip"] = np.zeros(point_rows, np.uint8)
        sc["skip"][sc["idx"][sc["rows"][b::8]]] = (1, 2, 255, 7, 128)
        sc["n_points"], sc["n_kp"] = n_points[b], n_kp[b]
        scenes.append(sc)
    return scenes, point_rows, rows


COUNT_ROWS, COUNT_POINT_ROWS = 64, 72
COUNT_PARAMS = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=16, refine_steps=5, seed=2)


@functools.lru_cache(maxsize=None)
def count_scenes():
    """-> [(name, scene)]: one good scene whose arrays are COUNT_POINT_ROWS and COUNT_ROWS long, told counts past its rows and below
    0.  The rule clamps a count to 0 .. rows: a count past the rows reads them all, a negative one none"""
    sc = make_scene(330, 44, 8, COUNT_ROWS, COUNT_POINT_ROWS, noise=0.5)
    told = (("n_kp = rows + 9", dict(n_kp=COUNT_ROWS + 9)), ("n_kp = -3", dict(n_kp=-3)),
            ("n_points = point_rows + 5", dict(n_points=COUNT_POINT_ROWS + 5)), ("n_points = -2", dict(n_points=-2)))
    return [(name, dict(sc, **kw)) for name, kw in told]


# ---- recovery -------------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=300, refine_steps=5)
RECOVERY_SEEDS = (1, 2, 3, 4)


def recovery_scene(seed: int):
    """200 correspondences, 40 % gross outliers, 0.5 px noise"""
    return make_scene(100 + seed, 200, 80, 256, 256, noise=0.5)


# ---- planted winners: 12 inliers of 40, so a hypothesis wins only with all six draws among them ----------------------------------------
BLOCK_SCENE = dict(rng_seed=31, n=40, n_out=28, n_kp=64, n_points=64)
BLOCK_PARAMS = dict(chi2=5.991, min_ratio=0.0, lambda_=1e-6, min_inliers=10, refine_steps=5)


# ---- the relocalisation chain: BoW match -> PnP RANSAC -> pose optimisation -> view -> projection search --------------------------------
CHAIN_ROWS = 64
CHAIN_PNP = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=64, refine_steps=5, seed=4)
CHAIN_BOW = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=0)
CHAIN_PROJ = dict(view_cos_limit=0.5, th=3.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10, one_to_one=True, check_right=False)


@functools.lru_cache(maxsize=None)
def chain_scene():
    """make_scene's lost frame (48 matches to the candidate keyframe's map points, 8 of them wrong, 0.3 px noise) with what the other
    stages read: descriptors (a correspondence's two rows a few bits apart, every other couple about 128), nodes (a correspondence's two
    rows share one; an unmatched train row has a node no query has), the candidate's keypoints (only their octaves matter), and for its
    map points a viewing direction and distance range under which the projection search predicts the keypoint's level"""
    rng = np.random.Generator(np.random.PCG64(0xC4A2))
    sc = dict(make_scene(80, 48, 8, CHAIN_ROWS, CHAIN_ROWS, octaves=(0, 1), noise=0.3))
    n = CHAIN_ROWS
    rows, cols = sc["rows"], sc["idx"][sc["rows"]]
    t_desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q_desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q_desc[rows] = PC.desc_near(rng, t_desc[cols])
    q_node, t_node = (np.arange(n) % 4).astype(np.int32), np.full(n, 5, np.int32)
    t_node[cols] = q_node[rows]
    t_kp = G.kp_rows(rng.uniform(20, W - 20, n).astype(f32), rng.uniform(20, H - 20, n).astype(f32), octave=rng.choice((0, 1), n))
    pts = sc["points"].copy()
    ow = -np.asarray(POSE[0]).T @ np.asarray(POSE[1])
    d = np.stack([pts[k] for k in "xyz"], 1).astype(np.float64) - ow
    dist = np.linalg.norm(d, axis=1)
    pts["nx"], pts["ny"], pts["nz"] = (d / dist[:, None]).T
    octave = np.zeros(n, np.int64)
    octave[cols] = sc["kp"]["octave"][rows]
    pts["max_dist"], pts["min_dist"] = dist * np.array([float(s) for s in PC.scale()])[octave] * 0.95, 0.3 * dist
    sc.update(points=pts, q_desc=q_desc, t_desc=t_desc, q_node=q_node, t_node=t_node, t_kp=t_kp, bow_idx=sc["idx"])
    return sc


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the chain on the references -> (bow match, pnp (result, flags, counts), pose (result, flags), view, projection match)"""
    import bow_ref
    import pose_ref
    sc = chain_scene()
    bow = bow_ref.match(sc["kp"], sc["q_desc"], sc["q_node"], sc["t_kp"], sc["t_desc"], sc["t_node"], **CHAIN_BOW)
    pnp = solve_scene(dict(sc, idx=bow[0]), CHAIN_PNP, 0)
    start = np.concatenate([pnp[0]["rcw"], pnp[0]["tcw"]])
    pose = pose_ref.optimise(sc["view"], start, PC.scale(), sc["points"], sc["kp"], bow[0], dict(idx_by_row=True))
    view = P.view_init(FX, FY, CX, CY, W, H, pose[0]["rcw"], pose[0]["tcw"], 0.0)
    proj = P.match(view, sc["points"], sc["t_desc"], sc["kp"], sc["q_desc"], PC.scale(), **CHAIN_PROJ)
    return bow, pnp, pose, view, proj
