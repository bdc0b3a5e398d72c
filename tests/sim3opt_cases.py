"""The synthetic scenes and cached references the Sim3 refinement tests share (test infrastructure, plain module).

    make_pair()   sim3_cases.make_pair's scene (a known Sim3, float32 inputs, gross mismatches on request) with what the refinement reads
                  on top: keypoints of both keyframes on the projections of their map points plus Gaussian pixel noise, rounded to
                  float32, and a start model a few pixels off the truth
    model_record() a sim3 result record from (R, t, s) in double, formed as the RANSAC forms it
    CASES         the paths of the rule (tests/test_sim3opt_ref.py asserts on the reference that each is what its name says)
    reference()   sim3opt_ref.optimise of a case, cached
    count_pair()  a pair with exactly n correspondences
    marks_tables() random and adversarial tables for the bookkeeping
    camera_pairs() three pairs under camera_cases.SIM3_PAIR_CAMERAS (non-square, off-centre, the two sides different), each its own scene
    pyramid_pair() a pair under cameras P and Q whose octaves are chosen for another pyramid table than the default
    LIMITS        the parameters at their limits on one pair from two starts, LIMITS_RECORDED what the reference gives
    singular_pair() a pair whose third pivot is 0 by structure: state 2 with finite sums
    frozen_pair() twelve exact correspondences and one keypoint two pixels off: the thresholds from both sides
    camera_batch_skip() skip bytes for sim3_cases.camera_batch() that differ between the query's frame and the train's
"""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import guided_cases as G
import proj_cases as PC
import proj_ref as P
import sim3_cases as SC
import sim3_ref as S
import sim3opt_ref as O

f32 = np.float32
START_OFF = dict(angle=0.004, s=1.01, t=(0.01, -0.008, 0.012))


def model_record(R, t, s, state=0, status=0) -> np.ndarray:
    """(R 3 x 3, t, s) in double -> a sim3 RESULT_DTYPE record: s.R, t, s and the inverse rounded to float32"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    m = np.zeros((), S.RESULT_DTYPE)
    m["sr12"], m["t12"], m["s12"] = (s * R).reshape(9), t, s
    m["sr21"], m["t21"] = (R.T / s).reshape(9), -(R.T @ t) / s
    m["state"], m["status"], m["iteration"] = state, status, -1
    return m


def true_model(s=SC.S_TRUE):
    return SC.rodrigues(SC.AXIS, SC.ANGLE), np.asarray(SC.T_TRUE, np.float64), s


def start_near(s=SC.S_TRUE, off=START_OFF, fix_scale=False) -> np.ndarray:
    R, t, s = true_model(s)
    dR = SC.rodrigues(np.array([0.6, -0.64, 0.48]), off["angle"])
    return model_record(dR @ R, t + np.asarray(off["t"]), s if fix_scale else s * off["s"])


def make_pair(rng_seed: int, n: int, n_out: int = 0, nq: int | None = None, nt: int | None = None, s: float = SC.S_TRUE, noise_px: float = 0.5,
              octaves=(0, 1, 2, 3), spread: float = 0.6, fix_scale: bool = False, cam1=SC.CAM, cam2=SC.CAM, scale=None):
    """-> sim3_cases.make_pair's dict with keypoints set and `start`, `outlier_rows` (the query rows of the planted mismatches); cam1,
    cam2: the cameras of the two views, which the planted keypoints are the projections under; scale: the pyramid table the octaves
    are meant for (the default table when None): a correspondence with an octave outside it gets no planted keypoint"""
    pr = dict(SC.make_pair(rng_seed, n, n_out, nq, nt, s=s, octaves=octaves, spread=spread, cam1=cam1, cam2=cam2))
    rng = np.random.Generator(np.random.PCG64(0x0517300 + rng_seed))
    c = S.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"],
                          PC.scale() if scale is None else scale, 1.0)
    q_kp, t_kp = pr["q_kp"].copy(), pr["t_kp"].copy()
    q_kp["x"], q_kp["y"] = rng.uniform(20, SC.W - 20, len(q_kp)).astype(f32), rng.uniform(20, SC.H - 20, len(q_kp)).astype(f32)
    t_kp["x"], t_kp["y"] = rng.uniform(20, SC.W - 20, len(t_kp)).astype(f32), rng.uniform(20, SC.H - 20, len(t_kp)).astype(f32)
    m = len(c["rows"])
    q_kp["x"][c["rows"]], q_kp["y"][c["rows"]] = c["u1"] + rng.normal(0, noise_px, m).astype(f32), c["v1"] + rng.normal(0, noise_px, m).astype(f32)
    t_kp["x"][c["cols"]], t_kp["y"][c["cols"]] = c["u2"] + rng.normal(0, noise_px, m).astype(f32), c["v2"] + rng.normal(0, noise_px, m).astype(f32)
    pr.update(q_kp=q_kp, t_kp=t_kp, start=start_near(s, fix_scale=fix_scale), outlier_rows=np.setdiff1d(pr["rows"], pr["inlier_rows"]))
    return pr


def _case(name, pair_kw, **params):
    return dict(name=name, pair_kw=pair_kw, params=dict(O.UPSTREAM, **params))


CASES = [
    _case("60 correspondences, 9 mismatches: iterations_more", dict(rng_seed=1, n=60, n_out=9, nq=64, nt=64), step_eps=0.0),
    _case("40 correspondences, no mismatch: iterations_same", dict(rng_seed=2, n=40, nq=64, nt=50), step_eps=0.0),
    _case("fix_scale on a scene of scale 1", dict(rng_seed=3, n=50, n_out=6, nq=64, nt=64, s=1.0, fix_scale=True), fix_scale=True),
    _case("a round ends early on step_eps", dict(rng_seed=4, n=30, nq=40, nt=40, noise_px=0.0), step_eps=1e-4),
    _case("state 3: 12 of 20 are mismatches, min_inliers 10", dict(rng_seed=5, n=20, n_out=12, nq=32, nt=32)),
    _case("300 correspondences over two slots' rounds", dict(rng_seed=6, n=300, n_out=40, nq=320, nt=310)),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_pair(k: int):
    return make_pair(**CASES[k]["pair_kw"])


def solve_pair(pr, params, status: int = 0, trace=None, scale=None, start=None):
    return O.optimise(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["q_skip"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["t_skip"], pr["idx"],
                      PC.scale() if scale is None else scale, pr["start"] if start is None else start, params, status, trace)


@functools.lru_cache(maxsize=None)
def reference(k: int):
    """-> (result record, flags, trace) of case k"""
    trace = []
    res, flags = solve_pair(case_pair(k), CASES[k]["params"], trace=trace)
    return res, flags, trace


@functools.lru_cache(maxsize=None)
def count_pair(n: int, fix_scale: bool = False):
    """exactly n correspondences in rows of max(n, 1) + 7, a tenth of them mismatches"""
    rows = max(n, 1) + 7
    if n == 0:
        pr = dict(make_pair(40, 1, 0, rows, rows, s=1.0 if fix_scale else SC.S_TRUE, fix_scale=fix_scale))
        pr["idx"] = np.full(rows, -1, np.int32)
        return pr
    return make_pair(40 + n, n, n // 10, rows, rows, s=1.0 if fix_scale else SC.S_TRUE, fix_scale=fix_scale)


def with_skips(pr, seed: int, every: int = 7):
    """skip bytes on both sides, some on correspondences"""
    rng = np.random.Generator(np.random.PCG64(0x5C1 + seed))
    pr = dict(pr)
    pr["q_skip"] = (rng.integers(0, every, len(pr["q_xyz"])) == 0).astype(np.uint8) * 3
    pr["t_skip"] = (rng.integers(0, every, len(pr["t_xyz"])) == 0).astype(np.uint8)
    return pr


def marks_tables(rows: int, seed: int):
    """-> dict idx idx12 idx21 q_skip t_skip nq nt: random tables with two rows naming one train row, idx out of range and negative,
    counts below the array length, and a prior match whose partner a search also found"""
    rng = np.random.Generator(np.random.PCG64(0x3A2C + 31 * rows + seed))
    nq, nt = max(rows - rows // 5, 1), max(rows - rows // 7, 1)
    idx = rng.integers(-2, rows + 2, rows).astype(np.int32)
    idx[rng.random(rows) < 0.5] = -1
    idx12 = rng.integers(-2, rows + 2, rows).astype(np.int32)
    idx21 = rng.integers(-2, rows + 2, rows).astype(np.int32)
    for i in range(rows):  # make half of the searches agree
        j = int(idx12[i])
        if 0 <= j < rows and rng.random() < 0.5:
            idx21[j] = i
    if rows >= 4:
        idx[0], idx[1] = 2, 2          # two rows naming one train row
        idx[2] = -1
        idx12[2], idx21[2] = 2, 2      # a mutual pair whose train row a prior match holds
        idx[3] = 1
        idx12[3], idx21[1] = 1, 3      # a prior match whose partner a search also found
    return dict(idx=idx, idx12=idx12, idx21=idx21, q_skip=(rng.random(rows) < 0.2).astype(np.uint8) * 5, t_skip=(rng.random(rows) < 0.2).astype(np.uint8),
                nq=nq, nt=nt)


# ---- odd cameras: three pairs per call under CC.SIM3_PAIR_CAMERAS ----------------------------------------------------------------------------
# Both residuals of the refinement, u - (fx.x/z + cx) and v - (fy.y/z + cy), read all four intrinsics of their side, so -- unlike the
# RANSAC -- no mix-up of camera_cases.PAIR_MIXUPS is exempt (tests/test_sim3opt_ref.py asserts it on the reference)
CAMERA_PAIR = dict(n=60, n_out=9, nq=64, nt=64)


@functools.lru_cache(maxsize=None)
def camera_pairs(cams=CC.SIM3_PAIR_CAMERAS):
    """pair b is its own scene under the cameras cams[b] = (camera of view 1, camera of view 2), its keypoints planted under them"""
    return [make_pair(70 + b, cam1=c1, cam2=c2, **CAMERA_PAIR) for b, (c1, c2) in enumerate(cams)]


@functools.lru_cache(maxsize=None)
def camera_reference():
    return [solve_pair(pr, O.UPSTREAM) for pr in camera_pairs()]


# ---- other pyramid tables ------------------------------------------------------------------------------------------------------------------
# name -> the octaves the keypoints of both sides are drawn from: about half of the correspondences have an octave outside the table
# on one side at least.  Under one level every correspondence that stays has octave 0 on both sides (w1 = w2 = 1); under sixteen the
# octaves of the two sides differ for most, so exchanged weights change the sums
PYRAMID_OCTAVES = {"one_level": (0, 0, 0, 1), "sixteen_levels": (-1, 0, 2, 5, 9, 13, 15, 16)}
PYRAMID_PAIR = dict(n=100, n_out=10, nq=128, nt=128)


@functools.lru_cache(maxsize=None)
def pyramid_pair(name: str):
    """-> (pair, the table): 100 correspondences under cameras P and Q, keypoints planted on those the table keeps"""
    sc = PC.scale_table(*PC.PYRAMIDS[name])
    return make_pair(33, octaves=PYRAMID_OCTAVES[name], cam1=CC.P, cam2=CC.Q, scale=sc, **PYRAMID_PAIR), sc


# ---- the parameters at their limits ----------------------------------------------------------------------------------------------------------
LIMITS_PAIR = dict(rng_seed=50, n=65, n_out=6, nq=72, nt=72)
LIMITS_CORR = 65
TINY_CHI2 = 1e-6  # no correspondence with half a pixel of noise is under it: round 0 removes every one
_ALL = dict(iterations0=32, iterations_more=32, iterations_same=32)
_ONE = dict(iterations0=1, iterations_more=1, iterations_same=1)
# name -> (parameter overrides on O.UPSTREAM, the states a pair may end in)
LIMITS = {
    "32 iterations in every round, step_eps 0": (dict(_ALL, step_eps=0.0), (0,)),
    "1 iteration in every round": (dict(_ONE), (0,)),
    "lambda 0 and step_eps 0": (dict(lambda_=0.0, step_eps=0.0), (0,)),
    "min_corr at the count": (dict(min_corr=LIMITS_CORR), (0,)),
    "min_corr one above the count": (dict(min_corr=LIMITS_CORR + 1), (1,)),
    "round 0 removes everything, min_inliers 0": (dict(chi2=TINY_CHI2, min_inliers=0), (0, 2)),
    "round 0 removes everything, min_inliers 0, lambda 0": (dict(chi2=TINY_CHI2, min_inliers=0, lambda_=0.0), (0, 2)),
}
# what sim3opt_ref gives for (the pair from start_near(), the pair from the truth): (state, steps, n_removed) each;
# tests/test_sim3opt_ref.py asserts it on the reference and tests/test_sim3opt.py on what the device is compared with
LIMITS_RECORDED = {
    "32 iterations in every round, step_eps 0": [(0, [32, 32], 6), (0, [32, 32], 6)],
    "1 iteration in every round": [(0, [1, 1], 6), (0, [1, 1], 6)],
    "lambda 0 and step_eps 0": [(0, [5, 10], 6), (0, [5, 10], 6)],
    "min_corr at the count": [(0, [5, 6], 6), (0, [5, 6], 6)],
    "min_corr one above the count": [(1, [0, 0], 0), (1, [0, 0], 0)],
    "round 0 removes everything, min_inliers 0": [(0, [5, 1], 65), (0, [5, 1], 65)],  # the second round runs on empty sums: the damping alone
    "round 0 removes everything, min_inliers 0, lambda 0": [(2, [5, 0], 65), (2, [5, 0], 65)],  # empty sums, no damping: the first pivot is 0
}


@functools.lru_cache(maxsize=None)
def limit_pairs():
    """-> [the 65-correspondence pair from a start a few pixels off, the same pair from the scene's own Sim3]"""
    pr = make_pair(**LIMITS_PAIR)
    return [pr, dict(pr, start=model_record(*true_model()))]


def limit_params(name: str):
    return dict(O.UPSTREAM, **LIMITS[name][0])


# ---- a singular system with finite sums ------------------------------------------------------------------------------------------------------
SINGULAR_PARAMS = dict(O.UPSTREAM, lambda_=0.0)
SINGULAR_POSES = ((np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), (0.25, -0.125, 0.5)),
                  (np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), (-0.5, 0.25, 0.125)))  # quarter turns: exact


@functools.lru_cache(maxsize=None)
def singular_pair(fix_scale: bool = False):
    """30 correspondences over 64 rows under cameras P and Q.  Every map point lies on the optical axis of its own camera, at its own
    depth, and the start model -- a quarter turn about that axis, a translation along it and the scale 2 (1 under fix_scale), all exact
    in float32 -- takes either axis onto the other.  So x = y = 0 in both mappings of every correspondence, and column 2 of all four
    Jacobian rows (the rotation about the optical axis: y.iz.fx and -x.iz.fy in e12, their counterparts through m0.b - m1.a and
    m3.b - m4.a in e21) is 0 times a finite number.  H22 and every H2q are sums of zeros, the first two pivots are positive (columns 0
    and 1 hold fy and -fx), and under lambda = 0 the third pivot of the Cholesky factorisation is 0 - 0 - 0: not > 0, with every sum
    finite (columns 5 and 6, the translation along the axis and the scale, are 0 in the same way; the third pivot is met first).  The keypoints lie a pixel about the principal points, so the residuals and the right-hand side are not 0.  The start is
    not the identity: a model that stays the start differs from one that was reset"""
    n, rows = 30, 64
    rng = np.random.Generator(np.random.PCG64(0x51A7 + int(fix_scale)))
    s = 1.0 if fix_scale else 2.0
    R, t = SINGULAR_POSES[0][0], np.array([0.0, 0.0, 0.5])
    h = rng.integers(24, 72, n) / 8.0  # depths 3 .. 9 in eighths
    x2 = np.stack([np.zeros(n), np.zeros(n), h], axis=1)
    x1 = s * (x2 @ R.T) + t
    world = [(x - np.asarray(pose[1])) @ pose[0] for x, pose in ((x1, SINGULAR_POSES[0]), (x2, SINGULAR_POSES[1]))]
    q_rows, t_rows = np.sort(rng.choice(rows, n, replace=False)), rng.permutation(rows)[:n]
    q_xyz, t_xyz = SC._points(rng.uniform(-5, 5, (rows, 3)) + [0, 0, 8.0]), SC._points(rng.uniform(-5, 5, (rows, 3)) + [0, 0, 8.0])
    q_xyz[q_rows], t_xyz[t_rows] = SC._points(world[0]), SC._points(world[1])
    kps = []
    for cam, at in ((CC.P, q_rows), (CC.Q, t_rows)):
        kp = G.kp_rows(rng.uniform(20, SC.W - 20, rows).astype(f32), rng.uniform(20, SC.H - 20, rows).astype(f32), octave=rng.choice((0, 1, 2, 3), rows))
        kp["x"][at], kp["y"][at] = (cam[2] + rng.normal(0, 1.0, n)).astype(f32), (cam[3] + rng.normal(0, 1.0, n)).astype(f32)
        kps.append(kp)
    idx = np.full(rows, -1, np.int32)
    idx[q_rows] = t_rows
    views = [P.view_init(*cam[:4], SC.W, SC.H, pose[0], pose[1], cam[4]) for cam, pose in zip((CC.P, CC.Q), SINGULAR_POSES)]
    return dict(view1=views[0], view2=views[1], q_xyz=q_xyz, q_kp=kps[0], t_xyz=t_xyz, t_kp=kps[1], idx=idx, q_skip=None, t_skip=None, rows=q_rows,
                start=model_record(R, t, s))


# ---- the thresholds from both sides ----------------------------------------------------------------------------------------------------------
FROZEN = dict(O.UPSTREAM, lambda_=1e300, step_eps=0.0, min_corr=3, min_inliers=0)  # no step moves the model


def frozen_pair(edge: int):
    """12 exact correspondences, one with a keypoint two pixels off in one keyframe only -> (pair, that query row, its chi-square)"""
    pr = dict(make_pair(70, 12, 0, 16, 16, noise_px=0.0))
    pr["start"] = model_record(*true_model())  # the scene's own Sim3 rounded to float32: every other chi-square is tiny
    row = int(pr["rows"][4])
    kp = pr["q_kp" if edge == 0 else "t_kp"].copy()
    kp["x"][row if edge == 0 else pr["idx"][row]] += np.float32(2.0)
    pr["q_kp" if edge == 0 else "t_kp"] = kp
    c = O.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale())
    R, t, s, _ = O.start(pr["start"], False)
    both = O.chi2(c, O.cameras(pr["view1"], pr["view2"], 10.0), R, t, s)
    n = int(np.nonzero(c["rows"] == row)[0][0])
    return pr, row, both, n


# ---- the batch form under a camera per frame, with skip bytes ----------------------------------------------------------------------------------
# the extracted keypoints of the batch are not the projections of its map points: a wide threshold and heavy damping keep the steps
# small and both rounds live
BATCH_PARAMS = dict(O.UPSTREAM, chi2=1e7, lambda_=1e3)


@functools.lru_cache(maxsize=None)
def camera_batch_starts():
    """the RANSAC's result for every pair of sim3_cases.camera_batch(): the start of its refinement"""
    return [SC.solve_pair(SC.batch_pair(b), SC.camera_params(20), b)[0] for b in range(len(SC.CAMERA_BATCH))]


def camera_batch_pair(b: int, frame_views=None, skip=None, train_skip_of=None):
    """pair b of the batch as sim3opt_ref reads it: skip [3, rows] gives the query side the bytes of frame b and the train side those
    of frame train_src[b] (or of frame train_skip_of, the frame a wrong kernel would read)"""
    pr = dict(SC.batch_pair(b, frame_views), start=camera_batch_starts()[b])
    if skip is not None:
        t = SC.CAMERA_BATCH_SRC[b] if train_skip_of is None else train_skip_of
        pr["q_skip"] = skip[b, :len(pr["q_xyz"])]
        pr["t_skip"] = None if SC.CAMERA_BATCH_SRC[b] < 0 else skip[t, :len(pr["t_xyz"])]
    return pr


@functools.lru_cache(maxsize=None)
def camera_batch_skip():
    """skip bytes [3, rows] for sim3_cases.camera_batch(): in frame 0 they lie on a few train rows of both pairs' correspondences, in
    frames 1 and 2 on a few of their own query rows' -- and a byte of frame 0 is never set where frames 1 or 2 have one, nor the
    other way round, so the train side read at frame b instead of frame train_src[b] keeps other correspondences"""
    kps, xyz, idx, _ = SC.camera_batch()
    skip = np.zeros((3, xyz.shape[1]), np.uint8)
    for b in (1, 2):
        rows = np.flatnonzero(idx[b] >= 0)
        skip[b, rows[1::9]] = 1 + b                # on the query side of pair b
        skip[0, idx[b][rows[4::7]]] = 7            # on the train side of pair b
    skip[0, np.flatnonzero(skip[1] | skip[2])] = 0
    rng = np.random.Generator(np.random.PCG64(0x5C2))
    free = np.flatnonzero(~(skip.any(axis=0)))
    skip[0, free[rng.random(len(free)) < 0.1]] = 1  # and on rows no correspondence has
    return skip


# ---- the loop-closing chain: BoW match -> RANSAC -> marks -> two projection searches -> mutual -> refinement -> Scw -> candidate check ------
CHAIN_ROWS = SC.CHAIN_ROWS
CHAIN_HIDDEN = 8  # true correspondences the BoW match cannot see (their rows lie in different vocabulary nodes): the searches find them
CHAIN_SEARCH = dict(view_cos_limit=0.5, th=7.5, chi2_mono=0.0, chi2_stereo=0.0, th_low=50, check_right=False)  # upstream's SearchBySim3 radius
CHAIN_OPT = dict(O.UPSTREAM)


@functools.lru_cache(maxsize=None)
def chain_scene():
    """sim3_cases.chain_scene with what the refinement and the search of keyframe 1's points in keyframe 2 read on top: keypoints of
    keyframe 2 on the projections of its map points, half a pixel of noise on both keyframes' matched keypoints, a distance range for
    keyframe 1's map points under which that search predicts level 1, and CHAIN_HIDDEN correspondences hidden from the BoW match"""
    rng = np.random.Generator(np.random.PCG64(0xC4A2))
    pr = dict(SC.chain_scene())
    c = SC.corr_of(pr)
    m = len(c["rows"])
    q_kp, t_kp = pr["q_kp"].copy(), pr["t_kp"].copy()
    t_kp["x"][c["cols"]], t_kp["y"][c["cols"]] = c["u2"], c["v2"]
    for kp, r in ((q_kp, c["rows"]), (t_kp, c["cols"])):
        kp["x"][r] += rng.normal(0, 0.5, m).astype(f32)
        kp["y"][r] += rng.normal(0, 0.5, m).astype(f32)
    # the camera centre of keyframe 2 in keyframe 1's world: X1 = T_TRUE in camera 1
    r1, t1 = SC.POSE1
    ow = np.asarray(r1).T @ (np.asarray(SC.T_TRUE) - np.asarray(t1))
    q_xyz = pr["q_xyz"].copy()
    dist = np.linalg.norm(np.stack([q_xyz[n] for n in "xyz"], 1).astype(np.float64) - ow, axis=1)
    q_xyz["max_dist"], q_xyz["min_dist"] = 1.1 * dist, 0.1
    t_node = pr["t_node"].copy()
    inl = np.isin(c["rows"], pr["inlier_rows"])
    hidden = np.flatnonzero(inl)[:CHAIN_HIDDEN]
    t_node[c["cols"][hidden]] = 6  # a node no query row has
    pr.update(q_kp=q_kp, t_kp=t_kp, q_xyz=q_xyz, t_node=t_node, hidden_rows=c["rows"][hidden])
    return pr


def chain_views(model):
    """(the view of keyframe 1's camera over keyframe 2's world, that of keyframe 2's camera over keyframe 1's world) under a model"""
    import fuse_ref
    srcw, t = S.to_scw(model, SC.POSE2[0], SC.POSE2[1])
    v12 = fuse_ref.view_sim3(SC.F, SC.F, SC.CX, SC.CY, SC.W, SC.H, srcw, t, 0.0)
    srcw, t = O.to_s21w(model, SC.POSE1[0], SC.POSE1[1])
    return v12, fuse_ref.view_sim3(SC.F, SC.F, SC.CX, SC.CY, SC.W, SC.H, srcw, t, 0.0)


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the chain on the references -> dict bow sim3 skip1 skip2 v12 v21 search21 search12 idx mutual opt view check check_ransac"""
    import bow_ref
    import fuse_ref
    pr, rows = chain_scene(), CHAIN_ROWS
    out = {}
    out["bow"] = bow_ref.match(pr["q_kp"], pr["q_desc"], pr["q_node"], pr["t_kp"], pr["t_desc"], pr["t_node"], **SC.CHAIN_BOW)
    idx = out["bow"][0]
    out["sim3"] = SC.solve_pair(dict(pr, idx=idx), SC.CHAIN_SIM3, 0)
    model = out["sim3"][0]
    assert model["state"] == 0
    out["skip1"], out["skip2"] = O.marks(idx, None, None, rows, rows)
    out["v12"], out["v21"] = chain_views(model)
    # keyframe 2's points in keyframe 1 (gives idx21, by train row), keyframe 1's points in keyframe 2 (gives idx12, by query row)
    out["search21"] = fuse_ref.match(out["v12"], pr["t_xyz"], pr["t_desc"], pr["q_kp"], pr["q_desc"], PC.scale(), skip=out["skip2"], taken=out["skip1"], **CHAIN_SEARCH)
    out["search12"] = fuse_ref.match(out["v21"], pr["q_xyz"], pr["q_desc"], pr["t_kp"], pr["t_desc"], PC.scale(), skip=out["skip1"], taken=out["skip2"], **CHAIN_SEARCH)
    out["idx"], out["mutual"] = O.mutual(idx, out["search12"][0], out["search21"][0], rows, rows)
    out["opt"] = solve_pair(dict(pr, idx=out["idx"]), CHAIN_OPT, start=model)
    refined = out["opt"][0]["model"]
    out["view"] = chain_views(refined)[0] if refined["state"] == 0 else None
    check = lambda v: fuse_ref.match(v, pr["t_xyz"], pr["t_desc"], pr["q_kp"], pr["q_desc"], PC.scale(), **fuse_ref.CANDIDATE_CHECK)  # noqa: E731
    out["check"] = None if out["view"] is None else check(out["view"])
    out["check_ransac"] = check(out["v12"])
    return out
