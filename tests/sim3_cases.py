"""The synthetic scenes and cached references the Sim3 RANSAC tests share (test infrastructure, plain module).

    make_pair()   map points of keyframe 2 at depth 3 - 9 in its camera, the same points under a known Sim3 (s = 1.3, 0.3 rad) in
                  keyframe 1's camera, both taken to world coordinates through the keyframes' poses and rounded to float32; gross
                  outliers on request; the correspondences scattered over the query rows, the train rows permuted
    CASES         the states and boundaries of the rule (tests/test_sim3_ref.py asserts on the reference that each is what its
                  name says)
    reference()   sim3_ref.solve of a case as pair number `pair` of a call, cached
"""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import guided_cases as G
import proj_cases as PC
import proj_ref as P
import sim3_ref as S

f32 = np.float32
F, CX, CY, W, H = 500.0, 320.0, 240.0, 640, 480
S_TRUE, ANGLE = 1.3, 0.3
AXIS = np.array([0.2, 0.9, -0.3]) / np.linalg.norm([0.2, 0.9, -0.3])
T_TRUE = np.array([0.4, -0.2, 0.6])
POSE1 = (PC.rot(0.02, -0.03, 0.01), (0.1, -0.05, 0.2))
POSE2 = (PC.rot(-0.015, 0.025, -0.02), (-0.2, 0.1, 0.05))
ROWS = 64  # rows of the pairs form the cases run through


def rodrigues(axis, angle) -> np.ndarray:
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


CAM = (F, F, CX, CY, 0.0)


def views(cam1=CAM, cam2=CAM):
    """the views of keyframes 1 and 2 under the cameras (fx, fy, cx, cy, bf) of either side"""
    return (P.view_init(*cam1[:4], W, H, POSE1[0], POSE1[1], cam1[4]), P.view_init(*cam2[:4], W, H, POSE2[0], POSE2[1], cam2[4]))


def _points(xyz) -> np.ndarray:
    pts = np.zeros(len(xyz), P.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["nz"], pts["min_dist"], pts["max_dist"] = 1.0, 0.1, 100.0
    return pts


def make_pair(rng_seed: int, n: int, n_out: int = 0, nq: int | None = None, nt: int | None = None, s: float = S_TRUE, octaves=(0, 1, 2, 3),
              same_point: bool = False, scatter: bool = True, spread: float = 1.0, cam1=CAM, cam2=CAM, noise: float = 0.0):
    """n correspondences of which the last n_out (in correspondence order) are gross outliers, over nq query and nt train rows ->
    dict view1 view2 q_xyz q_kp t_xyz t_kp idx (int32 [nq]) rows (the query rows of the correspondences, ascending) inlier_rows;
    spread narrows the scene about the optical axis of keyframe 2; cam1, cam2: the cameras of the two views; noise: the deviation of
    Gaussian noise on the coordinates of the correspondences' query points (world units; drawn last, so that the scene without it is
    unchanged).  The scene itself does not depend on the cameras: an exact correspondence has no reprojection error under any"""
    rng = np.random.Generator(np.random.PCG64(0x5130000 + rng_seed))
    nq = n if nq is None else nq
    nt = n if nt is None else nt
    assert nq >= n and nt >= n
    z = rng.uniform(3.0, 9.0, n)
    x2 = np.stack([rng.uniform(-0.5, 0.5, n) * spread * z, rng.uniform(-0.35, 0.35, n) * spread * z, z], axis=1)
    if same_point:
        x2[:] = x2[0]
    r12 = rodrigues(AXIS, ANGLE)
    x1 = s * (x2 @ r12.T) + T_TRUE
    if n_out:  # a gross outlier sees some other place of the scene in keyframe 1
        zo = rng.uniform(3.0, 9.0, n_out)
        x1[n - n_out:] = np.stack([rng.uniform(-0.5, 0.5, n_out) * spread * zo, rng.uniform(-0.35, 0.35, n_out) * spread * zo, zo], axis=1)
    w1 = (x1 - np.asarray(POSE1[1])) @ POSE1[0]  # R^T (X - t), row vectors
    w2 = (x2 - np.asarray(POSE2[1])) @ POSE2[0]
    rows = np.sort(rng.choice(nq, n, replace=False)) if scatter else np.arange(n)
    cols = rng.permutation(nt)[:n] if scatter else np.arange(n)
    order = rng.permutation(n) if n_out else np.arange(n)  # the outliers are not the last correspondences
    q_xyz, t_xyz = _points(rng.uniform(-5, 5, (nq, 3)) + [0, 0, 8.0]), _points(rng.uniform(-5, 5, (nt, 3)) + [0, 0, 8.0])
    q_xyz[rows], t_xyz[cols] = _points(w1[order]), _points(w2[order])
    q_kp = G.kp_rows(np.zeros(nq, f32), np.zeros(nq, f32), octave=rng.choice(octaves, nq))
    t_kp = G.kp_rows(np.zeros(nt, f32), np.zeros(nt, f32), octave=rng.choice(octaves, nt))
    idx = np.full(nq, -1, np.int32)
    idx[rows] = cols
    if noise:
        moved = np.stack([q_xyz[n][rows] for n in "xyz"], 1).astype(np.float64) + rng.normal(0.0, noise, (n, 3))
        q_xyz["x"][rows], q_xyz["y"][rows], q_xyz["z"][rows] = moved[:, 0], moved[:, 1], moved[:, 2]
    v1, v2 = views(cam1, cam2)
    return dict(view1=v1, view2=v2, q_xyz=q_xyz, q_kp=q_kp, t_xyz=t_xyz, t_kp=t_kp, idx=idx, q_skip=None, t_skip=None, rows=rows,
                inlier_rows=np.sort(rows[order < n - n_out]))


def _case(name, expect_state, pair_kw, **params):
    p = dict(chi2=9.210, min_inliers=20, max_iterations=40, fix_scale=False, seed=0)
    p.update(params)
    return dict(name=name, expect_state=expect_state, pair_kw=pair_kw, params=p)


# the table of the issue; every case fits ROWS rows
CASES = [
    _case("state 0: 60 correspondences, 24 gross outliers", 0, dict(rng_seed=1, n=60, n_out=24, nq=64, nt=64), seed=1),
    _case("boundary: 21 correspondences over min_inliers 20", 0, dict(rng_seed=2, n=21, nq=40, nt=30), seed=2),
    _case("boundary: 20 correspondences at min_inliers 20", 2, dict(rng_seed=3, n=20, nq=40, nt=30), seed=3),
    _case("state 2: 40 correspondences, 20 outliers, 8 iterations", 2, dict(rng_seed=4, n=40, n_out=20, nq=64, nt=50), seed=4, max_iterations=8),
    _case("smallest: 3 correspondences, min_inliers 2", 0, dict(rng_seed=5, n=3, nq=9, nt=5), seed=5, min_inliers=2),
    _case("state 1: 19 correspondences under min_inliers 20", 1, dict(rng_seed=6, n=19, nq=33, nt=64), seed=0),
    _case("state 1: 2 correspondences, min_inliers 0", 1, dict(rng_seed=7, n=2, nq=8, nt=8), seed=0, min_inliers=0),
    _case("fix_scale on a scene of scale 1", 0, dict(rng_seed=8, n=30, n_out=6, nq=64, nt=64, s=1.0), seed=3, fix_scale=True, min_inliers=10),
    _case("degenerate: every correspondence is one point", 2, dict(rng_seed=9, n=30, nq=64, nt=64, same_point=True), seed=0, min_inliers=5),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_pair(k: int):
    return make_pair(**CASES[k]["pair_kw"])


def solve_pair(pr, params, pair: int = 0, scale=None, status: int = 0):
    return S.solve(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["q_skip"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["t_skip"], pr["idx"],
                   PC.scale() if scale is None else scale, pair=pair, status=status, **params)


@functools.lru_cache(maxsize=None)
def reference(k: int, pair: int = 0):
    """-> (result record, flags, counts) of case k run as pair number `pair` of a call"""
    return solve_pair(case_pair(k), CASES[k]["params"], pair)


def corr_of(pr, chi2=9.210, scale=None):
    return S.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["q_skip"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["t_skip"], pr["idx"],
                             PC.scale() if scale is None else scale, chi2)


# ---- odd cameras: three pairs per call under CC.SIM3_PAIR_CAMERAS, noisy query points -------------------------------------------------------
# Without noise an inlier has no error under any camera and a gross outlier a huge one under every camera: the counts do not depend
# on the views.  At a deviation of 0.02 (about 1.7 px at the scene's depths) they do, and every pair still ends in state 0 at every
# min_inliers of CAMERA_MIN_INLIERS.  The result holds the first hypothesis above min_inliers: three values make it depend on more
# of the counts (tests/test_sim3_ref.py asserts that every mix-up of camera_cases changes the bytes of one call at least)
CAMERA_NOISE = 0.02
CAMERA_PAIR = dict(n=60, n_out=12, nq=ROWS, nt=ROWS)
CAMERA_MIN_INLIERS = (20, 30, 38)


def camera_params(min_inliers: int):
    return dict(chi2=9.210, min_inliers=min_inliers, max_iterations=40, fix_scale=False, seed=1)


@functools.lru_cache(maxsize=None)
def camera_pairs(cams=CC.SIM3_PAIR_CAMERAS):
    """pair b is its own noisy scene under the cameras cams[b] = (camera of view 1, camera of view 2)"""
    return [make_pair(90 + b, cam1=c1, cam2=c2, noise=CAMERA_NOISE, **CAMERA_PAIR) for b, (c1, c2) in enumerate(cams)]


def with_cameras(pr, cam1, cam2):
    """the pair seen through other cameras: the points stay, the views change"""
    v1, v2 = views(cam1, cam2)
    return dict(pr, view1=v1, view2=v2)


@functools.lru_cache(maxsize=None)
def camera_reference(min_inliers: int):
    return [solve_pair(pr, camera_params(min_inliers), b) for b, pr in enumerate(camera_pairs())]


CAMERA_BATCH = ["synth_t0", "synth_t1", "synth_t2"]
CAMERA_BATCH_SRC = [-1, 0, 0]


def frame_views(cams):
    """the views of the batch: frame 0 is keyframe 2 of both pairs, frames 1 and 2 are their keyframes 1"""
    return [views(cams[1], cams[0])[1], views(cams[1], cams[0])[0], views(cams[2], cams[0])[0]]


@functools.lru_cache(maxsize=None)
def camera_batch():
    """the batch form: frames 1 and 2 train on frame 0, each frame under its own camera (CC.SIM3_FRAME_CAMERAS).  Two noisy scenes over
    the keypoints of three extracted frames (their octaves are the frames' own): pair 1's train rows are the first half of frame
    0's rows, pair 2's the second half.  -> (keypoints of the frames, xyz [3][rows], idx [3][rows], views)"""
    kps = [G.features(name)[0] for name in CAMERA_BATCH]
    rows = max(len(k) for k in kps)
    half = len(kps[0]) // 2
    cams = CC.SIM3_FRAME_CAMERAS
    xyz, idx = np.zeros((3, rows), P.MAP_POINT_DTYPE), np.full((3, rows), -1, np.int32)
    for b in (1, 2):
        pr = make_pair(94 + b, 60, 12, len(kps[b]), half, cam1=cams[b], cam2=cams[0], noise=CAMERA_NOISE)
        xyz[b, :len(kps[b])], xyz[0, (b - 1) * half:b * half] = pr["q_xyz"], pr["t_xyz"]
        idx[b, :len(kps[b])] = np.where(pr["idx"] >= 0, pr["idx"] + (b - 1) * half, -1)
    return kps, xyz, idx, frame_views(cams)


def batch_pair(b: int, frame_views_=None):
    """pair b of the batch as sim3_ref reads it, under the batch's views or others"""
    kps, xyz, idx, vs = camera_batch()
    vs = vs if frame_views_ is None else frame_views_
    t = CAMERA_BATCH_SRC[b]
    nq, nt = len(kps[b]), len(kps[t]) if t >= 0 else 0
    return dict(view1=vs[b], view2=vs[max(t, 0)], q_xyz=xyz[b, :nq], q_kp=kps[b], t_xyz=xyz[max(t, 0), :nt], t_kp=kps[max(t, 0)][:nt], idx=idx[b, :nq],
                q_skip=None, t_skip=None)


def random_triples(rng, n: int):
    """well-spread random triples in both cameras, unrelated: Horn's least-squares answer, not an exact fit"""
    return rng.normal(0, 2, (n, 3, 3)).astype(f32) + f32([0, 0, 6]), rng.normal(0, 2, (n, 3, 3)).astype(f32) + f32([0, 0, 6])


def shortest_side_fraction(tri) -> float:
    """the shortest side of the triangle over its longest"""
    d = [np.linalg.norm(np.asarray(tri[a], np.float64) - np.asarray(tri[b], np.float64)) for a, b in ((0, 1), (1, 2), (2, 0))]
    return min(d) / max(d)


# ---- the loop-closing chain: BoW match -> Sim3 RANSAC -> Scw -> the candidate check's projection search ----------------------------------
CHAIN_ROWS = 64
CHAIN_SIM3 = dict(chi2=9.210, min_inliers=20, max_iterations=64, fix_scale=False, seed=4)
CHAIN_BOW = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=0)


@functools.lru_cache(maxsize=None)
def chain_scene():
    """make_pair's scene narrowed so that keyframe 1 sees all of it, with what the other stages read: keypoints of keyframe 1 on the
    projections of its map points, descriptors (a correspondence's two rows a few bits apart, every other couple about 128), nodes (a
    correspondence's two rows share one; an unmatched train row has a node no query has), and for the map points of keyframe 2 a
    viewing direction and distance range under which the candidate check predicts level 1"""
    rng = np.random.Generator(np.random.PCG64(0xC4A1))
    pr = dict(make_pair(80, 48, 8, CHAIN_ROWS, CHAIN_ROWS, octaves=(0, 1), spread=0.3))
    c = corr_of(pr)
    nq = nt = CHAIN_ROWS
    q_kp = G.kp_rows(rng.uniform(20, W - 20, nq).astype(f32), rng.uniform(20, H - 20, nq).astype(f32), octave=pr["q_kp"]["octave"])
    q_kp["x"][c["rows"]], q_kp["y"][c["rows"]] = c["u1"], c["v1"]
    t_kp = G.kp_rows(rng.uniform(20, W - 20, nt).astype(f32), rng.uniform(20, H - 20, nt).astype(f32), octave=pr["t_kp"]["octave"])
    t_desc = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q_desc = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    q_desc[c["rows"]] = PC.desc_near(rng, t_desc[c["cols"]])
    q_node, t_node = (np.arange(nq) % 4).astype(np.int32), np.full(nt, 5, np.int32)
    t_node[c["cols"]] = q_node[c["rows"]]
    # the camera centre of keyframe 1 in keyframe 2's world under the scene's Sim3, and the distance range of every map point
    r12, (r2, t2) = rodrigues(AXIS, ANGLE), POSE2
    ow = np.asarray(r2).T @ (-(r12.T @ T_TRUE) / S_TRUE - np.asarray(t2))
    t_xyz = pr["t_xyz"].copy()
    dist = np.linalg.norm(np.stack([t_xyz[n] for n in "xyz"], 1).astype(np.float64) - ow, axis=1)
    t_xyz["max_dist"], t_xyz["min_dist"] = 1.1 * dist, 0.1
    pr.update(q_kp=q_kp, t_kp=t_kp, t_xyz=t_xyz, q_desc=q_desc, t_desc=t_desc, q_node=q_node, t_node=t_node)
    return pr


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the chain on the references -> (bow match, sim3 (result, flags, counts), view or None, fusion match or None)"""
    import bow_ref
    import fuse_ref
    pr = chain_scene()
    bow = bow_ref.match(pr["q_kp"], pr["q_desc"], pr["q_node"], pr["t_kp"], pr["t_desc"], pr["t_node"], **CHAIN_BOW)
    sim3 = solve_pair(dict(pr, idx=bow[0]), CHAIN_SIM3, 0)
    if sim3[0]["state"] != 0:
        return bow, sim3, None, None
    srcw, t = S.to_scw(sim3[0], POSE2[0], POSE2[1])
    view = fuse_ref.view_sim3(F, F, CX, CY, W, H, srcw, t, 0.0)
    fuse = fuse_ref.match(view, pr["t_xyz"], pr["t_desc"], pr["q_kp"], pr["q_desc"], PC.scale(), **fuse_ref.CANDIDATE_CHECK)
    return bow, sim3, view, fuse
