"""The synthetic scenes and cached references the Sim3 refinement tests share (test infrastructure, plain module).

    make_pair()   sim3_cases.make_pair's scene (a known Sim3, float32 inputs, gross mismatches on request) with what the refinement reads
                  on top: keypoints of both keyframes on the projections of their map points plus Gaussian pixel noise, rounded to
                  float32, and a start model a few pixels off the truth
    model_record() a sim3 result record from (R, t, s) in double, formed as the RANSAC forms it
    CASES         the paths of the rule (tests/test_sim3opt_ref.py asserts on the reference that each is what its name says)
    reference()   sim3opt_ref.optimise of a case, cached
    count_pair()  a pair with exactly n correspondences
    marks_tables() random and adversarial tables for the bookkeeping
"""
from __future__ import annotations

import functools

import numpy as np

import proj_cases as PC
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
              octaves=(0, 1, 2, 3), spread: float = 0.6, fix_scale: bool = False):
    """-> sim3_cases.make_pair's dict with keypoints set and `start`, `outlier_rows` (the query rows of the planted mismatches)"""
    pr = dict(SC.make_pair(rng_seed, n, n_out, nq, nt, s=s, octaves=octaves, spread=spread))
    rng = np.random.Generator(np.random.PCG64(0x0517300 + rng_seed))
    c = S.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale(), 1.0)
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
