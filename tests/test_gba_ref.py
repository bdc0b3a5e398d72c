"""The global bundle adjustment on the CPU: the ABI surface, the host twin (ss_global_ba_host, the text the kernels compile) against the
reference (tests/gba_ref.py) bit for bit on the shared cases, the ladders and the single cases, the liveness of the cases, the
reference against an independent optimiser that forms no Schur complement, against tests/ba_ref.py inside its limits and against the
ground truth, the refused arguments with their messages and the steps under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cases as BC
import ba_ref as BR
import gba_cases as GC
import gba_ref as GR
import pose_cases as PO
import pose_ref as PR
import proj_cases as PC
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
# Ten times the largest deviation seen over the shared cases (DESIGN.md section 29 holds the table): head-room for inputs not sampled.
# (a) one step of the reference with its PCG driven to pcg_tol 1e-12 against numpy.linalg.solve on the damped un-reduced normal
#     equations, dc and dp relative to the step's largest entry or to 1, whichever is larger.  Without a fixed keyframe only the
#     damping holds the seven gauge directions, both solves lose the digits the conditioning costs, and the case has bounds of its own
STEP_BOUND_DC = 6.3e-12    # seen: 6.25e-13 (two_fixed_disagree)
STEP_BOUND_DP = 5.9e-11    # seen: 5.86e-12 (two_fixed_disagree)
FREE_BOUND_DC = 1.2e-8     # seen: 1.13e-09 (no_fixed)
FREE_BOUND_DP = 1.4e-9     # seen: 1.36e-10 (no_fixed)
# (b) end poses and points against ba_ref.optimise under the same schedule, the PCG at pcg_tol 1e-12 and 256 iterations, absolute
BA_BOUND_POSE = 1.7e-12    # seen: 1.68e-13 (noise_free)
BA_BOUND_POINT = 1.2e-10   # seen: 1.14e-11 (two_fixed_disagree)
# (c) the noise-free case under the default schedule against the ground truth, absolute: the keypoints are float32
TRUTH_BOUND_POSE = 2.3e-6  # seen: 2.26e-07
TRUTH_BOUND_POINT = 4.5e-5 # seen: 4.41e-06
NAMES = ("ss_global_ba_host", "ss_global_ba_obs_from_idx_host", "ss_global_ba_device", "ss_global_ba")


@pytest.fixture(autouse=True)
def _the_feature_is_there():
    """every test of this file, those of the reference alone included, is a test of the feature: without its symbols it fails here"""
    lib = binding.load()
    for n in NAMES:
        assert hasattr(lib, n), n


def _host(pr, params, scale=None):
    p = dict(GR.DEFAULTS, **params)
    return binding.global_ba_host(pr["views"], pr["start"], pr["fixed"], PC.scale() if scale is None else scale, pr["points"], pr["obs"],
                                  binding.gba_params(**p), pr.get("skip"))


def _same(tag, got, want):
    for name, g, w in zip(("poses", "xyz", "point flags", "observation flags"), got[:4], want[:4]):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{tag}: {name} differ at {np.argwhere(g != w)[:4].tolist()}"
    for name in GR.RESULT_DTYPE.names:
        assert got[4][name].tobytes() == want[4][name].tobytes(), f"{tag}: result.{name} {got[4][name]} != {want[4][name]}"


def _starts(pr):
    return np.array([list(R) + list(t) for R, t in (PR.start_pose(s)[:2] for s in pr["start"])])


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    lib = binding.load()
    for n in NAMES:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    assert lib.ss_abi_version() == 5
    assert C.sizeof(binding.GbaParams) == 104 and binding.GbaParams.pcg_tol.offset == 48 and binding.GbaParams.n_rounds.offset == 56
    assert binding.GbaParams.pcg_iterations.offset == 88 and binding.GbaParams.reserved.offset == 92
    assert binding.GBA_OBS_DTYPE == GR.OBS_DTYPE and GR.OBS_DTYPE.itemsize == 24 and binding.GBA_PROBLEM_DTYPE.itemsize == 32
    assert binding.GBA_RESULT_DTYPE == GR.RESULT_DTYPE and GR.RESULT_DTYPE.itemsize == 104
    assert GR.RESULT_DTYPE.fields["state"][1] == 24 and GR.RESULT_DTYPE.fields["steps"][1] == 52 and GR.RESULT_DTYPE.fields["pcg_iterations"][1] == 84
    for name, value in (("SS_GBA_MAX_KF", 16384), ("SS_GBA_MAX_POINTS", 1048576), ("SS_GBA_MAX_OBS", 4194304)):
        assert f"#define {name} {value}" in text and getattr(binding, name) == value
    assert binding.SS_GBA_MAX_KF == binding.SS_GRAPH_MAX_KF
    p = binding.gba_params()
    got = {k: (tuple(getattr(p, k)) if k == "iterations" else getattr(p, k)) for k in GR.DEFAULTS}
    assert got == {k: (int(v) if isinstance(v, bool) else v) for k, v in GR.DEFAULTS.items()}
    assert (p.n_rounds, p.iterations[0], p.robust_rounds) == (1, 10, 1)  # upstream's global schedule


# ---- the host twin against the reference, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(GC.CASES)), ids=GC.CASE_NAMES)
def test_host_twin_equals_the_reference_on_the_shared_cases(k):
    _same(GC.CASE_NAMES[k], _host(GC.case_problem(k), GC.CASES[k]["params"]), GC.reference(k))


@pytest.mark.parametrize("n_free", GC.KF_LADDER)
def test_host_twin_equals_the_reference_over_the_keyframe_ladder(n_free):
    pr = GC.kf_ladder_problem(n_free)
    want = GC.solve(pr, GC.LADDER)
    assert want[4]["state"] == 0 and want[4]["n_free"] == n_free and want[4]["n_fixed"] == 1 and want[4]["n_stereo"] > 0 and want[4]["accepted"].sum() > 0
    _same(f"{n_free} free keyframes", _host(pr, GC.LADDER), want)


@pytest.mark.parametrize("n_points", GC.POINT_LADDER)
def test_host_twin_equals_the_reference_over_the_point_ladder(n_points):
    pr = GC.point_ladder_problem(n_points)
    want = GC.solve(pr, GC.LADDER)
    assert want[4]["state"] == (1 if n_points == 0 else 0) and len(want[2]) == n_points and (n_points < 3 or want[4]["accepted"].sum() > 0)
    _same(f"{n_points} points", _host(pr, GC.LADDER), want)


@pytest.mark.parametrize("length", GC.LIST_LADDER)
def test_host_twin_equals_the_reference_over_the_list_lengths(length):
    pr = GC.list_ladder_problem(length)
    assert np.bincount(pr["obs"]["kf"], minlength=3).tolist() == [length] * 3
    want = GC.solve(pr, GC.LADDER)
    assert want[4]["state"] == 0 and want[4]["n_obs"] == 3 * length and want[4]["accepted"].sum() > 0
    _same(f"lists of {length}", _host(pr, GC.LADDER), want)


def test_a_point_seen_by_one_two_and_sixty_five_keyframes():
    pr = GC.seen_by_problem()
    assert np.bincount(pr["obs"]["point"])[:3].tolist() == [1, 2, 65]
    want = GC.solve(pr, GC.LADDER)
    assert want[2][:3].tolist() == [1, 0, 0] and want[4]["state"] == 0 and want[4]["accepted"].sum() > 0
    assert want[1][0].tolist() == [float(pr["points"][n][0]) for n in "xyz"] and want[1][2].tolist() != [float(pr["points"][n][2]) for n in "xyz"]
    _same("seen by 1, 2, 65", _host(pr, GC.LADDER), want)


def test_a_problem_the_local_bundle_adjustment_refuses():
    pr = GC.beyond_local_problem()
    d = pr["dense"]
    with pytest.raises(binding.OrbError):
        binding.local_ba_host(d["views"], d["start"], 33, PC.scale(), d["points"], d["kp"], d["idx"], binding.ba_params(), d["n_kp"])
    want = GC.solve(pr, GC.LADDER)
    assert want[4]["state"] == 0 and (want[4]["n_free"], want[4]["n_fixed"]) == (33, 32) and want[4]["accepted"].sum() > 0
    _same("65 keyframes, 33 free", _host(pr, GC.LADDER), want)


def test_the_record_order_is_free():
    """the table shuffled gives the same bytes, the observation flags in the table's order"""
    k = GC.CASE_NAMES.index("stereo_mixed")
    pr, params, want = GC.case_problem(k), GC.CASES[k]["params"], GC.reference(k)
    order = np.random.Generator(np.random.PCG64(77)).permutation(len(pr["obs"]))
    for tag, run in (("reference", GC.solve), ("host twin", _host)):
        got = run(dict(pr, obs=pr["obs"][order]), params)
        assert got[3].tobytes() == want[3][order].tobytes(), tag
        _same(tag, got[:3] + (got[3][np.argsort(order)],) + got[4:], want)


def test_free_keyframes_nobody_sees_stay_put():
    """keyframe 0 is free without a record, keyframe 1 is free and sees inactive points only: both keep their orthonormalised start,
    the others move, and the problem is state 0 under any lambda > 0; under lambda 0 the first pivot ends it in state 2"""
    pr = GC.lonely_problem()
    seen = np.bincount(pr["obs"]["kf"], minlength=6)
    assert seen[0] == 0 and seen[1] > 0 and (pr["obs"]["point"][pr["obs"]["kf"] == 1] < 10).all() and (np.bincount(pr["obs"]["point"], minlength=90)[:10] <= 1).all()
    for lam in (1e-4, 1e-300, 1e6):
        want = GC.solve(pr, dict(GC.LADDER, lambda_=lam, lambda_min=0.0))
        _same(f"lambda {lam}", _host(pr, dict(GC.LADDER, lambda_=lam, lambda_min=0.0)), want)
        assert want[4]["state"] == 0 and (want[2][:10] == 1).all()
        assert want[0][:2].tobytes() == _starts(pr)[:2].tobytes()
        assert lam > 1.0 or want[0][2].tobytes() != _starts(pr)[2].tobytes()
    want = GC.solve(pr, dict(GC.LADDER, lambda_=0.0, lambda_min=0.0))
    _same("lambda 0", _host(pr, dict(GC.LADDER, lambda_=0.0, lambda_min=0.0)), want)
    assert want[4]["state"] == 2 and want[4]["steps"].sum() == 0 and want[0].tobytes() == _starts(pr).tobytes()


def test_failure_states_on_the_reference_and_the_host_twin():
    """every keyframe fixed: state 1; a NaN point is no point; a start that is not finite: state 2 and the identity; a rolled start:
    state 4; points behind the cameras take no part and are classified out; one PCG iteration per step"""
    k = GC.CASE_NAMES.index("noisy_outliers")
    base, params = GC.case_problem(k), GC.CASES[k]["params"]
    all_fixed = dict(base, fixed=np.ones(8, np.uint8))
    nan_point = dict(base, points=base["points"].copy())
    nan_point["points"]["y"][33] = np.nan
    nan_start = dict(base, start=base["start"].copy())
    nan_start["start"][3, 4] = np.nan
    rolled = dict(base, start=base["start"].copy())
    rolled["start"][0] = PO.start_of(PC.rot(0.0, 0.0, 3.0) @ base["start"][0][:9].reshape(3, 3), base["start"][0][9:])
    behind = dict(base, points=base["points"].copy())
    behind["points"]["z"][5:15] = -behind["points"]["z"][5:15]
    for name, pr, p, state in (("all fixed", all_fixed, params, 1), ("a NaN point", nan_point, params, 0), ("a NaN start", nan_start, params, 2),
                               ("a rolled start", rolled, params, 4), ("behind", behind, params, 0), ("one PCG iteration", base, dict(params, pcg_iterations=1), 0)):
        want = GC.solve(pr, p)
        assert want[4]["state"] == state, (name, want[4])
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and all(np.isfinite(want[4][n]) for n in ("lambda_", "cost_before", "cost_after")), name
        _same(name, _host(pr, p), want)
    want = GC.solve(all_fixed, params)
    assert want[4]["steps"].sum() == 0 and (want[4]["n_free"], want[4]["n_fixed"]) == (0, 8) and want[0].tobytes() == _starts(base).tobytes()
    want = GC.solve(nan_point, params)
    assert want[2][33] == 2 and (want[3][base["obs"]["point"] == 33] == 2).all() and (want[1][33] == 0.0).all()
    want = GC.solve(nan_start, params)
    assert want[0][3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and want[4]["steps"].sum() == 0
    want = GC.solve(rolled, params)
    assert want[4]["steps"].sum() < 5 and want[4]["pcg_iterations"] > 0  # the step that is too large is not counted, its PCG iterations are
    want = GC.solve(behind, params)
    hit = (base["obs"]["point"] >= 5) & (base["obs"]["point"] < 15)
    assert (want[3][hit] == 1).all() and (want[2][5:15] == 1).all()
    want = GC.solve(base, dict(params, pcg_iterations=1))
    assert want[4]["pcg_iterations"] == want[4]["steps"].sum() == 5 and want[4]["accepted"].sum() > 0


def test_obs_from_idx_equals_the_reference():
    d = GC.case_problem(GC.CASE_NAMES.index("stereo_mixed"))["dense"]
    got = binding.global_ba_obs_from_idx(d["kp"], d["idx"], d["n_kp"], d["right"])
    want = GR.obs_from_idx(d["kp"], d["idx"], d["n_kp"], d["right"])
    assert got.tobytes() == want.tobytes() and len(got) == (d["idx"] >= 0).sum()
    key = got["point"].astype(np.int64) * 1000 + got["kf"]
    assert (np.diff(key) > 0).all() and (got["right"] > 0).any()
    r = BC.row_count_problem()  # counts below the rows, junk entries: no record for either
    got = binding.global_ba_obs_from_idx(r["kp"], r["idx"], r["n_kp"])
    assert got.tobytes() == GR.obs_from_idx(r["kp"], r["idx"], r["n_kp"]).tobytes() and (got["right"] == -1).all()
    assert len(got) == ((r["idx"] >= 0) & (r["idx"] < r["n_kp"][:, None])).sum()
    lib = binding.load()
    assert lib.ss_global_ba_obs_from_idx_host(None, None, None, 2, 4, None, 3, None, 0) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_global_ba_obs_from_idx_host(None, None, None, 0, 4, None, 3, None, 0) == 0


# ---- liveness -----------------------------------------------------------------------------------------------------------------------
def test_shared_cases_are_live():
    """on the reference: the PCG leaves by each of its three exits; a step is rejected, lambda rises and the next step starts from
    the state before; the classification removes every planted outlier; no point freezes"""
    exits, rejected = set(), False
    for k, case in enumerate(GC.CASES):
        pr, p = GC.case_problem(k), case["params"]
        poses, xyz, pflag, oflag, res, trace = GC.reference(k)
        steps = [t for t in trace if t["kind"] == "step"]
        assert res["state"] == 0 and res["n_frozen_max"] == 0 and res["n_obs"] == len(pr["obs"]) and res["accepted"].sum() > 0
        assert (oflag[pr["planted"]] == 1).all() and [t for t in trace if t["kind"] == "classify"][0]["removed"] >= pr["planted"].sum()
        assert (res["n_stereo"] > 0) == bool(p["check_right"]) and res["n_free"] == (pr["fixed"] == 0).sum()
        assert res["steps"].sum() == len(steps) and res["pcg_iterations"] == sum(t["pcg"] for t in steps)
        exits |= {t["left"] for t in steps}
        for a, b in zip(steps, steps[1:]):
            if not a["accepted"] and a["round"] == b["round"]:
                assert b["lam"] == a["lam"] * p["lambda_factor"] and b["X"].tobytes() == a["X"].tobytes() and b["R"].tobytes() == a["R"].tobytes()
                rejected = True
    assert rejected and "tolerance" in exits
    trace = []
    GC.solve(GC.case_problem(1), dict(GC.SHORT, pcg_iterations=2), trace=trace)
    exits |= {t["left"] for t in trace if t["kind"] == "step"}
    # a problem whose only free keyframe nobody sees: r = 0, so p.q is not > 0 before the first iteration
    trace = []
    lonely = GC.lonely_problem()
    want = GC.solve(dict(lonely, fixed=np.array([0, 1, 1, 1, 1, 1], np.uint8)), GC.LADDER, trace=trace)
    assert want[4]["pcg_iterations"] == 0 and want[4]["accepted"].sum() > 0 and want[1].tobytes() != GC.solve(lonely, dict(GC.LADDER, iterations=(1, 1, 0, 0)))[1].tobytes()
    exits |= {t["left"] for t in trace if t["kind"] == "step"}
    assert exits == {"cap", "curvature", "tolerance"}


def test_the_frozen_point_freezes_and_only_it():
    pr = BC.frozen_problem()
    g = dict(views=pr["views"], start=pr["start"], fixed=np.array([0, 1, 1], np.uint8), points=pr["points"], obs=GR.obs_from_idx(pr["kp"], pr["idx"], pr["n_kp"]), skip=None)
    params = dict(lambda_=0.0, lambda_min=0.0, n_rounds=1, iterations=(3, 0, 0, 0))
    trace = []
    want = GC.solve(g, params, trace=trace)
    steps = [t for t in trace if t["kind"] == "step"]
    assert want[4]["state"] == 0 and want[4]["n_frozen_max"] == 1 and len(steps) > 0
    for t in steps:
        assert t["active"][0] and not t["solved"][0] and t["solved"][1:].all() and (t["dp"][0] == 0.0).all()
    assert want[1][0].tolist() == [0.0, 0.0, 4.0] and want[2][0] == 0
    _same("frozen", _host(g, params), want)
    assert GC.solve(g, dict(params, lambda_=1e-4))[4]["n_frozen_max"] == 0


# ---- the rule itself -------------------------------------------------------------------------------------------------------------------
def _skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def _full_step(pr, tab, o, cams, step, p):
    """one damped step on the un-reduced normal equations of the state `step` was linearised at: the full Jacobian stacked row by
    row, numpy.linalg.solve, no Schur complement -> (dc [n_kf][6] with zeros for fixed keyframes, dp [P][3] with zeros where a point
    does not move)"""
    free = np.flatnonzero(pr["fixed"] == 0)
    kcol = {int(k): 6 * j for j, k in enumerate(free)}
    pcol = {int(i): 6 * len(free) + 3 * j for j, i in enumerate(np.flatnonzero(step["solved"]))}
    n = 6 * len(free) + 3 * len(pcol)
    rows, rhs, wts = [], [], []
    for s in np.flatnonzero(step["lin"]):
        k, i = int(tab.kf[s]), int(tab.pt[s])
        cam = cams[k]
        fx, fy, cx, cy, bf = (float(cam[m]) for m in ("fx", "fy", "cx", "cy", "bf"))
        R, t = step["R"][k].reshape(3, 3), step["t"][k]
        pc = R @ step["X"][i] + t
        x, y, z = pc
        r = [o["u"][s] - (fx * x / z + cx), o["v"][s] - (fy * y / z + cy)]
        Jp = [[fx / z, 0.0, -fx * x / z ** 2], [0.0, fy / z, -fy * y / z ** 2]]
        if o["stereo"][s]:
            r.append(o["ur"][s] - (fx * x / z + cx - bf / z))
            Jp.append([fx / z, 0.0, -(fx * x - bf) / z ** 2])
        r, Jp = np.array(r), np.array(Jp)
        e2 = o["w"][s] * float(r @ r)
        d = np.sqrt(p["chi2_stereo"] if o["stereo"][s] else p["chi2_mono"])
        w = o["w"][s] * d / np.sqrt(e2) if step["robust"] and e2 > d * d else o["w"][s]
        J = np.zeros((len(r), n))
        if k in kcol:
            J[:, kcol[k]:kcol[k] + 6] = -Jp @ np.hstack([-_skew(pc), np.eye(3)])
        if i in pcol:
            J[:, pcol[i]:pcol[i] + 3] = -Jp @ R
        rows.append(J), rhs.append(r), wts.append(np.full(len(r), w))
    J, r, w = np.vstack(rows), np.concatenate(rhs), np.concatenate(wts)
    H = J.T @ (w[:, None] * J)
    H[np.diag_indices(n)] += float(step["lam"]) * (1.0 + np.diag(H))
    delta = np.linalg.solve(H, -(J.T @ (w * r)))
    dc, dp = np.zeros((len(pr["fixed"]), 6)), np.zeros((len(step["X"]), 3))
    for k, col in kcol.items():
        dc[k] = delta[col:col + 6]
    for i, col in pcol.items():
        dp[i] = delta[col:col + 3]
    return dc, dp


TIGHT = dict(pcg_tol=1e-12, pcg_iterations=256)


@pytest.mark.parametrize("k", range(len(GC.CASES)), ids=GC.CASE_NAMES)
def test_reference_steps_against_the_unreduced_normal_equations(k):
    """(a): every step of the reference, its PCG driven to pcg_tol 1e-12, from the state it was linearised at"""
    pr, p = GC.case_problem(k), dict(GC.CASES[k]["params"], **TIGHT)
    trace = []
    GC.solve(pr, p, trace=trace)
    tab = GR.Tables(len(pr["views"]), len(pr["points"]), pr["obs"])
    _, _, o = GR.gather(tab, PC.scale(), pr["points"], pr.get("skip"), p["check_right"])
    cams = [PR.camera(v, p["chi2_mono"], p["chi2_stereo"]) for v in pr["views"]]
    worst_dc = worst_dp = 0.0
    steps = [t for t in trace if t["kind"] == "step"]
    for step in steps:
        dc, dp = _full_step(pr, tab, o, cams, step, p)
        worst_dc = max(worst_dc, np.abs(dc - step["dc"]).max() / max(1.0, np.abs(step["dc"]).max()))
        worst_dp = max(worst_dp, np.abs(dp - step["dp"]).max() / max(1.0, np.abs(step["dp"]).max()))
    print(f"{GC.CASE_NAMES[k]}: {len(steps)} steps, dc {worst_dc:.3g} dp {worst_dp:.3g}")
    held = bool(pr["fixed"].any())
    assert len(steps) > 0 and worst_dc <= (STEP_BOUND_DC if held else FREE_BOUND_DC) and worst_dp <= (STEP_BOUND_DP if held else FREE_BOUND_DP)


@pytest.mark.parametrize("k", [k for k, c in enumerate(GC.CASES) if c["name"] != "no_fixed"], ids=[n for n in GC.CASE_NAMES if n != "no_fixed"])
def test_reference_against_the_local_bundle_adjustment_inside_its_limits(k):
    """(b): the same problem through tests/ba_ref.py (a dense Cholesky of the reduced system) under the same schedule"""
    pr = GC.case_problem(k)
    p = {n: v for n, v in GC.CASES[k]["params"].items() if n in BR.DEFAULTS}
    d = pr["dense"]
    n_free = int((pr["fixed"] == 0).sum())
    assert (pr["fixed"][:n_free] == 0).all() and n_free < len(pr["fixed"]) <= 64 and n_free <= 32
    want = BR.optimise(d["views"], pr["start"], n_free, PC.scale(), d["points"], d["kp"], d["idx"], dict(BR.DEFAULTS, **p), d["n_kp"], d.get("skip"), d.get("right"))
    got = GC.solve(pr, dict(GC.CASES[k]["params"], **TIGHT))
    assert got[2].tobytes() == want[2].tobytes() and got[4]["state"] == want[4]["state"] == 0  # near convergence the steps taken may differ: step_eps sees rounding noise
    assert got[3].tobytes() == want[3][pr["obs"]["kf"], pr["obs"]["point"]].tobytes()
    worst_pose, worst_point = np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()
    print(f"{GC.CASE_NAMES[k]}: end poses {worst_pose:.3g} points {worst_point:.3g}")
    assert worst_pose <= BA_BOUND_POSE and worst_point <= BA_BOUND_POINT


def test_noise_free_case_returns_to_the_ground_truth():
    """(c): under the default schedule (one robust round of ten, pcg_tol 1e-2, 64 iterations at the most)"""
    k = GC.CASE_NAMES.index("noise_free")
    pr, p = GC.case_problem(k), GC.CASES[k]["params"]
    assert all(p[n] == GR.DEFAULTS[n] for n in ("n_rounds", "iterations", "robust_rounds", "pcg_tol", "pcg_iterations", "lambda_"))
    poses, xyz, pflag, oflag, res, _ = GC.reference(k)
    truth, txyz = pr["truth"]
    free = pr["fixed"] == 0
    before, after, points = np.abs(pr["start"][free] - truth[free]).max(), np.abs(poses[free] - truth[free]).max(), np.abs(xyz - txyz).max()
    print(f"noise-free: pose error {before:.3g} -> {after:.3g}, point error -> {points:.3g}, cost {res['cost_before']:.3g} -> {res['cost_after']:.3g}")
    assert before > 0.01 and after <= TRUTH_BOUND_POSE and points <= TRUTH_BOUND_POINT and (pflag == 0).all() and (oflag == 0).all()
    assert poses[~free].tobytes() == _starts(pr)[~free].tobytes()


# ---- refused arguments ------------------------------------------------------------------------------------------------------------------
def _refused(message, *args, **kw):
    with pytest.raises(binding.OrbError) as e:
        binding.global_ba_host(*args, **kw)
    assert e.value.code == binding.SS_ERR_INVALID_ARG and message in e.value.message, (message, e.value.message)


def test_refused_arguments_and_their_messages():
    pr = GC.case_problem(1)
    nan = float("nan")
    args = lambda p=None, obs=None, scale=None, **kw: (kw.get("views", pr["views"]), kw.get("start", pr["start"]), kw.get("fixed", pr["fixed"]),  # noqa: E731
                                                       PC.scale() if scale is None else scale, kw.get("points", pr["points"]), pr["obs"] if obs is None else obs,
                                                       p or binding.gba_params())
    for kw, message in ((dict(chi2_mono=0.0), "chi2_mono must be finite and > 0"), (dict(chi2_mono=nan), "chi2_mono"), (dict(chi2_stereo=float("inf")), "chi2_stereo must be"),
                        (dict(lambda_=-1.0), "lambda must be finite and >= 0"), (dict(lambda_=nan), "lambda must"), (dict(lambda_factor=1.0), "lambda_factor must be finite and > 1"),
                        (dict(lambda_min=-1e-9), "lambda_min"), (dict(step_eps=-1e-10), "step_eps"), (dict(pcg_tol=-1e-3), "pcg_tol must be finite and >= 0"),
                        (dict(pcg_tol=nan), "pcg_tol"), (dict(n_rounds=0), "n_rounds must be 1 .. 4"), (dict(n_rounds=5), "n_rounds"),
                        (dict(iterations=(0, 0, 0, 0)), "iterations must be 1 .. 32"), (dict(iterations=(33, 0, 0, 0)), "iterations"), (dict(robust_rounds=-1), "robust_rounds"),
                        (dict(robust_rounds=5), "robust_rounds must be 0 .. 4"), (dict(min_point_obs=0), "min_point_obs must be >= 1"),
                        (dict(pcg_iterations=0), "pcg_iterations must be 1 .. 256"), (dict(pcg_iterations=257), "pcg_iterations"),
                        (dict(reserved=(0, 0, 1)), "reserved fields must be 0"), (dict(reserved=(1, 0, 0)), "reserved")):
        _refused(message, *args(binding.gba_params(**kw)))
    binding.global_ba_host(*args(binding.gba_params(n_rounds=1, iterations=(1, 99, 0, 0), pcg_iterations=2)))  # only the rounds that run are checked
    obs = pr["obs"].copy()
    obs["kf"][7] = 8
    _refused("problem 0: record 7: kf 8 outside 0 .. 7", *args(obs=obs))
    obs["kf"][7] = -1
    _refused("record 7: kf -1 outside", *args(obs=obs))
    obs = pr["obs"].copy()
    obs["point"][9] = 300
    _refused("problem 0: record 9: point 300 outside 0 .. 299", *args(obs=obs))
    obs = pr["obs"].copy()
    obs[11] = obs[3]
    obs["u"][11] += 1.0
    _refused(f"record 11: the pair (kf {obs['kf'][3]}, point {obs['point'][3]}) has a record already", *args(obs=obs))
    for levels in (np.zeros(0, f32), np.ones(17, f32)):
        _refused("no pyramid table", *args(scale=levels))
    big = np.zeros(binding.SS_GBA_MAX_KF + 1, binding.PROJ_VIEW_DTYPE)
    _refused("n_kf 16385 outside 1 .. SS_GBA_MAX_KF (16384)", big, np.zeros((len(big), 12)), np.zeros(len(big), np.uint8), PC.scale(), pr["points"][:0],
             pr["obs"][:0], binding.gba_params())
    _refused("outside 0 .. SS_GBA_MAX_POINTS (1048576) points", pr["views"], pr["start"], pr["fixed"], PC.scale(),
             np.zeros(binding.SS_GBA_MAX_POINTS + 1, binding.MAP_POINT_DTYPE), pr["obs"][:0], binding.gba_params())
    _refused("n_obs 4194305 outside 0 .. SS_GBA_MAX_OBS (4194304)", pr["views"], pr["start"], pr["fixed"], PC.scale(), pr["points"],
             np.zeros(binding.SS_GBA_MAX_OBS + 1, GR.OBS_DTYPE), binding.gba_params())
    lib = binding.load()
    p = binding.gba_params()
    err = C.create_string_buffer(256)
    assert lib.ss_global_ba_host(None, None, None, 2, None, 0, None, None, 0, None, 0, C.byref(p), None, None, None, None, None, err, 256) == binding.SS_ERR_INVALID_ARG
    assert b"pyramid" in err.value
    sc = np.ascontiguousarray(PC.scale(), f32)
    assert lib.ss_global_ba_host(None, None, None, 2, sc.ctypes.data, len(sc), None, None, 0, None, 0, C.byref(p), None, None, None, None, None, err, 256) == binding.SS_ERR_INVALID_ARG
    assert err.value == b"global BA: NULL buffer"
    assert lib.ss_global_ba_host(None, None, None, 2, None, 0, None, None, 0, None, 0, None, None, None, None, None, None, None, 0) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_global_ba_device(None, None, None, None, 1, 1, None, None, 0, None, 0, None, 0, None, C.byref(p), None, None, None, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_global_ba(None, None, None, None, 2, None, None, 0, None, 0, C.byref(p), None, None, None, None, None) == binding.SS_ERR_INVALID_ARG


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/gba_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with the
    environment as it is"""
    exe = str(tmp_path / "gba_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "gba_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
