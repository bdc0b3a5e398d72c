"""CPU tests of the pose-only optimisation as tests/pose_ref.py states it, and of its C ABI surface: symbols and struct layouts, the
host twin ss_pose_opt_host (the text the kernels compile) against the reference bit for bit, the coefficient table against exact
fractions, the series against the closed form, the monocular rule against oracle/vo_oracle.pose_only, the stereo row against finite
differences, the thresholds from both sides, the liveness of the shared cases, refused arguments, and the stand-alone sanitizer run of
the steps."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import camera_cases as CC
import pose_cases as PCs
import pose_ref as PR
import proj_cases as PC
from oracle import vo_oracle as V
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def _host(fr, params, scale=None):
    p = dict(PR.UPSTREAM, **params)
    return binding.pose_opt_host(fr["view"], fr["start"], PC.scale() if scale is None else scale, fr["points"], fr["kp"], fr["idx"], binding.pose_opt_params(**p),
                                 skip=fr.get("skip"), right=fr.get("right"))


def _same(tag, got, want):
    flags, res = got
    wres, wflags = want
    for name in PR.RESULT_DTYPE.names:
        assert res[name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {res[name]} != {wres[name]}"
    assert np.array_equal(flags, wflags), f"{tag}: flags differ at {np.flatnonzero(flags != wflags)[:8]}"


def test_abi_surface():
    text = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    lib = binding.load()
    for n in ("ss_pose_opt_host", "ss_pose_opt_pairs_device", "ss_pose_opt_batch_device", "ss_pose_opt"):
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    assert C.sizeof(binding.PoseOptParams) == 64
    assert binding.POSE_RESULT_DTYPE == PR.RESULT_DTYPE and PR.RESULT_DTYPE.itemsize == 160 and 160 % 16 == 0
    assert PR.RESULT_DTYPE.fields["cost"][1] == 96 and PR.RESULT_DTYPE.fields["state"][1] == 104 and PR.RESULT_DTYPE.fields["steps"][1] == 124
    p = binding.pose_opt_params()
    assert {k: getattr(p, k) for k in PR.UPSTREAM} == {k: (int(v) if isinstance(v, bool) else v) for k, v in PR.UPSTREAM.items()}


def test_coefficients_are_the_correctly_rounded_reciprocal_factorials():
    """every literal of both tables equals the double next to 1 / n!; the C header and pose_ref.py hold the same literals; the series
    is long enough: the first term left out is below 2^-60 at q = pi^2"""
    assert len(PR.INV_FACT) == 2 * PR.SERIES + 2
    for n, v in enumerate(PR.INV_FACT):
        assert v == float(Fraction(1, math.factorial(n))), n  # Fraction -> float rounds correctly
    text = open(os.path.join(ROOT, "send-slam_amd", "csrc", "ss_pose_steps.h")).read()
    table = text[text.index("#define SS_POSE_INV_FACT"):text.index("/* what a frame's steps read")]
    lits = re.findall(r"0x1\.[0-9a-f]+p[+-]\d+", table)
    assert [float.fromhex(h) for h in lits] == PR.INV_FACT
    assert re.search(r"#define SS_POSE_SERIES (\d+)", text).group(1) == str(PR.SERIES)
    assert float.fromhex(re.search(r"#define SS_POSE_PI2 (\S+)", text).group(1)) == PR.PI2 == float(Fraction(math.pi) ** 2) == math.pi * math.pi
    q = Fraction(PR.PI2)
    for j in (1, 2, 3):
        assert q ** PR.SERIES / math.factorial(2 * PR.SERIES + j) < Fraction(1, 2 ** 60)
    assert q ** (PR.SERIES - 1) / math.factorial(2 * PR.SERIES - 1) > Fraction(1, 2 ** 60)  # one term fewer would not do


# measured on the sweep below: |A - sin(th)/th| 3.1e-16, |B - (1 - cos(th))/q| 1.9e-14, |C - (1 - A)/q| 2.8e-14 for th >= 0.05 (the closed
# forms of B and C cancel: their own error is 1e-16 / q); against the exact 40-term rational sums, over all q: 1.2e-16
SERIES_BOUND = (3.1e-15, 1.9e-13, 2.8e-13)  # ten times the measurement
SERIES_EXACT_BOUND = 1.2e-15


def test_series_against_the_closed_form():
    worst = [0.0, 0.0, 0.0]
    for q in np.linspace(0.0025, PR.PI2, 20001):
        th = math.sqrt(q)
        A, B, Cc = PR.series(q)
        a = math.sin(th) / th
        worst = [max(w, abs(float(v) - e)) for w, v, e in zip(worst, (A, B, Cc), (a, (1.0 - math.cos(th)) / q, (1.0 - a) / q))]
    print("series against the closed form:", worst)
    assert all(w <= b for w, b in zip(worst, SERIES_BOUND)), worst
    exact = 0.0
    for q in (0.0, 1e-20, 1e-8, 1e-3, 0.0025, 0.1, 1.0, 5.0, PR.PI2):
        fq = Fraction(q)
        for j, v in zip((1, 2, 3), PR.series(q)):
            e = sum((-fq) ** k / math.factorial(2 * k + j) for k in range(40))
            exact = max(exact, abs(float(Fraction(float(v)) - e)))
    print("series against exact rational sums:", exact)
    assert exact <= SERIES_EXACT_BOUND
    assert [float(v) for v in PR.series(0.0)] == [1.0, 0.5, PR.INV_FACT[3]]


def test_exponential_is_a_rotation_and_refuses_above_pi():
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(200):
        w = rng.normal(size=3)
        w *= rng.uniform(0, math.pi) / np.linalg.norm(w)
        dR, dt = PR.exp([f64(v) for v in w] + [f64(v) for v in rng.normal(size=3)])
        M = np.array(dR, f64).reshape(3, 3)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(M) - 1) < 1e-14
        th = np.linalg.norm(w)
        assert abs(np.trace(M) - (1 + 2 * math.cos(th))) < 1e-13
    z = [f64(0.0)] * 3
    assert PR.exp([f64(math.pi), f64(0.0), f64(0.0)] + z) is not None  # pi * pi rounds to PI2
    assert PR.exp([f64(np.nextafter(math.pi, 4.0)), f64(0.0), f64(0.0)] + z) is None
    assert PR.exp([f64(2.0), f64(2.0), f64(1.5)] + z) is None
    assert PR.exp([f64(np.nan), f64(0.0), f64(0.0)] + z) is not None  # passes, and ends in state 2 through the pose


@pytest.mark.parametrize("k", range(len(PCs.CASES)), ids=PCs.CASE_NAMES)
def test_host_twin_equals_the_reference_on_the_shared_cases(k):
    res, flags, _ = PCs.reference(k)
    _same(PCs.CASES[k]["name"], _host(PCs.case_frame(k), PCs.CASES[k]["params"]), (res, flags))


def test_host_twin_equals_the_reference_on_failures_counts_and_the_row_limit():
    for name, (fr, state) in PCs.failure_frames().items():
        want = PCs.solve_frame(fr, PR.UPSTREAM)
        assert want[0]["state"] == state, name
        _same(name, _host(fr, PR.UPSTREAM), want)
        assert np.isfinite(want[0]["rcw"]).all() and np.isfinite(want[0]["tcw"]).all() and np.isfinite(want[0]["cost"])
    for n in (0, 2, 3, 255, 256, 257):
        for by_row in (False, True):
            fr = PCs.make_frame(200 + n, max(n, 1), n_out=n // 8, n_border=n // 8, by_row=by_row, stereo_every=3, n_points=300, n_kp=280)
            if n == 0:
                fr = dict(fr, idx=np.full(len(fr["idx"]), -1, np.int32))
            p = dict(idx_by_row=by_row, check_right=True)
            want = PCs.solve_frame(fr, p)
            assert want[0]["n_obs"] == n and want[0]["state"] == (1 if n < 3 else 0)
            _same(f"n_obs {n}, idx_by_row {by_row}", _host(fr, p), want)
    fr = PCs.make_frame(63, 16384, n_out=2000, n_border=2000, stereo_every=2)
    fr["skip"] = (np.arange(16384) % 7 == 3).astype(np.uint8)
    want = PCs.solve_frame(fr, dict(check_right=True))
    assert want[0]["state"] == 0 and want[0]["n_obs"] == 16384 - int(fr["skip"].sum())
    _same("the row limit with skip bytes", _host(fr, dict(check_right=True)), want)
    void = PCs.solve_frame(fr, {}, status=-5)
    assert void[0]["status"] == -5 and void[0]["state"] == 1 and void[0]["n_obs"] == 0 and (void[1] == 2).all() and len(void[1]) == 16384
    other = tuple(f32(v) for v in (1.0, 1.5, 2.25))  # another pyramid table: octaves 3 .. 7 are out of range
    fr = PCs.case_frame(0)
    want = PCs.solve_frame(fr, {}, scale=other)
    assert 3 <= want[0]["n_obs"] < 300 * 3 // 8 + 30
    _same("another pyramid table", _host(fr, {}, scale=other), want)


# measured on the three scenes below (250 observations, 35 gross outliers): |R - R_oracle| 3.4e-16, |t - t_oracle| 6.7e-16; the pose from
# the off start and the pose from the truth as start (the optimum next to the ground truth) differ by 9.5e-16
ORACLE_BOUND_R, ORACLE_BOUND_T = 3.4e-15, 6.7e-15  # ten times the measurement


def test_monocular_rule_against_the_oracle():
    """oracle/vo_oracle.pose_only on float32-representable scenes with a known motion and planted gross outliers: equal inlier masks,
    the pose within the bound, and within that bound of the optimum reached from the ground truth"""
    cam = V.Camera(PC.FX, PC.FY, PC.CX, PC.CY)
    worst_r = worst_t = worst_o = 0.0
    for seed in (11, 12, 13):
        fr = PCs.make_frame(seed, 250, n_out=35)
        res, flags = PCs.solve_frame(fr, PR.UPSTREAM)
        o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale())
        n_in, R, t, inl = V.pose_only(cam, np.stack([o["X"], o["Y"], o["Z"]], 1), np.stack([o["u"], o["v"]], 1), o["w"], fr["start"][:9].reshape(3, 3),
                                      fr["start"][9:])
        assert res["state"] == 0 and n_in == res["n_inliers"] and np.array_equal(flags[o["slot"]] == 0, inl)
        assert not inl[np.isin(o["slot"], fr["obs_slots"][:35])].any() and n_in > 200  # the planted ones are out, the others mostly in
        worst_r, worst_t = max(worst_r, np.abs(R.reshape(9) - res["rcw"]).max()), max(worst_t, np.abs(t - res["tcw"]).max())
        best, _ = PCs.solve_frame(dict(fr, start=PCs.start_of(*fr["truth"])), PR.UPSTREAM)
        worst_o = max(worst_o, np.abs(best["rcw"] - res["rcw"]).max(), np.abs(best["tcw"] - res["tcw"]).max())
        assert np.abs(res["rcw"].reshape(3, 3) - PCs.R_TRUE).max() < 2e-3 and np.abs(res["tcw"] - PCs.T_TRUE).max() < 5e-3  # 0.6 px of noise
    print("against the oracle:", worst_r, worst_t, "against the optimum from the truth:", worst_o)
    assert worst_r <= ORACLE_BOUND_R and worst_t <= ORACLE_BOUND_T and worst_o <= ORACLE_BOUND_T


def test_jacobian_rows_against_finite_differences():
    """the three residuals under exp(delta).pose against the analytic rows, the stereo row among them"""
    fr = PCs.make_frame(21, 40, stereo_every=1)
    o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale(), right=fr["right"], check_right=True)
    assert o["stereo"].all()
    c = PR.camera(fr["view"], 5.991, 7.815)
    R, t, _ = PR.start_pose(fr["start"])
    _, res, J = PR.jacobians(o, c, R, t)
    h = 1e-6
    for a in range(6):
        d = [f64(0.0)] * 6
        for sign in (+1, -1):
            d[a] = f64(sign * h)
            dR, dt = PR.exp(d)
            Rn, tn = PR.update(dR, dt, R, t)
            r = PR.jacobians(o, c, Rn, tn)[1]
            if sign > 0:
                plus = r
        for row in range(3):
            fd = (plus[row] - r[row]) / (2 * h)
            an = np.zeros(len(fd)) if J[row][a] is None else J[row][a]
            assert np.abs(fd - an).max() < 1e-5 * max(1.0, np.abs(an).max()), (row, a, np.abs(fd - an).max())
    assert J[0][4] is None and J[1][3] is None and J[2][4] is None


def _axis_frame(d, e=None):
    """identity start; three exact observations and, in slot 0, a point on the axis seen d px to the right (and, with e, a right
    coordinate e px off).  lambda = 1e300 keeps every step below 1e-290, so the chi-square of slot 0 is w * d * d exactly"""
    z = 4.0
    xyz = np.array([[0.0, 0.0, z], [1.0, 0.5, z], [-1.0, 0.5, z], [0.5, -1.0, z]], f32)
    u, v = PC.FX * xyz[:, 0] / z + PC.CX, PC.FY * xyz[:, 1] / z + PC.CY
    ur = u - PC.BF / z
    u[0] += d
    right = np.full(4, -1.0, f32)
    if e is not None:
        right[0] = ur[0] + e
    kp = PCs.G.kp_rows(u.astype(f32), v.astype(f32), np.array([0, 0, 0, 0]))
    return {"view": PCs.view(), "start": PCs.start_of(np.eye(3), np.zeros(3)), "points": PCs.points_of(xyz), "kp": kp, "idx": np.arange(4, dtype=np.int32),
            "right": right, "skip": None}


def test_chi_square_thresholds_from_both_sides():
    """an outlier iff not chi2 <= th: at the threshold an inlier, one ulp below it an outlier, for both kinds"""
    base = dict(lambda_=1e300, n_rounds=1)
    fr = _axis_frame(2.5)  # chi2 = 6.25
    for th, flag in ((6.25, 0), (np.nextafter(6.25, 0.0), 1), (np.nextafter(6.25, 7.0), 0)):
        p = dict(base, chi2_mono=float(th))
        want = PCs.solve_frame(fr, p)
        assert want[1].tolist() == [flag, 0, 0, 0] and want[0]["state"] == 0 and want[0]["cost"] == (6.25 if flag == 0 else 0.0), (th, want)
        _same(f"mono threshold {th!r}", _host(fr, p), want)
    fr = _axis_frame(2.0, 1.5)  # chi2 = (4 + 0) + 2.25
    for th, flag in ((6.25, 0), (np.nextafter(6.25, 0.0), 1), (np.nextafter(6.25, 7.0), 0)):
        p = dict(base, chi2_stereo=float(th), chi2_mono=1.0, check_right=True)
        want = PCs.solve_frame(fr, p)
        assert want[1].tolist() == [flag, 0, 0, 0] and want[0]["n_stereo"] == 1 and want[0]["cost"] == (6.25 if flag == 0 else 0.0), (th, want)
        _same(f"stereo threshold {th!r}", _host(fr, p), want)
    # three inliers are enough, two are not
    p = dict(base, chi2_mono=1.0, min_obs=4)
    want = PCs.solve_frame(_axis_frame(2.5), p)
    assert want[0]["state"] == 3 and want[0]["n_inliers"] == 3
    _same("too few inliers", _host(_axis_frame(2.5), p), want)


@pytest.mark.parametrize("k", range(len(PCs.CASES)), ids=PCs.CASE_NAMES)
def test_shared_cases_are_live(k):
    """on the reference: round 0 removes every gross outlier, a later round re-admits an observation round 0 removed, and a round ends
    before its last step -- but for the case that runs every step with step_eps = 0"""
    case, fr = PCs.CASES[k], PCs.case_frame(k)
    res, flags, trace = PCs.reference(k)
    p = case["params"]
    o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale(), None, fr["right"], p["check_right"], p["idx_by_row"])
    gross = np.isin(o["slot"], fr["obs_slots"][:fr["n_out"]])
    assert res["state"] == 0 and len(trace) == p["n_rounds"] and res["n_obs"] == len(gross) == case["frame"]["n"]
    assert not trace[0][gross].any() and (~trace[0]).sum() > gross.sum() and (flags[o["slot"][gross]] == 1).all()
    assert any((~trace[0] & later).any() for later in trace[1:])
    steps = res["steps"][:p["n_rounds"]].tolist()
    if case["early"]:
        assert min(steps) < p["iterations"] and p["step_eps"] > 0
    else:
        assert steps == [p["iterations"]] * p["n_rounds"] and p["step_eps"] == 0
    assert (res["steps"][p["n_rounds"]:] == 0).all() and res["n_stereo"] == int(o["stereo"].sum())
    assert (res["n_stereo"] > 0) == bool(p["check_right"])


# ---- odd cameras: what makes tests/test_pose.py able to fail ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(PCs.CAMERA_KINDS))
def test_camera_frames_are_live_and_the_host_twin_agrees(kind):
    """the three frames under cameras A, B and the square one are what the shared cases are: state 0, the gross outliers removed in
    round 0, an observation re-admitted later, a round ended early; the host twin gives the reference's bytes"""
    p, fkw = PCs.camera_params(kind), PCs.CAMERA_KINDS[kind][0]
    for b, (fr, (res, flags, trace)) in enumerate(zip(PCs.camera_frames(kind), PCs.camera_reference(kind))):
        assert fr["view"].tobytes() == PCs.view(cam=CC.FRAME_CAMERAS[b]).tobytes()
        o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale(), None, fr["right"], p["check_right"], p["idx_by_row"])
        gross = np.isin(o["slot"], fr["obs_slots"][:fr["n_out"]])
        assert res["state"] == 0 and res["n_obs"] == len(gross) == PCs.CAMERA_FRAME["n"] and len(trace) == p["n_rounds"], (kind, b)
        assert not trace[0][gross].any() and (~trace[0]).sum() > gross.sum() and (flags[o["slot"][gross]] == 1).all(), (kind, b)
        assert any((~trace[0] & later).any() for later in trace[1:]), (kind, b)
        assert min(res["steps"][:p["n_rounds"]]) < p["iterations"] and res["n_inliers"] > 100
        assert (res["n_stereo"] > 40) == bool(fkw.get("stereo_every")) and res["n_stereo"] < res["n_obs"]
        assert np.abs(res["rcw"].reshape(3, 3) - PCs.R_TRUE).max() < 5e-3  # the camera that made the scene solves it
        _same(f"{kind}, frame {b}", _host(fr, p), (res, flags))


# a frame that reads no right coordinate does not read bf
POSE_EXEMPT = {("monocular", "bf of another frame"): "no observation of a monocular frame has a right coordinate: bf is not read"}


@pytest.mark.parametrize("mixup", list(CC.FRAME_MIXUPS))
@pytest.mark.parametrize("kind", list(PCs.CAMERA_KINDS))
def test_camera_mixups_change_the_reference(kind, mixup):
    """solved under the cameras a confused kernel would use, every frame whose camera the mix-up changes has other result bytes
    and other flags"""
    p = PCs.camera_params(kind)
    cams = list(CC.FRAME_CAMERAS)
    mixed = CC.FRAME_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed)
    assert hit, mixup
    for b in hit:
        fr, (res, flags, _) = PCs.camera_frames(kind)[b], PCs.camera_reference(kind)[b]
        wrong, wflags = PCs.solve_frame(dict(fr, view=PCs.view(cam=mixed[b])), p)
        if (kind, mixup) in POSE_EXEMPT:
            assert wrong.tobytes() == res.tobytes() and np.array_equal(wflags, flags), (kind, mixup, b)  # the exemption is not stale
            continue
        assert wrong["rcw"].tobytes() != res["rcw"].tobytes() and wrong["tcw"].tobytes() != res["tcw"].tobytes(), (kind, mixup, b)
        assert (wflags != flags).any(), (kind, mixup, b)
    assert sum(k == kind for k, _ in POSE_EXEMPT) <= 1


def test_a_view_without_baseline():
    """bf = 0: the stereo rows stay stereo rows, their third residual has no disparity term; any other bf gives other bytes"""
    fr = PCs.no_baseline_frame()
    p = dict(PR.UPSTREAM, check_right=True)
    res, flags = PCs.solve_frame(fr, p)
    assert fr["view"]["bf"] == 0 and res["state"] == 0 and res["n_stereo"] > 40 and res["n_inliers"] > 100
    _same("bf = 0", _host(fr, p), (res, flags))
    other, oflags = PCs.solve_frame(dict(fr, view=PCs.view(cam=CC.A)), p)
    assert other["rcw"].tobytes() != res["rcw"].tobytes() and (oflags != flags).any()


# ---- parameter limits, a singular system, other pyramid tables ---------------------------------------------------------------------------
def test_parameter_limits_on_the_reference():
    fr = PCs.make_frame(**PCs.LIMIT_FRAME)
    got = {}
    for name, (kw, states) in PCs.LIMITS.items():
        res, flags = PCs.solve_frame(fr, kw)
        assert res["n_obs"] == 65 and res["state"] in states, (name, res)
        _same(name, _host(fr, kw), (res, flags))
        got[name] = res
    assert got["eight rounds of 32 steps"]["steps"].tolist() == [32] * 8  # every byte of steps in use
    assert (got["eight robust rounds"]["steps"] > 0).all() and (got["no robust round"]["steps"][:4] > 0).all()
    assert got["no robust round"]["rcw"].tobytes() != got["eight robust rounds"]["rcw"].tobytes() != got["lambda 0"]["rcw"].tobytes()
    assert got["lambda 0"]["rcw"].tobytes() != PCs.solve_frame(fr, {})[0]["rcw"].tobytes()  # the damping is in the bytes
    assert got["min_obs at n_obs"]["steps"][0] > 0 and got["min_obs above n_obs"]["steps"].tolist() == [0] * 8
    assert got["min_obs above n_obs"]["n_inliers"] == 65


def test_singular_system_ends_in_state_2_through_a_pivot():
    """every observation is one map point on the optical axis, lambda = 0: the sums are finite, the third pivot is not > 0, the
    frame ends in state 2 with its start pose"""
    fr, p = PCs.singular_frame(), PCs.SINGULAR_PARAMS
    o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale(), idx_by_row=True)
    c = PR.camera(fr["view"], p["chi2_mono"], p["chi2_stereo"])
    R, t, ok = PR.start_pose(fr["start"])
    front, T = PR.terms(o, c, R, t, True)
    total = PR.tree(T, front)
    assert ok and front.all() and len(front) == 40 and np.isfinite(total).all()
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(PR.H_PAIRS):
        H[a, b] = H[b, a] = total[k]
    assert H[0, 0] > 0 and H[1, 1] - H[1, 0] * H[1, 0] / H[0, 0] > 0  # the first two pivots pass
    assert H[2, 2] == 0 and H[2, 0] == 0 and H[2, 1] == 0             # the third is 0 - 0 - 0
    assert PR.solve(total, 0.0) is None and PR.solve(total, 1e-6) is not None
    res, flags = PCs.solve_frame(fr, p)
    assert res["state"] == 2 and res["n_obs"] == 40 and res["steps"].tolist() == [0] * 8 and (flags == 0).all()
    assert res["rcw"].tolist() == [float(v) for v in R] and res["tcw"].tolist() == [float(v) for v in t]
    assert res["rcw"].tolist() != np.eye(3).reshape(9).tolist()  # the start, not the identity of a start that is not finite
    _same("singular", _host(fr, p), (res, flags))


@pytest.mark.parametrize("name", ["one_level", "sixteen_levels"])
def test_other_pyramid_tables_drop_the_rows_outside_them(name):
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    fr = PCs.pyramid_frame(n_levels)
    octave = fr["kp"]["octave"][fr["idx"][fr["obs_slots"]]]
    outside = int(((octave < 0) | (octave >= n_levels)).sum())
    res, flags = PCs.solve_frame(fr, {}, scale=sc)
    assert 20 < outside < 80 and res["n_obs"] == 120 - outside and res["state"] == 0 and res["n_inliers"] > 40
    assert set(octave.tolist()) == {0, 1, n_levels - 1, n_levels}
    assert (flags[fr["obs_slots"]][(octave < 0) | (octave >= n_levels)] == 2).all()
    _same(name, _host(fr, {}, scale=sc), (res, flags))


def test_refused_arguments():
    fr = PCs.case_frame(0)
    nan = float("nan")
    for kw in (dict(chi2_mono=0.0), dict(chi2_mono=nan), dict(chi2_stereo=float("inf")), dict(lambda_=-1.0), dict(lambda_=nan), dict(step_eps=-1e-10),
               dict(n_rounds=0), dict(n_rounds=9), dict(iterations=0), dict(iterations=33), dict(robust_rounds=-1), dict(robust_rounds=9), dict(min_obs=2),
               dict(reserved=(1, 0))):
        with pytest.raises(binding.OrbError) as e:
            binding.pose_opt_host(fr["view"], fr["start"], PC.scale(), fr["points"], fr["kp"], fr["idx"], binding.pose_opt_params(**kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    for levels in (np.zeros(0, f32), np.ones(17, f32)):
        with pytest.raises(binding.OrbError):
            binding.pose_opt_host(fr["view"], fr["start"], levels, fr["points"], fr["kp"], fr["idx"], binding.pose_opt_params())
    lib = binding.load()
    p = binding.pose_opt_params()
    assert lib.ss_pose_opt_pairs_device(None, None, None, None, 1, 1, None, None, None, 0, 1, None, None, None, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_pose_opt_batch_device(None, None, None, None, 1, 1, None, None, None, None, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_pose_opt(None, None, None, None, None, 0, None, None, 0, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_pose_opt_host(None, None, None, 0, None, None, 0, None, None, 0, None, None, None, None) == binding.SS_ERR_INVALID_ARG
    flags, res = binding.pose_opt_host(fr["view"], fr["start"], PC.scale(), fr["points"][:0], fr["kp"][:0], fr["idx"][:0], p)
    assert len(flags) == 0 and (res["state"], res["n_obs"]) == (1, 0)


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/pose_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "pose_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "pose_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 40000
