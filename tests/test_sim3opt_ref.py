"""CPU tests of the Sim3 refinement (include/sendslam_orb.h; tests/sim3opt_ref.py is the normative statement): the ABI, the scale's
series in exact fractions, the host twin ss_sim3_opt_host against the restatement bit for bit, both edges' Jacobians against central
differences through the retraction, every threshold from both sides, the liveness of the shared cases, the result against an
independent optimiser that uses g2o's closed-form Sim3 exponential and numerical Jacobians, the bookkeeping of SearchBySim3, the
inverse view, every refusal, and the steps under the address and undefined-behaviour sanitizers; and that the scenes of
tests/test_sim3opt.py under odd cameras, other pyramid tables, the parameters' limits, a singular system and skip bytes per frame
do what their names say: every confusion of camera_cases changes the bytes the GPU tests compare.  None needs a GPU."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import camera_cases as CC
import fuse_ref
import pose_ref as PR
import proj_cases as PC
import sim3_cases as SC
import sim3_ref as S
import sim3opt_cases as OC
import sim3opt_ref as O
from send_slam_amd import binding
from sim3opt_cases import FROZEN, frozen_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = np.float64


def host(pr, params, start=None, scale=None):
    p = binding.sim3_opt_params(**params)
    return binding.sim3_opt_host(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"],
                                 pr["start"] if start is None else start, PC.scale() if scale is None else scale, p, pr["q_skip"], pr["t_skip"])


def same(pr, params, start=None, ref=None, scale=None):
    """the host twin equals the restatement in every byte -> the restatement's (result, flags)"""
    res, flags = ref if ref is not None else OC.solve_pair(pr, params, start=start, scale=scale)
    f2, r2 = host(pr, params, start, scale)
    assert flags.tobytes() == f2.tobytes()
    for name in res.dtype.names:
        assert np.asarray(res[name]).tobytes() == np.asarray(r2[name]).tobytes(), (name, res[name], r2[name])
    return res, flags


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_sizes_and_offsets():
    lib = binding.load()
    for n in ("ss_sim3_opt_host", "ss_sim3_opt_pairs_device", "ss_sim3_opt_batch_device", "ss_sim3_opt", "ss_sim3_marks_pairs_device",
              "ss_sim3_mutual_pairs_device", "ss_sim3_marks_batch_device", "ss_sim3_mutual_batch_device", "ss_sim3_to_view21"):
        assert hasattr(lib, n) and n in binding.EXPORTS
    assert lib.ss_abi_version() == 5
    assert C.sizeof(binding.Sim3OptParams) == 64 and binding.Sim3OptParams.iterations0.offset == 24 and binding.Sim3OptParams.reserved.offset == 48
    d = binding.SIM3_OPT_RESULT_DTYPE
    assert d.itemsize == 272 and d == O.RESULT_DTYPE
    assert [d.fields[n][1] for n in ("r12", "t12", "s12", "cost", "state", "status", "n_corr", "n_removed", "n_inliers", "steps", "reserved", "model")] == \
        [0, 72, 96, 104, 112, 116, 120, 124, 128, 132, 140, 144]
    assert binding.SIM3_RESULT_DTYPE.itemsize == 128 and binding.SIM3_MUTUAL_DTYPE.itemsize == 8 and binding.SIM3_MUTUAL_DTYPE == O.MUTUAL_DTYPE


# ---- the series -------------------------------------------------------------------------------------------------------------------------
def test_scale_series_in_exact_fractions():
    assert Fraction(1, math.factorial(O.SERIES)) < Fraction(1, 2 ** 60) <= Fraction(1, math.factorial(O.SERIES - 1))  # at |sigma| = 1
    for k in range(O.SERIES):  # the table's entries are the doubles next to 1 / k!
        exact, v = Fraction(1, math.factorial(k)), PR.INV_FACT[k]
        assert abs(Fraction(v) - exact) <= min(abs(Fraction(np.nextafter(v, 0.0)) - exact), abs(Fraction(np.nextafter(v, 2.0)) - exact))
    for x in (1.0, -1.0, 0.5, -0.25, 1e-9, 0.0):
        exact = sum(Fraction(x) ** k / math.factorial(k) for k in range(60))
        assert abs(Fraction(float(O.exp_scale(x))) - exact) < Fraction(1, 2 ** 50)
    assert O.exp_scale(0.0) == 1.0
    text = open(os.path.join(ROOT, "send-slam_amd", "csrc", "ss_sim3opt_steps.h")).read()
    assert f"#define SS_SIM3OPT_SERIES {O.SERIES}" in text and f"#define SS_SIM3OPT_SUMS {O.SUMS}" in text


# ---- the host twin against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(OC.CASES)), ids=OC.CASE_NAMES)
def test_host_twin_shared_cases(k):
    res, flags, _ = OC.reference(k)
    same(OC.case_pair(k), OC.CASES[k]["params"], ref=(res, flags))


@pytest.mark.parametrize("fix", [False, True], ids=["scale", "fix_scale"])
@pytest.mark.parametrize("n", [0, 9, 10, 11, 255, 256, 257])
def test_host_twin_counts(n, fix):
    res, _ = same(OC.count_pair(n, fix), dict(O.UPSTREAM, fix_scale=fix))
    assert res["n_corr"] == n and (res["state"] == 1) == (n < 10)


def test_host_twin_full_pair_with_skips():
    rows = binding.SS_GUIDED_MAX_ROWS if hasattr(binding, "SS_GUIDED_MAX_ROWS") else 16384
    assert rows == 16384
    pr = OC.with_skips(OC.make_pair(90, rows, rows // 8, rows, rows), 1)
    res, flags = same(pr, O.UPSTREAM)
    assert res["state"] == 0 and 0 < res["n_corr"] < rows and (flags == 2).sum() == rows - res["n_corr"]


def test_host_twin_voided_pair_and_start_without_model():
    pr = OC.case_pair(0)
    for state, status in ((0, -7), (2, 0), (1, 0)):
        start = pr["start"].copy()
        start["state"], start["status"] = state, status
        res, flags = same(pr, O.UPSTREAM, start=start)
        assert res["state"] == 1 and res["status"] == status and res["n_corr"] == 0 and (flags == 2).all() and res["model"]["state"] == 1
    zero = np.zeros((), S.RESULT_DTYPE)
    res, flags = same(pr, O.UPSTREAM, start=zero)
    assert res["state"] == 2 and res["s12"] == 1.0 and not res["model"]["sr12"].any()
    shear = pr["start"].copy()
    shear["sr12"][1] += np.float32(1e-3)
    res, _ = same(pr, O.UPSTREAM, start=shear)
    assert res["state"] == 0
    R = res["r12"].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12


def test_host_twin_non_finite_inputs():
    pr = dict(OC.case_pair(0))
    q_kp, q_xyz = pr["q_kp"].copy(), pr["q_xyz"].copy()
    q_kp["x"][pr["rows"][3]] = np.nan
    q_xyz["z"][pr["rows"][5]] = np.nan
    pr.update(q_kp=q_kp, q_xyz=q_xyz)
    res, flags = same(pr, O.UPSTREAM)
    assert not np.isnan(np.frombuffer(res.tobytes()[:112], f64)).any() and not np.isnan(res["model"]["sr12"]).any()


# ---- the Jacobians ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix", [False, True], ids=["scale", "fix_scale"])
def test_jacobians_against_central_differences_through_the_retraction(fix):
    pr = OC.case_pair(2 if fix else 0)
    c = O.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale())
    k = O.cameras(pr["view1"], pr["view2"], 10.0)
    R, t, s, ok = O.start(pr["start"], fix)
    assert ok
    h = 1e-6
    for edge in (O.edge12, O.edge21):
        _, rx, ry, J0, J1, _ = edge(c, k, R, t, s)
        for a in range(6 if fix else 7):
            d = [f64(0.0)] * 7
            d[a] = f64(h)
            Rp, tp, sp = O.retract(d, R, t, s, fix)
            d[a] = f64(-h)
            Rm, tm, sm = O.retract(d, R, t, s, fix)
            ep, em = edge(c, k, Rp, tp, sp), edge(c, k, Rm, tm, sm)
            for J, i in ((J0, 1), (J1, 2)):
                num = (ep[i] - em[i]) / (2 * h)
                scale = np.maximum(np.abs(num), 1.0)
                assert (np.abs(num - J[a]) / scale).max() < 1e-6, (edge.__name__, a)


# ---- thresholds -------------------------------------------------------------------------------------------------------------------------
# sim3opt_cases.frozen_pair: 12 exact correspondences, one keypoint two pixels off, under FROZEN no step moves the model
@pytest.mark.parametrize("edge", [0, 1], ids=["e12", "e21"])
def test_chi_square_threshold_from_both_sides(edge):
    pr, row, both, n = frozen_pair(edge)
    th = float(both[edge][n])
    assert th > 10 * max(float(both[1 - edge][n]), float(np.delete(both[0], n).max()), float(np.delete(both[1], n).max())) > 0
    on, flags_on = same(pr, dict(FROZEN, chi2=th))
    below, flags_below = same(pr, dict(FROZEN, chi2=float(np.nextafter(th, 0.0))))
    R, t, s, _ = O.start(pr["start"], False)
    assert on["r12"].tolist() == [float(v) for v in R] and on["s12"] == s  # nothing moved
    assert flags_on[row] == 0 and on["n_removed"] == 0 and on["steps"].tolist() == [5, 5]
    assert flags_below[row] == 1 and below["n_removed"] == 1 and below["n_inliers"] == 11 and below["steps"].tolist() == [5, 10]


def test_min_corr_and_min_inliers_on_and_one_below():
    pr, row, both, n = frozen_pair(0)
    th = float(np.nextafter(float(both[0][n]), 0.0))  # one removal: 11 left
    assert same(pr, dict(FROZEN, chi2=th, min_corr=12))[0]["state"] == 0
    res, flags = same(pr, dict(FROZEN, chi2=th, min_corr=13))
    assert res["state"] == 1 and res["n_corr"] == 12 and (flags[pr["rows"]] == 0).all()
    assert same(pr, dict(FROZEN, chi2=th, min_inliers=11))[0]["state"] == 0
    res, flags = same(pr, dict(FROZEN, chi2=th, min_inliers=12))
    assert res["state"] == 3 and res["n_inliers"] == 11 and flags[row] == 1 and res["steps"].tolist() == [5, 0]


# ---- liveness of the shared cases --------------------------------------------------------------------------------------------------------
def test_shared_cases_are_what_their_names_say():
    for k in (0, 2, 5):  # round 0 removes every planted mismatch
        res, flags, trace = OC.reference(k)
        pr = OC.case_pair(k)
        assert res["state"] == 0 and len(pr["outlier_rows"]) > 0 and (flags[pr["outlier_rows"]] == 1).all()
        assert res["n_removed"] == int((~trace[0]).sum()) >= len(pr["outlier_rows"])
    assert OC.reference(0)[0]["steps"].tolist() == [5, 10] and OC.reference(0)[0]["n_removed"] > 0
    assert OC.reference(1)[0]["steps"].tolist() == [5, 5] and OC.reference(1)[0]["n_removed"] == 0
    early = OC.reference(3)[0]
    assert early["state"] == 0 and 0 < early["steps"][0] < 5 and 0 < early["steps"][1] < 5
    assert OC.reference(4)[0]["state"] == 3 and OC.reference(4)[0]["model"]["state"] == 3
    assert OC.reference(2)[0]["s12"] == 1.0 and OC.reference(5)[0]["n_corr"] == 300
    for k in range(len(OC.CASES)):
        res = OC.reference(k)[0]
        if res["state"] == 0:  # the embedded model is the result rounded once
            assert np.array_equal(res["model"]["sr12"], (res["s12"] * res["r12"]).astype(np.float32))
            assert res["model"]["n_inliers"] == res["n_inliers"]


def test_chain_is_live_on_the_references():
    """the chain of tests/test_sim3opt.py on the CPU references: the searches find the correspondences the BoW match cannot see, the
    mutual check adds them, the refinement keeps them, and the refined model's candidate check finds at least the RANSAC model's matches"""
    pr, ref = OC.chain_scene(), OC.chain_reference()
    hidden = pr["hidden_rows"]
    assert len(hidden) == OC.CHAIN_HIDDEN and (ref["bow"][0][hidden] < 0).all() and ref["sim3"][0]["state"] == 0
    assert np.array_equal(ref["search12"][0][hidden], pr["idx"][hidden]) and np.array_equal(ref["search21"][0][pr["idx"][hidden]], hidden)
    assert (ref["mutual"]["n_prior"], ref["mutual"]["n_new"]) == (int((ref["bow"][0] >= 0).sum()), OC.CHAIN_HIDDEN)
    res, flags = ref["opt"]
    assert res["state"] == 0 and res["n_corr"] == ref["mutual"]["n_prior"] + OC.CHAIN_HIDDEN and (flags[hidden] != 2).all()  # each is a correspondence of the refinement
    assert int((ref["check"][0] >= 0).sum()) >= int((ref["check_ransac"][0] >= 0).sum()) > 20


# ---- independence of the retraction ----------------------------------------------------------------------------------------------------------
def g2o_exp(d):
    """g2o's Sim3(const Vector7d &): the closed-form exponential with sin, cos and exp -> (R, t, s)"""
    w, u, sigma = np.asarray(d[:3], f64), np.asarray(d[3:6], f64), float(d[6])
    th = float(np.linalg.norm(w))
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    Om2, s, eps, I = Om @ Om, math.exp(sigma), 1e-5, np.eye(3)
    if abs(sigma) < eps:
        Cc = 1.0
        if th < eps:
            A, B, R = 0.5, 1.0 / 6.0, I + Om + Om2 / 2
        else:
            A, B = (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
            R = I + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om2
    else:
        Cc = (s - 1) / sigma
        if th < eps:
            A, B = ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s - 1) / sigma ** 3
            R = I + Om + Om2 / 2
        else:
            R = I + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om2
            a, b, c = s * math.sin(th), s * math.cos(th), th ** 2 + sigma ** 2
            A, B = (a * sigma + (1 - b) * th) / (th * c), (Cc - ((b - 1) * sigma + a * th) / c) / th ** 2
    return R, (A * Om + B * Om2 + Cc * I) @ u, s


def independent(pr, params):
    """the same schedule, Huber weights and removal rule on np.linalg.solve, g2o's exponential and central-difference Jacobians"""
    p = dict(O.UPSTREAM, **params)
    c = O.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale())
    K = [[float(np.float32(v[n])) for n in ("fx", "fy", "cx", "cy")] for v in (pr["view1"], pr["view2"])]
    R0, t0, s0, _ = O.start(pr["start"], p["fix_scale"])
    R, t, s = np.array(R0, f64).reshape(3, 3), np.array(t0, f64), float(s0)
    obs = [np.stack([c["u1"], c["v1"]], 1), np.stack([c["u2"], c["v2"]], 1)]
    w = [c["w1"], c["w2"]]
    nu = 6 if p["fix_scale"] else 7

    def residuals(R, t, s):
        Y = s * c["x2"] @ R.T + t
        Z = (c["x1"] - t) @ R / s
        out = []
        for P, (fx, fy, cx, cy), o in ((Y, K[0], obs[0]), (Z, K[1], obs[1])):
            out.append((o - np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1), P[:, 2] > 0))
        return out

    def moved(d, R, t, s):
        dR, dt, ds = g2o_exp(d)
        return dR @ R, ds * dR @ t + dt, ds * s

    active = np.ones(len(c["rows"]), bool)
    delta, n_removed = math.sqrt(p["chi2"]), 0
    for rnd in range(2):
        for _ in range(p["iterations0"] if rnd == 0 else p["iterations_more"] if n_removed else p["iterations_same"]):
            r0 = residuals(R, t, s)
            H, g = np.zeros((nu, nu)), np.zeros(nu)
            for e in range(2):
                J = np.zeros((len(active), 2, nu))
                for a in range(nu):
                    d = np.zeros(7)
                    d[a] = 1e-6
                    J[:, :, a] = (residuals(*moved(d, R, t, s))[e][0] - residuals(*moved(-d, R, t, s))[e][0]) / 2e-6
                r, front = r0[e]
                e2 = w[e] * (r ** 2).sum(1)
                wq = np.where((e2 > p["chi2"]) & (rnd == 0), w[e] * delta / np.sqrt(np.maximum(e2, 1e-300)), w[e]) * (active & front)
                H += np.einsum("n,nia,nib->ab", wq, J, J)
                g += np.einsum("n,nia,ni->a", wq, J, r)
            H[np.diag_indices(nu)] += p["lambda_"] * (1 + np.diag(H))
            d = np.zeros(7)
            d[:nu] = np.linalg.solve(H, -g)
            R, t, s = moved(d, R, t, s)
        (r12, f12), (r21, f21) = residuals(R, t, s)
        c12, c21 = np.where(f12, w[0] * (r12 ** 2).sum(1), 1e30), np.where(f21, w[1] * (r21 ** 2).sum(1), 1e30)
        active = active & (c12 <= p["chi2"]) & (c21 <= p["chi2"])
        if rnd == 0:
            n_removed = int((~active).sum())
    return R, t, s, active, c["rows"]


# synthetic pairs with a known Sim3: (seed, correspondences, planted mismatches, pixel noise, fix_scale)
SCENES = [(11, 80, 12, 0.4, False), (13, 64, 8, 0.4, True), (15, 40, 0, 0.5, False), (16, 150, 20, 0.2, False), (17, 100, 15, 0.2, True)]
# the largest deviations measured over SCENES against `independent` (summation order, libm, the retraction and the Jacobians differ);
# the bounds are ten times these, the margin DESIGN.md sections 20 and 21 give for the same reason
MEASURED = dict(R=4.6e-13, t=6.9e-12, s=1.3e-11)


def test_result_does_not_depend_on_the_retraction():
    worst = dict(R=0.0, t=0.0, s=0.0)
    for seed, n, n_out, noise, fix in SCENES:
        pr = OC.make_pair(seed, n, n_out, n + 8, n + 8, s=1.0 if fix else SC.S_TRUE, noise_px=noise, fix_scale=fix)
        params = dict(O.UPSTREAM, fix_scale=fix, step_eps=0.0)
        res, flags = same(pr, params)
        R, t, s, active, rows = independent(pr, params)
        # the independent optimiser itself removes every planted mismatch and no true match
        assert set(rows[~active]) == set(pr["outlier_rows"]), seed
        assert res["state"] == 0 and np.array_equal(flags[rows] == 0, active), seed
        worst["R"] = max(worst["R"], float(np.abs(res["r12"].reshape(3, 3) - R).max()))
        worst["t"] = max(worst["t"], float(np.abs(res["t12"] - t).max()))
        worst["s"] = max(worst["s"], float(abs(res["s12"] - s)))
    print("largest deviations from the independent optimiser:", worst)
    for name in worst:
        assert worst[name] <= 10 * MEASURED[name], (name, worst[name])


# ---- marks and mutual -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 4, 63, 64, 65, 300])
def test_marks_and_mutual_loops_against_array_forms(rows):
    for seed in range(3):
        tb = OC.marks_tables(rows, seed)
        idx, nq, nt = tb["idx"].astype(np.int64), tb["nq"], tb["nt"]
        i = np.arange(rows)
        valid = (i < nq) & (idx >= 0) & (idx < nt)
        s1, s2 = O.marks(tb["idx"], tb["q_skip"], tb["t_skip"], nq, nt)
        taken = np.isin(i, idx[valid])
        assert np.array_equal(s1, ((tb["q_skip"] != 0) | valid).astype(np.uint8))
        assert np.array_equal(s2, ((tb["t_skip"] != 0) | taken).astype(np.uint8))
        n1, n2 = O.marks(tb["idx"], None, None, nq, nt)
        assert np.array_equal(n1, valid.astype(np.uint8)) and np.array_equal(n2, taken.astype(np.uint8))
        out, summary = O.mutual(tb["idx"], tb["idx12"], tb["idx21"], nq, nt)
        j = tb["idx12"].astype(np.int64)
        jok = (i < nq) & (j >= 0) & (j < nt)
        jj = np.where(jok, j, 0)
        new = ~valid & jok & (tb["idx21"][jj] == i) & ~taken[jj]
        assert np.array_equal(out, np.where(valid, idx, np.where(new, j, -1)).astype(np.int32))
        assert (summary["n_prior"], summary["n_new"]) == (valid.sum(), new.sum())
        got = out[out >= 0]
        if rows >= 4:
            assert out[0] == 2 and out[1] == 2 and out[2] == -1 and out[3] == 1  # the adversarial rows of marks_tables
        assert len(set(got[~valid[out >= 0]].tolist())) == int(new.sum())  # no train row gained twice


# ---- the inverse view -----------------------------------------------------------------------------------------------------------------------
def _views_of_the_double_products(c):
    """ss_sim3_to_view21 and ss_sim3_to_view under the camera c (fx, fy, cx, cy, bf) against fuse_ref.view_sim3 of the double products"""
    res = OC.reference(0)[0]["model"]
    cam = binding.Camera(fx=c[0], fy=c[1], cx=c[2], cy=c[3], width=SC.W, height=SC.H)
    rcw1, tcw1 = np.asarray(SC.POSE1[0], f64), np.asarray(SC.POSE1[1], f64)
    view, srcw, t = binding.sim3_to_view21(cam, res, rcw1, tcw1)
    m, tt = O.to_s21w(res, rcw1, tcw1)
    assert srcw.tobytes() == m.tobytes() and t.tobytes() == tt.tobytes()
    assert bytes(view) == bytes(binding.fuse_view_sim3(cam, m, tt))
    assert bytes(view) == fuse_ref.view_sim3(c[0], c[1], c[2], c[3], SC.W, SC.H, m, tt, 0.0).tobytes()
    rcw2, tcw2 = np.asarray(SC.POSE2[0], f64), np.asarray(SC.POSE2[1], f64)
    view12, srcw, t = binding.sim3_to_view(cam, res, rcw2, tcw2)
    m, tt = S.to_scw(res, rcw2, tcw2)
    assert srcw.tobytes() == m.tobytes() and t.tobytes() == tt.tobytes()
    assert bytes(view12) == fuse_ref.view_sim3(c[0], c[1], c[2], c[3], SC.W, SC.H, m, tt, 0.0).tobytes()
    bad = res.copy()
    bad["state"] = 2
    with pytest.raises(binding.OrbError):
        binding.sim3_to_view21(cam, bad, rcw1, tcw1)
    return view, view12


def test_inverse_view_is_the_fuse_view_of_the_double_product():
    _views_of_the_double_products(SC.CAM)


@pytest.mark.parametrize("name", ["P", "Q"])
def test_views_under_odd_cameras(name):
    """fx != fy and cx, cy off the centre: a view built with two intrinsics exchanged has other bytes than the square camera shows"""
    c = getattr(CC, name)
    views = _views_of_the_double_products(c)
    for wrong in (CC.swap_f(c), CC.swap_c(c)):
        cam = binding.Camera(fx=wrong[0], fy=wrong[1], cx=wrong[2], cy=wrong[3], width=SC.W, height=SC.H)
        res = OC.reference(0)[0]["model"]
        assert bytes(binding.sim3_to_view21(cam, res, SC.POSE1[0], SC.POSE1[1])[0]) != bytes(views[0])
        assert bytes(binding.sim3_to_view(cam, res, SC.POSE2[0], SC.POSE2[1])[0]) != bytes(views[1])


# ---- odd cameras ----------------------------------------------------------------------------------------------------------------------------
def _differ(a, b):
    """(the result bytes differ, the flag bytes differ) of two (result, flags)"""
    return a[0].tobytes() != b[0].tobytes(), a[1].tobytes() != b[1].tobytes()


def test_camera_pairs_are_live():
    """every pair of the call ends in state 0, loses some correspondences but not all, and steps in both rounds"""
    for b, pr in enumerate(OC.camera_pairs()):
        res, flags = same(pr, O.UPSTREAM, ref=OC.camera_reference()[b])
        print(b, res["state"], res["n_corr"], res["n_removed"], res["steps"])
        assert res["state"] == 0 and res["n_corr"] == 60 and 0 < res["n_removed"] < res["n_corr"] and res["steps"][0] >= 1 and res["steps"][1] >= 1
        assert (flags[pr["outlier_rows"]] == 1).all()
    assert [tuple(CC.intrinsics(c) for c in pair) for pair in CC.SIM3_PAIR_CAMERAS][2][0] == (SC.F, SC.F, SC.CX, SC.CY)  # the square camera is one side of one pair


# the confusions one edge or one table of the refinement could make on top of camera_cases.PAIR_MIXUPS
EDGE_MIXUPS = {
    "cx and cy exchanged on side 1": lambda pairs: [(CC.swap_c(a), b) for a, b in pairs],
    "cx and cy exchanged on side 2": lambda pairs: [(a, CC.swap_c(b)) for a, b in pairs],
    "side 1 of every pair is pair 0's": lambda pairs: [(pairs[0][0], b) for a, b in pairs],
    "side 2 of every pair is pair 0's": lambda pairs: [(a, pairs[0][1]) for a, b in pairs],
}
PAIR_MIXUPS = dict(CC.PAIR_MIXUPS, **EDGE_MIXUPS)


@pytest.mark.parametrize("mixup", list(PAIR_MIXUPS))
def test_camera_mixups_change_the_reference_of_the_pairs_form(mixup):
    """the keypoints stay, the views are the ones a wrong kernel would use: the result bytes and the flag bytes change for exactly the
    pairs whose cameras the mix-up changes.  No mix-up is exempt: both residuals read fx, fy, cx and cy of their side"""
    cams = list(CC.SIM3_PAIR_CAMERAS)
    mixed = PAIR_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed, fields=(0, 1, 2, 3))
    assert hit, mixup
    for b, pr in enumerate(OC.camera_pairs()):
        wrong = same(SC.with_cameras(pr, *mixed[b]), O.UPSTREAM)
        assert _differ(wrong, OC.camera_reference()[b]) == ((True, True) if b in hit else (False, False)), (mixup, b, wrong[0]["state"])


@pytest.mark.parametrize("mixup", list(CC.FRAME_MIXUPS))
def test_camera_mixups_change_the_reference_of_the_batch_form(mixup):
    """the batch form: frame b's view is side 1 of pair b, frame train_src[b]'s its side 2; every mix-up changes the result bytes of
    every pair one of whose two views it changes, and bf, which no step reads, changes nothing"""
    cams = list(CC.SIM3_FRAME_CAMERAS)
    mixed = CC.FRAME_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed, fields=(0, 1, 2, 3))
    assert bool(hit) != (mixup == "bf of another frame")
    wrong_views = SC.frame_views(mixed)
    for b, t in enumerate(SC.CAMERA_BATCH_SRC):
        right = same(OC.camera_batch_pair(b), OC.BATCH_PARAMS)
        wrong = same(OC.camera_batch_pair(b, wrong_views), OC.BATCH_PARAMS)
        if t < 0:
            assert right[0]["state"] == 1 and (right[1] == 2).all()
            continue
        assert OC.camera_batch_starts()[b]["state"] == 0 and right[0]["state"] == 0 and right[0]["n_corr"] == 60 and min(right[0]["steps"]) >= 1
        assert _differ(wrong, right)[0] == (b in hit or t in hit), (mixup, b)
        if not hit:
            assert _differ(wrong, right) == (False, False)


def test_batch_form_train_view_is_that_of_the_trains_frame():
    """side 2 of pair b is views[train_src[b]]: with views[b] there, as a table filled by frame number would have it, or with the two
    frames' views exchanged, the result bytes differ"""
    vs = SC.camera_batch()[3]
    for b, t in enumerate(SC.CAMERA_BATCH_SRC):
        if t < 0:
            continue
        right = OC.solve_pair(OC.camera_batch_pair(b), OC.BATCH_PARAMS)
        for v1, v2 in ((vs[b], vs[b]), (vs[t], vs[b]), (vs[t], vs[t])):
            wrong = same(dict(OC.camera_batch_pair(b), view1=v1, view2=v2), OC.BATCH_PARAMS)
            assert wrong[0]["n_corr"] == right[0]["n_corr"] and _differ(wrong, right)[0], b


def test_batch_form_skip_bytes_are_those_of_the_trains_frame():
    """one skip array serves both sides: the query side reads frame b's bytes, the train side frame train_src[b]'s.  Under
    camera_batch_skip() the train side read at frame b keeps other correspondences, in the refinement and in the marks"""
    skip = OC.camera_batch_skip()
    kps, xyz, idx, _ = SC.camera_batch()
    assert skip.shape == idx.shape and not (skip[0].astype(bool) & (skip[1] | skip[2]).astype(bool)).any()
    for b, t in enumerate(SC.CAMERA_BATCH_SRC):
        right = same(OC.camera_batch_pair(b, skip=skip), OC.BATCH_PARAMS)
        if t < 0:
            assert right[0]["state"] == 1 and (right[1] == 2).all()
            continue
        plain = same(OC.camera_batch_pair(b), OC.BATCH_PARAMS)
        wrong = same(OC.camera_batch_pair(b, skip=skip, train_skip_of=b), OC.BATCH_PARAMS)
        rows = np.flatnonzero(idx[b] >= 0)
        assert skip[b][rows].any() and skip[t][idx[b][rows]].any()  # bytes on correspondences of both sides
        assert right[0]["state"] == 0 and 20 < right[0]["n_corr"] < plain[0]["n_corr"] == 60
        assert right[0]["n_corr"] != wrong[0]["n_corr"] and _differ(wrong, right) == (True, True), b
        nq, nt = len(kps[b]), len(kps[t])
        m_right, m_wrong = O.marks(idx[b], skip[b], skip[t], nq, nt), O.marks(idx[b], skip[b], skip[b], nq, nt)
        assert m_right[0].tobytes() == m_wrong[0].tobytes() and m_right[1].tobytes() != m_wrong[1].tobytes(), b


# ---- other pyramid tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.PYRAMID_OCTAVES))
def test_pyramid_pairs_are_live(name):
    """more than 20 correspondences fall to the octave test, at least 30 stay, the pair ends in state 0 under its table -- and another
    table, or exchanged weights, give other bytes"""
    pr, sc = OC.pyramid_pair(name)
    assert len(sc) == PC.PYRAMIDS[name][1]
    res, flags = same(pr, O.UPSTREAM, scale=sc)
    matched = np.flatnonzero(pr["idx"] >= 0)
    o1, o2 = pr["q_kp"]["octave"][matched], pr["t_kp"]["octave"][pr["idx"][matched]]
    inside = (o1 >= 0) & (o1 < len(sc)) & (o2 >= 0) & (o2 < len(sc))
    print(name, len(matched), int(inside.sum()), res["n_corr"], res["n_removed"], res["steps"])
    assert len(matched) == 100 and res["n_corr"] == inside.sum() >= 30 and (~inside).sum() > 20
    assert (~((o1 >= 0) & (o1 < len(sc)))).sum() > 5 and (~((o2 >= 0) & (o2 < len(sc)))).sum() > 5  # on either side
    assert res["state"] == 0 and 0 < res["n_removed"] < res["n_corr"] and min(res["steps"]) >= 1 and (flags[matched[~inside]] == 2).all()
    if len(sc) == 1:
        assert not o1[inside].any() and not o2[inside].any()  # one level: what stays has octave 0 on both sides
    else:
        assert (o1[inside] != o2[inside]).sum() > inside.sum() // 2  # the octaves of the two sides differ for most
        swapped = dict(pr, q_kp=pr["q_kp"].copy(), t_kp=pr["t_kp"].copy())
        swapped["q_kp"]["octave"][matched[inside]], swapped["t_kp"]["octave"][pr["idx"][matched[inside]]] = o2[inside], o1[inside]
        assert _differ(OC.solve_pair(swapped, O.UPSTREAM, scale=sc), (res, flags))[0]  # w1 for w2
    default = OC.solve_pair(pr, O.UPSTREAM)
    assert default[0]["n_corr"] != res["n_corr"] and _differ(default, (res, flags)) == (True, True)  # a kernel with the default table built in


# ---- the parameters at their limits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.LIMITS))
def test_limits_are_what_was_recorded(name):
    assert list(OC.LIMITS) == list(OC.LIMITS_RECORDED)
    allowed = OC.LIMITS[name][1]
    for pr, (state, steps, n_removed) in zip(OC.limit_pairs(), OC.LIMITS_RECORDED[name]):
        res, flags = same(pr, OC.limit_params(name))
        print(name, res["state"], res["steps"], res["n_removed"], res["n_inliers"])
        assert res["n_corr"] == OC.LIMITS_CORR and res["state"] in allowed
        assert (int(res["state"]), res["steps"].tolist(), int(res["n_removed"])) == (state, steps, n_removed)
    a, b = OC.limit_pairs()
    assert a["start"].tobytes() != b["start"].tobytes() and b["start"].tobytes() == OC.model_record(*OC.true_model()).tobytes()


def test_limits_cover_what_their_names_say():
    rec = OC.LIMITS_RECORDED
    assert rec["32 iterations in every round, step_eps 0"][0][1] == [32, 32] and rec["1 iteration in every round"][0][1] == [1, 1]
    assert [r[0] for r in rec["min_corr at the count"]] == [0, 0] and [r[0] for r in rec["min_corr one above the count"]] == [1, 1]
    for name in ("round 0 removes everything, min_inliers 0", "round 0 removes everything, min_inliers 0, lambda 0"):
        for pr in OC.limit_pairs():  # the second round starts with no correspondence left
            res, flags = OC.solve_pair(pr, OC.limit_params(name))
            assert res["n_removed"] == OC.LIMITS_CORR and res["n_inliers"] == 0 and res["steps"][0] == 5 and (flags[pr["rows"]] == 1).all()
    assert rec["round 0 removes everything, min_inliers 0"][0][:2] == (0, [5, 1])       # lambda alone gives the pivots
    assert rec["round 0 removes everything, min_inliers 0, lambda 0"][0][:2] == (2, [5, 0])  # no pivot: state 2 in the second round
    res, _ = OC.solve_pair(OC.limit_pairs()[0], OC.limit_params("round 0 removes everything, min_inliers 0, lambda 0"))
    R, t, s, _ = O.start(OC.limit_pairs()[0]["start"], False)
    assert res["r12"].tolist() != [float(v) for v in R] and not res["model"]["sr12"].any()  # the model of round 0 stays, no model is embedded


# ---- a singular system with finite sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix", [False, True], ids=["scale", "fix_scale"])
def test_singular_pair_ends_in_state_2_with_finite_sums(fix):
    """the third pivot is 0 by structure; the model stays the start, which is not the identity"""
    pr = OC.singular_pair(fix)
    p = dict(OC.SINGULAR_PARAMS, fix_scale=fix)
    res, flags = same(pr, p)
    R, t, s, ok = O.start(pr["start"], fix)
    assert ok and [float(v) for v in R] != [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and float(t[2]) == 0.5 and float(s) == (1.0 if fix else 2.0)
    assert res["state"] == 2 and res["n_corr"] == 30 and res["steps"].tolist() == [0, 0] and (flags[pr["rows"]] == 0).all()
    assert res["r12"].tolist() == [float(v) for v in R] and res["t12"].tolist() == [float(v) for v in t] and res["s12"] == s
    m = res["model"]
    assert m["state"] == 2 and not any(np.asarray(m[n]).any() for n in ("sr12", "t12", "s12", "sr21", "t21"))
    c = O.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale())
    assert not c["x1"][:, :2].any() and not c["x2"][:, :2].any() and len(set(c["x2"][:, 2].tolist())) > 10  # on the axes, at their own depths
    total = O.sums(c, O.cameras(pr["view1"], pr["view2"], p["chi2"]), R, t, s, True, np.ones(30, bool))
    H = {ab: float(total[q]) for q, ab in enumerate(O.H_PAIRS)}
    assert np.isfinite(total).all() and H[(0, 0)] > 0 and H[(1, 1)] - H[(0, 1)] ** 2 / H[(0, 0)] > 0
    assert all(H[(min(2, q), max(2, q))] == 0.0 for q in range(7)) and np.abs(total[28:30]).min() > 1.0  # the third pivot is 0 - 0 - 0
    assert O.solve(total, 0.0, 6 if fix else 7) is None and O.solve(total, 1e-8, 6 if fix else 7) is not None
    assert OC.solve_pair(pr, dict(p, lambda_=1e-8))[0]["state"] != 2  # the damping alone makes the system regular


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(chi2=0.0), dict(chi2=float("nan")), dict(chi2=float("inf")), dict(lambda_=-1.0), dict(lambda_=float("nan")), dict(step_eps=-1e-9),
           dict(iterations0=0), dict(iterations0=33), dict(iterations_more=0), dict(iterations_same=33), dict(min_corr=2), dict(min_inliers=-1),
           dict(reserved=(0, 0, 0, 1))]


@pytest.mark.parametrize("bad", REFUSED, ids=[str(b) for b in REFUSED])
def test_host_twin_refuses(bad):
    with pytest.raises(binding.OrbError) as e:
        host(OC.case_pair(1), dict(O.UPSTREAM, **bad))
    assert e.value.code == binding.SS_ERR_INVALID_ARG


def test_host_twin_refuses_null_and_takes_an_empty_pair():
    lib = binding.load()
    assert lib.ss_sim3_opt_host(None, None, None, 0, None, None, None, 0, None, None, None, 0, None, None, None, None, None) == binding.SS_ERR_INVALID_ARG
    pr = OC.case_pair(1)
    flags, res = binding.sim3_opt_host(pr["view1"], pr["q_xyz"][:0], pr["q_kp"][:0], pr["view2"], pr["t_xyz"][:0], pr["t_kp"][:0], pr["idx"][:0],
                                       pr["start"], PC.scale(), binding.sim3_opt_params())
    assert len(flags) == 0 and (res["state"], res["n_corr"]) == (1, 0)


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------------
def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/sim3opt_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "sim3opt_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sim3opt_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 40000
