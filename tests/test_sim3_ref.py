"""CPU tests of the Sim3 RANSAC as tests/sim3_ref.py states it, and of its C ABI surface: symbols and struct layouts, the draw, the
host twins ss_sim3_model_host and ss_sim3_check_host (the text the kernels compile) against the reference bit for bit, the model
against an independent derivation through numpy.linalg.eigh, the thresholds from both sides, the states and the selection on the
shared cases, upstream's sequential loop against the selection rule, refused arguments, and the stand-alone sanitizer run of the
steps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import proj_cases as PC
import sim3_cases as SC
import sim3_ref as S
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")
f32 = np.float32


def _same_model(got, want, tag):
    for name in S.MODEL_FIELDS:
        a, b = np.asarray(got[name]).view(np.int32), np.asarray(want[name]).view(np.int32)
        assert np.array_equal(a, b), f"{tag}: {name} {got[name]} != {want[name]}"


def test_symbols_structs_and_constants(tmp_path):
    names = ["ss_sim3_model_host", "ss_sim3_check_host", "ss_sim3_to_view", "ss_sim3_pairs_device", "ss_sim3_batch_device", "ss_sim3"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("sim3_pairs_device", "sim3_batch_device", "sim3"):
        assert callable(getattr(binding.OrbContext, m))
    for m in ("sim3_params", "sim3_model_host", "sim3_check_host", "sim3_to_view"):
        assert callable(getattr(binding, m))
    assert C.sizeof(binding.Sim3Params) == 32 and C.sizeof(binding.Sim3Result) == 128 and binding.SIM3_RESULT_DTYPE.itemsize == 128
    assert binding.SIM3_RESULT_DTYPE == S.RESULT_DTYPE
    assert tuple(n for n, _ in binding.Sim3Result._fields_) == S.RESULT_DTYPE.names
    assert binding.SS_SIM3_MAX_ITERATIONS == S.MAX_ITERATIONS == 1024
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_sim3_params) == 32, "params");\n'
                   '_Static_assert(sizeof(ss_sim3_result) == 128 && sizeof(ss_sim3_result) % 16 == 0, "result");\n'
                   '_Static_assert(offsetof(ss_sim3_params, min_inliers) == 4 && offsetof(ss_sim3_params, max_iterations) == 8 && '
                   'offsetof(ss_sim3_params, fix_scale) == 12 && offsetof(ss_sim3_params, seed) == 16 && offsetof(ss_sim3_params, reserved) == 20, '
                   '"params fields");\n'
                   '_Static_assert(offsetof(ss_sim3_result, t12) == 36 && offsetof(ss_sim3_result, s12) == 48 && offsetof(ss_sim3_result, sr21) == 52 && '
                   'offsetof(ss_sim3_result, t21) == 88 && offsetof(ss_sim3_result, state) == 100 && offsetof(ss_sim3_result, n_corr) == 104 && '
                   'offsetof(ss_sim3_result, n_inliers) == 108 && offsetof(ss_sim3_result, best_inliers) == 112 && '
                   'offsetof(ss_sim3_result, iteration) == 116 && offsetof(ss_sim3_result, status) == 120 && offsetof(ss_sim3_result, reserved) == 124, '
                   '"result fields");\n'
                   '_Static_assert(SS_SIM3_MAX_ITERATIONS == 1024 && SS_TRI_SWEEPS == 6, "constants");\n'
                   '_Static_assert(SS_GUIDED_MAX_ROWS == 16384 && SS_ABI_VERSION == 5 && SS_MAX_LEVELS == 16, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5
    assert "tests/sim3_ref.py is its normative" in text and "real binary stays unpinned, as for the guided, bag-of-words, projection, epipolar" in text
    for word in ("the draw stream", "atan2 and Rodrigues", "the model in double", "max_iterations is the caller's number", "iterate(20)", "chi2 is a parameter"):
        assert word in text, word  # every deviation is listed


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 64, 16384])
def test_draws_are_distinct_in_range_and_the_literal_array_form(n):
    seen = set()
    for seed, pair in ((0, 0), (1, 0), (0xDEADBEEF, 7), (0xFFFFFFFF, 65535)):
        for t in range(300):
            d = S.draw(seed, pair, t, n)
            assert len(set(d)) == 3 and all(0 <= v < n for v in d), (n, seed, pair, t, d)
            assert d == S.draw_literal(seed, pair, t, n), (n, seed, pair, t)
            if n == 3:
                assert sorted(d) == [0, 1, 2]
            seen.update(d)
    if n <= 64:
        assert seen == set(range(n))  # every index is drawn some time
    # the stream depends on the seed, the pair and the hypothesis
    assert len({tuple(S.draw(s, p, t, 16384)) for s in (0, 1) for p in (0, 1) for t in (0, 1)}) == 8


def test_mix32_is_the_written_function():
    assert S.mix32(0, 0, 0) == 0 and S.mix32(0, 0, 1) != S.mix32(0, 1, 0)
    h = (1 ^ (2 * 0x9E3779B1 & S.M32)) + 3 * 0x85EBCA77 & S.M32
    h ^= h >> 16
    h = h * 0x7FEB352D & S.M32
    h ^= h >> 15
    h = h * 0x846CA68B & S.M32
    assert S.mix32(1, 2, 3) == h ^ (h >> 16)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _special_triples():
    a = f32([[0, 0, 5], [1, 0, 5], [0, 1, 6]])
    collinear = f32([[0, 0, 4], [1, 1, 5], [2, 2, 6]])
    same = f32([[1, 2, 3]] * 3)
    half_turn = a * f32([-1, -1, 1])  # 180 degrees about z: q.w = 0
    inf = a.copy()
    inf[1, 1] = np.inf
    nan = a.copy()
    nan[2, 0] = np.nan
    huge = a * f32(1e30)
    return [("identity", a, a), ("collinear", collinear, collinear * f32(2)), ("collinear against a triangle", a, collinear),
            ("three identical points", same, same), ("identical against a triangle", a, same), ("180 degrees about z", half_turn, a),
            ("180 degrees about x", a * f32([1, -1, -1]), a), ("an infinite coordinate", inf, a), ("a NaN coordinate", a, nan),
            ("huge coordinates", huge, a), ("huge on both sides", huge, huge)]


def test_model_twin_agrees_with_the_restatement():
    rng = np.random.Generator(np.random.PCG64(0x513))
    x1, x2 = SC.random_triples(rng, 400)
    zero = 0
    for fix in (False, True):
        p = binding.sim3_params(fix_scale=fix)
        for k in range(len(x1)):
            _same_model(binding.sim3_model_host(p, x1[k], x2[k]), S.model(x1[k], x2[k], fix), f"random triple {k}, fix_scale {fix}")
        for name, a, b in _special_triples():
            got, want = binding.sim3_model_host(p, a, b), S.model(a, b, fix)
            _same_model(got, want, f"{name}, fix_scale {fix}")
            assert all(np.isfinite(got[n]).all() for n in S.MODEL_FIELDS), name  # NaN -> the defined zero model
            zero += int(not np.any(got["sr12"]))
            if name == "180 degrees about z":
                assert np.allclose(got["sr12"].reshape(3, 3), np.diag([-1, -1, 1.0]), atol=1e-6) and np.allclose(got["t12"], 0, atol=1e-5)
        got = binding.sim3_model_host(p, x1[0], x2[0])
        assert (got["state"], got["iteration"], got["n_corr"], got["status"]) == (0, -1, 0, 0)
    assert zero >= 6  # identical points without fix_scale, NaN and infinite coordinates give the zero model
    # exact correspondences of the synthetic scene give back its Sim3
    c = SC.corr_of(SC.make_pair(11, 30))
    m = binding.sim3_model_host(binding.sim3_params(), c["x1"][[0, 9, 17]], c["x2"][[0, 9, 17]])
    assert abs(float(m["s12"]) - SC.S_TRUE) < 1e-5 and np.allclose(m["sr12"].reshape(3, 3), SC.S_TRUE * SC.rodrigues(SC.AXIS, SC.ANGLE), atol=1e-5)
    assert np.allclose(m["t12"], SC.T_TRUE, atol=1e-4)
    assert np.allclose(m["sr21"].reshape(3, 3) @ m["sr12"].reshape(3, 3), np.eye(3), atol=1e-6)


MIN_SIDE = 0.25       # no side of a case's triangles is under this fraction of the longest
EIGH_MEASURED = 1.16e-7  # the largest deviation of s.R and t12 from the eigh route over the 300 cases, as measured when this was written


def _conditioned_triples(rng, n):
    """triangles near equilateral by construction (noise of at most 0.2 radius on a radius-r circle: the shortest side is at least
    0.42 of the longest) in keyframe 2, the same under a random similarity plus 1 % noise in keyframe 1"""
    out = []
    for _ in range(n):
        r, c = rng.uniform(0.5, 3.0), rng.normal(0, 1, 3) + [0, 0, 6]
        basis = SC.rodrigues(*(lambda a: (a / np.linalg.norm(a), rng.uniform(0, np.pi)))(rng.normal(0, 1, 3)))
        tri = np.array([[np.cos(2 * np.pi * k / 3), np.sin(2 * np.pi * k / 3), 0.0] for k in range(3)]) * r
        x2 = c + tri @ basis.T + rng.uniform(-1, 1, (3, 3)) * (0.2 * r / np.sqrt(3))
        axis = rng.normal(0, 1, 3)
        rot, s, t = SC.rodrigues(axis / np.linalg.norm(axis), rng.uniform(0, 3.0)), rng.uniform(0.5, 2.0), rng.normal(0, 1, 3)
        x1 = s * (x2 @ rot.T) + t + rng.normal(0, 0.01 * r, (3, 3))
        out.append((x1.astype(f32), x2.astype(f32)))
    return out


def _horn_eigh(x1, x2):
    """Horn 1987 through numpy: the quaternion by numpy.linalg.eigh, the rotation by angle and axis (upstream's route)"""
    p1, p2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    o1, o2 = p1.mean(0), p2.mean(0)
    a, b = p1 - o1, p2 - o2
    m = b.T @ a
    n = np.array([[m[0, 0] + m[1, 1] + m[2, 2], m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]],
                  [0, m[0, 0] - m[1, 1] - m[2, 2], m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]],
                  [0, 0, -m[0, 0] + m[1, 1] - m[2, 2], m[1, 2] + m[2, 1]],
                  [0, 0, 0, -m[0, 0] - m[1, 1] + m[2, 2]]])
    n = n + np.triu(n, 1).T
    w, v = np.linalg.eigh(n)
    q = v[:, np.argmax(w)]
    vec = q[1:]
    ang = np.arctan2(np.linalg.norm(vec), q[0])
    rot = SC.rodrigues(vec / np.linalg.norm(vec), 2 * ang)
    p3 = b @ rot.T
    s = (a * p3).sum() / (p3 * p3).sum()
    return s * rot, o1 - s * rot @ o2


def test_model_against_an_independent_derivation():
    """Measured over these 300 cases: the largest deviation of s.R and t12 from the eigh route is 1.16e-7, which is the float32
    rounding of the model's entries (2^-24 of entries of magnitude 1 to 4) and nothing of the Jacobi sweeps.  The bound is ten times
    that, for LAPACK builds that differ in the last bits."""
    rng = np.random.Generator(np.random.PCG64(0xE16))
    cases = _conditioned_triples(rng, 300)
    worst = 0.0
    p = binding.sim3_params()
    for x1, x2 in cases:
        assert SC.shortest_side_fraction(x1) >= MIN_SIDE and SC.shortest_side_fraction(x2) >= MIN_SIDE
        got = binding.sim3_model_host(p, x1, x2)
        sr, t = _horn_eigh(x1, x2)
        worst = max(worst, float(np.abs(got["sr12"].reshape(3, 3) - sr).max()), float(np.abs(got["t12"] - t).max()))
    print("largest deviation of s.R, t12 from the eigh route:", worst)
    assert worst <= 10 * EIGH_MEASURED


# ---- thresholds --------------------------------------------------------------------------------------------------------------------
def test_thresholds_from_both_sides_and_the_octave_table():
    sc1 = np.ones(8, f32)  # scale 1 on every level: max = chi2
    pr = SC.make_pair(21, 12, octaves=(0,))
    v1, v2 = pr["view1"], pr["view2"]
    rows, cols = pr["rows"], pr["idx"][pr["rows"]]
    c = SC.corr_of(pr, scale=sc1)
    # a model a little off the scene's, so that both errors are ordinary positive numbers
    x1 = c["x1"][[0, 5, 9]] + f32([[0.01, 0, 0], [0, 0.01, 0], [0, 0, -0.01]])
    m = S.model(x1, c["x2"][[0, 5, 9]])
    e1, e2 = S.errors(c, m, v1, v2)
    assert (e1 > 0).all() and (e2 > 0).all() and np.isfinite(e1).all() and np.isfinite(e2).all()
    q, t = pr["q_xyz"][rows], pr["t_xyz"][cols]
    qk, tk = pr["q_kp"][rows], pr["t_kp"][cols]
    big = binding.sim3_params(chi2=1e30)
    out, err = binding.sim3_check_host(big, v1, v2, sc1, q, qk, t, tk, m)
    assert (out == 0).all() and np.array_equal(err[:, 0].view(np.int32), e1.view(np.int32)) and np.array_equal(err[:, 1].view(np.int32), e2.view(np.int32))
    for k in range(len(rows)):
        one = (q[k:k + 1], qk[k:k + 1], t[k:k + 1], tk[k:k + 1])
        lo, hi = float(min(e1[k], e2[k])), float(max(e1[k], e2[k]))
        first_is_larger = e1[k] >= e2[k]
        # chi2 on the larger error: rejected under the strict <, by the test that error belongs to; one ulp above: accepted
        assert binding.sim3_check_host(binding.sim3_params(chi2=hi), v1, v2, sc1, *one, m)[0][0] == (2 if first_is_larger else 3)
        assert binding.sim3_check_host(binding.sim3_params(chi2=float(np.nextafter(f32(hi), f32(np.inf)))), v1, v2, sc1, *one, m)[0][0] == 0
        # chi2 on the smaller error: that test rejects too; test 1 is reported first
        assert binding.sim3_check_host(binding.sim3_params(chi2=lo), v1, v2, sc1, *one, m)[0][0] == 2
        if e1[k] < e2[k]:  # e1 < chi2 <= e2: the second test alone
            assert binding.sim3_check_host(binding.sim3_params(chi2=float(np.nextafter(f32(lo), f32(np.inf)))), v1, v2, sc1, *one, m)[0][0] == 3
    # the reference takes the same side at every threshold
    for k in range(len(rows)):
        for e in (e1[k], e2[k]):
            for chi2 in (e, np.nextafter(e, f32(np.inf))):
                ck = SC.corr_of(pr, chi2=float(chi2), scale=sc1)
                want = S.inliers(ck, m, v1, v2)[k]
                got = binding.sim3_check_host(binding.sim3_params(chi2=float(chi2)), v1, v2, sc1, q[k:k + 1], qk[k:k + 1], t[k:k + 1], tk[k:k + 1], m)[0][0]
                assert (got == 0) == bool(want)
    # an octave at the last table entry is a correspondence with that entry's scale; one outside the table is none
    sc = PC.scale()
    for side in (0, 1):
        for octave, want in ((len(sc) - 1, True), (len(sc), False), (-1, False), (1 << 30, False)):
            kp = [qk[:1].copy(), tk[:1].copy()]
            kp[side]["octave"] = octave
            out, err = binding.sim3_check_host(big, v1, v2, sc, q[:1], kp[0], t[:1], kp[1], m)
            assert (out[0] != 1) == want, (side, octave)
            pr2 = dict(pr, q_kp=pr["q_kp"].copy(), t_kp=pr["t_kp"].copy())
            pr2["q_kp" if side == 0 else "t_kp"]["octave"][rows[0] if side == 0 else cols[0]] = octave
            c2 = SC.corr_of(pr2, scale=sc)
            assert (rows[0] in c2["rows"]) == want
            if want:
                s_last = sc[len(sc) - 1]
                assert c2["max1" if side == 0 else "max2"][0] == f32(9.210) * (s_last * s_last)
                # the error that sits exactly on chi2 * s^2 is rejected, chi2 one ulp up accepts it
                e = err[0, side]
                chi_on = f32(e) / (s_last * s_last)
                for chi2 in np.nextafter(chi_on, f32(0)), chi_on, np.nextafter(chi_on, f32(np.inf)):
                    mx = f32(chi2) * (s_last * s_last)
                    got = binding.sim3_check_host(binding.sim3_params(chi2=float(chi2)), v1, v2, sc, q[:1], kp[0], t[:1], kp[1], m)[0][0]
                    other_ok = err[0, 1 - side] < f32(chi2) * (sc[kp[1 - side]["octave"][0]] ** 2)
                    assert (got == 0) == bool(e < mx and other_ok)


# ---- selection and states ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SC.CASES)), ids=SC.CASE_NAMES)
def test_cases_reach_their_states_on_the_reference(k):
    case, pr = SC.CASES[k], SC.case_pair(k)
    p = case["params"]
    for pair in (0, 1, 2):  # the pair numbers the GPU test runs them under
        res, flags, counts = SC.reference(k, pair)
        assert res["state"] == case["expect_state"], (case["name"], pair, res)
        assert res["n_corr"] == case["pair_kw"]["n"] == len(pr["rows"])
        if res["state"] == 1:
            assert counts is None and not flags.any() and res["best_inliers"] == 0 and res["iteration"] == -1
            continue
        # every count again, one hypothesis at a time
        c = SC.corr_of(pr, p["chi2"])
        again = [int(S.inliers(c, S.hypothesis(c, t, p["seed"], pair, p["fix_scale"]), pr["view1"], pr["view2"]).sum()) for t in range(p["max_iterations"])]
        assert again == list(counts) and res["best_inliers"] == max(again)
        over = [t for t, n in enumerate(again) if n > p["min_inliers"]]
        if res["state"] == 0:
            assert res["iteration"] == over[0] and res["n_inliers"] == again[over[0]] == flags.sum()
            assert np.array_equal(np.flatnonzero(flags), pr["inlier_rows"]), case["name"]  # the known inlier set
            assert all(n <= p["min_inliers"] for n in again[:over[0]])
        else:
            assert not over and not flags.any() and res["n_inliers"] == 0 and res["iteration"] == -1
            assert not any(np.any(res[n]) for n in S.MODEL_FIELDS)
    by = {c["name"]: SC.reference(i)[0] for i, c in enumerate(SC.CASES)}
    assert by["boundary: 20 correspondences at min_inliers 20"]["best_inliers"] == 20  # the strict >
    assert by["degenerate: every correspondence is one point"]["best_inliers"] == 0
    assert by["fix_scale on a scene of scale 1"]["s12"] == 1.0
    assert abs(float(by["state 0: 60 correspondences, 24 gross outliers"]["s12"]) - SC.S_TRUE) < 1e-4


@pytest.mark.parametrize("k", range(len(SC.CASES)), ids=SC.CASE_NAMES)
def test_upstream_sequential_loop_selects_the_same_model(k):
    case, pr = SC.CASES[k], SC.case_pair(k)
    p = case["params"]
    c = SC.corr_of(pr, p["chi2"])
    for pair in (0, 1, 2):
        res = SC.reference(k, pair)[0]
        t, m, best = S.upstream_iterate(pr["view1"], pr["view2"], c, p["min_inliers"], p["max_iterations"], p["fix_scale"], p["seed"], pair)
        assert t == res["iteration"] and best == (res["n_inliers"] if res["state"] == 0 else res["best_inliers"])
        if t >= 0:
            _same_model(m, res, case["name"])
        else:
            assert res["state"] in (1, 2)


# ---- odd cameras: what makes the camera tests of tests/test_sim3.py able to fail -----------------------------------------------------------
# the principal point cancels in both reprojection errors: (fx x / z + cx) - (fx x' / z' + cx)
SIM3_EXEMPT = {"cx and cy exchanged": "both projections of an error carry the same principal point, which the difference removes"}


def _differs(a, b):
    """in the bytes tests/test_sim3.py compares: the result record and the flags"""
    return a[0].tobytes() != b[0].tobytes() or not np.array_equal(a[1], b[1])


def test_camera_pairs_are_what_their_name_says():
    """noisy scenes of 60 correspondences with 12 gross outliers under (P, Q), (Q, P) and (square, P): state 0 at every min_inliers of
    the calls, with more inliers than min_inliers and fewer than correspondences; the noise-free scene does not depend on the cameras"""
    assert len({(pr["view1"].tobytes(), pr["view2"].tobytes()) for pr in SC.camera_pairs()}) == 3
    for m in SC.CAMERA_MIN_INLIERS:
        for b, (res, flags, counts) in enumerate(SC.camera_reference(m)):
            assert res["state"] == 0 and res["n_corr"] == 60 and m < res["n_inliers"] == flags.sum() < 60, (m, b, res)
            assert set(np.flatnonzero(flags).tolist()) <= set(SC.camera_pairs()[b]["inlier_rows"].tolist())
            assert (counts[:res["iteration"]] <= m).all() and len(set(counts.tolist())) > 10
    assert len({int(r[0]["iteration"]) for m in SC.CAMERA_MIN_INLIERS for r in SC.camera_reference(m)}) >= 4
    for b, pr in enumerate(SC.camera_pairs()):  # the host twin under the winner: both errors of every correspondence, bit for bit
        res, flags, _ = SC.camera_reference(20)[b]
        c = SC.corr_of(pr)
        e1, e2 = S.errors(c, res, pr["view1"], pr["view2"])
        out, err = binding.sim3_check_host(binding.sim3_params(), pr["view1"], pr["view2"], PC.scale(), pr["q_xyz"][c["rows"]], pr["q_kp"][c["rows"]],
                                           pr["t_xyz"][c["cols"]], pr["t_kp"][c["cols"]], res)
        assert np.array_equal(err[:, 0].view(np.int32), e1.view(np.int32)) and np.array_equal(err[:, 1].view(np.int32), e2.view(np.int32)), b
        assert np.array_equal(out == 0, flags[c["rows"]] == 1) and {0, 2} <= set(out.tolist())
    clean = SC.make_pair(90, **SC.CAMERA_PAIR)
    p = SC.camera_params(20)
    plain = SC.solve_pair(clean, p)
    for c1, c2 in CC.SIM3_PAIR_CAMERAS:
        other = SC.solve_pair(SC.with_cameras(clean, c1, c2), p)
        assert np.array_equal(other[1], plain[1]) and np.array_equal(other[2], plain[2])  # the gap the noise closes


@pytest.mark.parametrize("mixup", list(CC.PAIR_MIXUPS))
def test_camera_mixups_change_the_reference_of_the_pairs_form(mixup):
    """every pair whose cameras a mix-up changes has other result bytes or flags in one of the calls at least"""
    cams = list(CC.SIM3_PAIR_CAMERAS)
    mixed = CC.PAIR_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed, fields=(0, 1, 2, 3))
    assert hit, mixup
    for b in hit:
        wrong = SC.with_cameras(SC.camera_pairs()[b], *mixed[b])
        live = [_differs(SC.solve_pair(wrong, SC.camera_params(m), b), SC.camera_reference(m)[b]) for m in SC.CAMERA_MIN_INLIERS]
        counts = [not np.array_equal(SC.solve_pair(wrong, SC.camera_params(m), b)[2], SC.camera_reference(m)[b][2]) for m in SC.CAMERA_MIN_INLIERS[:1]]
        if mixup in SIM3_EXEMPT:
            assert not any(live) and not any(counts), (mixup, b)  # the exemption is not stale
        else:
            assert any(live) and all(counts), (mixup, b, live)
    assert len(SIM3_EXEMPT) <= 1


@pytest.mark.parametrize("mixup", [m for m in CC.FRAME_MIXUPS if m != "bf of another frame"])  # no step of the rule reads bf
def test_camera_mixups_change_the_reference_of_the_batch_form(mixup):
    """the batch form: frame b's view is side 1 of pair b, frame train_src[b]'s its side 2"""
    cams = list(CC.SIM3_FRAME_CAMERAS)
    wrong_views = SC.frame_views(CC.FRAME_MIXUPS[mixup](cams))
    for b in (1, 2):
        right = [SC.solve_pair(SC.batch_pair(b), SC.camera_params(m), b) for m in SC.CAMERA_MIN_INLIERS]
        wrong = [SC.solve_pair(SC.batch_pair(b, wrong_views), SC.camera_params(m), b) for m in SC.CAMERA_MIN_INLIERS]
        live = [_differs(w, r) for w, r in zip(wrong, right)]
        for m, r in zip(SC.CAMERA_MIN_INLIERS, right):
            assert r[0]["state"] == 0 and r[0]["n_corr"] == 60 and m < r[0]["n_inliers"] < 60
        assert any(live) != (mixup in SIM3_EXEMPT), (mixup, b, live)
    assert SC.solve_pair(SC.batch_pair(0), SC.camera_params(20), 0)[0]["state"] == 1
    kps = SC.camera_batch()[0]
    assert max(len(k) for k in kps) <= 600 and len({int(o) for o in kps[1]["octave"][SC.camera_batch()[2][1][:len(kps[1])] >= 0]}) > 3


def test_to_view_is_upstreams_composition():
    cam = binding.Camera(fx=SC.F, fy=SC.F, cx=SC.CX, cy=SC.CY, width=SC.W, height=SC.H)
    res = SC.reference(0)[0]
    rcw2, tcw2 = SC.POSE2
    view, srcw, t = binding.sim3_to_view(cam, res, rcw2, tcw2, bf=40.0)
    want_m, want_t = S.to_scw(res, rcw2, tcw2)
    assert np.array_equal(srcw, want_m) and np.array_equal(t, want_t)
    assert bytes(view) == bytes(binding.fuse_view_sim3(cam, want_m, want_t, bf=40.0))
    # it takes keyframe 2's world points into keyframe 1's camera, up to the scale: the projections agree with the direct ones
    pr = SC.case_pair(0)
    rows = pr["inlier_rows"][:5]
    w2 = np.stack([pr["t_xyz"][n][pr["idx"][rows]] for n in "xyz"], 1).astype(np.float64)
    x1 = w2 @ srcw.T + t
    w1 = np.stack([pr["q_xyz"][n][rows] for n in "xyz"], 1).astype(np.float64)
    direct = w1 @ np.asarray(SC.POSE1[0]).T + SC.POSE1[1]
    assert np.allclose(x1, direct, atol=1e-4)
    with pytest.raises(binding.OrbError) as e:
        binding.sim3_to_view(cam, SC.reference(2)[0], rcw2, tcw2)  # state 2: no model
    assert e.value.code == binding.SS_ERR_INVALID_ARG


def test_chain_is_live_on_the_reference():
    """BoW match -> Sim3 RANSAC -> Scw -> the candidate check's projection search on the references, before the device is asked: the
    match finds the planted couples, the RANSAC the planted inliers, and the projection search names, for the map point of every
    RANSAC inlier, the query row it was matched to"""
    pr = SC.chain_scene()
    bow, (res, flags, counts), view, fuse = SC.chain_reference()
    assert np.array_equal(bow[0], pr["idx"]) and bow[3]["n_final"] == 48
    assert res["state"] == 0 and np.array_equal(np.flatnonzero(flags), pr["inlier_rows"]) and res["n_inliers"] == 40
    rows = np.flatnonzero(flags)
    assert all(fuse[0][pr["idx"][i]] == i for i in rows)
    assert fuse[4]["n_add"] >= len(rows) and set(int(v) for v in fuse[3]["level"][fuse[3]["state"] == 0]) == {1}


def test_invalid_arguments_are_refused_without_a_device():
    """the parameter check of the device calls (one function in the library) through the host twins, which need no context; the
    checks that need one (rows) are in tests/test_sim3.py"""
    a = f32([[0, 0, 5], [1, 0, 5], [0, 1, 6]])
    nan, inf = float("nan"), float("inf")
    bad = [dict(chi2=0.0), dict(chi2=-1.0), dict(chi2=nan), dict(chi2=inf), dict(min_inliers=-1), dict(max_iterations=0), dict(max_iterations=-5),
           dict(max_iterations=1025), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, -1))]
    pr = SC.make_pair(3, 4)
    for kw in bad:
        with pytest.raises(binding.OrbError) as e:
            binding.sim3_model_host(binding.sim3_params(**kw), a, a)
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
        with pytest.raises(binding.OrbError) as e:
            binding.sim3_check_host(binding.sim3_params(**kw), pr["view1"], pr["view2"], PC.scale(), pr["q_xyz"][:1], pr["q_kp"][:1], pr["t_xyz"][:1],
                                    pr["t_kp"][:1], S.model(a, a))
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    for good in (dict(chi2=1e-30), dict(min_inliers=0), dict(max_iterations=1), dict(max_iterations=1024), dict(seed=0xFFFFFFFF), dict(min_inliers=1 << 30)):
        binding.sim3_model_host(binding.sim3_params(**good), a, a)
    for levels in (np.zeros(0, f32), np.ones(17, f32)):
        with pytest.raises(binding.OrbError):
            binding.sim3_check_host(binding.sim3_params(), pr["view1"], pr["view2"], levels, pr["q_xyz"][:1], pr["q_kp"][:1], pr["t_xyz"][:1], pr["t_kp"][:1],
                                    S.model(a, a))
    lib = binding.load()
    p = binding.sim3_params()
    assert lib.ss_sim3_pairs_device(None, None, None, None, None, None, None, None, None, None, 0, 1, None, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_sim3_batch_device(None, None, None, None, None, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_sim3(None, None, None, None, None, 0, None, None, None, None, 0, None, C.byref(p), None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_sim3_model_host(None, None, None, None) == binding.SS_ERR_INVALID_ARG


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/sim3_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "sim3_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sim3_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 50000
