"""CPU tests of the two-view initialisation as tests/two_view_ref.py states it, and of its C ABI surface: symbols and struct layouts,
the draw, the host twins ss_two_view_model_host, ss_two_view_check_host, ss_two_view_accept_host and ss_two_view_host (the text the
kernels compile) against the restatement bit for bit, the models against an independent derivation (numpy.linalg.svd on the same DLT
matrices) and the planted motions, the thresholds from both sides, the states and reasons on the shared cases, the tracker's own
sst_two_view on the same scenes, the recovery of planted inliers, refused arguments, and the stand-alone sanitizer run of the steps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_ref
import proj_cases as PC
import two_view_cases as TC
import two_view_ref as R
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")
f32 = np.float32

# The largest deviation of a model of MODEL_N octuples with exact projections from numpy's SVD of the same DLT matrix (the smallest
# right singular vector; for F then the truncation of the third singular value), both scaled to unit Frobenius norm and one sign,
# measured once with this file (the tests print it): H 1.8e-13, F 6.7e-10 (DESIGN.md section 30 holds them too).  The bounds are ten
# times those figures.  The conditioning guard: the second smallest singular value of the DLT matrix over the largest
MODEL_N = 300
MIN_GAP = 1e-3
BOUND_H = 1.8e-12
BOUND_F = 6.7e-9
# the third singular value of the twin's F, taken back to normalised coordinates by numpy, over the first: measured 4.8e-16 (numpy's
# own inverse and products are in that figure), asserted at ten times
BOUND_RANK2 = 4.8e-15
# the planted motion on exact scenes (rotation angle, angle of the translation direction; radians): measured 5.3e-7 and 4.8e-6 over the
# exact cases, where the rounding of u, v to float32 is the data's own error; asserted at ten times
BOUND_MOTION = (5.3e-6, 4.8e-5)


def _params(**kw):
    return binding.two_view_params(**kw)


def test_symbols_structs_and_constants(tmp_path):
    names = ["ss_two_view_host", "ss_two_view_model_host", "ss_two_view_check_host", "ss_two_view_accept_host", "ss_two_view_beats_host",
             "ss_two_view_point_tests_host", "ss_two_view_pairs_device", "ss_two_view_batch_device", "ss_two_view"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("two_view_pairs_device", "two_view_batch_device", "two_view"):
        assert callable(getattr(binding.OrbContext, m))
    assert C.sizeof(binding.TwoViewParams) == 64 and binding.TWO_VIEW_RESULT_DTYPE.itemsize == 192
    assert binding.SS_TWO_VIEW_MAX_ITERATIONS == 1024 and binding.SS_TWO_VIEW_COS_1DEG == float(np.cos(np.deg2rad(1.0)))
    p = _params()
    assert (p.chi2_h, p.chi2_f, p.chi2_score, p.rh_threshold, p.min_triangulated, p.max_iterations) == (5.991, 3.841, 5.991, 0.45, 50, 200)
    off_p = dict(chi2_h=0, chi2_f=8, chi2_score=16, rh_threshold=24, cos_min_parallax=32, min_triangulated=40, max_iterations=44, seed=48, reserved=52)
    off_r = dict(r21=0, t21=72, score_h=96, score_f=104, cos_parallax=112, state=120, reason=124, status=128, model=132, iteration_h=136, iteration_f=140,
                 n_corr=144, n_inliers=148, n_good=152, n_triangulated=156, reserved=160)
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_two_view_params) == 64 && sizeof(ss_two_view_result) == 192, "sizes");\n' +
                   "".join(f'_Static_assert(offsetof(ss_two_view_params, {f}) == {o}, "{f}");\n' for f, o in off_p.items()) +
                   "".join(f'_Static_assert(offsetof(ss_two_view_result, {f}) == {o}, "{f}");\n' for f, o in off_r.items()) +
                   '_Static_assert(SS_TWO_VIEW_MAX_ITERATIONS == 1024 && SS_ABI_VERSION == 5 && SS_GUIDED_MAX_ROWS == 16384, "constants");\n'
                   '_Static_assert(offsetof(ss_two_view_result, r21) == offsetof(ss_pnp_result, rcw) && offsetof(ss_two_view_result, t21) == '
                   'offsetof(ss_pnp_result, tcw), "the twelve doubles lie as the other results have them");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    for f, o in off_p.items():
        assert getattr(binding.TwoViewParams, f).offset == o, f
    for f, o in off_r.items():
        assert binding.TWO_VIEW_RESULT_DTYPE.fields[f][1] == o, f
    assert lib.ss_abi_version() == 5
    for word in ("the draw stream", "inverse iteration and Jacobi where upstream calls cv::SVD", "cosines instead of degrees", "rh_threshold is a",
                 "every hypothesis is scored", "parity with the real binary stays unpinned", "triangulation in normalised coordinates",
                 "an octave outside the", "tests/two_view_ref.py is"):
        assert word in text, word  # every deviation is listed


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 9, 64, 16384])
def test_draws_are_distinct_in_range_and_the_twin_draws_them(n):
    """the eight draws of the restatement are distinct, in range, a permutation at 8 and the literal swap-with-last; ss_two_view_host
    with one hypothesis is the restatement of that hypothesis' eight draws bit for bit, whatever the seed and the problem number"""
    assert binding.TWO_VIEW_RESULT_DTYPE == R.RESULT_DTYPE and binding.MAP_POINT_DTYPE == R.MAP_POINT_DTYPE
    for seed, problem in ((0, 0), (1, 0), (0xDEADBEEF, 7), (0xFFFFFFFF, 65535)):
        for t in range(200):
            d = R.draw(seed, problem, t, n)
            assert len(set(d)) == 8 and all(0 <= v < n for v in d), (n, seed, problem, t, d)
            assert d == pnp_ref.draw_literal(seed, problem, t, n, 8), (n, seed, problem, t)
            if n == 8:
                assert sorted(d) == list(range(8))
    # at 16 384 all but 300 matches are gross outliers: the one hypothesis then has few inliers to triangulate and the restatement stays quick
    sc = TC.make_scene(100 + n, n, 0, n + 2, n + 1, motion=TC.WIDE) if n <= 64 else TC.make_scene(100 + n, n, n - 300, n, n, motion=TC.WIDE)
    seen = set()
    for seed, problem in ((0, 0), (1, 0), (0, 1), (0xFFFFFFFF, 65535), (77, 3))[:5 if n <= 64 else 2]:
        p = dict(max_iterations=1, seed=seed, min_triangulated=0)
        want, got = TC.solve_scene(sc, p, problem), TC.host(sc, p, problem)
        _same(got, want, f"N {n}, seed {seed}, problem {problem}")
        seen.add(float(want[3]["score_f"]))
    assert len(seen) >= (1 if n == 8 else 2)  # at 8 every hypothesis draws all eight


def _same(got, want, tag):
    """(flags, points, point rows, result) of a twin against the restatement's, bit for bit"""
    for name in R.RESULT_DTYPE.names:
        assert np.asarray(got[3][name]).tobytes() == np.asarray(want[3][name]).tobytes(), f"{tag}: result.{name} {got[3][name]} != {want[3][name]}"
    assert np.array_equal(got[0], want[0]), f"{tag}: flags"
    assert got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]), f"{tag}: points"


def _corr(sc):
    rows = sc["rows"]
    j = sc["idx"][rows]
    return np.stack([sc["kp1"]["x"][rows], sc["kp1"]["y"][rows], sc["kp2"]["x"][j], sc["kp2"]["y"][j]], axis=1).astype(f32)


def _normalise(c):
    """step 2 in numpy -> (normalised n x 4, T1, T2)"""
    c = np.asarray(c, np.float64)
    m = c.mean(axis=0)
    d = np.abs(c - m).mean(axis=0)
    T = lambda a, b: np.array([[1 / d[a], 0, -m[a] / d[a]], [0, 1 / d[b], -m[b] / d[b]], [0, 0, 1.0]])  # noqa: E731
    return (c - m) / d, T(0, 1), T(2, 3)


def _dlt_f(p):
    return np.stack([p[:, 2] * p[:, 0], p[:, 2] * p[:, 1], p[:, 2], p[:, 3] * p[:, 0], p[:, 3] * p[:, 1], p[:, 3], p[:, 0], p[:, 1], np.ones(len(p))], axis=1)


def _dlt_h(p):
    rows = []
    for u1, v1, u2, v2 in p:
        rows += [[0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2], [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]]
    return np.array(rows)


def _svd_models(c8, norm_of=None):
    """H21 and F21 of eight correspondences by numpy's SVD under the normalisation of `norm_of` (default: their own) -> (H, F, gaps)"""
    pn, T1, T2 = _normalise(c8 if norm_of is None else norm_of)
    if norm_of is not None:
        c = np.asarray(norm_of, np.float64)
        m, d = c.mean(axis=0), np.abs(c - c.mean(axis=0)).mean(axis=0)
        pn = (np.asarray(c8, np.float64) - m) / d
    _, sh, vh = np.linalg.svd(_dlt_h(pn))
    _, sf, vf = np.linalg.svd(_dlt_f(pn), full_matrices=True)
    Hn, Fn = vh[8].reshape(3, 3), vf[8].reshape(3, 3)
    u, s, vt = np.linalg.svd(Fn)
    Fn = u @ np.diag([s[0], s[1], 0.0]) @ vt
    return np.linalg.inv(T2) @ Hn @ T1, T2.T @ Fn @ T1, (sh[7] / sh[0], sf[6] / sf[0])


def _unit_diff(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def test_the_draws_of_the_twin_are_the_restatements():
    """ss_two_view_host with one hypothesis scores the F of that hypothesis' eight draws: the score of numpy's F of the restated draws
    under the problem's normalisation is the twin's to rounding, and the seed and the problem number each change it"""
    sc = TC.case_scene(3)
    c = _corr(sc)
    seen = set()
    for seed, problem in ((0, 0), (1, 0), (0, 1), (0xFFFFFFFF, 65535), (77, 3)):
        res = TC.host(sc, dict(max_iterations=1, seed=seed), problem)[3]
        d = pnp_ref.draw(seed, problem, 0, len(c), 8)
        _, F, _ = _svd_models(c[d], norm_of=c)
        out = binding.two_view_check_host(_params(), sc["view"], c, f21=F)
        assert res["iteration_f"] == 0 and abs(out["score_f"] - res["score_f"]) <= 1e-6 * res["score_f"], (seed, problem, out["score_f"], res["score_f"])
        seen.add(float(res["score_f"]))
    assert len(seen) == 5


# ---- the model twin against numpy's SVD ------------------------------------------------------------------------------------------------
def _octuples(shape, count):
    rng = np.random.Generator(np.random.PCG64(0x0C7))
    for k in range(count):
        x1 = TC.camera_points(rng, 8, shape)
        m = (TC.MOTION, TC.WIDE, TC.FORWARD, TC.PLANAR_MOTION)[k % 4]
        x2 = x1 @ np.asarray(m[0]).T + np.asarray(m[1])
        yield np.concatenate([TC.project(x1), TC.project(x2)], axis=1).astype(f32)


def test_h_and_f_of_exact_octuples_are_numpys():
    worst_h = worst_f = worst_rank = 0.0
    used_h = used_f = 0
    for shape in ("planar", "general"):
        for c8 in _octuples(shape, MODEL_N):
            H, F, gaps = _svd_models(c8)
            h21, h12, f21, ok = binding.two_view_model_host(c8)
            if shape == "planar" and gaps[0] >= MIN_GAP:  # the conditioning guard: a DLT matrix of clear rank 8
                assert ok[0] == 1
                worst_h = max(worst_h, _unit_diff(h21, H))
                assert np.abs(h21 @ h12 - np.eye(3)).max() < 1e-9
                used_h += 1
            if shape == "general" and gaps[1] >= MIN_GAP:
                assert ok[1] == 1
                worst_f = max(worst_f, _unit_diff(f21, F))
                _, T1, T2 = _normalise(c8)
                s = np.linalg.svd(np.linalg.inv(T2.T) @ f21 @ np.linalg.inv(T1), compute_uv=False)
                worst_rank = max(worst_rank, s[2] / s[0])
                used_f += 1
    print(f"largest deviation from numpy's SVD: H {worst_h:.2e} over {used_h}, F {worst_f:.2e} over {used_f}; sigma3 / sigma1 of F {worst_rank:.2e}")
    assert used_h > MODEL_N // 2 and used_f > MODEL_N // 2
    assert worst_h <= BOUND_H and worst_f <= BOUND_F and worst_rank <= BOUND_RANK2


def test_degenerate_octuples_give_zero_models_or_finite_ones():
    """coincident, collinear, repeated, huge, infinite and NaN sets: every entry is finite, a refused model is all 0.0; a set that does
    not normalise gives two zero models"""
    base = next(_octuples("general", 1))
    sets = {"coincident": np.repeat(base[:1], 8, axis=0), "collinear": base[0] + np.arange(8)[:, None] * np.array([7.0, 3.0, 7.0, 3.0], f32),
            "repeated": base[[0, 0, 1, 1, 2, 2, 3, 3]], "planar": next(_octuples("planar", 1))}
    for name, v in (("1e30", 1e30), ("inf", np.inf), ("nan", np.nan)):
        sets[name] = base.copy()
        sets[name][3, 2] = v
    for name, c8 in sets.items():
        h21, h12, f21, ok = binding.two_view_model_host(c8.astype(f32))
        for m, good in ((h21, ok[0]), (h12, ok[0]), (f21, ok[1])):
            assert np.isfinite(m).all() and (good or not m.any()), name
        if name in ("coincident", "inf", "nan"):
            assert ok == (0, 0), name
    assert binding.two_view_model_host(sets["planar"])[3][0] == 1  # a plane voids F at the most, never H


# ---- the thresholds from both sides ----------------------------------------------------------------------------------------------------
EYE = np.eye(3)
F_X = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])  # a translation along x: the lines are the rows


def test_chi_squares_from_both_sides():
    """H = I: chi = (u1 - u2)^2 + (v1 - v2)^2 both ways; F of an x translation: chi = (v1 - v2)^2 both ways.  A displacement of 2 is
    a chi-square of exactly 4"""
    v = TC.view()
    c = np.array([[100, 50, 102, 50], [100, 50, 100, 50]], f32)
    below = float(np.nextafter(4.0, 0.0))
    for th, inl, score in ((4.0, 1, 2 * (4.0 - 4.0) + 2 * 4.0), (below, 0, 2 * below)):
        out = binding.two_view_check_host(_params(chi2_h=th), v, c, h21=EYE, h12=EYE)
        assert out["chi_h"].tolist() == [[4.0, 4.0], [0.0, 0.0]] and out["in_h"].tolist() == [inl, 1] and out["score_h"] == score
    c = np.array([[100, 50, 300, 52], [100, 50, 7, 50]], f32)
    for th, inl in ((4.0, 1), (below, 0)):
        out = binding.two_view_check_host(_params(chi2_f=th, chi2_score=6.0), v, c, f21=F_X)
        assert out["chi_f"].tolist() == [[4.0, 4.0], [0.0, 0.0]] and out["in_f"].tolist() == [inl, 1]
        assert out["score_f"] == (2 * (6.0 - 4.0) if inl else 0.0) + 2 * 6.0  # chi2_score is what an accepted term is taken from
    out = binding.two_view_check_host(_params(chi2_f=4.0, chi2_score=float(np.nextafter(6.0, 7.0))), v, c, f21=F_X)
    assert out["score_f"] == 2 * (np.nextafter(6.0, 7.0) - 4.0) + 2 * np.nextafter(6.0, 7.0)
    nan = np.array([[100, 50, np.nan, 52]], f32)
    assert binding.two_view_check_host(_params(), v, nan, h21=EYE, h12=EYE, f21=F_X)["in_h"].tolist() == [0]  # a NaN fails


def test_rh_threshold_from_both_sides():
    sc = TC.case_scene(1)
    p = TC.CASES[1]["params"]
    res = TC.host(sc, p)[3]
    rh = res["score_h"] / (res["score_h"] + res["score_f"])
    assert TC.host(sc, dict(p, rh_threshold=rh))[3]["model"] == 1  # RH > rh_threshold is strict
    assert TC.host(sc, dict(p, rh_threshold=float(np.nextafter(rh, 0.0))))[3]["model"] == 2


def test_cos_min_parallax_in_its_two_forms():
    for k, model in ((3, 1), (1, 2)):
        sc, p = TC.case_scene(k), TC.CASES[k]["params"]
        res = TC.host(sc, p)[3]
        c = float(res["cos_parallax"])
        assert res["state"] == 0 and res["model"] == model and c < binding.SS_TWO_VIEW_COS_1DEG
        at = TC.host(sc, dict(p, cos_min_parallax=c))[3]
        if model == 1:  # F: cos < cos_min_parallax
            assert (at["state"], at["reason"]) == (3, 4) and TC.host(sc, dict(p, cos_min_parallax=float(np.nextafter(c, 1.0))))[3]["state"] == 0
        else:           # H: cos <= cos_min_parallax
            assert at["state"] == 0
            low = TC.host(sc, dict(p, cos_min_parallax=float(np.nextafter(c, 0.0))))[3]
            assert (low["state"], low["reason"]) == (3, 4)
        assert at["cos_parallax"] == c


def test_min_triangulated_from_both_sides():
    """F: n_good >= min_triangulated with 120 good points; H: n_good > min_triangulated with 200"""
    sc, p = TC.case_scene(3), TC.CASES[3]["params"]
    assert TC.host(sc, dict(p, min_triangulated=120))[3]["state"] == 0
    r = TC.host(sc, dict(p, min_triangulated=121))[3]
    assert (r["state"], r["reason"], r["n_good"]) == (3, 2, 120)
    sc, p = TC.case_scene(1), TC.CASES[1]["params"]
    assert TC.host(sc, dict(p, min_triangulated=199))[3]["state"] == 0
    r = TC.host(sc, dict(p, min_triangulated=200))[3]
    assert (r["state"], r["reason"], r["n_good"]) == (3, 2, 200)


def _with_extra(sc, x1_extra):
    """the scene with more exact correspondences appended: points x1_extra in frame 1's coordinates (any depth, negative too)"""
    x1 = np.asarray(x1_extra, np.float64)
    x2 = x1 @ np.asarray(sc["motion"][0]).T + np.asarray(sc["motion"][1])
    uv1, uv2 = TC.project(x1), TC.project(x2)
    n = len(x1)
    add = lambda kp, uv: np.concatenate([kp, TC.G.kp_rows(uv[:, 0].astype(f32), uv[:, 1].astype(f32), octave=1)])  # noqa: E731
    idx = np.concatenate([sc["idx"], len(sc["kp2"]) + np.arange(n, dtype=np.int32)])
    return dict(sc, kp1=add(sc["kp1"], uv1), kp2=add(sc["kp2"], uv2), idx=idx)


def test_the_nine_tenths_rule_with_literal_counts():
    """F: 120 good points and m exact correspondences of points BEHIND camera 1 (inliers of F that no hypothesis with the true
    translation can triangulate): N_in = 120 + m; 120 >= (int)(0.9 * 134) = 120 is accepted, 120 >= (int)(0.9 * 135) = 121 is not"""
    sc, p = TC.case_scene(3), dict(TC.CASES[3]["params"], min_triangulated=0)
    rng = np.random.Generator(np.random.PCG64(11))
    behind = -TC.camera_points(rng, 15)
    r = TC.host(_with_extra(sc, behind[:14]), p)[3]
    assert (r["state"], r["n_inliers"], r["n_good"]) == (0, 134, 120), r
    r = TC.host(_with_extra(sc, behind), p)[3]
    assert (r["state"], r["reason"], r["n_inliers"], r["n_good"]) == (3, 2, 135, 120), r


def test_the_seven_tenths_rule_with_literal_counts():
    """F: 100 good points of which k lie so far away that their cosine is above 0.99998: they are good under (R, t) and under (R, -t)
    alike.  100 and 70 (not > 0.7 * 100): not ambiguous, the order statistic lands on a far point and the reason is low parallax;
    100 and 71: ambiguous"""
    rng = np.random.Generator(np.random.PCG64(12))
    near = TC.make_scene(3, 30, 0, 30, 30, scatter=False)
    far = TC.camera_points(rng, 71) * 4000.0
    p = dict(max_iterations=12, seed=3, min_triangulated=0)
    found = {}
    for k in (70, 71):
        sc = _with_extra(dict(near, kp1=near["kp1"][:100 - k], kp2=near["kp2"][:100 - k], idx=near["idx"][:100 - k]), far[:k])
        assert len(sc["kp1"]) == 100
        # the winner must come from near points only, or F is ill-determined: look for a seed on the CPU
        for seed in range(200):
            r = TC.host(sc, dict(p, seed=seed))[3]
            if r["model"] == 1 and r["n_inliers"] == 100 and r["n_good"] == 100 and r["state"] == 3:
                found[k] = int(r["reason"])
                break
    assert found == {70: 4, 71: 3}, found


def test_parallax_exemption_and_reprojection_bound_are_what_the_outputs_say():
    """0.99998 and 4 sigma^2 on a scan: points of growing depth pass from triangulated to good-only exactly where the cosine the twin
    reports crosses 0.99998, and points of growing vertical disparity stop being good where the squared reprojection errors recomputed
    from the twin's own X cross 4.0"""
    v = TC.view()
    R, t = np.eye(3), np.array([1.0, 0.0, 0.0])
    z = np.geomspace(20.0, 2000.0, 400)
    x1 = np.stack([0.1 * z, -0.05 * z, z], axis=1)
    c = np.concatenate([TC.project(x1), TC.project(x1 + t)], axis=1).astype(f32)
    out = binding.two_view_check_host(_params(), v, c, r21=R, t21=t)
    assert (out["good"] > 0).all() and np.array_equal(out["good"] == 2, out["cos"] < 0.99998)
    assert (out["good"] == 2).any() and (out["good"] == 1).any()
    dy = np.linspace(0.0, 6.0, 601)
    x1 = np.tile([0.3, 0.2, 5.0], (len(dy), 1))
    c = np.concatenate([TC.project(x1), TC.project(x1 + t) + np.stack([0 * dy, dy], axis=1)], axis=1).astype(f32)
    out = binding.two_view_check_host(_params(), v, c, r21=R, t21=t)
    X = out["xyz"]
    e1 = ((TC.project(X) - c[:, :2].astype(np.float64)) ** 2).sum(axis=1)
    e2 = ((TC.project(X + t) - c[:, 2:].astype(np.float64)) ** 2).sum(axis=1)
    worst = np.maximum(e1, e2)
    clear = np.abs(worst - 4.0) > 1e-6
    assert np.array_equal((out["good"] > 0)[clear], (worst <= 4.0)[clear]) and (worst[clear] > 4.0).any() and (worst[clear] < 4.0).any()
    assert clear.sum() >= len(dy) - 2


# ---- states, reasons, recovery ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(TC.CASES)), ids=TC.CASE_NAMES)
def test_cases_are_what_their_names_say(k):
    case, sc = TC.CASES[k], TC.case_scene(k)
    flag, pts, rows, res = TC.reference(k)
    state, reason, model = case["expect"]
    for name, v in (("state", state), ("reason", reason), ("model", model)):
        assert v is None or res[name] == v, (name, res)
    assert res["n_corr"] == len(sc["rows"]) and not flag[np.setdiff1d(np.arange(len(flag)), sc["rows"])].any()
    assert len(pts) == res["n_triangulated"] == int((flag == 3).sum()) and np.array_equal(rows[:, 0], np.flatnonzero(flag == 3))
    assert np.array_equal(rows[:, 1], sc["idx"][rows[:, 0]])
    if res["state"] == 0:
        assert abs(np.linalg.norm(res["t21"]) - 1.0) < 1e-12 and abs(np.linalg.det(res["r21"].reshape(3, 3)) - 1.0) < 1e-9
        assert res["n_good"] >= res["n_triangulated"] > 0 and int((flag >= 2).sum()) == res["n_inliers"]
        # the points are the planted ones up to the scale of the translation
        where = np.searchsorted(sc["rows"], rows[:, 0])
        X = np.stack([pts["x"], pts["y"], pts["z"]], axis=1) * np.linalg.norm(sc["motion"][1])
        noisy = "noise" in case["name"]
        assert np.median(np.linalg.norm(X - sc["xyz"][where], axis=1)) < (0.5 if noisy else 1e-3)
        scale = np.asarray(PC.scale(), np.float64)
        d = np.sqrt(pts["x"].astype(np.float64) ** 2 + pts["y"] ** 2 + pts["z"] ** 2)
        assert np.allclose(pts["max_dist"], d * scale[sc["kp1"]["octave"][rows[:, 0]]], rtol=1e-6) and np.allclose(pts["min_dist"], pts["max_dist"] / scale[-1], rtol=1e-6)
    else:
        assert not res["r21"].any() and not res["t21"].any() and flag.max(initial=0) <= 1 and len(pts) == 0
        assert (flag[sc["rows"]] == 1).all()
    if res["state"] != 3:
        assert res["reason"] == 0


def test_exact_scenes_recover_the_planted_motion():
    worst = [0.0, 0.0]
    for k, case in enumerate(TC.CASES):
        res = TC.reference(k)[3]
        if res["state"] == 0 and "exact" in case["name"]:
            e = TC.motion_error(res, TC.case_scene(k)["motion"])
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"largest error of the planted motion on the exact cases: rotation {worst[0]:.2e} rad, translation direction {worst[1]:.2e} rad")
    assert 0.0 < worst[0] <= BOUND_MOTION[0] and 0.0 < worst[1] <= BOUND_MOTION[1]


def test_the_planar_scenes_expected_to_succeed_are_accepted_by_the_rule_alone():
    for k in (1, 2):
        res = TC.reference(k)[3]
        assert (res["state"], res["model"]) == (0, 2) and TC.motion_error(res, TC.PLANAR_MOTION)[0] < 0.01


@pytest.mark.parametrize("k", range(len(TC.RECOVERY)))
def test_ninety_percent_of_the_planted_inliers_are_flagged(k):
    sc, p = TC.recovery_scene(k)
    flag, pts, rows, res = TC.host(sc, p)
    hit = int((flag[sc["inlier_rows"]] >= 2).sum())
    assert res["state"] == 0 and len(sc["inlier_rows"]) == 210 and hit >= 189, (hit, res)
    e = TC.motion_error(res, sc["motion"])
    assert e[0] < 0.05 and e[1] < 0.15, e


@pytest.mark.parametrize("k", [1, 3])
def test_pose_and_block_feed_the_projection_search_unchanged(k):
    """r21, t21 through ss_proj_view_init and the block of points through ss_proj_points_host (the frustum step of ss_match_proj_*),
    with no conversion: every triangulated point whose keypoint lies in the image is in view of frame 2 and lands on the keypoint it was triangulated from; in the
    view of frame 1 (the identity) it lands on its reference keypoint"""
    sc = TC.case_scene(k)
    flag, pts, rows, res = TC.reference(k)
    assert res["state"] == 0 and len(pts) > 100
    cam = binding.Camera(fx=TC.FX, fy=TC.FY, cx=TC.CX, cy=TC.CY, width=TC.W, height=TC.H)
    for view, kp, col in ((binding.proj_view(cam, res["r21"], res["t21"], 0.0), sc["kp2"], 1), (binding.proj_view(cam, np.eye(3), np.zeros(3), 0.0), sc["kp1"], 0)):
        out = binding.proj_points_host(view, binding.proj_params(extent_w=TC.W, extent_h=TC.H), PC.scale(), pts)
        want = kp[rows[:, col]]
        seen = out["state"] == 0
        inside = (want["x"] >= 0) & (want["x"] < TC.W) & (want["y"] >= 0) & (want["y"] < TC.H)  # the scenes do not clip to the image
        assert np.array_equal(seen, inside) and seen.sum() > 100, np.unique(out["state"][~inside])
        assert np.abs(out["u"] - want["x"])[seen].max() < 0.01 and np.abs(out["v"] - want["y"])[seen].max() < 0.01


def test_the_problem_number_and_the_octave_table_matter():
    sc, p = TC.case_scene(0), TC.CASES[0]["params"]
    a, b = TC.host(sc, p, 0)[3], TC.host(sc, p, 1)[3]
    assert a["iteration_f"] != b["iteration_f"]
    short = TC.host(sc, p, 0, scale=PC.scale()[:2])[3]  # octaves 2 and 3 fall outside a table of two levels: fewer correspondences
    assert short["n_corr"] < a["n_corr"]


# ---- the twins against the restatement, bit for bit -----------------------------------------------------------------------------------
def _degenerate_sets():
    base = next(_octuples("general", 1))
    sets = {"coincident": np.repeat(base[:1], 8, axis=0), "collinear": base[0] + np.arange(8)[:, None] * np.array([7.0, 3.0, 7.0, 3.0], f32),
            "repeated rows": base[[0, 0, 1, 1, 2, 2, 3, 3]], "one plane": next(_octuples("planar", 1)), "no motion": np.concatenate([base[:, :2], base[:, :2]], axis=1)}
    for name, v in (("1e30", 1e30), ("infinite", np.inf), ("NaN", np.nan), ("3e38", 3e38)):
        sets[name] = base.copy()
        sets[name][3, 2] = v
    return sets


def _model_restated(c8):
    c8 = np.asarray(c8, f32)
    m, d = R.normalise(c8)
    if not R.norm_ok(m, d):
        return [0.0] * 9, [0.0] * 9, [0.0] * 9, 0, 0
    return R.model_of(c8, list(range(8)), m, d)


def test_the_model_twin_is_the_restatement_bit_for_bit():
    sets = [(f"{shape} {k}", c8) for shape in ("general", "planar") for k, c8 in enumerate(_octuples(shape, 40))] + list(_degenerate_sets().items())
    rng = np.random.Generator(np.random.PCG64(21))
    sets += [(f"noisy {k}", (c8 + rng.normal(0, 1.0, c8.shape)).astype(f32)) for k, c8 in enumerate(_octuples("general", 20))]
    zero = 0
    for name, c8 in sets:
        h21, h12, f21, ok_h, ok_f = _model_restated(c8)
        g = binding.two_view_model_host(c8)
        assert g[3] == (ok_h, ok_f), (name, g[3], ok_h, ok_f)
        for got, want in zip(g[:3], (h21, h12, f21)):
            assert got.tobytes() == np.array(want, np.float64).tobytes(), name
        zero += (not ok_h) + (not ok_f)
    assert zero >= 6  # the degenerate sets do reach the zero models


@pytest.mark.parametrize("k", range(len(TC.CASES)), ids=TC.CASE_NAMES)
def test_the_whole_rule_twin_is_the_restatement_bit_for_bit(k):
    _same(TC.reference(k), TC.restatement(k), TC.CASES[k]["name"])
    if k == 0:
        _same(TC.host(TC.case_scene(k), TC.CASES[k]["params"], 5), TC.solve_scene(TC.case_scene(k), TC.CASES[k]["params"], 5), "as problem 5")


def test_degenerate_coordinates_in_a_whole_problem_bit_for_bit():
    base = TC.case_scene(3)
    p = dict(max_iterations=16, seed=2)
    for value in (1e30, np.inf, np.nan):
        sc = dict(base, kp1=base["kp1"].copy(), kp2=base["kp2"].copy())
        sc["kp2"]["x"][sc["idx"][sc["rows"][5]]] = value
        sc["kp1"]["y"][sc["rows"][17]] = value
        _same(TC.host(sc, p), TC.solve_scene(sc, p), f"a coordinate of {value}")
    still = TC.make_scene(9, 100, 0, 128, 128, motion=(np.eye(3), (0.0, 0.0, 0.0)))
    _same(TC.host(still, p), TC.solve_scene(still, p), "no motion")


def test_the_check_twin_is_the_restatement_bit_for_bit():
    """steps 4 and 8 of a noisy scene under numpy's models and the planted motion: every chi-square, flag, score, cosine and point"""
    sc = TC.make_scene(31, 300, 60, 320, 320, noise=1.0, motion=TC.WIDE)
    c = _corr(sc)
    H, Fm, _ = _svd_models(c[sc["out"] == 0][:8], norm_of=c)
    H12 = np.linalg.inv(H)
    Rm, t = np.asarray(sc["motion"][0]).reshape(9), TC.unit(sc["motion"][1])
    cam = (TC.FX, TC.FY, TC.CX, TC.CY)
    out = binding.two_view_check_host(_params(), sc["view"], c, h21=H, h12=H12, f21=Fm, r21=Rm, t21=t)
    c64 = [[np.float64(v) for v in row] for row in c]
    th = [R.term_h(list(H.reshape(9)), list(H12.reshape(9)), *q, np.float64(5.991)) for q in c64]
    tf = [R.term_f(list(Fm.reshape(9)), *q, np.float64(3.841), np.float64(5.991)) for q in c64]
    assert out["chi_h"].tobytes() == np.array([[v[2], v[3]] for v in th]).tobytes() and out["in_h"].tolist() == [int(v[1]) for v in th]
    assert out["chi_f"].tobytes() == np.array([[v[2], v[3]] for v in tf]).tobytes() and out["in_f"].tolist() == [int(v[1]) for v in tf]
    assert np.float64(out["score_h"]).tobytes() == R.tree_sum([v[0] for v in th]).tobytes()
    assert np.float64(out["score_f"]).tobytes() == R.tree_sum([v[0] for v in tf]).tobytes()
    rt = [R.check_rt(list(Rm), list(t), cam, *q) for q in c64]
    assert out["good"].tolist() == [(2 if R.triangulated(o["cos"]) else 1) if g else 0 for g, o in rt]
    assert out["cos"].tobytes() == np.array([o["cos"] for _, o in rt]).tobytes() and out["xyz"].tobytes() == np.array([o["X"] for _, o in rt]).tobytes()
    assert 0 < sum(g for g, _ in rt) < len(rt) and 0 < sum(v[1] for v in tf) < len(tf)


def test_the_reprojection_bound_and_the_parallax_exemption_against_the_restatement():
    """the two scans of the test above it in this file, now against the restatement's own errors and cosines: the good flag is
    e <= 4.0 and the triangulated flag cos < 0.99998 on the numbers the rule itself forms, with no band left out"""
    v, cam = TC.view(), (TC.FX, TC.FY, TC.CX, TC.CY)
    Rm, t = [np.float64(x) for x in np.eye(3).reshape(9)], [np.float64(1.0), np.float64(0.0), np.float64(0.0)]
    dy = np.linspace(3.9, 4.1, 801)
    x1 = np.tile([0.3, 0.2, 5.0], (len(dy), 1))
    c = np.concatenate([TC.project(x1), TC.project(x1 + np.array([1.0, 0, 0])) + np.stack([0 * dy, dy], axis=1)], axis=1).astype(f32)
    out = binding.two_view_check_host(_params(), v, c, r21=np.eye(3), t21=[1.0, 0, 0])
    rt = [R.check_rt(Rm, t, cam, *[np.float64(q) for q in row]) for row in c]
    worst = np.array([max(o["e1"], o["e2"] if o["e2"] is not None else 0.0) for _, o in rt])
    assert np.array_equal(out["good"] > 0, worst <= 4.0) and (worst > 4.0).any() and (worst <= 4.0).any()
    assert np.abs(worst - 4.0).min() < 1e-3  # the scan does come close to the bound
    z = np.geomspace(150.0, 170.0, 801)
    x1 = np.stack([0.1 * z, -0.05 * z, z], axis=1)
    c = np.concatenate([TC.project(x1), TC.project(x1 + np.array([1.0, 0, 0]))], axis=1).astype(f32)
    out = binding.two_view_check_host(_params(), v, c, r21=np.eye(3), t21=[1.0, 0, 0])
    cos = np.array([R.check_rt(Rm, t, cam, *[np.float64(q) for q in row])[1]["cos"] for row in c])
    assert out["cos"].tobytes() == cos.tobytes() and np.array_equal(out["good"] == 2, cos < 0.99998) and (out["good"] > 0).all()
    assert (out["good"] == 2).any() and (out["good"] == 1).any() and np.abs(cos - 0.99998).min() < 1e-7


def test_the_parallax_exemption_exactly_at_its_bound():
    """0.99998 from both sides and at equality, on the whole of step 8: one correspondence (a point at depth 156.245 seen under
    R = I, t = (1, 0, 0), its coordinates float32) checked under t = (1, 0, s) for three values of s, found on the CPU by bisection
    and a walk over neighbouring doubles, at which the cosine the rule forms is nextafter(0.99998, 0), 0.99998 and
    nextafter(0.99998, 1).  Twin and restatement: triangulated below the bound, good only at it and above it"""
    v, cam = TC.view(), (TC.FX, TC.FY, TC.CX, TC.CY)
    c = np.array([[368.0, 217.5, 371.2001037597656, 217.5]], f32)
    eye = [np.float64(x) for x in np.eye(3).reshape(9)]
    bound = np.float64(0.99998)
    for s, want_cos, want_good in ((-0.15755872993344053, np.nextafter(bound, 0.0), 2), (-0.15755872993337555, bound, 1),
                                   (-0.15755872993344153, np.nextafter(bound, 1.0), 1)):
        out = binding.two_view_check_host(_params(), v, c, r21=np.eye(3), t21=[1.0, 0.0, s])
        g, o = R.check_rt(eye, [np.float64(1.0), np.float64(0.0), np.float64(s)], cam, *[np.float64(q) for q in c[0]])
        assert o["cos"] == want_cos and out["cos"][0] == want_cos, (s, o["cos"], out["cos"][0], want_cos)
        assert g and out["good"][0] == want_good and R.triangulated(o["cos"]) == (want_good == 2), (s, out["good"][0])


def test_the_tests_of_step_8_on_literal_numbers():
    """ss_tv_triangulated, ss_tv_exempt and ss_tv_reprojects, the three functions ss_tv_check_rt calls, fed literal doubles: 0.99998
    and 4 sigma^2 = 4.0 at equality and at their neighbours on both sides; a NaN fails each"""
    t = binding.two_view_point_tests_host
    c, e = 0.99998, 4.0
    below_c, above_c, below_e, above_e = float(np.nextafter(c, 0.0)), float(np.nextafter(c, 1.0)), float(np.nextafter(e, 0.0)), float(np.nextafter(e, 5.0))
    assert t(below_c, below_e) == (True, False, True)
    assert t(c, e) == (False, True, True)          # cos < 0.99998 is strict, cos >= 0.99998 and err <= 4.0 are not
    assert t(above_c, above_e) == (False, True, False)
    assert t(float("nan"), float("nan")) == (False, False, False) and t(-1.0, 0.0) == (True, False, True) and t(1.0, float("inf")) == (False, True, False)
    for cos in (below_c, c, above_c):
        assert t(cos, 0.0)[0] == R.triangulated(np.float64(cos)) and t(cos, 0.0)[1] == bool(np.float64(cos) >= R.COS_TRI)
    for err in (below_e, e, above_e):
        assert t(0.0, err)[2] == bool(np.float64(err) <= R.TH2)


# ---- steps 5, 8 and 9 on literal numbers -----------------------------------------------------------------------------------------------
def test_the_order_of_the_selection_and_its_ties():
    b = binding.two_view_beats_host
    assert b(2.0, 5, 1.0, 0) and not b(1.0, 0, 2.0, 5)                       # the larger score
    assert b(1.0, 3, 1.0, 4) and not b(1.0, 4, 1.0, 3) and not b(1.0, 3, 1.0, 3)  # equal scores: the smaller t
    assert b(float(np.nextafter(1.0, 2.0)), 9, 1.0, 0) and not b(float(np.nextafter(1.0, 0.0)), 0, 1.0, 9)
    assert b(0.0, 1, -1.0, 0) and not b(float("nan"), 0, 0.0, 1)             # a real model beats the zero model; a NaN beats nothing
    for args in ((2.0, 5, 1.0, 0), (1.0, 3, 1.0, 4), (1.0, 4, 1.0, 3), (0.0, 1, -1.0, 0)):
        assert b(*args) == R.beats(np.float64(args[0]), args[1], np.float64(args[2]), args[3])
    # a whole problem in which every real model scores exactly 0.0: the winners are the first hypotheses with a model
    sc, p = TC.make_scene(**TC.TIE_SCENE), dict(TC.TIE_PARAMS, max_iterations=48)
    want = TC.solve_scene(sc, p)
    _same(TC.host(sc, p), want, "ties")
    sh, sf = [s[0] for s in want[4]], [s[1] for s in want[4]]
    assert max(sh) == 0.0 and max(sf) == 0.0 and sh.count(0.0) > 10 and sf.count(0.0) > 10
    assert want[3]["iteration_h"] == sh.index(0.0) and want[3]["iteration_f"] == sf.index(0.0) and want[3]["state"] == 2


def test_pick_and_accept_with_literal_counts():
    """the first largest count is the best, the second as upstream's loop leaves it; then every rule of step 9 from both sides"""
    acc = lambda model, good, n_in, cos=0.9, **kw: binding.two_view_accept_host(_params(**kw), model, good, n_in, cos)  # noqa: E731
    assert acc(1, [10, 80, 80, 3], 80, min_triangulated=0)[1:] == (1, 80, 80)  # upstream's loop: an equal count is no new best, but it is the second
    assert acc(2, [5, 100, 60, 74, 0, 0, 0, 0], 100)[1:] == (1, 100, 74)
    # H, the 0.75 rule: second < 0.75 * best
    assert acc(2, [100, 74, 0, 0, 0, 0, 0, 0], 100)[0] == 0 and acc(2, [100, 75, 0, 0, 0, 0, 0, 0], 100)[0] == 3
    assert acc(2, [74, 100, 0, 0, 0, 0, 0, 0], 100)[0] == 0 and acc(2, [75, 100, 0, 0, 0, 0, 0, 0], 100)[0] == 3
    # H: best > min_triangulated, best > 0.9 * N_in
    assert acc(2, [51] + [0] * 7, 51)[0] == 0 and acc(2, [50] + [0] * 7, 50)[0] == 2
    assert acc(2, [91] + [0] * 7, 101)[0] == 0 and acc(2, [90] + [0] * 7, 100)[0] == 2
    # F, the 0.7 rule: at most one count > 0.7 * best
    assert acc(1, [100, 70, 70, 70], 100)[0] == 0 and acc(1, [100, 71, 0, 0], 100)[0] == 3
    # F: best >= max((int)(0.9 * N_in), min_triangulated)
    assert acc(1, [50, 0, 0, 0], 55)[0] == 0 and acc(1, [49, 0, 0, 0], 50)[0] == 2 and acc(1, [90, 0, 0, 0], 101)[0] == 0 and acc(1, [90, 0, 0, 0], 102)[0] == 2
    # the parallax: F strict, H not
    c1 = binding.SS_TWO_VIEW_COS_1DEG
    assert acc(1, [100, 0, 0, 0], 100, cos=c1)[0] == 4 and acc(1, [100, 0, 0, 0], 100, cos=float(np.nextafter(c1, 0.0)))[0] == 0
    assert acc(2, [100] + [0] * 7, 100, cos=c1)[0] == 0 and acc(2, [100] + [0] * 7, 100, cos=float(np.nextafter(c1, 1.0)))[0] == 4
    assert acc(1, [0, 0, 0, 0], 100)[:2] == (2, -1)
    # and the restatement says the same on a sweep of counts
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(400):
        model = int(rng.integers(1, 3))
        good = [int(v) for v in rng.integers(0, 120, 4 if model == 1 else 8)]
        n_in, cos = int(rng.integers(80, 130)), float(rng.choice([0.99, c1, 0.99999]))
        best, best_good, second = R.pick(good)
        want = R.accept(model, good, best_good, second, n_in, np.float64(cos), dict(R.UPSTREAM))
        assert acc(model, good, n_in, cos=cos) == (want, best, best_good, second), (model, good, n_in, cos)


# ---- the tracker's own form on the same scenes -------------------------------------------------------------------------------------------
def test_sst_two_view_recovers_the_same_motions(tmp_path):
    """sst_two_view (csrc/ss_track.cpp: an independent implementation with its own draw stream) and the rule on a general and a planar
    scene with known motion: both recover the planted rotation and translation direction.  The bound is ten times the restatement's
    own largest error on these scenes (rotation 1.2e-7 rad, translation direction 3.0e-6 rad: the float32 rounding of the coordinates;
    the test prints all four)"""
    exe = str(tmp_path / "two_view_vs_track")
    csrc = os.path.join(ROOT, "send-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "native", "two_view_vs_track.cpp"), os.path.join(csrc, "ss_track.cpp")])
    for k, model in ((3, 1), (1, 2)):
        sc = TC.case_scene(k)
        c = _corr(sc)
        path = tmp_path / f"corr{k}.bin"
        path.write_bytes(np.int32(len(c)).tobytes() + c.tobytes())
        out = subprocess.run([exe, str(path), str(TC.FX), str(TC.FY), str(TC.CX), str(TC.CY)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        v = [float(x) for x in out.stdout.split()]
        assert int(v[0]) == len(c) and int(v[1]) == model, v[:2]  # every point triangulated, the same model chosen
        track = np.zeros(1, R.RESULT_DTYPE)[0]
        track["r21"], track["t21"] = v[2:11], v[11:14]
        mine = TC.restatement(k)[3]
        e_track, e_mine = TC.motion_error(track, sc["motion"]), TC.motion_error(mine, sc["motion"])
        print(f"case {k}: sst_two_view {e_track[0]:.2e} {e_track[1]:.2e} rad, the rule {e_mine[0]:.2e} {e_mine[1]:.2e} rad")
        for e in (e_track, e_mine):
            assert e[0] <= 1.2e-6 and e[1] <= 3.0e-5, (k, e_track, e_mine)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_without_a_device():
    sc = TC.case_scene(3)
    ok = dict(TC.CASES[3]["params"])
    nan, inf = float("nan"), float("inf")
    for bad in (dict(chi2_h=0.0), dict(chi2_h=nan), dict(chi2_f=inf), dict(chi2_f=-1.0), dict(chi2_score=0.0), dict(chi2_score=nan), dict(rh_threshold=-0.1),
                dict(rh_threshold=1.1), dict(rh_threshold=nan), dict(cos_min_parallax=1.5), dict(cos_min_parallax=nan), dict(min_triangulated=-1),
                dict(max_iterations=0), dict(max_iterations=1025), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 1))):
        with pytest.raises(binding.OrbError) as e:
            TC.host(sc, dict(ok, **bad))
        assert e.value.code == binding.SS_ERR_INVALID_ARG, bad
        with pytest.raises(binding.OrbError):
            binding.two_view_check_host(_params(**dict(ok, **bad)), sc["view"], np.zeros((1, 4), f32), f21=F_X)
    for good in (dict(max_iterations=1), dict(max_iterations=1024), dict(rh_threshold=0.0), dict(rh_threshold=1.0), dict(min_triangulated=0)):
        TC.host(TC.case_scene(9), dict(ok, **good))
    for levels in (np.zeros(0, f32), np.ones(17, f32)):
        with pytest.raises(binding.OrbError):
            TC.host(sc, ok, scale=levels)
    with pytest.raises(binding.OrbError):
        TC.host(sc, ok, problem=-1)
    lib = binding.load()
    p = _params()
    inval = binding.SS_ERR_INVALID_ARG
    assert lib.ss_two_view_pairs_device(None, None, None, 1, None, None, 1, 1, None, 0, None, None, None, C.byref(p), None, None, None, None, None) == inval
    assert lib.ss_two_view_batch_device(None, None, None, 0, None, C.byref(p), None, None, None, None, None) == inval
    assert lib.ss_two_view(None, None, None, 0, None, 0, None, C.byref(p), None, None, None, None, None) == inval
    assert lib.ss_two_view_model_host(None, None, None, None, None) == inval
    assert lib.ss_two_view_host(None, None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, None) == inval
    empty = dict(sc, kp1=sc["kp1"][:0], idx=sc["idx"][:0])
    flag, pts, rows, res = TC.host(empty, ok)
    assert res["state"] == 1 and res["n_corr"] == 0 and len(flag) == 0 and len(pts) == 0


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/two_view_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "two_view_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "two_view_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 80000
