"""CPU tests of map-point fusion as tests/fuse_ref.py states it, and of its C ABI surface: the host twins ss_fuse_points_host and
ss_fuse_check_host (the text the kernel compiles) against the reference bit for bit, ss_fuse_view_sim3, struct layouts, refused
arguments, upstream's sequential loops against the order-free rule, the stand-alone sanitizer run of the steps, and that the shared
cases are what they claim to be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import fuse_cases as FC
import fuse_ref as F
import guided_cases as G
import guided_ref as R
import proj_cases as PC
import proj_ref as P
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")
f32 = np.float32


def _same(got, want, tag):
    """two POINT_DTYPE arrays, bit for bit (NaN bits included)"""
    assert got.dtype == want.dtype == F.POINT_DTYPE and len(got) == len(want)
    for name in F.POINT_DTYPE.names:
        a, b = got[name].view(np.int32), want[name].view(np.int32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {got[name][bad[:8]]} != {want[name][bad[:8]]}"


def test_symbols_structs_and_constants(tmp_path):
    names = ["ss_fuse_view_sim3", "ss_fuse_points_host", "ss_fuse_check_host", "ss_match_fuse_pairs_device", "ss_match_fuse_batch_device", "ss_match_fuse"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("match_fuse_pairs_device", "match_fuse_batch_device", "match_fuse"):
        assert callable(getattr(binding.OrbContext, m))
    for m in ("fuse_params", "fuse_view_sim3", "fuse_points_host", "fuse_check_host"):
        assert callable(getattr(binding, m))
    assert C.sizeof(binding.FuseParams) == 40 and C.sizeof(binding.FuseSummary) == 32
    assert binding.FUSE_POINT_DTYPE.itemsize == 32 and binding.FUSE_ACTION_DTYPE.itemsize == 8 and binding.FUSE_SUMMARY_DTYPE.itemsize == 32
    assert binding.FUSE_POINT_DTYPE == F.POINT_DTYPE and binding.FUSE_ACTION_DTYPE == F.ACTION_DTYPE
    assert tuple(n for n, _ in binding.FuseSummary._fields_) == F.SUMMARY_FIELDS
    assert (binding.SS_FUSE_NONE, binding.SS_FUSE_ADD, binding.SS_FUSE_REPLACE, binding.SS_FUSE_DUPLICATE) == (0, 1, 2, 3) == \
        (F.ACT_NONE, F.ACT_ADD, F.ACT_REPLACE, F.ACT_DUPLICATE)
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_fuse_point) == 32, "point");\n'
                   '_Static_assert(sizeof(ss_fuse_action) == 8, "action");\n'
                   '_Static_assert(sizeof(ss_fuse_params) == 40, "params");\n'
                   '_Static_assert(sizeof(ss_fuse_summary) == 32, "summary");\n'
                   '_Static_assert(offsetof(ss_fuse_point, dot) == 12 && offsetof(ss_fuse_point, radius) == 20 && offsetof(ss_fuse_point, level) == 24 && '
                   'offsetof(ss_fuse_point, state) == 28, "point fields");\n'
                   '_Static_assert(offsetof(ss_fuse_action, other) == 4, "action fields");\n'
                   '_Static_assert(offsetof(ss_fuse_params, th) == 4 && offsetof(ss_fuse_params, chi2_mono) == 8 && offsetof(ss_fuse_params, chi2_stereo) == 12 && '
                   'offsetof(ss_fuse_params, th_low) == 16 && offsetof(ss_fuse_params, check_right) == 20 && offsetof(ss_fuse_params, extent_w) == 24 && '
                   'offsetof(ss_fuse_params, extent_h) == 28 && offsetof(ss_fuse_params, reserved) == 32, "params fields");\n'
                   '_Static_assert(offsetof(ss_fuse_summary, n_in_view) == 12 && offsetof(ss_fuse_summary, n_candidates) == 16 && '
                   'offsetof(ss_fuse_summary, n_add) == 20 && offsetof(ss_fuse_summary, n_replace) == 24 && offsetof(ss_fuse_summary, n_duplicate) == 28, '
                   '"summary fields");\n'
                   '_Static_assert(SS_FUSE_NONE == 0 && SS_FUSE_ADD == 1 && SS_FUSE_REPLACE == 2 && SS_FUSE_DUPLICATE == 3, "actions");\n'
                   '_Static_assert(SS_GUIDED_MAX_ROWS == 16384 && SS_ABI_VERSION == 5 && SS_MAX_LEVELS == 16, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5
    # the header states both facts about the rule's standing where the other stages state theirs
    assert "tests/fuse_ref.py is its normative" in text and "real binary stays unpinned, as for the guided, bag-of-words, projection and epipolar" in text


CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, width=640, height=480)


def _view_bytes(v):
    return np.frombuffer(bytes(v), P.VIEW_DTYPE)[0].tobytes()


def test_view_sim3_agrees_with_its_restatement():
    rng = np.random.Generator(np.random.PCG64(0x51A3))
    cam = binding.Camera(**CAM)
    args = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["width"], CAM["height"])
    # general scaled poses
    for _ in range(50):
        rcw, t, s = PC.rot(*rng.normal(0, 1, 3)), rng.normal(0, 10, 3), float(rng.uniform(0.05, 20.0))
        want = F.view_sim3(*args, s * rcw, t, 40.0)
        assert want is not None and _view_bytes(binding.fuse_view_sim3(cam, s * rcw, t, bf=40.0)) == want.tobytes()
    # s = 1 is ss_proj_view_init on the same R, t: the basis rows here have a norm of exactly 1
    for rcw in (np.eye(3), np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]]), np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0.0]])):
        t = rng.normal(0, 3, 3)
        assert (rcw[0] ** 2).sum() == 1.0
        assert _view_bytes(binding.fuse_view_sim3(cam, rcw, t, bf=40.0)) == _view_bytes(binding.proj_view(cam, rcw, t, bf=40.0))
        # s = 2: every division is exact, so the view is the one of the unscaled pose with t / 2
        assert _view_bytes(binding.fuse_view_sim3(cam, 2.0 * rcw, 2.0 * t, bf=40.0)) == _view_bytes(binding.proj_view(cam, rcw, t, bf=40.0))
        assert F.view_sim3(*args, 2.0 * rcw, 2.0 * t, 40.0).tobytes() == P.view_init(*args, rcw, t, 40.0).tobytes()
    # refused: s = 0, NaN and infinite entries in row 0, NULL pointers
    bad = [np.zeros((3, 3)), np.array([[np.nan, 0, 0], [0, 1, 0], [0, 0, 1.0]]), np.array([[1.0, np.inf, 0], [0, 1, 0], [0, 0, 1]]),
           np.array([[1e200, 1e200, 0], [0, 1, 0], [0, 0, 1.0]])]
    for m in bad:
        assert F.view_sim3(*args, m, (0, 0, 0), 40.0) is None
        with pytest.raises(binding.OrbError) as e:
            binding.fuse_view_sim3(cam, m, (0.0, 0.0, 0.0))
        assert e.value.code == binding.SS_ERR_INVALID_ARG
    assert binding.load().ss_fuse_view_sim3(None, None, None, C.c_float(0), None) == binding.SS_ERR_INVALID_ARG


def _random_points(rng, n):
    pts = np.zeros(n, P.MAP_POINT_DTYPE)
    pts["x"], pts["y"] = rng.normal(0, 2, n), rng.normal(0, 1.5, n)
    pts["z"] = rng.uniform(-1, 9, n)
    nrm = rng.normal(0, 1, (n, 3)) + np.array([0, 0, 2.0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    pts["nx"], pts["ny"], pts["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    dist = np.sqrt(pts["x"].astype(np.float64) ** 2 + pts["y"].astype(np.float64) ** 2 + pts["z"].astype(np.float64) ** 2)
    pts["max_dist"] = dist * rng.uniform(0.7, 4.5, n)
    pts["min_dist"] = dist * rng.uniform(0.1, 1.4, n)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38], np.float32)
    for k in rng.integers(0, n, n // 50):  # one odd field in two rows of a hundred
        pts[P.MAP_POINT_DTYPE.names[rng.integers(0, 8)]][k] = odd[rng.integers(0, len(odd))]
    return pts


def _check_all(params, sc, pts, kp, right, taken):
    kw = dict(chi2_mono=params.chi2_mono, chi2_stereo=params.chi2_stereo, check_right=bool(params.check_right))
    return np.array([F.check(pts[k], kp["x"][k], kp["y"][k], kp["octave"][k], None if right is None else right[k], None if taken is None else taken[k],
                             sc, **kw) for k in range(len(pts))], np.uint8)


def test_host_twins_agree_with_the_reference_on_the_tables():
    for sc in [PC.scale()] + [PC.scale_table(*PC.PYRAMIDS[n]) for n in PC.PYRAMIDS]:
        view, points, skip, groups, tk, td, pd = FC.boundary_table(sc)
        want = F.eval_points(view, points, skip, scale=sc, **FC.B_LIMITS)
        _same(binding.fuse_points_host(view, binding.fuse_params(**FC.B_LIMITS), sc, points, skip), want, f"boundary table, {len(sc)} levels")
        # every point of the table against every train row of it
        pi, tj = np.repeat(np.arange(len(points)), len(tk)), np.tile(np.arange(len(tk)), len(points))
        for p in (binding.fuse_params(**FC.B_LIMITS), binding.fuse_params(chi2_mono=0.0, **FC.B_LIMITS)):
            got = binding.fuse_check_host(p, sc, want[pi], tk[tj])
            assert np.array_equal(got, _check_all(p, sc, want[pi], tk[tj], None, None)), len(sc)
    view = FC.candidate_view()
    for c in [c for t in [None] + [PC.scale_table(*PC.PYRAMIDS[n]) for n in PC.PYRAMIDS] for c in FC.candidate_cases(t)]:
        sc = c["scale"]
        p = binding.fuse_params(**c["params"])
        pts = F.eval_points(view, c["points"], None, c["params"]["view_cos_limit"], c["params"]["th"], sc)
        _same(binding.fuse_points_host(view, p, sc, c["points"]), pts, c["name"])
        n = len(c["t_kp"])
        got = binding.fuse_check_host(p, sc, np.repeat(pts, n), c["t_kp"], c["right"], c["taken"])
        want = _check_all(p, sc, np.repeat(pts, n), c["t_kp"], c["right"], c["taken"])
        assert np.array_equal(got, want), (c["name"], got, want)
        if c["cands"] is not None:
            assert list(np.flatnonzero(got == 0)) == c["cands"], (c["name"], got)


def test_host_twins_agree_with_the_reference_on_random_points_and_couples():
    """the compiler's float steps against numpy's: 10 000 random points under three poses, then 10 000 random couples"""
    sc = PC.scale()
    rng = np.random.Generator(np.random.PCG64(0xF0000))
    pts = _random_points(rng, 10000)
    skip = (rng.random(len(pts)) < 0.05).astype(np.uint8) * rng.integers(1, 256, len(pts)).astype(np.uint8)
    states, evaluated = np.zeros(6, int), []
    for k, (limit, th) in enumerate([(0.5, 3.0), (0.5, 8.0), (-1.0, 2.5)]):
        view = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, PC.POSES[k][0], PC.POSES[k][1], PC.BF)
        part, sk = pts[k::3], skip[k::3]
        want = F.eval_points(view, part, sk, limit, th, sc)
        _same(binding.fuse_points_host(view, binding.fuse_params(view_cos_limit=limit, th=th), sc, part, sk), want, f"random points, pose {k}")
        states += np.bincount(want["state"], minlength=6)
        assert set(want["level"][want["state"] == 0]) == set(range(8))
        evaluated.append(want)
    print("states", states)
    assert (states > 20).all()  # every test rejects something, and plenty is in view
    want = F.eval_points(view, part, None, 0.5, 3.0, [f32(1), f32(2), f32(4)])
    _same(binding.fuse_points_host(view, binding.fuse_params(), [1, 2, 4], part), want, "three levels")
    assert len(binding.fuse_points_host(view, binding.fuse_params(), sc, pts[:0])) == 0
    # couples: points in view, a train row about a radius away on an octave around the level
    o = np.concatenate(evaluated)
    o = o[o["state"] == 0]
    o = o[rng.integers(0, len(o), 10000)]
    n = len(o)
    kp = G.kp_rows(o["u"] + (rng.normal(0, 0.6, n) * o["radius"]).astype(np.float32), o["v"] + (rng.normal(0, 0.6, n) * o["radius"]).astype(np.float32),
                   octave=o["level"] + rng.integers(-2, 3, n))
    right = np.where(rng.random(n) < 0.4, f32(-1), o["u_right"] + rng.normal(0, 3, n).astype(np.float32)).astype(np.float32)
    taken = (rng.random(n) < 0.1).astype(np.uint8)
    seen = set()
    for kw in (dict(check_right=True), dict(), dict(chi2_mono=0.0), dict(chi2_mono=50.0, chi2_stereo=80.0, check_right=True)):
        p = binding.fuse_params(**kw)
        for r, t in ((right, taken), (right, None), (None, taken)):
            if r is None and p.check_right:
                continue
            got = binding.fuse_check_host(p, sc, o, kp, r, t)
            want = _check_all(p, sc, o, kp, r, t)
            assert np.array_equal(got, want), (kw, np.flatnonzero(got != want)[:8])
            seen |= set(int(v) for v in got)
    assert seen == {0, 1, 2, 3, 4}


def test_invalid_arguments_are_refused_without_a_device():
    """the parameter check of the device calls (one function in the library) through the host twins, which need no context; the
    checks that need one (row counts, point_src) are in tests/test_fuse.py"""
    sc = PC.scale()
    view, points, skip, groups, tk, *_ = FC.boundary_table()
    pts = F.eval_points(view, points[:4], None, scale=sc, **FC.B_LIMITS)
    nan, inf = float("nan"), float("inf")
    bad = [dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(th=inf), dict(view_cos_limit=nan), dict(th_low=-1), dict(th_low=257),
           dict(check_right=True, chi2_stereo=0.0), dict(check_right=True, chi2_stereo=nan), dict(check_right=True, chi2_stereo=inf),
           dict(check_right=True, chi2_stereo=-7.8), dict(reserved=(1, 0)), dict(reserved=(0, -1))]
    for kw in bad:
        for call in (lambda p: binding.fuse_points_host(view, p, sc, points), lambda p: binding.fuse_check_host(p, sc, pts, tk[:4])):
            with pytest.raises(binding.OrbError) as e:
                call(binding.fuse_params(**kw))
            assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    for good in (dict(th_low=0), dict(th_low=256), dict(view_cos_limit=-inf), dict(chi2_mono=nan), dict(chi2_mono=-1.0), dict(chi2_mono=0.0),
                 dict(chi2_stereo=nan), dict(chi2_mono=0.0, chi2_stereo=nan, check_right=True), dict(th=1e-30)):
        assert len(binding.fuse_points_host(view, binding.fuse_params(**good), sc, points)) == len(points)
    for levels in (np.zeros(0, np.float32), np.ones(17, np.float32)):
        with pytest.raises(binding.OrbError):
            binding.fuse_points_host(view, binding.fuse_params(), levels, points)
        with pytest.raises(binding.OrbError):
            binding.fuse_check_host(binding.fuse_params(), levels, pts, tk[:4])
    # no context, no call
    lib = binding.load()
    p = binding.fuse_params(extent_w=320, extent_h=240)
    assert lib.ss_match_fuse_pairs_device(None, None, None, None, 0, 1, None, None, None, None, None, None, None, 0, 1, None, None, C.byref(p), None, None,
                                          None, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_match_fuse_batch_device(None, None, None, None, 0, 1, None, None, None, None, None, None, C.byref(p), None, None, None, None,
                                          None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_match_fuse(None, None, None, None, None, 0, None, None, 0, None, None, None, C.byref(p), None, None, None, None,
                             None) == binding.SS_ERR_INVALID_ARG


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/fuse_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "fuse_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "fuse_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 50000


# ---- the shared cases are live, on the REFERENCE alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default"] + list(PC.PYRAMIDS))
def test_boundary_table_is_live(name):
    """across every boundary the state, the level or the radius changes; u on max_x and v on max_y are rejected here and accepted
    by the projection search, whose bound is closed"""
    sc = PC.scale() if name == "default" else PC.scale_table(*PC.PYRAMIDS[name])
    view, points, skip, groups, *_ = FC.boundary_table(sc)
    pts = F.eval_points(view, points, skip, scale=sc, **FC.B_LIMITS)
    for gname, a, live in groups:
        rows = [(int(pts["state"][i]), int(pts["level"][i]), float(pts["radius"][i])) for i in range(a, a + 3)]
        assert (len(set(rows)) > 1) == live, (gname, rows)
    assert {int(s) for s in pts["state"]} == {0, 1, 2, 3, 4, 5}
    assert list(pts["state"][-3:]) == [1, 1, 0]
    assert set(int(v) for v in pts["level"][pts["state"] == 0]) == set(range(len(sc)))
    by = {g[0]: g[1] for g in groups}
    for gname in ("u on max_x", "v on max_y"):
        a = by[gname]
        assert [int(pts["state"][i]) for i in range(a, a + 3)] == [0, 3, 3], gname
        proj = P.eval_points(view, points[a:a + 3], 0.5, 1.0, 0.0, sc)
        assert [int(s) for s in proj["state"]] == [0, 0, 2], gname
    for gname in ("u on min_x", "v on min_y"):
        a = by[gname]
        assert [int(pts["state"][i]) for i in range(a, a + 3)] == [3, 0, 0], gname
    a = by["z at 0"]
    assert [int(pts["state"][i]) for i in range(a, a + 3)] == [2, 2, 3]  # z of 1e-45: invz is infinite and u = 0 * inf is NaN
    a = by["dot on view_cos_limit * dist"]
    assert [int(pts["state"][i]) for i in range(a, a + 3)] == [5, 0, 0]
    ref = FC.boundary_reference(sc)
    assert ref[4]["n_candidates"] > 20 and ref[4]["n_add"] + ref[4]["n_duplicate"] > 10


@pytest.mark.parametrize("name", ["default"] + list(PC.PYRAMIDS))
def test_candidate_cases_do_what_they_are_named_for(name):
    by = {}
    sc = None if name == "default" else PC.scale_table(*PC.PYRAMIDS[name])
    if sc is None:  # the default table: level 2, rows 1 and 2 of the octave case, a 4 px offset in a window of 4.32 px
        c = FC.candidate_cases()[0]
        assert (c["level"], c["expect"], c["cands"]) == (2, 1, [1, 2]) and float(FC.candidate_cases()[8]["t_kp"]["x"][0]) == 164.0
    for c in FC.candidate_cases(sc):
        idx, d1, act, pts, summ, found = FC.case_reference(c)
        by[c["name"]] = (c, idx, d1, found)
        assert pts["state"][0] == 0 and pts["u"][0] == 160 and pts["v"][0] == 120 and pts["u_right"][0] == 130, c["name"]
        assert pts["level"][0] == c["level"] == (0 if "level 0" in c["name"] else min(2, len(c["scale"]) - 1)), c["name"]
        if c["expect"] is not None:
            assert idx[0] == c["expect"], (c["name"], idx, d1)
        if c["cands"] is not None:
            assert found[2][0] == c["cands"], (c["name"], found[2])
    # the projection search accepts octave -1 at level 0, where this rule does not
    c = by["octave -1 at level 0"][0]
    assert P.match(FC.candidate_view(), c["points"], c["p_desc"], c["t_kp"], c["t_desc"], c["scale"], th=1.0, ratio_den=0)[0][0] == 0
    # the window: of the three rows around each of u + radius, u - radius some are in and some are out
    for name in ("x on the radius", "y on the radius"):
        cands = by[name][3][2][0]
        assert 0 < len([j for j in cands if j < 3]) < 3 and 0 < len([j for j in cands if j >= 3]) < 3, (name, cands)
    assert by["d1 one above th_low"][2][0] == 50 and by["a distance of 256 at th_low 255"][2][0] == 256
    # the taken row and the equal distances change the winner
    c = by["a taken row changes the winner"][0]
    assert F.match(FC.candidate_view(), c["points"], c["p_desc"], c["t_kp"], c["t_desc"], c["scale"], **c["params"])[0][0] == 0


def test_outcome_frames_on_the_reference():
    view = FC.candidate_view()
    for f in FC.outcome_frames():
        idx, d1, act, pts, summ, _ = F.match(view, f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), train_point=f["train_point"],
                                             **F.LOCAL_MAPPING)
        assert list(idx) == [0, 0, 0] and list(d1) == [9, 8, 8], f["name"]
        assert [(int(a), int(o)) for a, o in act] == f["expect"], (f["name"], act)


def test_scenes_are_live():
    """Liveness is a condition on the reference: every state occurs in every scene, the chi-square test and th_low reject something,
    every action occurs (a DUPLICATE is not required of the checker scene while the chi-square test is on)"""
    lm, sim3 = FC.PARAM_SETS[0], FC.PARAM_SETS[4]
    assert lm["name"] == "local_mapping" and sim3["params"]["chi2_mono"] == 0.0
    for k in range(len(PC.SCENES)):
        idx, d1, act, pts, summ, found = FC.scene_reference(k, lm)
        states = np.bincount(pts["state"], minlength=6)
        above = int(((found[0] >= 0) & (idx < 0)).sum())
        print(f"scene {k}: states {states}, visited {sum(len(v) for v in found[3])}, failed tests {found[4]}, bests above th_low {above}, {summ}")
        assert (states >= 1).all(), (k, states)
        assert found[4][4] >= 1 and found[4][0] >= 1 and above >= 1, (k, found[4], above)
        assert summ["n_add"] >= 1 and summ["n_replace"] >= 1 and (k == 2 or summ["n_duplicate"] >= 1), (k, summ)
        s3 = FC.scene_reference(k, sim3)[4]
        print(f"scene {k}, chi-square off: {s3}")
        assert s3["n_add"] >= 1 and s3["n_replace"] >= 1 and s3["n_duplicate"] >= 1, (k, s3)
        # the taken mask and th_low 37 each change something somewhere
    changed = {name: 0 for name in FC.SET_NAMES}
    for pset in FC.PARAM_SETS:
        for k in range(len(PC.SCENES)):
            a, b = FC.scene_reference(k, pset), FC.scene_reference(k, lm)
            changed[pset["name"]] += int((a[0] != b[0]).sum() + (a[2] != b[2]).sum())
    print(changed)
    assert all(v > 0 for n, v in changed.items() if n != "local_mapping"), changed
    # th 3 and th 4 visit the same rows once the chi-square test is on: with 5.99 it is tighter than any window of th >= 2.45
    for k in range(len(PC.SCENES)):
        p = lm["params"]
        s = FC.scenes()[k]
        a = FC.scene_found(k, 3.0, p["chi2_mono"], p["chi2_stereo"], False, False)
        b = F.search(FC.scene_points(k, 4.0), s["p_desc"], s["t_kp"], s["t_desc"], PC.scale(), p["chi2_mono"], p["chi2_stereo"], False, s["right"], None)
        assert a[2] == b[2], k


# ---- upstream's loops ----------------------------------------------------------------------------------------------------------
def _upstream_fuse(s, pts, p, taken):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th), Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) and SearchByProjection(pKF, Scw, vpPoints,
    vpMatched, th, ratioHamming), restated literally in what this library deviates from: the points are walked in sequence; a
    point's candidates come from GetFeaturesInArea in the order of upstream's 64 x 48 grid; a row replaces the best only when
    dist < bestDist; AddMapPoint is visible to the points behind it.  Step 1 and the float tests of a couple are the rule's.
    -> (row or -1, action, other) per point; a point fused into a row an earlier point added is DUPLICATE of that point"""
    grid = R.UpstreamGrid(s["t_kp"], G.W, G.H)
    assert grid.dropped == 0
    holder = {j: ("id", int(v)) for j, v in enumerate(s["train_point"]) if v >= 0}  # pKF->GetMapPoint(idx)
    out = []
    for i in range(len(pts)):
        o = pts[i]
        if o["state"] != 0:
            out.append((-1, F.ACT_NONE, -1))
            continue
        best_dist, best_idx = 256, -1
        for j in grid.features_in_area(o["u"], o["v"], o["radius"], -(1 << 15), 1 << 15):
            if F.check(o, s["t_kp"]["x"][j], s["t_kp"]["y"][j], s["t_kp"]["octave"][j], s["right"][j], s["taken"][j] if taken else None, PC.scale(),
                       p["chi2_mono"], p["chi2_stereo"], p["check_right"]) != 0:
                continue
            dist = int(R._POPCOUNT[s["p_desc"][i] ^ s["t_desc"][j]].sum())
            if dist < best_dist:
                best_dist, best_idx = dist, j
        if best_dist <= p["th_low"] and best_idx >= 0:
            if best_idx in holder:
                kind, who = holder[best_idx]
                out.append((best_idx, F.ACT_REPLACE if kind == "id" else F.ACT_DUPLICATE, who))
            else:
                holder[best_idx] = ("point", i)
                out.append((best_idx, F.ACT_ADD, -1))
        else:
            out.append((-1, F.ACT_NONE, -1))
    return out


@pytest.mark.parametrize("pset", [FC.PARAM_SETS[0], FC.PARAM_SETS[1], FC.PARAM_SETS[4], FC.PARAM_SETS[9]], ids=lambda s: s["name"])
def test_upstream_loops_against_the_order_free_rule(pset):
    """every point on which the two forms differ is of one of two kinds: its best distance is tied between candidates (upstream keeps
    the first in grid order, the rule the lowest row), or it names a train row that more than one point names (upstream lets the
    first point in order add, the rule the closest).  Seen on the three scenes (differing points of each: on a tie / on a shared
    row): local_mapping 0 / 8, 0 / 7, 0 / 0; local_mapping_right 0 / 14, 0 / 6, 0 / 0; sim3_th4_taken0_low50 0 / 8, 1 / 15, 0 / 0;
    sim3_th8_taken0_low37 0 / 6, 1 / 15, 0 / 4; every other point agrees."""
    p = pset["params"]
    for k in range(len(PC.SCENES)):
        s = FC.scenes()[k]
        idx, d1, act, pts, summ, found = FC.scene_reference(k, pset)
        up = _upstream_fuse(s, pts, p, pset["taken"])
        named = np.bincount(idx[idx >= 0], minlength=len(s["t_kp"]))
        ties = shared = same = 0
        for i, (row, action, other) in enumerate(up):
            if (row, action, other) == (int(idx[i]), int(act["action"][i]), int(act["other"][i])):
                same += 1
                continue
            dists = [int(R._POPCOUNT[s["p_desc"][i] ^ s["t_desc"][j]].sum()) for j in found[2][i]]
            tie = len(dists) > 1 and sorted(dists)[0] == sorted(dists)[1]
            share = any(r >= 0 and named[r] > 1 for r in (row, int(idx[i])))
            assert tie or share, (k, i, (row, action, other), idx[i], act[i], dists)
            ties += tie
            shared += (not tie) and share
        print(f"{pset['name']} scene {k}: {same} points agree, {ties} differ on a distance tie, {shared} on a row several points name")
        assert same > 100 or k == 2


def test_end_to_end_chain_is_live_on_the_reference():
    """epi_ref's block fused into the third keyframe by fuse_ref: at least one REPLACE and one ADD, before the device is asked"""
    import epi_cases as EC
    total = {"n_in_view": 0, "n_add": 0, "n_replace": 0}
    for k in range(len(EC.SCENES)):
        tri, w = FC.end_to_end_reference(k)
        assert len(tri[1]) == w[4]["n_points"]
        for f in total:
            total[f] += w[4][f]
    print(total)
    assert total["n_replace"] >= 1 and total["n_add"] >= 1, total


# ---- odd cameras: what makes the camera tests of tests/test_fuse.py able to fail -----------------------------------------------------------
FORMS = [(w, sh) for w in FC.CAMERA_SETS for sh in (False, True)]
FORM_IDS = [f"{w}_{'one_shared_block' if sh else 'own_blocks'}" for w, sh in FORMS]


def test_camera_views_are_the_librarys():
    """ss_proj_view_init, ss_fuse_view_sim3 and ss_sim3_to_view under cameras A, B and the square one give the reference's views"""
    for which in FC.CAMERA_SETS:
        for k in range(3):
            want = FC.camera_view(k, which, CC.FRAME_CAMERAS[k])
            assert _view_bytes(FC.library_view(binding, k, which)) == want.tobytes(), (which, k)
            assert [float(want[n]) for n in ("fx", "fy", "cx", "cy", "bf")] == list(CC.FRAME_CAMERAS[k])
    # the Sim3 views are the plain ones up to the rounding of s.R / s
    for k in range(3):
        a, b = FC.camera_view(k, "fuse", CC.A), FC.camera_view(k, "sim3_search", CC.A)
        assert np.abs(a["rcw"] - b["rcw"]).max() < 1e-6 and np.abs(a["tcw"] - b["tcw"]).max() < 1e-6


@pytest.mark.parametrize("which,shared", FORMS, ids=FORM_IDS)
def test_camera_scenes_are_live(which, shared):
    """every state of step 1 on every frame, rows outside the image under the off-centre principal points, chi-square rejections
    under Fuse, adds and replacements on the frames' own blocks"""
    for k in range(3):
        idx, d1, act, pts, summ, found = FC.camera_reference(k, which, shared)
        assert set(pts["state"].tolist()) == {0, 1, 2, 3, 4, 5} and (pts["state"] == 3).sum() >= 10 and summ["n_in_view"] > 200, (k, summ)
        assert summ["n_candidates"] >= 20 and found[4][3] > 0 and (which != "fuse" or found[4][4] > 20), (k, summ, found[4])
        if not shared and (k < 2 or which == "sim3_search"):
            assert summ["n_add"] > 20 and summ["n_replace"] > 15, (k, summ)
        view, s = FC.camera_view(k, which, CC.FRAME_CAMERAS[k]), FC.camera_scenes()
        p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **FC.CAMERA_SETS[which])
        twin = binding.fuse_points_host(view, p, PC.scale(), s[0 if shared else k]["points"], FC.camera_skip(k, shared))
        assert twin.tobytes() == pts.tobytes(), (which, k)  # the host twin
    assert FC.camera_reference(0, which, shared)[4]["n_duplicate"] > 5


@pytest.mark.parametrize("mixup", list(CC.FRAME_MIXUPS))
@pytest.mark.parametrize("which,shared", FORMS, ids=FORM_IDS)
def test_camera_mixups_change_the_reference(which, shared, mixup):
    """seen through the camera a confused kernel would use, every frame whose camera the mix-up changes has other point records;
    where the frame has matches at all (its own block, or block 0 for frame 0) and the mix-up moves the projection or reaches a
    test (bf under check_right), other idx, d1 and actions too.  No mix-up is exempt"""
    cams = list(CC.FRAME_CAMERAS)
    mixed = CC.FRAME_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed)
    assert hit, mixup
    bf_only = mixup == "bf of another frame"
    for k in hit:
        right, wrong = FC.camera_reference(k, which, shared), FC.camera_reference(k, which, shared, mixed[k])
        live = (right[3]["state"] == 0) & (wrong[3]["state"] == 0)
        fields = ("u_right",) if bf_only else ("u", "v", "u_right")
        assert live.sum() > 100 and all((right[3][f][live] != wrong[3][f][live]).any() for f in fields), (mixup, k)
        if bf_only and not FC.CAMERA_SETS[which]["check_right"]:
            continue  # u_right is computed and stored, no test reads it
        assert (right[1] != wrong[1]).any(), (mixup, k)
        if not shared or k == 0:
            assert (right[0] != wrong[0]).any() and right[2].tobytes() != wrong[2].tobytes(), (mixup, k)
