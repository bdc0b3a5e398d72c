"""CPU tests of the map-point projection search as tests/proj_ref.py states it, and of its C ABI surface: the host twin
ss_proj_points_host (the text the kernel compiles) against the reference bit for bit, ss_proj_view_init, struct layouts, refused
arguments, the two forms of the candidate set and of the level, the stand-alone sanitizer run of the steps, and that the shared
cases are what they claim to be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
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
    assert got.dtype == want.dtype == P.POINT_DTYPE and len(got) == len(want)
    for name in P.POINT_DTYPE.names:
        a, b = got[name].view(np.int32), want[name].view(np.int32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {got[name][bad[:8]]} != {want[name][bad[:8]]}"


def test_symbols_structs_and_constants(tmp_path):
    names = ["ss_proj_view_init", "ss_proj_points_host", "ss_match_proj_pairs_device", "ss_match_proj_batch_device", "ss_match_proj"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("match_proj_pairs_device", "match_proj_batch_device", "match_proj"):
        assert callable(getattr(binding.OrbContext, m))
    assert callable(binding.proj_params) and callable(binding.proj_view) and callable(binding.proj_points_host)
    assert C.sizeof(binding.ProjView) == 96 and C.sizeof(binding.ProjParams) == 40 and C.sizeof(binding.ProjSummary) == 32
    assert binding.MAP_POINT_DTYPE.itemsize == 32 and binding.PROJ_POINT_DTYPE.itemsize == 32 and binding.PROJ_SUMMARY_DTYPE.itemsize == 32
    assert binding.PROJ_VIEW_DTYPE.itemsize == 96
    assert binding.PROJ_VIEW_DTYPE == P.VIEW_DTYPE and binding.MAP_POINT_DTYPE == P.MAP_POINT_DTYPE and binding.PROJ_POINT_DTYPE == P.POINT_DTYPE
    assert tuple(n for n, _ in binding.ProjSummary._fields_) == P.SUMMARY_FIELDS
    assert tuple(n for n, _ in binding.ProjView._fields_) == P.VIEW_DTYPE.names
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_proj_view) == 96, "view");\n'
                   '_Static_assert(sizeof(ss_map_point) == 32, "map point");\n'
                   '_Static_assert(sizeof(ss_proj_point) == 32, "point");\n'
                   '_Static_assert(sizeof(ss_proj_summary) == 32, "summary");\n'
                   '_Static_assert(sizeof(ss_proj_params) == 40, "params");\n'
                   '_Static_assert(offsetof(ss_proj_view, ow) == 48 && offsetof(ss_proj_view, fx) == 60 && offsetof(ss_proj_view, min_x) == 80, "view fields");\n'
                   '_Static_assert(offsetof(ss_map_point, min_dist) == 24 && offsetof(ss_proj_point, level) == 24, "fields");\n'
                   '_Static_assert(offsetof(ss_proj_params, th_high) == 12 && offsetof(ss_proj_params, extent_w) == 32, "params fields");\n'
                   '_Static_assert(offsetof(ss_proj_summary, n_in_view) == 12 && offsetof(ss_proj_summary, reserved) == 28, "summary fields");\n'
                   '_Static_assert(SS_GUIDED_MAX_ROWS == 16384 && SS_ABI_VERSION == 5 && SS_MAX_LEVELS == 16, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5


def test_view_init_agrees_with_its_restatement():
    rng = np.random.Generator(np.random.PCG64(0x71E3))
    poses = list(PC.POSES) + [(np.eye(3), (0.0, 0.0, 0.0)), (PC.rot(0.7, -1.1, 2.0), (3.25, -17.0, 0.001))]
    poses += [(PC.rot(*rng.normal(0, 1, 3)), tuple(rng.normal(0, 10, 3))) for _ in range(50)]
    for rcw, tcw in poses:
        cam = binding.Camera(fx=517.3, fy=516.5, cx=318.6, cy=255.3, width=640, height=480)
        got = np.frombuffer(bytes(binding.proj_view(cam, rcw, tcw, bf=40.0)), P.VIEW_DTYPE)[0]
        want = P.view_init(517.3, 516.5, 318.6, 255.3, 640, 480, rcw, tcw, 40.0)
        assert got.tobytes() == want.tobytes(), (got, want)
    assert float(want["max_x"]) == 640 and float(want["max_y"]) == 480 and float(want["min_x"]) == 0 and float(want["bf"]) == 40
    assert binding.load().ss_proj_view_init(None, None, None, C.c_float(0), None) == binding.SS_ERR_INVALID_ARG


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


def test_host_twin_agrees_with_the_reference_bit_for_bit():
    """the compiler's float steps against numpy's: the boundary table, then 10 000 random points under three poses"""
    sc = PC.scale()
    view, points, groups, *_ = PC.boundary_table()
    p = binding.proj_params(**PC.B_LIMITS)
    _same(binding.proj_points_host(view, p, sc, points), P.eval_points(view, points, **PC.B_LIMITS, scale=sc), "boundary table")
    rng = np.random.Generator(np.random.PCG64(0x10000))
    pts = _random_points(rng, 10000)
    states = np.zeros(6, int)
    for k, (limit, th, far) in enumerate([(0.5, 1.0, 0.0), (0.5, 3.0, 6.0), (-1.0, 2.5, 0.0)]):
        view = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, PC.POSES[k][0], PC.POSES[k][1], PC.BF)
        part = pts[k::3]
        want = P.eval_points(view, part, limit, th, far, sc)
        _same(binding.proj_points_host(view, binding.proj_params(view_cos_limit=limit, th=th, far_limit=far), sc, part), want, f"random points, pose {k}")
        states += np.bincount(want["state"], minlength=6)
        assert set(want["level"][want["state"] == 0]) == set(range(8))
    print("states", states)
    assert (states > 20).all()  # every test rejects something, and plenty is in view
    # another table: three levels of scale 2
    want = P.eval_points(view, part, 0.5, 1.0, 0.0, [f32(1), f32(2), f32(4)])
    _same(binding.proj_points_host(view, binding.proj_params(), [1, 2, 4], part), want, "three levels")
    assert len(binding.proj_points_host(view, binding.proj_params(), sc, pts[:0])) == 0


def test_invalid_arguments_are_refused_without_a_device():
    """the parameter check of the device calls (one function in the library) through the host twin, which needs no context; the
    checks that need one (row counts, point_src) are in tests/test_proj.py"""
    sc = PC.scale()
    view, points, *_ = PC.boundary_table()
    bad = [dict(th=0.0), dict(th=-1.0), dict(th=float("nan")), dict(th=float("inf")), dict(view_cos_limit=float("nan")), dict(th_high=-1),
           dict(th_high=257), dict(ratio_num=-1), dict(ratio_num=32768), dict(ratio_den=-1), dict(ratio_den=32768)]
    for kw in bad:
        with pytest.raises(binding.OrbError) as e:
            binding.proj_points_host(view, binding.proj_params(**kw), sc, points)
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    for good in (dict(th_high=0), dict(th_high=256), dict(ratio_num=32767, ratio_den=32767), dict(ratio_den=0), dict(view_cos_limit=float("-inf")),
                 dict(far_limit=float("nan")), dict(th=1e-30)):
        assert len(binding.proj_points_host(view, binding.proj_params(**good), sc, points)) == len(points)
    for levels in (np.zeros(0, np.float32), np.ones(17, np.float32)):
        with pytest.raises(binding.OrbError):
            binding.proj_points_host(view, binding.proj_params(), levels, points)
    # no context, no call
    lib = binding.load()
    p = binding.proj_params(extent_w=320, extent_h=240)
    assert lib.ss_match_proj_pairs_device(None, None, None, None, 0, 1, None, None, None, None, None, 0, 1, None, None, C.byref(p), None, None, None,
                                          None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_match_proj_batch_device(None, None, None, None, 0, 1, None, None, None, None, C.byref(p), None, None, None, None,
                                          None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_match_proj(None, None, None, None, 0, None, None, 0, None, None, C.byref(p), None, None, None, None, None) == binding.SS_ERR_INVALID_ARG


@pytest.mark.parametrize("k,th", [(0, 1.0), (1, 3.0), (2, 3.0)])
def test_upstream_grid_and_box_test_give_the_same_candidates(k, th):
    """Frame::GetFeaturesInArea(u, v, radius, level - 1, level) on upstream's 64 x 48 grid, as written, against the box form the
    reference's search runs on.  A keypoint the upstream grid drops would be a documented difference: the extractor keeps 19 px
    from the border, so there is none here."""
    s = PC.scenes()[k]
    proj = PC.scene_proj(k, th)
    win = P.windows_of(proj)
    grid = R.UpstreamGrid(s["t_kp"], G.W, G.H)
    assert grid.dropped == 0
    cands = PC.scene_found(k, th, False, False)[4]
    total = 0
    for i in range(len(proj)):
        if proj["state"][i] != 0:
            assert cands[i] == []
            continue
        lvl = int(proj["level"][i])
        up = sorted(grid.features_in_area(proj["u"][i], proj["v"][i], proj["radius"][i], lvl - 1, lvl))
        assert up == R.box_candidates(win[i], s["t_kp"]) == cands[i], (i, up, cands[i])
        total += len(up)
    assert total > 200


def _levels_table(ratio, sc):
    """level_table, element-wise: the number of entries below the ratio, capped"""
    return np.minimum(np.searchsorted(np.asarray(sc, np.float32), ratio, side="left"), len(sc) - 1)


def _levels_log(ratio, factor, n):
    with np.errstate(all="ignore"):
        v = np.ceil(np.log(ratio.astype(np.float32)) / np.log(f32(factor)))
    return np.clip(v, 0, n - 1).astype(np.int64)


def test_level_table_form_against_the_float_log_form():
    """scale 1.2, 8 levels: 2 M ratios in [0.3, 5] plus +-3000 ulp around every table entry.  Every disagreement between the rule's
    table form and upstream's ceil(logf(ratio) / logScaleFactor) lies within 2 float32 ulp of a table entry.  Seen with
    numpy's float32 log: 4 disagreeing ratios, 1, 1, 1 and 2 ulp above scale[3], scale[5], scale[6]."""
    sc = np.array(PC.scale(), np.float32)
    assert len(sc) == 8 and sc[1] == f32(1.2)
    rng = np.random.Generator(np.random.PCG64(0x1065))
    near = np.concatenate([(s.view(np.int32) + np.arange(-3000, 3001, dtype=np.int32)).view(np.float32) for s in sc.reshape(-1, 1)])
    ratio = np.concatenate([rng.uniform(0.3, 5.0, 2_000_000).astype(np.float32), near, sc])
    table, log = _levels_table(ratio, sc), _levels_log(ratio, 1.2, 8)
    # the element-wise forms are the serial ones
    for r in np.concatenate([ratio[:2000], near[::97], sc]):
        assert _levels_table(np.array([r], np.float32), sc)[0] == P.level_table(r, sc)
        assert _levels_log(np.array([r], np.float32), 1.2, 8)[0] == P.level_log(r, 1.2, 8)
    bad = np.flatnonzero(table != log)
    ulp = np.array([np.abs(ratio[bad].view(np.int32).astype(np.int64)[:, None] - sc.view(np.int32).astype(np.int64)[None, :]).min(axis=1)]).reshape(-1) if len(bad) else np.zeros(0, int)
    print("disagreements", len(np.unique(ratio[bad])), "ratios", np.unique(ratio[bad]), "ulp from a table entry", ulp, "levels", table[bad], log[bad])
    assert (ulp <= 2).all()
    assert set(table) == set(range(8))


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/proj_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process
    without any preloaded library"""
    exe = str(tmp_path / "proj_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "proj_steps_asan.cpp")])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 50000


def test_boundary_table_is_live():
    """on the REFERENCE: across every boundary the state, the level or the radius changes"""
    view, points, groups, *_ = PC.boundary_table()
    proj = P.eval_points(view, points, **PC.B_LIMITS, scale=PC.scale())
    for name, a, live in groups:
        rows = [(int(proj["state"][i]), int(proj["level"][i]), float(proj["radius"][i])) for i in range(a, a + 3)]
        assert (len(set(rows)) > 1) == live, (name, rows)
    assert {int(s) for s in proj["state"]} == {0, 1, 2, 3, 4, 5}
    assert sum(1 for _, _, live in groups if not live) == 1


def test_ratio_cases_do_what_they_are_named_for():
    """the level-aware test on the reference, with the expectation written out in proj_cases.RATIO_CASES.  Under 8 / 10 the test
    rejects d1 * 10 > d2 * 8: at one level 8 against 9 is rejected, 8 against 10 is accepted (equality accepts) and so is 8
    against 11."""
    view, frames = PC.ratio_frames()
    for f in frames:
        idx, d1, d2, proj, summ, cands = P.match(view, f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), right=f["right"], taken=f["taken"],
                                                 **PC.RATIO_PARAMS)
        assert proj["state"][0] == 0 and idx[0] == f["expect"], (f["name"], idx, d1, d2)
    by = {f["name"]: f for f in frames}
    # the taken row and the right-eye test change the winner: without them row 0 wins
    for name in ("taken_row", "right_eye", "right_eye_on_the_radius"):
        f = by[name]
        idx = P.match(view, f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), **dict(PC.RATIO_PARAMS, check_right=False))[0]
        assert idx[0] == 0 != f["expect"], name


def test_scenes_give_every_filter_work():
    """no vacuous pass on the GPU: levels cover every octave, every frustum test rejects points, and the ratio test, one_to_one,
    the taken mask and the right-eye test each change the result of every scene"""
    for k in range(len(PC.SCENES)):
        base = dict(ratio=(8, 10), one_to_one=False, th=3.0, check_right=False, taken=False)
        idx, d1, d2, proj, summ, cands = PC.scene_reference(k, base)
        assert set(proj["level"][proj["state"] == 0]) == set(range(8))
        assert {int(s) for s in proj["state"]} == {0, 1, 2, 3, 4}
        assert summ["n_candidates"] > 2 * summ["n_in_view"] and 30 < summ["n_accepted"] < summ["n_in_view"]
        assert PC.scene_reference(k, dict(base, ratio=(0, 0)))[4]["n_accepted"] > summ["n_accepted"]
        uni = PC.scene_reference(k, dict(base, one_to_one=True))[4]
        assert uni["n_unique"] < uni["n_accepted"] == summ["n_accepted"]
        for change in (dict(taken=True), dict(check_right=True), dict(th=1.0)):
            other = PC.scene_reference(k, dict(base, **change))
            assert other[4]["n_candidates"] < summ["n_candidates"] and not np.array_equal(other[0], idx), change
        assert (d2[idx >= 0] != P.NONE).any() and (d2[idx >= 0] == P.NONE).any()


def test_capacity_frames_need_both_conflict_passes():
    for b in range(2):
        idx, d1, d2, proj, summ, cands = PC.capacity_reference(b)
        loose = PC.capacity_reference(b, one_to_one=False)[0]
        wanted, times = np.unique(loose[loose >= 0], return_counts=True)
        contested = wanted[times >= 2]
        print(b, summ, "contested rows below / from 8192:", int((contested < 8192).sum()), int((contested >= 8192).sum()))
        assert summ["n_points"] == summ["n_train"] == PC.CAP_ROWS == binding.SS_GUIDED_MAX_ROWS
        assert (contested >= 8192).sum() > 500 and summ["n_unique"] < summ["n_accepted"] - 1000
        if b == 0:
            assert (contested < 8192).sum() > 500


# ---- the limit cases of tests/proj_cases.py reach what they are meant for ---------------------------------------------------------
def test_scale_table_is_the_context_table_and_other_tables_are_live():
    assert PC.scale_table(1.2, 8) == tuple(PC.scale())
    assert set(PC.PYRAMIDS.values()) == {(1.2, 1), (1.2, 2), (2.0, 4), (1.1, binding.SS_MAX_LEVELS)}
    for name, (factor, n) in PC.PYRAMIDS.items():
        sc = PC.scale_table(factor, n)
        assert len(sc) == n and sc[0] == 1 and all(a < b for a, b in zip(sc, sc[1:]))
        view, points, groups, tk, td, pd = PC.boundary_table(sc)
        p = binding.proj_params(**PC.B_LIMITS)
        proj = P.eval_points(view, points, **PC.B_LIMITS, scale=sc)
        _same(binding.proj_points_host(view, p, sc, points), proj, name)
        for g, a, live in groups:
            rows = [(int(proj["state"][i]), int(proj["level"][i]), float(proj["radius"][i])) for i in range(a, a + 3)]
            assert (len(set(rows)) > 1) == live, (name, g, rows)
        ratio = [g for g, _, _ in groups if g.startswith("ratio on")]
        assert len(ratio) == n and sum(1 for _, _, live in groups if not live) == 1
        seen = set(int(v) for v in proj["level"][proj["state"] == 0])
        assert seen == set(range(n)), (name, seen)
        # a ratio below scale[0] gives level 0, one above the last entry the last level; the window takes octaves level - 1 .. level
        below, above = proj[len(points) - 17], proj[len(points) - 1]
        assert below["state"] == 0 and below["level"] == 0 and above["state"] == 0 and above["level"] == n - 1
        want = P.match(view, points, pd, tk, td, sc, th_high=256, ratio_num=0, ratio_den=0, **PC.B_LIMITS)
        octs = {int(tk["octave"][j]) for c in want[5] for j in c}
        assert octs == set(range(-1, n)), (name, octs)  # octave -1 is a candidate of level 0, octave n of nobody
    assert tuple(PC.scale_table(2.0, 4)) == (1, 2, 4, 8)


def test_other_grids_are_the_documented_ones():
    shapes = []
    for w, h in PC.EXTENTS:
        s = G.grid_shift(w, h)
        shapes.append((s, ((min(w, G.CAP_FAR) - 1) >> s) + 1, ((min(h, G.CAP_FAR) - 1) >> s) + 1))
    print(shapes)
    assert shapes == [(8, 63, 47), (12, 4096, 1), (5, 2, 2), (5, 157, 2), (5, 1, 1), (5, 4, 3)]
    spread = np.concatenate([s["t_kp"]["x"] for s in PC.scenes()]).max(), np.concatenate([s["t_kp"]["y"] for s in PC.scenes()]).max()
    assert spread[0] > 200 and spread[1] > 160  # train rows lie outside 100 x 80, 33 x 33 and 1 x 1
    assert any(c["one_to_one"] and c["check_right"] and c["taken"] for c in PC.EXTENT_COMBOS) and len(PC.EXTENT_COMBOS) >= 2


def test_edge_table_windows_reach_beyond_the_image_and_hold_every_row():
    view, points, pd, tk, td = PC.edge_table()
    assert float(view["max_x"]) == PC.E_W and float(view["max_y"]) == PC.E_H
    small, huge = PC.edge_reference(PC.E_THS[0]), PC.edge_reference(PC.E_THS[-1])
    proj = small[3]
    ok = proj["state"] == 0
    for name, lo, hi in (("u", 0, PC.E_W), ("v", 0, PC.E_H)):  # on each bound, and one step inside it
        vals = set(float(v) for v in proj[name][ok])
        assert {float(lo), float(hi), float(np.nextafter(f32(hi), f32(0)))} <= vals and 0 < min(vals - {float(lo)}) < 2.0 ** -15, (name, sorted(vals))
    assert (proj["state"] == 2).sum() == len(points) - ok.sum() > 30  # one step outside
    sides = lambda p: sum(c.astype(int) for c in (p["u"] - p["radius"] < 0, p["u"] + p["radius"] > PC.E_W, p["v"] - p["radius"] < 0, p["v"] + p["radius"] > PC.E_H))
    assert {1, 2} <= set(int(v) for v in sides(small[3][ok]))
    assert set(int(v) for v in sides(PC.edge_reference(PC.E_THS[2])[3][ok])) == {4}
    # th = 1e30: the window holds every train row; the candidates are the rows of the two octaves
    assert np.isfinite(huge[3]["radius"][ok]).all() and huge[3]["radius"][ok].min() > 1e30
    for i in np.flatnonzero(ok):
        lvl = int(huge[3]["level"][i])
        assert huge[5][i] == [j for j in range(len(tk)) if lvl - 1 <= tk["octave"][j] <= lvl], i
    assert huge[4]["n_candidates"] > PC.edge_reference(PC.E_THS[2])[4]["n_candidates"]
    kx, ky = tk["x"], tk["y"]
    assert ((kx == 319) & (ky == 239)).any() and ((kx == 0) & (ky == 0)).any() and ((kx == 320) & (ky == 240)).any()
    assert (kx < 0).any() and (kx > PC.E_W).any() and (ky < 0).any() and (ky > PC.E_H).any()
    used = {j for c in small[5] for j in c}
    assert {j for j in range(len(tk)) if kx[j] in (0, 319, 320) or ky[j] in (0, 239, 240)} & used  # border rows are candidates


def test_far_descriptor_and_count_cases():
    f = PC.far_descriptor_frame()
    kw = dict(PC.RATIO_PARAMS, check_right=False)
    for th_high, idx in ((256, 0), (255, -1)):
        got = P.match(f["view"], f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), **dict(kw, th_high=th_high))
        assert got[0][0] == idx and got[1][0] == 256 and got[2][0] == P.NONE
    base, counts = PC.count_frames()
    assert len(base["points"]) == len(base["t_kp"]) == PC.COUNT_ROWS == 65
    assert {0, 1, 63, 64, 65} <= {k for k, _ in counts} and {0, 1, 63, 64, 65} <= {nt for _, nt in counts}
    assert any(k > 65 for k, _ in counts) and any(nt > 65 for _, nt in counts)
    full = PC.count_reference(65, 65)
    assert full[4]["n_unique"] < full[4]["n_accepted"] and full[4]["n_candidates"] > 100
    assert PC.count_reference(64, 65)[4] != full[4] != PC.count_reference(65, 64)[4]  # the 65th row of either side matters
    assert PC.count_reference(70, 1 << 30)[4] == full[4]


# ---- odd cameras: what makes the camera tests of tests/test_proj.py able to fail -----------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["own_blocks", "one_shared_block"])
def test_camera_scenes_are_live(shared):
    """the three scenes under cameras A, B and the square one: matches on every frame, every rejection state of step 1, rows outside
    the image under the off-centre principal points, right-eye rejections under each frame's own bf; at most 500 points a frame"""
    for k, s in enumerate(PC.camera_scenes()):
        assert s["view"].tobytes() == PC.camera_view(k, CC.FRAME_CAMERAS[k]).tobytes() and len(s["points"]) <= 500 and len(s["t_kp"]) <= 500
        idx, d1, d2, proj, summ, cands = PC.camera_reference(k, shared)
        assert summ["n_unique"] > (50 if not shared or k == 0 else 5) and summ["n_candidates"] > 300, (k, summ)
        assert (proj["state"] == 2).sum() >= 10 and {1, 2, 3, 4} <= set(proj["state"].tolist()), k
        b = PC.camera_scenes()[0 if shared else k]
        blind = P.search(proj, b["p_desc"], s["t_kp"], s["t_desc"], False, None, s["taken"])[4]
        assert sum(len(c) for c in blind) > summ["n_candidates"], k  # the right-eye test rejected candidates
        p = PC.combo_params(binding, PC.CAMERA_COMBO, extent_w=G.W, extent_h=G.H)
        assert binding.proj_points_host(s["view"], p, PC.scale(), b["points"]).tobytes() == proj.tobytes(), k  # the host twin
    assert len({s["view"][n].tobytes() for s in PC.camera_scenes() for n in ("fx", "fy", "cx", "cy", "bf")}) == 14  # all different but the square camera's fx and fy


@pytest.mark.parametrize("mixup", list(CC.FRAME_MIXUPS))
@pytest.mark.parametrize("shared", [False, True], ids=["own_blocks", "one_shared_block"])
def test_camera_mixups_change_the_reference(shared, mixup):
    """seen through the camera a confused kernel would use, every frame whose camera the mix-up changes has other idx, d1, d2 and
    projection records.  No mix-up is exempt"""
    cams = list(CC.FRAME_CAMERAS)
    mixed = CC.FRAME_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed)
    assert hit, mixup
    for k in hit:
        right, wrong = PC.camera_reference(k, shared), PC.camera_reference(k, shared, mixed[k])
        for j, name in enumerate(("idx", "d1", "d2")):
            assert (right[j] != wrong[j]).any(), (mixup, k, name)
        fields = ("u_right",) if mixup == "bf of another frame" else ("u", "v", "u_right")
        live = (right[3]["state"] == 0) & (wrong[3]["state"] == 0)
        assert live.sum() > 100 and all((right[3][f][live] != wrong[3][f][live]).any() for f in fields), (mixup, k)
