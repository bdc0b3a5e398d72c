"""CPU tests of the map points from depth: upstream's loop against the closed form of the selection; the host twin ss_unproject_host
(the text the kernel compiles) against tests/unproject_ref.py, byte for byte; the refusals; the steps under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import unproject_cases as K
import unproject_ref as U
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["ss_unproject_view_init", "ss_unproject_host", "ss_unproject_pairs_device", "ss_unproject_batch_device", "ss_unproject"]


def test_header_structs_and_exports():
    lib = binding.load()
    assert lib.ss_abi_version() == 5
    text = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\(", code), name
        assert name in binding.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(binding.UnprojectView) == 168 == binding.UNPROJECT_VIEW_DTYPE.itemsize == U.VIEW_DTYPE.itemsize
    assert C.sizeof(binding.UnprojectParams) == 16 and binding.UNPROJECT_INFO_DTYPE.itemsize == 4 and binding.UNPROJECT_SUMMARY_DTYPE.itemsize == 40
    assert binding.UNPROJECT_SUMMARY_DTYPE.names == U.SUMMARY_FIELDS
    assert (binding.SS_UNPROJECT_ALL, binding.SS_UNPROJECT_CLOSE) == (U.ALL, U.CLOSE)
    for name, value in (("ALL", 0), ("CLOSE", 1), ("CREATED", 0), ("KEPT", 1), ("FAR", 2), ("NO_DEPTH", 3), ("OCTAVE", 4), ("DEGENERATE", 5)):
        assert re.search(r"#define SS_UNPROJECT_%s %d\b" % (name, value), text), name
        assert getattr(binding, "SS_UNPROJECT_" + name) == value
    assert "parity with the real binary stays unpinned" in text[text.index("map points from depth"):]


def test_view_init_equals_the_reference_and_the_epipolar_pair():
    for cam, pose in zip(CC.FRAME_CAMERAS, K.POSES):
        v = binding.unproject_view(K.binding_camera(cam), *pose)
        assert bytes(v) == K.ref_view(cam, pose).tobytes()
        pair = binding.epi_pair(K.binding_camera(cam), *pose, K.binding_camera(cam), *pose)
        assert bytes(v.ow) == bytes(pair.ow1) and v.invfx == pair.invfx1 and v.invfy == pair.invfy1
    lib = binding.load()
    r, t, v = np.eye(3).ravel(), np.zeros(3), binding.UnprojectView()
    cam = K.binding_camera(CC.A)
    for args in ((None, r.ctypes.data, t.ctypes.data, C.byref(v)), (C.byref(cam), None, t.ctypes.data, C.byref(v)),
                 (C.byref(cam), r.ctypes.data, None, C.byref(v)), (C.byref(cam), r.ctypes.data, t.ctypes.data, None)):
        assert lib.ss_unproject_view_init(*args) == binding.SS_ERR_INVALID_ARG


def test_the_closed_form_is_upstreams_loop_on_random_frames():
    """ties at the cut, +inf, NaN, 0 and negative depths; max_points from 0 to beyond the rows; limits on, between and outside the
    values"""
    rng = np.random.Generator(np.random.PCG64(0xC105ED))
    values = np.array(K.DEPTHS + K.NO_DEPTHS, np.float32)
    frames = differing = 0
    for _ in range(20000):
        rows = int(rng.integers(0, 60))
        depth = rng.choice(values, rows) if rng.random() < 0.7 else rng.uniform(-1, 6, rows).astype(np.float32)
        octave = np.where(rng.random(rows) < 0.05, 8, rng.integers(0, 8, rows))
        n = int(rng.integers(-2, rows + 3))
        ranked = U.ranked_rows(depth, octave, U.clamp(n, rows), 8)
        mp, limit, mode = int(rng.integers(0, 70)), rng.choice(np.array([0.25, 1.0, 3.0, 3.25, 4.0, 1e30, np.inf], np.float32)), int(rng.random() < 0.9)
        a, b = U.select_literal(depth, ranked, mode, mp, limit), U.select_closed(depth, ranked, mode, mp, limit)
        frames += 1
        differing += a != b
        assert a == b, (depth, n, mp, limit, mode)
        if mode == U.CLOSE and len(ranked) > mp + 1:
            assert len(a) >= min(len(ranked), mp + 1)
    print("frames", frames, "differing", differing)


def _reference_and_twin(view_ref, view_twin, mode, mp, kp, desc, depth, **kw):
    want = U.frame(view_ref, mode, mp, K.CLOSE_LIMIT, K.scale(), kp, desc, depth, **kw)
    closed = U.frame(view_ref, mode, mp, K.CLOSE_LIMIT, K.scale(), kp, desc, depth, literal=False, **kw)
    got = K.twin_frame(view_twin, mode, mp, K.CLOSE_LIMIT, kp, desc, depth, **kw)
    K.same_frame("closed form", closed, want)
    K.same_frame("twin", got, want)
    return want


@pytest.mark.parametrize("name,max_points,depth", K.selection_cases(), ids=[c[0] for c in K.selection_cases()])
def test_selection_cases(name, max_points, depth):
    f = K.frames_case()
    b = max_points % K.F
    ref, twin = K.ref_views()[b], K.twin_views()[b]
    want = _reference_and_twin(ref, twin, U.CLOSE, max_points, f["kp"][b], f["desc"][b], depth, has_point=f["has_point"][b], outlier=f["outlier"][b])
    s = want["summary"]
    print(name, s)
    live = s["n_depth"] - int(((depth > 0) & ((f["kp"][b]["octave"] < 0) | (f["kp"][b]["octave"] > 7))).sum())
    assert s["n_processed"] == min(live, max(s["n_not_far"], max_points) + 1)
    assert s["n_tracked_close"] + s["n_untracked_close"] == s["n_close"] <= s["n_not_far"]
    if name == "max5_all_equal":
        rows = np.flatnonzero(want["state"] <= U.KEPT)
        assert rows.tolist() == [i for i in range(K.ROWS) if f["kp"][b]["octave"][i] in range(8)][:6], "the lower rows win among equal depths"
    # every row: StereoInitialization
    _reference_and_twin(ref, twin, U.ALL, max_points, f["kp"][b], f["desc"][b], depth, has_point=f["has_point"][b])


@pytest.mark.parametrize("counts", K.COUNTS, ids=["counts_70_1_0", "counts_past_the_rows_and_below_0"])
@pytest.mark.parametrize("flags", ["null", "all_0", "all_1", "mixed"])
def test_frames_under_three_cameras(counts, flags):
    """non-square, off-centre cameras under rotated and translated poses; has_point NULL, all 0, all 1 and mixed"""
    f = K.frames_case()
    states = set()
    for b in range(K.F):
        hp = {"null": None, "all_0": np.zeros(K.ROWS, np.uint8), "all_1": np.full(K.ROWS, 7, np.uint8), "mixed": f["has_point"][b]}[flags]
        for mode in (U.ALL, U.CLOSE):
            want = _reference_and_twin(K.ref_views()[b], K.twin_views()[b], mode, K.MAX_POINTS, f["kp"][b], f["desc"][b], f["depth"][b], n=counts[b],
                                       has_point=hp, outlier=f["outlier"][b])
            states |= set(want["state"].tolist())
            assert want["summary"]["n_kp"] == U.clamp(counts[b], K.ROWS) and (want["state"][want["summary"]["n_kp"]:] == -1).all()
            if flags == "all_1":
                assert want["summary"]["n_created"] == 0 and want["summary"]["n_kept"] == want["summary"]["n_processed"]
            if flags in ("null", "all_0"):
                assert want["summary"]["n_kept"] == 0 and want["summary"]["n_tracked_close"] == 0
    if flags == "mixed":
        assert states == {-1, 0, 1, 2, 3, 4, 5}, states  # +inf depths give state 5, the two rows outside the table state 4


def test_null_and_zero_flags_give_the_same_bytes_and_a_stereo_point_array_is_read_in_place():
    f = K.frames_case()
    v = K.twin_views()[0]
    a = K.twin_frame(v, U.CLOSE, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][0], f["desc"][0], f["depth"][0])
    b = K.twin_frame(v, U.CLOSE, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][0], f["desc"][0], f["depth"][0], has_point=np.zeros(K.ROWS, np.uint8))
    c = K.twin_frame(v, U.CLOSE, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][0], f["desc"][0], K.stereo_points(f["depth"][0]))
    K.same_frame("zero flags", b, a)
    K.same_frame("stride 16", c, a)
    assert a["summary"]["n_created"] > 0


def test_camera_mixups_change_the_bytes():
    f = K.frames_case()
    base = [U.frame(v, U.ALL, 0, K.CLOSE_LIMIT, K.scale(), f["kp"][b], f["desc"][b], f["depth"][b]) for b, v in enumerate(K.ref_views())]
    for name, mix in CC.FRAME_MIXUPS.items():
        if name.startswith("bf"):
            continue  # no bf in this family: the depth is given
        mixed = mix(list(CC.FRAME_CAMERAS))
        for b in CC.changed(CC.FRAME_CAMERAS, mixed, fields=(0, 1, 2, 3)):
            other = U.frame(K.ref_view(mixed[b], K.POSES[b]), U.ALL, 0, K.CLOSE_LIMIT, K.scale(), f["kp"][b], f["desc"][b], f["depth"][b])
            assert other["points"].tobytes() != base[b]["points"].tobytes(), (name, b)
            # the host twin under the mixed camera computes the reference's bytes for it, not the right camera's
            twin = K.twin_frame(binding.unproject_view(K.binding_camera(mixed[b]), *K.POSES[b]), U.ALL, 0, K.CLOSE_LIMIT, f["kp"][b], f["desc"][b], f["depth"][b])
            K.same_frame(f"{name}, frame {b}", twin, other)


def test_a_non_finite_pose_gives_state_5():
    f = K.frames_case()
    for bad in ((np.eye(3), (0.0, np.nan, 0.0)), (np.where(np.eye(3) > 0, np.inf, 0.0), (0.0, 0.0, 0.0)), (np.eye(3), (np.inf, 0.0, 0.0))):
        with np.errstate(all="ignore"):
            ref, twin = K.ref_view(CC.A, bad), binding.unproject_view(K.binding_camera(CC.A), *bad)
        want = _reference_and_twin(ref, twin, U.ALL, 0, f["kp"][0], f["desc"][0], f["depth"][0])
        assert want["summary"]["n_created"] == 0 and (want["state"] == U.DEGENERATE).sum() == want["summary"]["n_processed"] > 0


def test_refusals():
    f = K.frames_case()
    kp, desc, depth, v, sc = f["kp"][0], f["desc"][0], f["depth"][0], K.twin_views()[0], K.scale()
    ok = binding.unproject_params(U.CLOSE, 5, 3.0)
    for bad in (dict(mode=2), dict(mode=-1), dict(max_points=-1), dict(close_limit=float("nan")), dict(close_limit=float("inf")), dict(reserved=1)):
        p = binding.UnprojectParams(**dict(dict(mode=1, max_points=5, close_limit=3.0, reserved=0), **bad))
        with pytest.raises(binding.OrbError) as e:
            binding.unproject_host(v, p, sc, kp, desc, depth)
        assert e.value.code == binding.SS_ERR_INVALID_ARG, bad
    lib = binding.load()
    info, pts, pd, pr = np.zeros(K.ROWS, binding.UNPROJECT_INFO_DTYPE), np.zeros(K.ROWS, binding.MAP_POINT_DTYPE), np.zeros((K.ROWS, 32), np.uint8), np.zeros((K.ROWS, 2), np.int32)
    n_pts, summary = np.zeros(1, np.int32), np.zeros(1, binding.UNPROJECT_SUMMARY_DTYPE)

    def call(stride=4, depth_at=depth.ctypes.data, n_levels=8, rows=K.ROWS, view=C.byref(v), kp_at=kp.ctypes.data, n_at=n_pts.ctypes.data):
        return lib.ss_unproject_host(view, C.byref(ok), sc.ctypes.data, n_levels, kp_at, desc.ctypes.data, K.ROWS, rows, depth_at, stride, None, None,
                                     info.ctypes.data, pts.ctypes.data, pd.ctypes.data, pr.ctypes.data, n_at, summary.ctypes.data)
    assert call() == binding.SS_OK and n_pts[0] > 0
    for kw in (dict(stride=0), dict(stride=-4), dict(stride=6), dict(depth_at=depth.ctypes.data + 2), dict(depth_at=None), dict(n_levels=0),
               dict(n_levels=17), dict(rows=-1), dict(rows=binding.SS_GUIDED_MAX_ROWS + 1), dict(view=None), dict(kp_at=None), dict(n_at=None)):
        assert call(**kw) == binding.SS_ERR_INVALID_ARG, kw
    # no rows: nothing is read
    r = binding.unproject_host(v, ok, sc, kp[:0], desc[:0], depth[:0])
    assert len(r[0]) == 0 and len(r[1]) == 0 and int(r[4]["n_kp"]) == 0


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/unproject_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "unproject_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "unproject_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
