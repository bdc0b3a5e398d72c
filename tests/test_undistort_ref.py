"""CPU tests of Frame's keypoint post-processing: the host twins ss_undistort_host, ss_undistort_bounds_host, ss_proj_view_set_bounds and
ss_depth_host (the text the kernels compile) against oracle/vo_oracle.py::undistort, tests/undistort_ref.py and the tracker's own
routine, bit for bit; the refusals; the steps under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import proj_ref as P
import undistort_cases as UC
import undistort_ref as UR
from oracle import vo_oracle as vo
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERAS = ["D", "P", "T", "Z"]
NEW_EXPORTS = ["ss_undistort_bounds_host", "ss_proj_view_set_bounds", "ss_undistort_host", "ss_undistort_pairs_device", "ss_undistort_batch_device",
               "ss_get_batch_raw_xy", "ss_depth_params_from_camera", "ss_depth_host", "ss_depth_pairs_device", "ss_depth_batch_device"]


def xy_of(kp):
    return np.stack([kp["x"], kp["y"]], axis=1)


def same_bits(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    bad = np.flatnonzero(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)) if len(got) else []
    assert len(bad) == 0, f"{tag}: {len(bad)} bytes differ, first at {bad[:4]}"


@pytest.mark.parametrize("name", CAMERAS)
def test_host_twin_equals_the_oracle_bit_for_bit(name):
    cam = UC.camera(name)
    kp = UC.kp_rows(*UC.edge_positions().T)
    want = vo.undistort(UR.vo_camera(cam), xy_of(kp)).astype(np.float32)
    got = binding.undistort_host(cam, kp)
    same_bits(name, xy_of(got), want)
    for f in ("size", "angle", "response", "octave"):
        assert got[f].tobytes() == kp[f].tobytes(), f
    if name == "Z":
        assert got.tobytes() == kp.tobytes()
    else:
        assert np.abs(xy_of(got) - xy_of(kp)).max() > (0.3 if name == "T" else 5.0)
    # out aliasing kp
    alias = kp.copy()
    assert binding.undistort_host(cam, alias, in_place=True) is alias
    assert alias.tobytes() == got.tobytes()
    assert len(binding.undistort_host(cam, kp[:0])) == 0


def test_the_corner_shift_of_the_tracker_test_camera():
    """tests/test_track.py's camera at a 640 x 480 corner: tens of pixels, far beyond any search window"""
    cam = binding.Camera(fx=520.0, fy=515.0, cx=318.0, cy=242.0, k1=-0.28, k2=0.07, p1=1e-3, p2=-5e-4, width=640, height=480)
    un = binding.undistort_host(cam, UC.kp_rows([640.0], [480.0]))
    shift = float(np.hypot(un["x"][0] - 640.0, un["y"][0] - 480.0))
    print("corner shift", shift)
    assert shift > 50.0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("undistort") / "libtrack_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests/native/track_shim.cpp"),
                           os.path.join(ROOT, "send-slam_amd/csrc/ss_track.cpp")])
    return C.CDLL(so)


@pytest.mark.parametrize("name", CAMERAS)
def test_host_twin_equals_the_tracker(shim, name):
    """ss_track keeps sst_undistort: its doubles, rounded once, are the twin's floats"""
    cam = UC.camera(name)
    rng = np.random.default_rng(11)
    xy = np.concatenate([UC.edge_positions(), rng.uniform([-5, -5], [UC.W + 5, UC.H + 5], (400, 2)).astype(np.float32)])
    xy = np.ascontiguousarray(xy, np.float32)
    k = np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.p1, cam.p2], np.float64)
    out = np.zeros((len(xy), 2))
    shim.shim_undistort(k.ctypes.data_as(C.c_void_p), len(xy), xy.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    got = binding.undistort_host(cam, UC.kp_rows(xy[:, 0], xy[:, 1]))
    same_bits(name, xy_of(got), out.astype(np.float32))


@pytest.mark.parametrize("name", CAMERAS)
def test_non_finite_rows_go_through_the_same_operations(name):
    cam = UC.camera(name)
    kp = UC.kp_rows(*UC.nonfinite_positions().T)
    got = xy_of(binding.undistort_host(cam, kp))
    want = UR.undistort(cam, xy_of(kp))
    assert np.array_equal(got, want, equal_nan=True), (got, want)


@pytest.mark.parametrize("name", ["D", "P", "T"])
def test_the_denominator_stays_positive_over_the_whole_image(name):
    """so cv::undistortPoints' icdist < 0 bail-out, which the rule lacks, cannot matter"""
    low = UR.min_denominator(UC.camera(name), UC.W, UC.H)
    print(name, "smallest denominator", low)
    assert low > 0.5
    if name == "D":
        assert 0.79 < low < 0.80  # 0.796, as measured


def test_camera_d_moves_a_fifth_of_the_image_outside():
    xs, ys = np.meshgrid(np.arange(0, UC.W, 4, dtype=np.float32), np.arange(0, UC.H, 4, dtype=np.float32))
    un = UR.undistort(UC.camera("D"), np.stack([xs.ravel(), ys.ravel()], axis=1))
    outside = (un[:, 0] < 0) | (un[:, 0] >= UC.W) | (un[:, 1] < 0) | (un[:, 1] >= UC.H)
    print("outside", outside.mean())
    assert 0.18 < outside.mean() < 0.24


@pytest.mark.parametrize("name", CAMERAS)
def test_bounds(name):
    cam = UC.camera(name)
    got = binding.undistort_bounds_host(cam)
    want = UR.bounds(cam, UC.W, UC.H)
    print(name, got)
    assert got.tobytes() == want.tobytes(), (got, want)
    if name == "Z":
        assert got.tolist() == [0.0, float(UC.W), 0.0, float(UC.H)]
    if name in UC.MEASURED_BOUNDS:
        assert np.abs(got - np.array(UC.MEASURED_BOUNDS[name], np.float32)).max() < 0.006
    # a non-square sensor: width and height are the camera's
    wide = UC.camera(name, width=400, height=200)
    assert binding.undistort_bounds_host(wide).tobytes() == UR.bounds(wide, 400, 200).tobytes()


def test_set_bounds_lets_a_point_of_the_undistorted_margin_into_view():
    cam = UC.camera("D")
    view = binding.proj_view(cam, np.eye(3), np.zeros(3), bf=26.0)
    before = bytes(view)
    max_x = float(binding.undistort_bounds_host(cam)[1])
    u = 340.0
    assert UC.W < u < max_x
    # a point at depth 1 that projects to (u, cy + 10), seen head-on, inside its distance range
    x, y = (u - UC.CX) / UC.FX, 10.0 / UC.FY
    d = float(np.sqrt(x * x + y * y + 1.0))
    pt = np.zeros(1, binding.MAP_POINT_DTYPE)
    pt["x"], pt["y"], pt["z"], pt["nx"], pt["ny"], pt["nz"], pt["min_dist"], pt["max_dist"] = x, y, 1.0, x / d, y / d, 1.0 / d, 0.5, 2.0
    params, scale = binding.proj_params(), np.array([1.2 ** k for k in range(8)], np.float32)
    ref_view = P.view_init(cam.fx, cam.fy, cam.cx, cam.cy, UC.W, UC.H, np.eye(3), np.zeros(3), 26.0)
    assert bytes(view) == ref_view.tobytes()
    assert binding.proj_points_host(view, params, scale, pt)["state"][0] == 2
    assert P.eval_point(ref_view, pt[0], 0.5, 1.0, 0.0, scale)["state"] == 2
    assert binding.proj_view_set_bounds(view, cam) is view
    after = bytes(view)
    assert after[:-16] == before[:-16] and after[-16:] == UR.bounds(cam, UC.W, UC.H).tobytes()
    ref_view["min_x"], ref_view["max_x"], ref_view["min_y"], ref_view["max_y"] = UR.bounds(cam, UC.W, UC.H)
    got, want = binding.proj_points_host(view, params, scale, pt), P.eval_point(ref_view, pt[0], 0.5, 1.0, 0.0, scale)
    assert got["state"][0] == 0 and want["state"] == 0
    assert got[0].tobytes() == want.tobytes()
    assert abs(float(got["u"][0]) - u) < 1e-3
    # a view that came from ss_fuse_view_sim3: the same four fields, nothing else
    sim = binding.fuse_view_sim3(cam, 2.0 * np.eye(3), np.array([0.2, 0.0, 0.4]), bf=26.0)
    sim_before = bytes(sim)
    binding.proj_view_set_bounds(sim, cam)
    assert bytes(sim)[:-16] == sim_before[:-16] and bytes(sim)[-16:] == after[-16:]
    # ... and views from ss_sim3_to_view and ss_sim3_to_view21
    res = np.zeros((), binding.SIM3_RESULT_DTYPE)
    res["sr12"], res["t12"], res["s12"] = (1.5 * np.eye(3)).ravel(), (0.1, 0.0, 0.2), 1.5
    res["sr21"], res["t21"] = (np.eye(3) / 1.5).ravel(), (-0.1 / 1.5, 0.0, -0.2 / 1.5)
    for make in (binding.sim3_to_view, binding.sim3_to_view21):
        v = make(cam, res, np.eye(3), np.zeros(3), bf=26.0)[0]
        v_before = bytes(v)
        assert v_before[-16:] == before[-16:]  # 0 .. width, 0 .. height
        binding.proj_view_set_bounds(v, cam)
        assert bytes(v)[:-16] == v_before[:-16] and bytes(v)[-16:] == after[-16:]
    # the zero camera leaves ss_proj_view_init's bounds as they are
    zero = binding.proj_view(UC.camera("Z"), np.eye(3), np.zeros(3))
    zero_before = bytes(zero)
    binding.proj_view_set_bounds(zero, UC.camera("Z"))
    assert bytes(zero) == zero_before


@pytest.mark.parametrize("over", [dict(width=0), dict(height=-1), dict(fx=float("nan")), dict(cy=float("inf")), dict(k2=float("nan")), dict(p1=float("-inf")),
                                  dict(fy=0.0)], ids=lambda o: next(iter(o)))
def test_bounds_refuse_invalid_cameras(over):
    cam = UC.camera("D", **over)
    with pytest.raises(binding.OrbError) as e:
        binding.undistort_bounds_host(cam)
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    view = binding.proj_view(UC.camera("D"), np.eye(3), np.zeros(3))
    before = bytes(view)
    with pytest.raises(binding.OrbError) as e:
        binding.proj_view_set_bounds(view, cam)
    assert e.value.code == binding.SS_ERR_INVALID_ARG and bytes(view) == before


def test_undistort_host_refuses_a_focal_length_that_does_not_divide():
    kp = UC.kp_rows([1.0], [2.0])
    for over in (dict(fx=0.0), dict(fy=float("nan")), dict(fx=float("inf"))):
        with pytest.raises(binding.OrbError) as e:
            binding.undistort_host(UC.camera("D", **over), kp)
        assert e.value.code == binding.SS_ERR_INVALID_ARG
    lib = binding.load()
    assert lib.ss_undistort_host(None, kp.ctypes.data, 1, kp.ctypes.data) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_undistort_host(C.byref(UC.camera("D")), kp.ctypes.data, -1, kp.ctypes.data) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_undistort_host(C.byref(UC.camera("D")), None, 1, kp.ctypes.data) == binding.SS_ERR_INVALID_ARG


# ---- depth ----
def _depth_case(kind, factor, bf=26.0, close=3.0):
    img, kp = UC.depth_frames(kind)[0], UC.depth_kp()[0]
    un = binding.undistort_host(UC.camera("D", width=UC.DEPTH_W, height=UC.DEPTH_H), kp)
    p = binding.depth_params(bf, factor, close, 1 if kind == "u16" else 0)
    got = binding.depth_host(p, img, kp, un, width=UC.DEPTH_W)
    want = UR.depth(bf, factor, close, img, UC.DEPTH_W, xy_of(kp), un["x"])
    return got, want, kp, img


@pytest.mark.parametrize("kind,factor", [("u16", 5000.0), ("f32", 1.0), ("f32", 1.0 + 5e-6), ("f32", 0.0), ("u16", 0.0), ("f32", 0.5), ("u16", -1000.0),
                                         ("f32", 9e-6)])
def test_depth_host_rule(kind, factor):
    (right, depth, summary), (w_right, w_depth, w_summary), kp, img = _depth_case(kind, factor)
    same_bits("depth", depth, w_depth)
    same_bits("right", right, w_right)
    assert {f: int(summary[f]) for f in UR.SUMMARY_FIELDS} == dict(w_summary, status=0)
    print(kind, factor, w_summary)
    if factor >= 0:
        assert 0 < w_summary["n_depth"] < len(kp) and (kind == "u16" and factor == 0.0 or 0 < w_summary["n_close"] < w_summary["n_depth"])
    else:
        assert w_summary["n_depth"] == 0  # every sample negative
    if kind == "f32" and factor in (1.0, 1.0 + 5e-6, 0.0, 9e-6):  # no multiply: the samples themselves
        live = depth > 0
        cols, rows = kp["x"][live].astype(np.int64), kp["y"][live].astype(np.int64)
        assert depth[live].tobytes() == img[rows, cols].tobytes()
    assert (right[depth <= 0] == -1).all() and (depth[~(depth > 0)] == -1).all()


def test_depth_takes_the_truncated_raw_pixel_and_the_undistorted_x():
    img = np.arange(1, 1 + UC.DEPTH_W * UC.DEPTH_H, dtype=np.float32).reshape(UC.DEPTH_H, UC.DEPTH_W)
    raw = UC.kp_rows([10.75, 0.0, -0.5, UC.DEPTH_W - 0.01, UC.DEPTH_W, 5.0, np.nan], [20.5, 0.0, 4.0, 3.0, 3.0, -1.0, 2.0])
    un = raw.copy()
    un["x"] += np.float32(1000.0)
    p = binding.depth_params(bf=8.0, depth_map_factor=1.0, close_limit=100.0)
    right, depth, summary = binding.depth_host(p, img, raw, un)
    # (10.75, 20.5) reads pixel (10, 20), not the rounded (11, 21)
    assert depth[0] == img[20, 10] != img[21, 11]
    assert depth[1] == img[0, 0] and depth[2] == img[4, 0] and depth[3] == img[3, UC.DEPTH_W - 1]
    assert (depth[4:] == -1).all() and (right[4:] == -1).all()
    for i in range(4):
        assert right[i] == np.float32(un["x"][i] - np.float32(np.float32(8.0) / depth[i]))
    assert (int(summary["n_kp"]), int(summary["n_depth"]), int(summary["n_close"])) == (7, 4, int((depth[:4] < 100).sum()))
    # kp_un NULL: the raw keypoints serve as both
    right2, depth2, _ = binding.depth_host(p, img, raw)
    assert depth2.tobytes() == depth.tobytes() and right2[0] == np.float32(raw["x"][0] - np.float32(np.float32(8.0) / depth[0]))


def test_depth_host_refusals_and_the_calibration_helper():
    img = np.ones((4, 4), np.float32)
    kp = UC.kp_rows([1.0], [1.0])
    for bad in (dict(depth_type=2), dict(bf=float("nan")), dict(depth_map_factor=float("inf"))):
        with pytest.raises(binding.OrbError) as e:
            binding.depth_host(binding.depth_params(**dict(dict(bf=1.0), **bad)), img, kp)
        assert e.value.code == binding.SS_ERR_INVALID_ARG
    with pytest.raises(binding.OrbError):  # a width the rows do not hold
        binding.depth_host(binding.depth_params(1.0), img, kp, width=5)
    cam = UC.camera("D")
    p = binding.depth_params_from_camera(cam, 1)
    assert p.bf == np.float32(cam.baseline * cam.fx) and p.depth_map_factor == np.float32(5000.0) and p.depth_type == 1
    assert p.close_limit == np.float32(cam.baseline * cam.fx * cam.th_depth / cam.fx)
    with pytest.raises(binding.OrbError):
        binding.depth_params_from_camera(cam, 3)


# ---- the header and the build ----
def test_header_constants_and_abi():
    lib = binding.load()
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    assert re.search(r"#define SS_ABI_VERSION 5\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\(", code), name
        assert name in binding.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(binding.DepthParams) == 16 and binding.DEPTH_SUMMARY_DTYPE.itemsize == 16
    assert [n for n, _ in binding.DepthParams._fields_] == ["bf", "depth_map_factor", "close_limit", "depth_type"]
    assert binding.DEPTH_SUMMARY_DTYPE.names == UR.SUMMARY_FIELDS
    assert C.sizeof(binding.ProjView) == 96 and binding.KP_DTYPE.itemsize == 24


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/undistort_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "undistort_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "undistort_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
