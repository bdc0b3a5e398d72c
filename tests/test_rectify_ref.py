"""CPU tests of the rectification rule as tests/rectify_ref.py states it, of the host map builder of the library against it
(ss_rectify_build_map needs no device), and of the C ABI surface: declared / exported / bound symbols, struct layout."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import rectify_ref as R
import stereo_ref
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")


def _random(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=shape, dtype=np.uint8)


def _shift_maps(w, h, dx, dy):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return x + np.float32(dx), y + np.float32(dy)


def test_identity_model_maps_every_pixel_to_itself():
    w, h = 53, 37
    mx, my = R.build_map(R.identity(w, h))
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    assert np.array_equal(mx, x.astype(np.float32)) and np.array_equal(my, y.astype(np.float32))
    for shape in ((h, w), (h, w, 3)):
        src = _random(shape, 1)
        assert np.array_equal(R.remap(src, mx, my), src)


def test_integer_shift_and_half_pixel_shift():
    w, h = 40, 30
    src = _random((h, w), 2)
    out = R.remap(src, *_shift_maps(w, h, 3, -2))  # dst(y, x) = src(y - 2, x + 3)
    want = np.zeros_like(src)
    want[2:, :w - 3] = src[:h - 2, 3:]
    assert np.array_equal(out, want)
    out = R.remap(src, *_shift_maps(w, h, 0.5, 0))
    p = src.astype(np.int32)
    q = np.concatenate([p[:, 1:], np.zeros((h, 1), np.int32)], axis=1)  # the neighbour past the right edge is the border, 0
    assert np.array_equal(out, ((p + q + 1) >> 1).astype(np.uint8))


def test_weights_sum_to_32768():
    a, b = np.meshgrid(np.arange(32), np.arange(32))
    assert (sum(R.weights(a, b)) == 32768).all() and a.size == 1024
    assert (R.WTAB.sum(axis=2) == 32768).all() and R.WTAB.min() >= 0


def test_fixed_point_conversion_on_crafted_values():
    w = 320

    def one(v):
        i, f = R.to_fixed(np.array([v], np.float32))
        return int(i[0]), int(f[0])

    # ties: k + 1/64 is 32 k + 0.5 -> the even neighbour, 32 k; k + 3/64 is 32 k + 1.5 -> 32 k + 2
    assert one(7 + 1 / 64) == (7, 0) and one(7 + 3 / 64) == (7, 2) and one(8 + 1 / 64) == (8, 0)
    assert one(-7 - 1 / 64) == (-7, 0) and one(-7 - 3 / 64) == (-8, 30)
    assert one(-1.0) == (-1, 0) and one(-1 / 32) == (-1, 31) and one(-1 + 1 / 32) == (-1, 1)
    assert one(w - 1) == (w - 1, 0) and one(w) == (w, 0) and one(w - 1 + 1 / 64) == (w - 1, 0)
    assert one(40000.0) == (32767, 0)  # s = 1 280 000 fits, the integer part saturates
    for v in (1e30, -1e30, np.inf, -np.inf, np.nan):
        assert one(v) == (-32768, 0), v  # INT32_MIN >> 5 clamped, INT32_MIN & 31
    assert one(-0.0) == (0, 0) and one(0.0) == (0, 0)
    # t just inside int32 on both sides (67108860 is the last float32 below 2^26), and 2^26 itself, whose t = 2^31 is outside
    assert one(67108860.0) == (32767, 0) and one(-67108864.0) == (-32768, 0) and one(67108864.0) == (-32768, 0)


MODELS = {"A": R.model_a, "identity": lambda: R.identity(320, 240), "k3": R.model_k3}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_library_builder_equals_the_reference_bit_for_bit(name):
    m = MODELS[name]()
    mx, my = R.build_map(m)
    gx, gy = binding.rectify_build_map(binding.rectify_model(**m))
    assert gx.shape == mx.shape == (m["height"], m["width"])
    for tag, got, want in (("map_x", gx, mx), ("map_y", gy, my)):
        bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert len(bad) == 0, f"{name} {tag}: {len(bad)} values differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}"
    if name == "k3":  # every coefficient is in play
        assert all(m[k] != 0 for k in ("k1", "k2", "p1", "p2", "k3")) and np.count_nonzero(np.abs(m["R"]) < 1e-6) == 0


def test_library_builder_rejects_a_singular_camera():
    m = R.model_a()
    m["fx_new"] = 0.0
    assert R.build_map(m) is None
    with pytest.raises(binding.OrbError) as e:
        binding.rectify_build_map(binding.rectify_model(**m))
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    m = R.model_a()
    m["R"] = np.full((3, 3), np.nan)
    assert R.build_map(m) is None
    with pytest.raises(binding.OrbError) as e:
        binding.rectify_build_map(binding.rectify_model(**m))
    assert e.value.code == binding.SS_ERR_INVALID_ARG


def test_the_running_sum_is_not_the_product_form():
    """the builder's _x += ir[0] along a row differs in the last bits from j * ir[0] + base: the rule is the running sum"""
    m = R.model_a()
    ir = R.inverse_new_camera(m)
    j = np.arange(m["width"], dtype=np.float64)
    base = 100.0 * ir[1] + ir[2]
    run = np.cumsum(np.concatenate([[base], np.full(m["width"] - 1, ir[0])]))
    assert np.count_nonzero(run != j * ir[0] + base) > 0


def test_model_a_exercises_every_branch():
    """no vacuous pass on the GPU: asserted on the reference"""
    mx, my = R.build_map(R.model_a())
    _, a = R.to_fixed(mx)
    _, b = R.to_fixed(my)
    cls = R.tap_classes(mx, my)
    pairs = len(set((a * 32 + b).ravel().tolist()))
    inside, outside, partial = (cls == 4).mean(), (cls == 0).mean(), int(((cls > 0) & (cls < 4)).sum())
    print(f"model A: {pairs} (a, b) pairs, {100 * inside:.1f} % inside, {100 * outside:.1f} % outside, {partial} partial")
    assert pairs >= 1000 and partial >= 500 and outside >= 0.05 and inside >= 0.5


@pytest.mark.parametrize("name,shape", [("A", (240, 320)), ("E", (240, 320)), ("k3", (240, 320)), ("A_small", (61, 97, 3))])
def test_closed_and_literal_forms_agree(name, shape):
    m = {"A": R.model_a, "E": R.model_e, "k3": R.model_k3, "A_small": lambda: R.scaled(R.model_a(), 97, 61)}[name]()
    mx, my = R.build_map(m)
    src = _random(shape, 11)
    lit, branches = R.remap_literal(src, mx, my)
    assert np.array_equal(R.remap(src, mx, my), lit)
    cls = R.tap_classes(mx, my)
    assert branches == [int((cls == 4).sum()), int((cls == 0).sum()), int(((cls > 0) & (cls < 4)).sum())]
    if name.startswith("A"):
        assert min(branches) > 0, branches


def test_closed_and_literal_forms_agree_on_crafted_edges():
    w, h = 24, 16
    mx, my = _shift_maps(w, h, 0, 0)
    vals = np.array([-1, -1 + 1 / 32, w - 1, w - 1 + 1 / 64, w, np.nan, np.inf, -np.inf, 1e30, -1e30, 40000], np.float32)
    mx[0, :len(vals)] = vals
    mx[h - 1, :len(vals)] = vals
    my[:len(vals), 0] = np.where(vals == w - 1, h - 1, np.where(vals == w, h, vals)).astype(np.float32)
    my[:len(vals), w - 1] = my[:len(vals), 0]
    src = _random((h, w), 5) | 1
    lit, branches = R.remap_literal(src, mx, my)
    assert np.array_equal(R.remap(src, mx, my), lit) and min(branches) > 0


def test_tile_boxes_on_crafted_maps():
    """the box rule on maps whose boxes are known by hand"""
    w, h = 256, 16
    ident = R.identity_map(w, h)
    # identity, gray: a tile reads its own 128 columns and 8 rows; a = b = 0, so the taps right and below weigh nothing
    assert R.tile_boxes(*ident, 1).tolist() == [[128 * 8, 128 * 8], [128 * 8, 128 * 8]]
    assert R.tile_boxes(*ident, 3).tolist() == [[384 * 8, 384 * 8]] * 2
    # half a pixel to the right: the second tap column counts, except past the right edge; the range grows to the next 16
    mx, my = _shift_maps(w, h, 0.5, 0)
    assert R.tile_boxes(mx, my, 1).tolist() == [[144 * 8, 128 * 8], [144 * 8, 128 * 8]]
    # 3 columns to the right and a quarter down, 4 channels: bytes 12 .. 524 -> 0 .. 528 and 524 .. 1024 -> 512 .. 1024, 9 rows
    # (8 in the last tile row, whose lower taps are outside)
    mx, my = _shift_maps(w, h, 3, 0.25)
    assert R.tile_boxes(mx, my, 4).tolist() == [[528 * 9, 512 * 9], [528 * 8, 512 * 8]]
    # everything outside: empty
    assert R.tile_boxes(*_shift_maps(w, h, w, 0), 1).tolist() == [[0, 0], [0, 0]]
    assert R.box_classes(np.array([[0, 1, 8192], [8193, 10240, 10241]])) == [1, 2, 2, 1]


ROTATED = [(640, 484, 45, 1), (336, 61, 8, 3), (336, 61, 8, 4)]


@pytest.mark.parametrize("w,h,degrees,ch", ROTATED)
def test_rotated_maps_reach_every_form_of_the_staging(w, h, degrees, ch):
    """no vacuous pass on the GPU: the rotated maps of tests/test_rectify.py have tiles without a weighted tap, tiles whose box
    fits two 16-byte chunks per lane, tiles that need the third (8193 - 10240 B) and tiles that fall back to the gather
    loop, in one launch; every map of the suite before them stayed at or below 6144 B"""
    got = R.box_classes(R.tile_boxes(*R.rotation_map(w, h, degrees), ch))
    print(w, h, degrees, ch, dict(zip(R.BOX_CLASSES, got)))
    assert min(got) >= 1, got
    assert (w * ch) % 16 == 0 and h % R.TILE_H != 0 and (ch == 1 or w % R.TILE_W != 0)
    assert got == {1: [22, 71, 19, 193], 3: [1, 12, 2, 9], 4: [1, 10, 2, 11]}[ch]
    for name, m, c in (("A_hd", R.scaled(R.model_a(), 1280, 720, focal=4.0), 1), ("E", R.model_e(), 1), ("E", R.model_e(), 3)):
        if ch == 1:
            assert 0 < R.tile_boxes(*R.build_map(m), c).max() <= 6144, name


def test_end_to_end_input_stays_meaningful(oracle):
    """the raw pair the GPU chain test rectifies: after the remap the reference still finds depth on it"""
    left, right = R.end_to_end_pair()
    mx, my = R.build_map(R.model_e())
    rl, rr = R.remap(left, mx, my), R.remap(right, mx, my)
    assert not np.array_equal(rl, left)
    p = oracle.default_params(n_features=500, lapping_x0=0, lapping_x1=0)
    st = Counter()
    kL, dL, kR, dR, pts, summ = stereo_ref.stereo_pair(rl, rr, p, 500.0, 0.1, 35.0, st)
    print(summ, dict(st))
    assert summ["n_depth"] >= 0.4 * summ["n_left"] and st["median_cut"] >= 1 and st["guard"] == 0


def test_symbols_are_declared_exported_and_bound(tmp_path):
    names = ["ss_rectify_build_map", "ss_rectify_set_map", "ss_rectify_batch_device", "ss_extract_stereo_raw"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("set_rectify_map", "set_rectify_model", "rectify_batch_device", "extract_stereo_raw"):
        assert callable(getattr(binding.OrbContext, m))
    assert callable(binding.rectify_build_map)
    assert C.sizeof(binding.RectifyModel) == 184 and binding.SS_MAX_RECTIFY_MAPS == 16
    assert tuple(n for n, _ in binding.RectifyModel._fields_) == R.MODEL_FIELDS
    assert binding.RectifyModel.R.offset == 72 and binding.RectifyModel.fx_new.offset == 144 and binding.RectifyModel.height.offset == 180
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_rectify_model) == 184, "model");\n'
                   '_Static_assert(offsetof(ss_rectify_model, fx) == 0 && offsetof(ss_rectify_model, cy) == 24, "intrinsics");\n'
                   '_Static_assert(offsetof(ss_rectify_model, k1) == 32 && offsetof(ss_rectify_model, k3) == 64, "distortion");\n'
                   '_Static_assert(offsetof(ss_rectify_model, R) == 72 && offsetof(ss_rectify_model, fx_new) == 144, "rotation");\n'
                   '_Static_assert(offsetof(ss_rectify_model, cy_new) == 168 && offsetof(ss_rectify_model, width) == 176, "new camera");\n'
                   '_Static_assert(offsetof(ss_rectify_model, height) == 180, "size");\n'
                   '_Static_assert(SS_MAX_RECTIFY_MAPS == 16 && SS_MAX_RECTIFY_MAPS == 2 * SS_MAX_CAMERAS && SS_ABI_VERSION == 5, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5
