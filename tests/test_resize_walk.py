"""k_resize_walk: a wave walks a band of 32 destination rows, 64 lanes x four destination columns, the sums of the last two
source rows in registers; a lane's four columns come out of one 12-byte load per source row.

Every GPU case compares EVERY level of every frame it looks at with oracle.pyramid, byte for byte, through
ctx.debug_fetch(0, frame, level, (h, w)), and asserts which kernel built each level and where level 0 was read through
ctx.debug_fetch(5, ...) (two int32 per level: the kernel the last batch launched for it -- 1 k_resize, 2 / 5 k_resize_walk with
bands of 32 / 16 rows, 4 k_resize_lds -- and whether level 0 was read in place), against the rules restated here: the window
rule from the tap tables (_walk_fits: the four columns of every lane within 7 bytes of the first, rows advancing
monotonically) and the launch-size rule (_expected_kernels: bands of 32 rows where the launch's waves fill the chip's wave
slots, 32 per compute unit, else bands of 16 where those do, else the tile form).  The library chooses by the launch's size
alone, so every case runs a batch large enough that ALL its levels take k_resize_walk and level 1 takes the bands of 32 rows
(_batch_size: a few hundred to a few thousand small frames, the case's distinct frames repeated); the first frames and the last
one are compared.

What the shapes are for (test_shapes_are_what_they_claim asserts it on the CPU):
  widths   level widths of 4k + 1 .. 4k + 3; of exactly 256 (one full wave), 257 .. 260 (a second wave with ONE live lane, its
           dword partly or wholly inside the width) and 1025 (five waves across, the last with one live lane); pyramids that end
           in a level 67 or 68 wide.  The ABI accepts no level below 67 x 67 (a 35-px cell inside 16-px borders), so a level
           narrower than one wave's 64 lanes x 4 columns exists in every case, one narrower than 64 px in none.
  heights  the same limit rules out a level of fewer rows than one band; level heights of 95, 96 and 97 (a band multiple - 1,
           + 0, + 1: a last band of 31, 32 rows and of a single row), 79 .. 81 (a last band of half a band's rows) and 67, 68
           (two bands + 3, + 4).
  scales   1.1, 1.2, 1.25, 1.5 and 2.0 advance one or two source rows per destination row and spread a lane's columns up to the
           window's limit (k = 6 at 2.0); 3.0 spreads them over 10 bytes, fails the window rule and must take k_resize; 1.004
           rounds a level to its parent's size: the last row's taps are clipped at the bottom (s1 == s0) and the last columns'
           second tap is past the width with weight 0.
  level 0  in place with pitch == w (a multiple of 16: the last lane's window crosses the pitch, and the last row of the last
           frame ends where the buffer's contents do), with a larger pitch, copied (SENDSLAM_FORCE_INGEST=1, and a width that
           is no multiple of 16), colour input, frames a frame stride apart that is larger than the frame.
  padding  the same in-place batch with the bytes between w and the pitch 0x00 and then 0xFF: all levels identical, the only
           practical check that no result depends on bytes outside [0, w).
"""
import functools

import numpy as np
import pytest

import patterns

BAND = 32
MAX_LEVELS = 8


def _params(oracle, w, h, scale):
    """the deepest pyramid (<= 8 levels) the geometry accepts for this image: every level at least 67 x 67"""
    best = None
    for n in range(1, MAX_LEVELS + 1):
        p = oracle.default_params(n_features=300, scale_factor=scale, n_levels=n)
        try:
            oracle.geometry(p, w, h)
        except ValueError:
            break
        best = n
    assert best is not None and best >= 2, (w, h, scale)
    return dict(n_features=300, scale_factor=scale, n_levels=best)


def _dims(oracle, w, h, scale):
    kw = _params(oracle, w, h, scale)
    g = oracle.geometry(oracle.default_params(**kw), w, h)
    return [(g.w[l], g.h[l]) for l in range(g.n_levels)]


def _axis(dn, sn, is_x):
    """cv::resize's INTER_LINEAR taps of the 8-bit path (s0, s1, a1 != 0) per destination index"""
    scale = 1.0 / (dn / sn)
    out = []
    for d in range(dn):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if is_x:
            if s < 0:
                f, s = np.float32(0), 0
            if s >= sn - 1:
                f, s = np.float32(0), sn - 1
            s0, s1 = s, min(s + 1, sn - 1)
        else:
            s0, s1 = min(max(s, 0), sn - 1), min(max(s + 1, 0), sn - 1)
        out.append((s0, s1, int(np.rint(f * np.float32(2048))) != 0))
    return out


def _walk_fits(src, dst):
    (sw, sh), (dw, dh) = src, dst
    ys = _axis(dh, sh, False)
    for y, (s0, s1, _) in enumerate(ys):
        if not (s0 <= s1 <= s0 + 1):
            return False
        if y and (s0 < ys[y - 1][0] or s1 < ys[y - 1][1]):
            return False
    xs = _axis(dw, sw, True)
    xs += [xs[-1]] * 3  # the table is padded with its last entry
    for c in range(0, dw, 4):
        for s0, s1, a1 in xs[c:c + 4]:
            if not (0 <= s0 - xs[c][0] <= 6) or (a1 and s1 != s0 + 1):
                return False
    return True


def _wave_slots():
    import torch
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def _waves(dim, band):
    return (dim[0] + 255) // 256 * ((dim[1] + band - 1) // band)


def _batch_size(dims, slots):
    """frames for which every level's launch fills the wave slots with bands of 16 rows, and level 1's with bands of 32"""
    n = max(-(-slots // min(_waves(d, 16) for d in dims[1:])), -(-slots // _waves(dims[1], 32)))
    assert n <= 4096  # max_batch
    return n


def _expected_kernels(dims, n_frames=0, slots=0):
    """per level: 0 level 0, 1 k_resize, 2 / 5 k_resize_walk with bands of 32 / 16 rows, 4 k_resize_lds.  n_frames == 0: 2 for
    every level the window rule admits"""
    out = [0]
    for l in range(1, len(dims)):
        fits = _walk_fits(dims[l - 1], dims[l])
        if fits and (n_frames == 0 or _waves(dims[l], 32) * n_frames >= slots):
            out.append(2)
        elif fits and _waves(dims[l], 16) * n_frames >= slots:
            out.append(5)
        else:  # the tile form where its 112-byte x 80-row window holds the tile's source
            sx = np.float32(dims[l - 1][0]) / np.float32(dims[l][0])
            sy = np.float32(dims[l - 1][1]) / np.float32(dims[l][1])
            out.append(4 if np.float32(64) * sx + np.float32(18) <= 112 and np.float32(64) * sy + np.float32(3) <= 80 else 1)
    return out


def _bottom_clipped(src_h, dst_h):
    return [y for y, (s0, s1, _) in enumerate(_axis(dst_h, src_h, False)) if s0 == s1]


@functools.lru_cache(maxsize=None)
def _noise(w, h, seed=0):
    return patterns.noise(w, h, 7000 * w + h + seed)


_REF = {}


def _reference(oracle, img, kw):
    """oracle.pyramid(img), computed once per (image, parameters) and never written to"""
    key = (img.shape, img.tobytes(), tuple(sorted(kw.items())))
    if key not in _REF:
        levels = oracle.pyramid(img, oracle.default_params(**kw))
        for lv in levels:
            lv.setflags(write=False)
        _REF[key] = levels
    return _REF[key]


def _check_levels(oracle, ctx, frame, img, kw, what, level0_from_device=False):
    """every level of `frame` against the oracle's pyramid of img (or, where level 0 is the library's own gray conversion, of
    the level 0 it holds); returns the levels"""
    h, w = img.shape[:2]
    if level0_from_device:
        img = ctx.debug_fetch(0, frame, 0, (h, w)).reshape(h, w).copy()
    want = _reference(oracle, img, kw)
    got = []
    for l, ref in enumerate(want):
        lv = ctx.debug_fetch(0, frame, l, ref.shape).reshape(ref.shape)
        bad = np.argwhere(lv != ref)
        assert bad.size == 0, f"{what}: frame {frame} level {l} ({ref.shape[1]}x{ref.shape[0]}): {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}"
        got.append(lv)
    return got


def _check_kernels(oracle, ctx, w, h, scale, n_frames, in_place, what):
    dims = _dims(oracle, w, h, scale)
    got = [ctx.debug_fetch(5, 0, l, (2,), np.int32) for l in range(len(dims))]
    ran = [int(g[0]) for g in got]
    assert ran == _expected_kernels(dims, n_frames, _wave_slots()), f"{what}: kernels per level {ran}"
    assert all(int(g[1]) == int(in_place) for g in got), f"{what}: level 0 in place: {got[0][1]}, expected {in_place}"
    return ran


def _device(frames, n, pitch, rows_per_frame=None, fill=0x5A):
    """n frames (frames[b % len(frames)]) in a device buffer of rows `pitch` bytes and frames `rows_per_frame` rows apart, the
    other bytes `fill`; the buffer's contents end with the last row of the last frame"""
    import torch
    k, h, w = frames.shape
    rows = h if rows_per_frame is None else rows_per_frame
    buf = np.full((n, rows, pitch), fill, np.uint8)
    buf[:, :h, :w] = frames[np.arange(n) % k]
    flat = buf.reshape(-1)[:((n - 1) * rows + h) * pitch]
    return torch.from_numpy(np.ascontiguousarray(flat)).to(torch.device("cuda:0"))


def _run_gray(oracle, frames, scale, pitch, what, rows_per_frame=None, fill=0x5A, in_place=True, walk_everywhere=True):
    """the distinct `frames` repeated to a batch that fills the chip; returns the levels of the first len(frames) frames and of
    the last one"""
    from send_slam_amd import binding
    k, h, w = frames.shape
    kw = _params(oracle, w, h, scale)
    rows = h if rows_per_frame is None else rows_per_frame
    n = _batch_size(_dims(oracle, w, h, scale), _wave_slots())
    d = _device(frames, n, pitch, rows_per_frame, fill)
    out = []
    with binding.OrbContext(0, max_batch=n, **kw) as ctx:
        ctx.extract_batch_device(d.data_ptr(), n, w, h, row_stride=pitch, frame_stride=pitch * rows)
        ctx.synchronize()
        ran = _check_kernels(oracle, ctx, w, h, scale, n, in_place, what)
        if walk_everywhere:
            assert ran[1] == 2 and all(r in (2, 5) for r in ran[1:]), f"{what}: kernels per level {ran}"
        for b in list(range(k)) + [n - 1]:
            out.append(_check_levels(oracle, ctx, b, frames[b % k], kw, what, level0_from_device=not in_place))
            if not in_place:
                assert np.array_equal(out[-1][0], frames[b % k]), f"{what}: level 0 of frame {b} is not the input"
    return out


# (image w, image h, scale factor): what the case is there for is asserted in test_shapes_are_what_they_claim
WIDTHS = [(131, 98, 1.2), (239, 241, 1.2), (307, 81, 1.2), (308, 81, 1.2), (310, 97, 1.2), (311, 82, 1.2), (312, 81, 1.2), (1230, 81, 1.2)]
HEIGHTS = [(150, 114, 1.2), (150, 115, 1.2), (150, 116, 1.2), (150, 95, 1.2), (150, 96, 1.2), (150, 97, 1.2), (120, 81, 1.2)]
SCALES = [(173, 131, 1.1), (190, 157, 1.25), (257, 211, 1.5), (268, 270, 2.0), (536, 278, 2.0), (100, 100, 1.004)]
TOO_WIDE = (243, 210, 3.0)
IN_PLACE = [(240, 98, 240), (240, 98, 256), (304, 131, 304), (131, 98, 144), (131, 98, 192)]  # (w, h, pitch)


def test_shapes_are_what_they_claim(oracle):
    """CPU: the level sizes, kernels and table rows the GPU cases are chosen for"""
    lw = {c: [d[0] for d in _dims(oracle, *c)] for c in WIDTHS + HEIGHTS + SCALES}
    lh = {c: [d[1] for d in _dims(oracle, *c)] for c in WIDTHS + HEIGHTS + SCALES}
    assert lw[(307, 81, 1.2)][1] == 256 and lw[(308, 81, 1.2)][1] == 257 and lw[(310, 97, 1.2)][1] == 258
    assert lw[(311, 82, 1.2)][1] == 259 and lw[(312, 81, 1.2)][1] == 260 and lw[(1230, 81, 1.2)][1] == 1025
    assert len(lw[(239, 241, 1.2)]) == 8 and lw[(239, 241, 1.2)][7] == 67
    all_w = [w for c in WIDTHS for w in lw[c][1:]]
    assert {w % 4 for w in all_w} == {0, 1, 2, 3} and min(all_w) < 70
    assert [lh[c][1] for c in HEIGHTS] == [95, 96, 97, 79, 80, 81, 68] and lh[(239, 241, 1.2)][7] == 67
    assert {h % BAND for h in (95, 96, 97, 67)} == {31, 0, 1, 3}
    for c in WIDTHS + HEIGHTS + SCALES:
        assert all(h >= 67 for h in lh[c])  # the ABI's limit: never fewer rows than a band
        ran = _expected_kernels(_dims(oracle, *c))
        assert ran[1:] == [2] * (len(ran) - 1), (c, ran)
    with pytest.raises(ValueError):  # no level below 67 px: the narrowest cases above end at that limit
        oracle.geometry(oracle.default_params(n_features=300, scale_factor=1.2, n_levels=4), 131, 98)
    # scale factor 2: a lane's columns are 0, 2, 4, 6 bytes from its first, every row advances two source rows
    d = _dims(oracle, 268, 270, 2.0)
    assert d[:2] == [(268, 270), (134, 135)]
    xs = _axis(134, 268, True)
    assert max(xs[c + 3][0] - xs[c][0] for c in range(0, 132, 4)) == 6
    ys = _axis(135, 270, False)
    assert {ys[y + 1][1] - ys[y][1] for y in range(134)} == {2}
    ys = _axis(lh[(150, 96, 1.2)][1], 96, False)
    assert {ys[y + 1][1] - ys[y][1] for y in range(len(ys) - 1)} == {1, 2}
    # 3.0: ten bytes per lane, outside the window
    d = _dims(oracle, *TOO_WIDE)
    assert len(d) == 2 and _expected_kernels(d) == [0, 1]
    # 1.004: level 1 as large as level 0, its last row clipped at the bottom, its last column's second tap at the width
    d = _dims(oracle, 100, 100, 1.004)
    assert d[0] == d[1] == (100, 100) and len(d) >= 3 and d[2] != d[1]
    assert _bottom_clipped(100, 100) == [99] and _axis(100, 100, True)[99][:2] == (99, 99)
    for c in WIDTHS + HEIGHTS + SCALES[:-1]:
        dd = _dims(oracle, *c)
        assert all(_bottom_clipped(dd[l - 1][1], dd[l][1]) == [] for l in range(1, len(dd))), c
    assert all(p % 16 == 0 and p >= w for w, _, p in IN_PLACE) and sum(p == w for w, _, p in IN_PLACE) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDTHS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_widths_vs_oracle(oracle, case):
    """level widths around the lane and the wave grain; level 0 copied: none of the widths is a multiple of 16"""
    w, h, scale = case
    assert w % 16
    _run_gray(oracle, _noise(w, h)[None], scale, w, f"{w}x{h}", in_place=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEIGHTS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_heights_vs_oracle(oracle, case):
    w, h, scale = case
    pitch = (w + 15) // 16 * 16
    _run_gray(oracle, _noise(w, h)[None], scale, pitch, f"{w}x{h}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCALES, ids=lambda c: f"{c[0]}x{c[1]}-scale{c[2]}")
def test_scale_factors_vs_oracle(oracle, case):
    w, h, scale = case
    pitch = (w + 15) // 16 * 16
    _run_gray(oracle, np.stack([_noise(w, h), _noise(w, h, 1)]), scale, pitch, f"{w}x{h} at {scale}")


@pytest.mark.gpu
def test_scale_factor_outside_the_window_takes_k_resize(oracle):
    w, h, scale = TOO_WIDE
    pitch = (w + 15) // 16 * 16
    _run_gray(oracle, _noise(w, h)[None], scale, pitch, f"{w}x{h} at {scale}", walk_everywhere=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", IN_PLACE, ids=lambda c: f"{c[0]}x{c[1]}-pitch{c[2]}")
def test_level0_in_place_vs_oracle(oracle, case):
    """two distinct frames; with pitch == w the last lane's 12-byte window crosses the pitch in every row, and the last row of the last
    frame is the end of the buffer's contents"""
    w, h, pitch = case
    _run_gray(oracle, np.stack([_noise(w, h), _noise(w, h, 1)]), 1.2, pitch, f"{w}x{h} in place, pitch {pitch}")


@pytest.mark.gpu
def test_level0_forced_ingest_vs_oracle(oracle, monkeypatch):
    """SENDSLAM_FORCE_INGEST=1 (read at ss_create): the same aligned buffer, level 0 copied into the pyramid block"""
    monkeypatch.setenv("SENDSLAM_FORCE_INGEST", "1")
    w, h = 240, 98
    _run_gray(oracle, np.stack([_noise(w, h), _noise(w, h, 1)]), 1.2, 240, "forced ingest", in_place=False)


@pytest.mark.gpu
def test_colour_input_vs_oracle(oracle):
    """three channels: level 0 is the gray conversion (the oracle's, byte for byte), written into the pyramid block"""
    import torch
    from send_slam_amd import binding
    w, h = 197, 131
    rgb = np.stack([_noise(w, h, s) for s in (2, 3, 4)], axis=-1)
    col = np.ascontiguousarray(np.stack([rgb, rgb[::-1]]))
    kw = _params(oracle, w, h, 1.2)
    cam = binding.Camera(type=b"PinHole", fx=500, fy=500, cx=w / 2, cy=h / 2, width=w, height=h, fps=30, rgb=1,
                         th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
    n = _batch_size(_dims(oracle, w, h, 1.2), _wave_slots())
    d = torch.from_numpy(col[np.arange(n) % 2]).to(torch.device("cuda:0"))
    with binding.OrbContext(0, max_batch=n, **kw) as ctx:
        ctx.set_calibration(1, cam)
        ctx.extract_batch_device(d.data_ptr(), n, w, h, 3)
        ctx.synchronize()
        ran = _check_kernels(oracle, ctx, w, h, 1.2, n, False, "colour")
        assert ran[1] == 2 and all(r in (2, 5) for r in ran[1:])
        for b in (0, 1, n - 1):
            _check_levels(oracle, ctx, b, oracle.gray(col[b % 2], 1), kw, "colour")


@pytest.mark.gpu
def test_three_frames_a_larger_stride_apart_vs_oracle(oracle):
    w, h = 256, 99
    frames = np.stack([_noise(w, h, s) for s in range(3)])
    _run_gray(oracle, frames, 1.2, 272, "three frames, stride of 104 rows", rows_per_frame=104)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(250, 98, 256), (131, 98, 160), (1230, 81, 1232)], ids=lambda c: f"{c[0]}x{c[1]}-pitch{c[2]}")
def test_padding_independence(oracle, case):
    """the same in-place batch, the bytes between w and the pitch (and between the frames) 0x00, then 0xFF"""
    w, h, pitch = case
    frames = np.stack([_noise(w, h), _noise(w, h, 1)])
    a = _run_gray(oracle, frames, 1.2, pitch, "padding 0x00", rows_per_frame=h + 2, fill=0x00)
    b = _run_gray(oracle, frames, 1.2, pitch, "padding 0xFF", rows_per_frame=h + 2, fill=0xFF)
    for fa, fb in zip(a, b):
        for l, (la, lb) in enumerate(zip(fa, fb)):
            assert np.array_equal(la, lb), f"level {l} depends on the padding"


@pytest.mark.gpu
def test_small_launches_take_the_tile_form(oracle):
    """one frame, and a batch just below the wave slots: k_resize_lds, the same bytes"""
    from send_slam_amd import binding
    w, h = 240, 98
    img = _noise(w, h)
    kw = _params(oracle, w, h, 1.2)
    dims = _dims(oracle, w, h, 1.2)
    below = (_wave_slots() - 1) // _waves(dims[1], 16)  # the largest batch whose level 1 does not fill the slots
    for n in (1, below):
        d = _device(img[None], n, 240)
        with binding.OrbContext(0, max_batch=n, **kw) as ctx:
            ctx.extract_batch_device(d.data_ptr(), n, w, h, row_stride=240, frame_stride=240 * h)
            ctx.synchronize()
            ran = _check_kernels(oracle, ctx, w, h, 1.2, n, True, f"{n} frames")
            assert ran[1] == 4 and all(r in (4, 1) for r in ran[1:]), ran  # 1: a level whose rounded size puts the tile's window past 80 rows
            _check_levels(oracle, ctx, n - 1, img, kw, f"{n} frames")
