"""k_fast_score stages every rim region by 16-byte loads: the pieces of a staged row that lie outside the image's row.

A region is staged as rows of 96 bytes that start at x0 - 16: six pieces of 16 bytes, one per thread and round.  An interior
region loads all six.  A rim region loads the pieces that lie inside the image's row -- bytes [0, pitch) of it -- and stages
zeros for the others: piece 0 at the left rim (x0 = 0), the last one to four at the right rim, where the row ends (its pitch,
a multiple of 16) before the window does.  The three columns BORDER_REFLECT_101 defines left of 0 and right of w - 1 are then
written over what was staged there (zeros, or the row's padding bytes w .. pitch - 1), so no result may depend on the
padding.  Everything goes through the C ABI (ss_extract_batch_device on a device buffer with its own pitch) and is compared
exactly with oracle/orb_oracle, with the checks of test_fast_stacked.py (_check_frame: blurred level on columns < w, response
map, survivors per cell, quadtree selection, keypoints, descriptors, level counts) and of test_fast_border.py (the same
without the response map, where the kernel's bound is 19 px instead of 3).  Every case runs on one context in this order:

  1. one frame (a block per tile), then a batch large enough for blocks of two tiles (first and last frame), both checked
     WITHOUT the response map, before any ss_debug_fetch(2);
  2. the batch again through _check_frame, which fetches selector 2: the kernel runs again, now with the map;
  3. one frame with the map kept, through _check_frame, and the bytes of step 1 required of it;
  4. the same frames in buffers whose padding columns hold 255 and 0 instead: the bytes of step 1 again.

Widths (one level), and what the tightest pitch the in-place path takes makes of the right rim:
  w    w % 16  w % 64  pitch
  129     1       1     144   x0 = 128: window 112 .. 207, pieces at 112 and 128 inside, the last of them ends at the pitch,
                              four outside; x0 = 64 (at the rim: 132 > 129): window 48 .. 143 ends exactly at the pitch
  138    10      10     144   x0 = 128 as for 129; x0 = 64 is an inner column
  140    12      12     144   as 138
  143    15      15     144   as 138
  144     0      16     144   pitch == w: the last in-row piece ends where the buffer's row does
  200     8       8     208   x0 = 192: pieces at 176 and 192 inside, four outside
  257     1       1     272   x0 = 256: pieces at 240 and 256 inside; x0 = 192 (at the rim: 260 > 257) loads all six
A looser pitch (+16, +32, the next multiple of 64) moves the first piece outside the row to the right: three, two or one
outside.  The library's own levels have pitches that are multiples of 64; a width that is no multiple of 16 given as its own
pitch is ingested into such a level (the in-place path needs rows 16 bytes apart).

One tile wide.  The ABI accepts no level narrower than 67 px (asserted below), so a level of one tile column does not exist;
the narrowest levels are 67 and 68 wide: the block at x0 = 0 is at the left AND at the right rim (x0 + 68 > w or == w), and
the last column is 3 or 4 px wide.  The 8-level pyramid at 239 x 241 ends in a level 67 wide.

Heights 131, 140, 146, 193: a lone last tile of 3 rows, and 12, 18 and 1 row(s) into a third or seventh tile row -- corners
(left / right AND top / bottom) in all of them.

Content.  Uniform noise (corners in every rim row and column: test_fast_rim.py asserts it for its frames, the same generator
and seeds), the synthetic scene, and the padding fills of step 4.  An over-read is not looked for by a fault: the predicate
is one unsigned comparison, gx <= pitch - 16 with gx < 0 wrapped, reviewed in the kernel; the frame buffers here end with
their last row.
"""
import numpy as np
import pytest

import patterns
from send_slam_amd import synth
from test_fast_border import _check_frame_without_map, _same
from test_fast_stacked import _check_frame, _frames_for_pairs

ONE = dict(n_features=200, n_levels=1)
EIGHT = dict(n_features=500)
# (w, h, pitch).  pitch % 16 == 0: level 0 in place; otherwise the library's own copy (pitch a multiple of 64)
SHAPES = [(129, 140, 129), (140, 140, 140), (138, 146, 138), (200, 131, 200), (257, 193, 257), (143, 140, 143), (144, 131, 144)]
NARROW = [(67, 67, 67), (68, 100, 68), (67, 98, 80), (68, 67, 80)]
IN_PLACE = [(129, 140, 144), (138, 146, 144), (138, 146, 160), (138, 146, 176), (143, 140, 144), (144, 131, 160), (200, 131, 208), (257, 193, 272),
            (129, 140, 192), (80, 100, 80), (208, 131, 208)]
PYRAMID = (239, 241)


def _noise(w, h):
    return patterns.noise(w, h, 1000 * w + h)  # test_fast_rim's frames


def _content(name, w, h):
    return _noise(w, h) if name == "noise" else synth.frame(7, w, h)


def _device_frames(img, n, pitch, fill):
    """n copies of img in a device buffer of rows `pitch` bytes apart that ends with its last row; the padding columns hold
    `fill` (None: 255 - the row's last pixel, a byte no row holds at its end)"""
    import torch
    h, w = img.shape
    padded = np.empty((n, h, pitch), np.uint8)
    padded[:, :, w:] = (255 - img[:, w - 1:w]) if fill is None else fill
    padded[:, :, :w] = img
    return torch.from_numpy(padded).to(torch.device("cuda:0"))


def _extract(ctx, d, frames, w, h, pitch):
    ctx.extract_batch_device(d.data_ptr(), frames, w, h, row_stride=pitch)
    ctx.synchronize()
    return {b: ctx.fetch_frame(b) for b in sorted({0, frames - 1})}


def _check(oracle, img, pitch, what, **params):
    from send_slam_amd import binding
    p = oracle.default_params(**params)
    h, w = img.shape
    n = _frames_for_pairs(oracle, p, w, h)
    what = f"{what}, pitch {pitch}"
    d = _device_frames(img, n, pitch, None)
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        one = _extract(ctx, d, 1, w, h, pitch)[0]
        _check_frame_without_map(oracle, ctx, 0, img, p, what + ", single frame", one)
        batch = _extract(ctx, d, n, w, h, pitch)
        for b in (0, n - 1):
            _check_frame_without_map(oracle, ctx, b, img, p, f"{what}, frame {b} of {n}", batch[b])
        for b in (0, n - 1):
            _check_frame(oracle, ctx, b, img, p, f"{what}, frame {b} of {n}, map fetched", batch[b])
        again = _extract(ctx, d, 1, w, h, pitch)[0]
        _check_frame(oracle, ctx, 0, img, p, what + ", single frame, map kept", again)
        _same(again, one, what + ", single frame")
    if pitch > w:
        for fill in (255, 0):
            d = _device_frames(img, n, pitch, fill)
            with binding.OrbContext(0, max_batch=n, **params) as ctx:
                _same(_extract(ctx, d, 1, w, h, pitch)[0], one, f"{what}, single frame, padding {fill}")
                other = _extract(ctx, d, n, w, h, pitch)
                for b in (0, n - 1):
                    _same(other[b], batch[b], f"{what}, frame {b} of {n}, padding {fill}")
    return one[0]


def test_shapes_reach_the_pieces_outside_the_row(oracle):
    """what the sizes are there for, from the arithmetic of the staging (CPU)"""
    p1 = oracle.default_params(**ONE)
    for w, h, pitch in SHAPES + NARROW + IN_PLACE:
        oracle.geometry(p1, w, h)  # accepted
        assert pitch >= w
    for w in (63, 64, 66):  # no level of one tile column
        with pytest.raises(Exception):
            oracle.geometry(p1, w, 100)
    g = oracle.geometry(oracle.default_params(**EIGHT), *PYRAMID)
    assert g.n_levels == 8 and g.w[7] == 67

    def outside(w, pitch):
        """per tile column at the left or the right rim: the pieces of its window that are not loaded"""
        out = {}
        for x0 in range(0, w, 64):
            if not (x0 >= 4 and x0 + 68 <= w):
                out[x0] = [c for c in range(6) if not (0 <= x0 - 16 + 16 * c and x0 - 16 + 16 * c + 16 <= pitch)]
        return out

    def effective(w, pitch):
        return pitch if pitch % 16 == 0 else (w + 63) // 64 * 64  # in place, or the library's own copy

    widths = {w for w, _, _ in SHAPES}
    assert {w % 16 for w in widths} >= {0, 1, 8, 15} and all(1 <= w % 64 <= 20 for w in widths)
    for w, h, pitch in SHAPES + NARROW + IN_PLACE:
        o = outside(w, effective(w, pitch))
        assert o[0][0] == 0, (w, pitch)                          # the left rim's first piece
        assert all(len(v) <= 4 for v in o.values()), (w, pitch)  # the pieces that hold columns of the image are loaded
    assert outside(129, 144) == {0: [0], 64: [], 128: [2, 3, 4, 5]}
    assert outside(144, 144) == {0: [0], 128: [2, 3, 4, 5]}      # x0 = 64 is an inner column: 132 <= 144
    assert outside(200, 208) == {0: [0], 192: [2, 3, 4, 5]}
    assert outside(257, 272) == {0: [0], 192: [], 256: [2, 3, 4, 5]}
    assert outside(67, 80) == {0: [0], 64: [2, 3, 4, 5]} and outside(67, 128) == {0: [0], 64: [5]}
    assert outside(138, 160) == {0: [0], 128: [3, 4, 5]} and outside(138, 176) == {0: [0], 128: [4, 5]} and outside(129, 192) == {0: [0], 64: [], 128: [5]}
    # in place: pitches that are multiples of 16 but not of 64, pitch == w among them, and one of 64
    assert all(pitch % 16 == 0 for _, _, pitch in IN_PLACE)
    assert {pitch % 64 for _, _, pitch in IN_PLACE} >= {0, 16, 32, 48}
    assert sum(w == pitch for w, _, pitch in IN_PLACE + SHAPES if pitch % 16 == 0) >= 3
    # the last row of the last frame ends where the buffer does: no piece that is loaded ends behind its row
    for w, h, pitch in IN_PLACE:
        for x0 in range(0, w, 64):
            for c in range(6):
                gx = x0 - 16 + 16 * c
                if (gx & 0xFFFFFFFF) <= pitch - 16:  # the kernel's predicate
                    assert 0 <= gx and gx + 16 <= pitch


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("content", ["noise", "synth"])
def test_widths_vs_oracle(oracle, case, content):
    w, h, pitch = case
    _check(oracle, _content(content, w, h), pitch, content, **ONE)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NARROW, ids=lambda c: f"{c[0]}x{c[1]}-pitch{c[2]}")
@pytest.mark.parametrize("content", ["noise", "synth"])
def test_left_and_right_rim_in_one_block_vs_oracle(oracle, case, content):
    w, h, pitch = case
    _check(oracle, _content(content, w, h), pitch, content, **ONE)


@pytest.mark.gpu
@pytest.mark.parametrize("case", IN_PLACE, ids=lambda c: f"{c[0]}x{c[1]}-pitch{c[2]}")
def test_level0_in_place_vs_oracle(oracle, case):
    w, h, pitch = case
    _check(oracle, _noise(w, h), pitch, "noise in place", **ONE)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch", [239, 240, 256])
@pytest.mark.parametrize("content", ["noise", "synth"])
def test_eight_level_pyramid_vs_oracle(oracle, content, pitch):
    """levels of the library's own layout down to one 67 px wide; level 0 ingested (239), in place at the tightest pitch and at
    a pitch of 64"""
    kps = _check(oracle, _content(content, *PYRAMID), pitch, content, **EIGHT)
    assert len(kps) > 0
