"""k_fast_score without the response map: nothing outside the rectangle the cell windows can use is tested, queued or scored.

ComputeKeyPointsOctTree's cell windows start 16 px inside a level and FAST leaves a 3-px rim inside each window, so a level's
pixels are evaluated in 19 <= x < w - 19, 19 <= y < h - 19 only.  With the response map (`score != NULL`: a context that has
been asked for ss_debug_fetch(2)) the kernel tests and scores 3 <= x < w - 3, 3 <= y < h - 3, which is what
oracle.fast_score_map fills; without it (normal operation) the compass test, the ring around a region and the queue stop at
19, and a wave whose eight rows lie outside skips its compass rows.  The path under test is the one WITHOUT the map, so every
case goes in this order, once as a single frame (a block per tile) and once as a batch large enough for blocks of two tiles:

  1. a fresh context, extract;
  2. survivors per cell (selector 3), quadtree selection (selector 4), blurred levels, keypoints, descriptors and level
     counts exactly against the oracle, BEFORE any ss_debug_fetch(2);
  3. on the same context test_fast_stacked's _check_frame, which fetches selector 2 (the kernel runs again, now with the map)
     and compares the whole map and everything else again;
  4. extract again -- the context now keeps the map -- and require the bytes of step 1.

Sizes (one level, noise): 67 x 67 is the smallest level (valid rectangle 29 x 29); 83 x 83 and 115 x 83 end the rectangle
exactly on a tile or seam boundary (w - 19 = 64 / 96, h - 19 = 64); 147 x 100 has w - 19 = 128; at 140 x 140 and 138 x 146
the block at (64, 64) is staged as an interior one (x0 + 68 <= w, y0 + 68 <= h) yet holds dead columns and rows
(w - 19 < x0 + 64); 131 x 98 and 200 x 130 end in a lone last tile / two rows into a lower half.  The 8-level pyramid is taken
at 239 x 241.  The dot lattice at 200 x 130 fills the list: the dead frame may decide whether 2 n > FT_QUEUE (corners behind
the queue or in place), and either form must give the same result.
"""
import numpy as np
import pytest

import patterns
from send_slam_amd import synth
from test_fast_stacked import _check_frame, _diff, _frames_for_pairs, _triples

EDGE = 19
SHAPES = [(67, 67), (83, 83), (115, 83), (147, 100), (140, 140), (138, 146), (131, 98), (200, 130)]
PYRAMID = (239, 241)
ONE = dict(n_features=200, n_levels=1)
EIGHT = dict(n_features=500)


def _noise(w, h):
    return patterns.noise(w, h, 1000 * w + h)  # test_fast_rim's frames


def _check_frame_without_map(oracle, ctx, frame, img, p, what, got):
    """_check_frame without selector 2: nothing here makes the context allocate the response map"""
    h, w = img.shape
    g = oracle.geometry(p, w, h)
    for l, lv in enumerate(oracle.pyramid(img, p)):
        lh, lw = lv.shape
        where = f"{what} {w}x{h}, no map: level {l} ({lw}x{lh})"
        out, want = ctx.debug_fetch(1, frame, l, (lh, lw)), oracle.blur(lv)
        assert np.array_equal(out, want.reshape(-1)), f"{where} blurred level: {_diff(out, want, lw)}"
        ocand = oracle.candidates(lv, p.ini_th_fast, p.min_th_fast)
        out, want = ctx.debug_fetch(3, frame, l, (lw * lh,), np.int32).reshape(-1, 3), _triples(ocand)
        assert out.shape == want.shape and np.array_equal(out, want), f"{where} survivors per cell: {len(out)} against the oracle's {len(want)}"
        osel = _triples(oracle.distribute(ocand, lw, lh, g.quota[l])) + np.array([16, 16, 0])
        out = ctx.debug_fetch(4, frame, l, ((4 * g.quota[l] + 64) * 3,), np.int32).reshape(-1, 3)
        assert out.shape == osel.shape and np.array_equal(out, osel), f"{where} quadtree selection"
    kps, desc, counts = got
    okps, odesc, ocounts = oracle.extract(img, p)
    assert np.array_equal(counts, ocounts), f"{what} {w}x{h}, no map: level counts {list(counts)} != {list(ocounts)}"
    assert kps.tobytes() == okps.tobytes(), f"{what} {w}x{h}, no map: keypoints"
    assert np.array_equal(desc, odesc), f"{what} {w}x{h}, no map: descriptors"


def _same(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), f"{what}: with the map kept the extraction differs from the one without it"


def _check(oracle, img, what, **params):
    import torch
    from send_slam_amd import binding
    p = oracle.default_params(**params)
    h, w = img.shape
    with binding.OrbContext(0, **params) as ctx:
        first = ctx.extract(img)
        _check_frame_without_map(oracle, ctx, 0, img, p, what + ", single frame", first)
        _check_frame(oracle, ctx, 0, img, p, what + ", single frame, map fetched", first)
        _same(ctx.extract(img), first, what + ", single frame")
    n = _frames_for_pairs(oracle, p, w, h)
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (n, h, w)))).to(torch.device("cuda:0"))
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        first = {b: ctx.fetch_frame(b) for b in (0, n - 1)}
        for b in (0, n - 1):
            _check_frame_without_map(oracle, ctx, b, img, p, f"{what}, frame {b} of {n}", first[b])
        for b in (0, n - 1):
            _check_frame(oracle, ctx, b, img, p, f"{what}, frame {b} of {n}, map fetched", first[b])
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        for b in (0, n - 1):
            _same(ctx.fetch_frame(b), first[b], f"{what}, frame {b} of {n}")
    return first[0][0]


def test_why_these_inputs_can_fail(oracle):
    """CPU.  On each noise frame the oracle's survivors touch all four edges of the rectangle (image x = 19 and w - 20, y = 19
    and h - 20), at least 3 on each: a mask one pixel too tight loses candidates.  The oracle's response map holds at least 999
    non-zero pixels outside the rectangle: comparing the whole map shows a bound that leaked into the path with the map."""
    p1 = oracle.default_params(**ONE)
    frames = [(_noise(w, h), p1) for w, h in SHAPES] + [(_noise(*PYRAMID), oracle.default_params(**EIGHT))]
    for img, p in frames:
        h, w = img.shape
        oracle.geometry(p, w, h)  # accepted
        cand = oracle.candidates(img, p.ini_th_fast, p.min_th_fast)  # level 0; relative to the (16, 16) border origin
        x, y = cand["x"] + 16, cand["y"] + 16
        assert x.min() == EDGE and x.max() == w - EDGE - 1 and y.min() == EDGE and y.max() == h - EDGE - 1, (w, h)
        on_edge = [int((x == EDGE).sum()), int((x == w - EDGE - 1).sum()), int((y == EDGE).sum()), int((y == h - EDGE - 1).sum())]
        assert min(on_edge) >= 3, (w, h, on_edge)
        sc = oracle.fast_score_map(img, p.min_th_fast)
        outside = sc > 0
        outside[EDGE:h - EDGE, EDGE:w - EDGE] = False
        assert int(outside.sum()) >= 999, (w, h, int(outside.sum()))
    # what the sizes are there for
    assert SHAPES[0] == (67, 67) and 67 - 2 * EDGE == 29
    assert (83 - EDGE, 115 - EDGE, 147 - EDGE) == (64, 96, 128) and SHAPES[1][1] - EDGE == 64 and SHAPES[2][1] - EDGE == 64
    for w, h in (SHAPES[4], SHAPES[5]):  # the block at (64, 64): interior for staging, dead columns and rows
        assert 64 + 68 <= w and 64 + 68 <= h and 68 <= w - 64 < 83 and 68 <= h - 64 < 83
    assert (98 + 31) // 32 == 4 and 1 <= 98 % 64 - 32 <= 4 and (130 + 31) // 32 == 5  # rim in a lower half only; a lone last tile
    assert int((oracle.fast_score_map(patterns.dots(200, 130, 1, 3), p1.min_th_fast) > 0).sum()) > 200 * 130 // 10  # a dense list


@pytest.mark.gpu
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_level_noise_without_the_map(oracle, size):
    w, h = size
    _check(oracle, _noise(w, h), "noise", **ONE)


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["noise", "synth"])
def test_eight_level_pyramid_without_the_map(oracle, content):
    w, h = PYRAMID
    img = _noise(w, h) if content == "noise" else synth.frame(5, w, h)
    kps = _check(oracle, img, content, **EIGHT)
    assert len(kps) > 0


@pytest.mark.gpu
def test_dense_list_without_the_map(oracle):
    _check(oracle, patterns.dots(200, 130, 1, 3), "dots", **ONE)
