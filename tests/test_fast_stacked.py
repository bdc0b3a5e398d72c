"""k_fast_score takes two vertically adjacent 64 x 32 tiles per block: the pairing, the seam inside a block and the lone tile.

A block handles the tiles (tx, 2k) and (tx, 2k + 1) of a level as one 64 x 64 region: rows 31 | 32 of the region are a seam
without a ring (the NMS of either row reads the scores the other half wrote), rows 63 | 64 are the boundary between two blocks
(a ring row on either side), and a level with an odd number of tile rows ends in blocks of one tile.  Tiles are paired only
in a launch with more tiles than the chip has block slots; a smaller one (a single frame) runs the same kernel with a block
per tile, so every case runs as a single frame AND as a batch large enough to be paired.  Everything here goes
through the C ABI and is compared exactly with oracle/orb_oracle: the response map (ss_debug_fetch(2): the kernel's
`score != NULL` path), the NMS survivors per cell (the candidates of a level are the survivors of its cells, cell by cell),
the quadtree selection, and the final keypoints and descriptors.

Sizes.  The ABI accepts no level lower than 67 rows (a 35-px cell inside 16-px borders), so a level has at least three tile
rows: level-0 tile-row counts of 1 and 2 -- a lone tile alone, one pair alone -- do not exist.  The smallest there are:
  67   three tile rows: one pair and a lone tile of 3 rows (the smallest height and width the ABI accepts)
  96   three tile rows, the image ends exactly on the seam position of the last block: a pair and a FULL lone tile
  98   four tile rows: the image ends 2 rows into the lower half of the second pair (the rim path in a lower half only)
  128  four tile rows, the image ends on a block boundary
  130  five tile rows: two pairs and a lone tile of 2 rows
Widths 67 and 131: two and three tile columns, the last one 3 px wide.  One level suffices for these (n_levels = 1); the
8-level pyramid is taken at 239 x 241 (239 is the smallest side that admits eight levels), where the levels' tile-row counts are
both odd and even (asserted below from the geometry).
"""
import numpy as np
import pytest

import patterns
from send_slam_amd import synth

SHAPES = [(67, 67), (131, 96), (67, 98), (131, 128), (131, 130)]
PYRAMID = (239, 241)


def _triples(a):
    return np.stack([a["x"], a["y"], a["response"]], axis=1).astype(np.int64).reshape(-1, 3)


def _diff(got, want, w):
    bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    y, x = divmod(int(bad[0]), w)
    return f"{len(bad)} differ, first at (x={x}, y={y}): got {int(np.asarray(got).reshape(-1)[bad[0]])}, oracle {int(np.asarray(want).reshape(-1)[bad[0]])}"


def _check_frame(oracle, ctx, frame, img, p, what, got=None):
    """frame `frame` of the context's last extraction against the oracle's extraction of img: per level the blurred level,
    the response map, the candidates (NMS survivors cell by cell) and the quadtree selection, then keypoints and descriptors"""
    h, w = img.shape
    g = oracle.geometry(p, w, h)
    for l, lv in enumerate(oracle.pyramid(img, p)):
        lh, lw = lv.shape
        where = f"{what} {w}x{h}: level {l} ({lw}x{lh})"
        out, want = ctx.debug_fetch(1, frame, l, (lh, lw)), oracle.blur(lv)
        assert np.array_equal(out, want.reshape(-1)), f"{where} blurred level: {_diff(out, want, lw)}"
        out, want = ctx.debug_fetch(2, frame, l, (lh, lw)), oracle.fast_score_map(lv, p.min_th_fast)
        assert np.array_equal(out, want.reshape(-1)), f"{where} response map: {_diff(out, want, lw)}"
        ocand = oracle.candidates(lv, p.ini_th_fast, p.min_th_fast)
        out, want = ctx.debug_fetch(3, frame, l, (lw * lh,), np.int32).reshape(-1, 3), _triples(ocand)
        assert out.shape == want.shape and np.array_equal(out, want), f"{where} survivors per cell: {len(out)} against the oracle's {len(want)}"
        osel = _triples(oracle.distribute(ocand, lw, lh, g.quota[l])) + np.array([16, 16, 0])
        out = ctx.debug_fetch(4, frame, l, ((4 * g.quota[l] + 64) * 3,), np.int32).reshape(-1, 3)
        assert out.shape == osel.shape and np.array_equal(out, osel), f"{where} quadtree selection"
    kps, desc, counts = got
    okps, odesc, ocounts = oracle.extract(img, p)
    assert np.array_equal(counts, ocounts), f"{what} {w}x{h}: level counts {list(counts)} != {list(ocounts)}"
    assert kps.tobytes() == okps.tobytes(), f"{what} {w}x{h}: keypoints"
    assert np.array_equal(desc, odesc), f"{what} {w}x{h}: descriptors"
    return kps


def _tiles(oracle, p, w, h):
    """64 x 32 tiles of all levels of a frame"""
    g = oracle.geometry(p, w, h)
    return sum(((g.w[l] + 63) // 64) * ((g.h[l] + 31) // 32) for l in range(g.n_levels))


def _frames_for_pairs(oracle, p, w, h):
    """The library pairs tiles only in a launch with more tiles than the chip has block slots (eight per CU); a smaller launch
    -- a single frame -- runs a block per tile.  -> the smallest batch of w x h frames whose launch is paired."""
    import torch
    slots = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    n = slots // _tiles(oracle, p, w, h) + 1
    assert n * _tiles(oracle, p, w, h) > slots >= _tiles(oracle, p, w, h)
    return n


def _check(oracle, img, what, **params):
    """img as a single frame (a block per tile) and as every frame of a batch large enough for blocks of two tiles; of the
    batch the first and the last frame are compared"""
    import torch
    from send_slam_amd import binding
    p = oracle.default_params(**params)
    h, w = img.shape
    n = _frames_for_pairs(oracle, p, w, h)
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        got = ctx.extract(img)
        kps = _check_frame(oracle, ctx, 0, img, p, what + ", single frame", got)
        d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (n, h, w)))).to(torch.device("cuda:0"))
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        for b in (0, n - 1):
            _check_frame(oracle, ctx, b, img, p, f"{what}, frame {b} of {n}", ctx.fetch_frame(b))
        return kps


def seam_ties(w, h):
    """Single bright pixels on 0, each a corner with R = 255 (its FAST ring holds no other dot): pairs that are 8-neighbours
    of each other across row 31 | 32 (the seam inside a block), 63 | 64 (two blocks), 95 | 96, and across the tile columns
    63 | 64 and 127 | 128 -- vertical, horizontal and both diagonals -- alternately of equal value (a tie: `>` drops both)
    and of values 255 / 200 (one survives).  Pairs are 8 px apart, so no ring meets another pair."""
    img = np.zeros((h, w), np.uint8)
    k = 0

    def pair(xa, ya, xb, yb):
        nonlocal k
        if min(xa, xb) >= 3 and max(xa, xb) < w - 3 and min(ya, yb) >= 3 and max(ya, yb) < h - 3:
            img[ya, xa] = 255
            img[yb, xb] = 255 if k % 2 == 0 else 200
            k += 1

    for y in (31, 63, 95):
        for i, x in enumerate(range(20, w - 8, 8)):
            pair(x, y, x + (-1, 0, 1)[i % 3], y + 1)
    for x in (63, 127):
        for i, y in enumerate(range(20, h - 8, 8)):
            if (y + 8) % 32 >= 16:  # keep clear of the row pairs above
                pair(x, y, x + 1, y + (-1, 0, 1)[i % 3])
    # the four pixels around a corner where a row seam and a column seam cross
    for x, y in ((63, 31), (63, 63)):
        img[y - 1:y + 3, x - 1:x + 3] = 0
        img[y, x] = img[y + 1, x + 1] = 255
    return img


def _tile_rows(h):
    return (h + 31) // 32


def test_shapes_cover_pair_lone_and_rim(oracle):
    """what the sizes are there for, from the geometry (CPU: a size that loses its property fails here)"""
    assert [_tile_rows(h) for _, h in SHAPES] == [3, 3, 4, 4, 5]
    p1 = oracle.default_params(n_features=200, n_levels=1)
    for w, h in SHAPES:
        oracle.geometry(p1, w, h)  # accepted
    with pytest.raises(Exception):
        oracle.geometry(p1, 66, 67)
    with pytest.raises(Exception):
        oracle.geometry(p1, 67, 66)
    assert SHAPES[1][1] % 64 == 32 and SHAPES[3][1] % 64 == 0          # ends on a seam / on a block boundary
    assert 1 <= SHAPES[2][1] % 64 - 32 <= 4                            # 1 .. 4 rows into a lower half
    assert 1 <= SHAPES[4][1] % 64 <= 4 and 1 <= SHAPES[0][1] % 64 <= 4  # a lone tile of a few rows
    g = oracle.geometry(oracle.default_params(n_features=500), *PYRAMID)
    rows = [_tile_rows(g.h[l]) for l in range(8)]
    assert g.n_levels == 8 and any(r % 2 for r in rows) and any(r % 2 == 0 for r in rows), rows
    with pytest.raises(Exception):
        oracle.geometry(oracle.default_params(n_features=500), PYRAMID[0] - 1, PYRAMID[1])
    assert _tile_rows(g.h[5]) == 4 and g.h[5] % 64 == 33               # a level that ends one row into a lower half
    t = seam_ties(200, 140)
    sc = oracle.fast_score_map(t, 7)
    for y in (31, 63, 95):
        assert (sc[y] == 254).sum() >= 10 and (sc[y + 1] > 0).sum() >= 10, y
    assert (sc[:, 63] > 0).sum() >= 4 and (sc[:, 64] > 0).sum() >= 4 and (sc[:, 127] > 0).sum() >= 4
    cand = oracle.candidates(t, 20, 7)
    assert 0 < len(cand) < (sc > 0).sum()  # ties dropped, unequal pairs keep one


@pytest.mark.gpu
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("content", ["noise", "dots"])
def test_one_level_shapes_vs_oracle(oracle, size, content):
    """random bytes / the dot lattice: the queue holds (nearly) every pixel of both halves"""
    w, h = size
    img = patterns.noise(w, h, 11) if content == "noise" else patterns.dots(w, h, 1, 3)
    _check(oracle, img, content, n_features=200, n_levels=1)


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["noise", "dots", "synth"])
def test_eight_level_pyramid_vs_oracle(oracle, content):
    w, h = PYRAMID
    img = {"noise": lambda: patterns.noise(w, h, 12), "dots": lambda: patterns.dots(w, h), "synth": lambda: synth.frame(5, w, h)}[content]()
    kps = _check(oracle, img, content, n_features=500)
    assert len(kps) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(200, 140), (131, 98), (200, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_across_seams_vs_oracle(oracle, size):
    _check(oracle, seam_ties(*size), "seam ties", n_features=200, n_levels=1)


@pytest.mark.gpu
def test_batch_of_three_with_an_empty_frame(oracle):
    """one launch over three frames, the middle one constant: its tile slots are written empty, its neighbours' are theirs"""
    import torch
    from send_slam_amd import binding
    w, h = 131, 130
    frames = np.stack([patterns.noise(w, h, 13), patterns.flat(w, h, 90), seam_ties(w, h)])
    params = dict(n_features=200, n_levels=1)
    p = oracle.default_params(**params)
    d = torch.from_numpy(frames).to(torch.device("cuda:0"))
    with binding.OrbContext(0, max_batch=3, **params) as ctx:
        ctx.extract_batch_device(d.data_ptr(), 3, w, h)
        ctx.synchronize()
        for b in range(3):
            kps = _check_frame(oracle, ctx, b, frames[b], p, f"batch frame {b}", ctx.fetch_frame(b))
            assert (len(kps) == 0) == (b == 1)


@pytest.mark.gpu
def test_large_batch_with_empty_frames(oracle):
    """the same three frames over and over in a batch large enough for blocks of two tiles: the first three and the last three"""
    import torch
    from send_slam_amd import binding
    w, h = 131, 130
    three = [patterns.noise(w, h, 13), patterns.flat(w, h, 90), seam_ties(w, h)]
    params = dict(n_features=200, n_levels=1)
    p = oracle.default_params(**params)
    n = -(-_frames_for_pairs(oracle, p, w, h) // 3) * 3
    d = torch.from_numpy(np.stack([three[b % 3] for b in range(n)])).to(torch.device("cuda:0"))
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        for b in (0, 1, 2, n - 3, n - 2, n - 1):
            kps = _check_frame(oracle, ctx, b, three[b % 3], p, f"batch frame {b} of {n}", ctx.fetch_frame(b))
            assert (len(kps) == 0) == (b % 3 == 1)
