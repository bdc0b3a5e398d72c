"""k_fast_score's queue: one loop per wave over sixteen verdicts a thread, entries of two kinds, the blur over the whole region.

After the compass test a thread holds the verdicts of four pixels (columns 4 tx + i) of four rows (region rows 32 hf + 2 ty + rr)
in one word and a wave writes its candidates in one loop; a region entry is a constant of the thread + the index of the bit, a
ring entry (the 1-px ring around the region and its four corner pixels) keeps explicit coordinates under a flag bit
(csrc/ss_fast_queue.h); a queue longer than half the list (2 n > FT_QUEUE) keeps its corners in their entries.  The Gaussian's
horizontal pass runs once over a region of two halves (five blocks of 16 rows) and as three blocks in a block of one half.

Everything goes through the C ABI and is compared exactly with oracle/orb_oracle, like tests/test_fast_stacked.py: per level
the blurred level, the response map (ss_debug_fetch(2): the kernel with the bound at 3 px), the survivors per cell and the quadtree
selection, then keypoints and descriptors -- those of a context that never asked for the map, whose kernel stops 19 px from the
edges.  Every case runs as a single frame (a block per tile: every block one half) and as the smallest batch that is paired.

Each case first establishes on the CPU, from a numpy restatement of the compass rule and the kernel's thread mapping (queue()),
that it reaches the path it is there for, and asserts it.  Shapes (the smallest the ABI accepts where this code can go wrong):
  67 x 67    a pair and a lone tile of 3 rows: the blur's three-block path beside the five-block one
  131 x 98   the image ends 2 rows into a lower half: the fifth horizontal block's clamped rows
  131 x 130  two pairs and a lone tile of 2 rows
  239 x 241  the 8-level pyramid: lone halves with candidates (levels 1, 3 and 6)
"""
import functools

import numpy as np
import pytest

import patterns

FT_QUEUE = 2 * 64 * 32 + 2 * (64 + 2) + 4 * 32  # csrc/ss_kernels.hip
SHAPES = [(67, 67), (131, 98), (131, 130)]
PYRAMID = (239, 241)
MIN_TH = 7


def compass(lv, min_th):
    """the kernel's compass rule on every pixel whose ring is inside the level"""
    a = lv.astype(np.int32)
    v = a[3:-3, 3:-3]
    p0, p8, p4, p12 = a[6:, 3:-3], a[:-6, 3:-3], a[3:-3, 6:], a[3:-3, :-6]
    dark = v - np.maximum(np.minimum(p0, p8), np.minimum(p4, p12))
    bright = np.minimum(np.maximum(p0, p8), np.maximum(p4, p12)) - v
    out = np.zeros(lv.shape, bool)
    out[3:-3, 3:-3] = np.maximum(dark, bright) > min_th
    return out


def queue(lv, bound, paired, min_th=MIN_TH):
    """What every block of a level queues with the bound at `bound` px: a list of dicts with the block's origin and rows, `lanes`
    [hf, ty, tx] (the candidates of thread (ty, tx) in half hf: two rows, four columns), the ring entries per side, the ring's
    corner pixels (queued untested inside the bound) and n, the length of the queue."""
    h, w = lv.shape
    box = np.zeros((h + 130, w + 130), bool)  # origin at (1, 1); room for a ring and for rows / columns past the level
    box[1 + bound:1 + h - bound, 1 + bound:1 + w - bound] = True
    live = np.zeros_like(box)
    live[1:h + 1, 1:w + 1] = compass(lv, min_th)
    live &= box
    tile_rows = (h + 31) // 32
    out = []
    y0 = 0
    while y0 < 32 * tile_rows:
        hrows = 64 if paired and y0 + 32 < 32 * tile_rows else 32
        for x0 in range(0, w, 64):
            X, Y = x0 + 1, y0 + 1
            region = np.zeros((64, 64), np.int32)
            region[:hrows] = live[Y:Y + hrows, X:X + 64]
            # y = 32 hf + 2 ty + rr, x = 4 tx + i
            lanes = region.reshape(2, 16, 2, 16, 4).sum(axis=(2, 4))
            sides = {"top": int(live[Y - 1, X:X + 64].sum()), "bottom": int(live[Y + hrows, X:X + 64].sum()),
                     "left": int(live[Y:Y + hrows, X - 1].sum()), "right": int(live[Y:Y + hrows, X + 64].sum())}
            corners = {"tl": bool(box[Y - 1, X - 1]), "tr": bool(box[Y - 1, X + 64]), "bl": bool(box[Y + hrows, X - 1]), "br": bool(box[Y + hrows, X + 64])}
            out.append({"x0": x0, "y0": y0, "hrows": hrows, "lanes": lanes, "sides": sides, "corners": corners,
                        "n": int(lanes.sum()) + sum(sides.values()) + sum(corners.values())})
        y0 += hrows
    return out


def paths(blocks):
    """the paths a launch with these blocks takes"""
    lanes = np.stack([b["lanes"] for b in blocks]).reshape(len(blocks), 2, 4, 4, 16)  # block, hf, wave, ty & 3, tx
    half_max = lanes.max(axis=(3, 4))                # block, hf, wave
    merged_max = lanes.sum(axis=1).max(axis=(2, 3))  # block, wave
    return {
        "thread_with_16_flags": bool((lanes.sum(axis=1) == 16).any()),
        "merged_below_sum": bool((merged_max < half_max.sum(axis=1)).any()),
        "loop_never_entered": bool((lanes == 0).all()),
        "dense": any(2 * b["n"] > FT_QUEUE for b in blocks),
        "not_dense": any(2 * b["n"] <= FT_QUEUE for b in blocks),
        "ring_all_sides": all(any(b["sides"][s] for b in blocks) for s in ("top", "bottom", "left", "right")),
        "ring_all_corners": all(any(b["corners"][c] for b in blocks) for c in ("tl", "tr", "bl", "br")),
        "one_half_with_candidates": any(b["hrows"] == 32 and b["lanes"].sum() > 0 for b in blocks),
        "ring_entries_alone": any(b["lanes"].sum() == 0 and sum(b["sides"].values()) > 0 for b in blocks),
    }


def image(content, w, h):
    if content == "noise":
        return patterns.noise(w, h, 21)
    if content == "dots_rows":   # dot rows 12 px apart: a wave's candidates of the upper half sit in other lanes than the lower half's
        return patterns.dots(w, h, 1, 3, sx=2, sy=12)
    if content == "dots_cols":   # dot columns 16 px apart: every candidate of a wave in one thread column in four
        return patterns.dots(w, h, 5, 2, sx=16, sy=6)
    if content == "mixed_contrast":
        return patterns.mixed_contrast(w, h, 1, 2)
    if content == "flat":
        return patterns.flat(w, h, 90)
    raise KeyError(content)


WIDE = [(131, 98), (131, 130)]  # shapes with a block whose ring lies inside the bound on every side (at 67 x 67 none has one)
# content -> (bound, paired, path, shapes): what the case is there for, on those single-level shapes
NEEDS = {
    "noise": [(3, True, "thread_with_16_flags", SHAPES), (3, True, "dense", SHAPES), (3, True, "not_dense", SHAPES),
              (3, True, "ring_all_sides", WIDE), (3, True, "ring_all_corners", WIDE),
              (19, True, "thread_with_16_flags", WIDE), (19, True, "ring_all_sides", WIDE), (19, True, "ring_all_corners", WIDE),
              (3, False, "one_half_with_candidates", SHAPES), (19, False, "one_half_with_candidates", SHAPES)],
    "dots_rows": [(3, True, "merged_below_sum", SHAPES), (19, True, "merged_below_sum", WIDE), (3, True, "not_dense", SHAPES)],
    "dots_cols": [(3, True, "merged_below_sum", SHAPES), (19, True, "merged_below_sum", WIDE), (3, True, "not_dense", SHAPES)],
    "mixed_contrast": [(3, True, "not_dense", SHAPES), (19, False, "one_half_with_candidates", SHAPES), (3, True, "ring_entries_alone", SHAPES)],
    "flat": [(3, True, "loop_never_entered", SHAPES), (19, True, "loop_never_entered", SHAPES), (3, False, "loop_never_entered", SHAPES)],
}


def _assert_paths(content, img):
    h, w = img.shape
    reached = {}
    for bound, paired, name, shapes in NEEDS[content]:
        if (w, h) not in shapes:
            continue
        if (bound, paired) not in reached:
            reached[bound, paired] = paths(queue(img, bound, paired))
        assert reached[bound, paired][name], f"{content} {w}x{h}, bound {bound}, {'paired' if paired else 'a block per tile'}: {name} not reached"


def ring_dot(kind, w=131, h=130):
    """one isolated bright pixel (a corner with R = 255) on the ring of a block of the paired 131 x 130 launch, so that the
    block's queue holds ring entries and nothing else: ring rows (below block (0, 0) / above block (0, 1)), ring columns (right
    of block (0, 0) / left of block (1, 0)) and the ring's corner pixels (of block (0, 0) / of block (1, 1))"""
    x, y = {"row_below": (20, 64), "row_above": (20, 63), "col_right": (64, 40), "col_left": (63, 40), "corner_br": (64, 64), "corner_tl": (63, 63)}[kind]
    img = np.zeros((h, w), np.uint8)
    img[y, x] = 255
    return img, x, y


RING_DOTS = ["row_below", "row_above", "col_right", "col_left", "corner_br", "corner_tl"]


def _ring_dot_block(kind):
    """the block (of the paired launch) on whose ring the dot sits, and where: (x0, y0, side or corner)"""
    return {"row_below": (0, 0, "bottom"), "row_above": (0, 64, "top"), "col_right": (0, 0, "right"), "col_left": (64, 0, "left"),
            "corner_br": (0, 0, "br"), "corner_tl": (64, 64, "tl")}[kind]


def _assert_ring_dot(kind):
    img, x, y = ring_dot(kind)
    assert compass(img, MIN_TH).sum() == 1 and compass(img, MIN_TH)[y, x]  # the dot and nothing else passes the compass test
    x0, y0, where = _ring_dot_block(kind)
    for bound in (3, 19):
        blk = [b for b in queue(img, bound, True) if (b["x0"], b["y0"]) == (x0, y0)][0]
        assert blk["lanes"].sum() == 0 and blk["hrows"] == 64
        if where in blk["sides"]:
            assert blk["sides"] == {**dict.fromkeys(blk["sides"], 0), where: 1}   # the block's only tested entry
        else:
            assert sum(blk["sides"].values()) == 0 and blk["corners"][where]      # queued untested, scored in phase 2
            assert (x, y) == (x0 + (64 if where == "br" else -1), y0 + (64 if where == "br" else -1))


def test_cases_reach_their_paths(oracle):
    """CPU: every case of this file meets the conditions it is there for (the GPU tests assert them again, case by case)"""
    assert FT_QUEUE == 4356
    for content in NEEDS:
        for w, h in SHAPES:
            _assert_paths(content, image(content, w, h))
    for kind in RING_DOTS:
        _assert_ring_dot(kind)
    _assert_pyramid_paths(oracle, "noise")
    # what the shapes are there for
    assert [(h + 31) // 32 for _, h in SHAPES] == [3, 4, 5] and 1 <= 98 % 64 - 32 <= 4 and 67 % 64 <= 4 and 130 % 64 <= 4


def _assert_pyramid_paths(oracle, content):
    """the pyramid: a block of one half with candidates in the paired launch (a level with an odd number of tile rows whose
    last tile reaches inside the bound of 3 px), dense and sparse queues at either bound"""
    w, h = PYRAMID
    p = oracle.default_params(n_features=500)
    levels = oracle.pyramid(image(content, w, h), p)
    assert len(levels) == 8
    at3 = [paths(queue(lv, 3, True, p.min_th_fast)) for lv in levels]
    at19 = [paths(queue(lv, 19, True, p.min_th_fast)) for lv in levels]
    if content == "noise":
        assert any(a["one_half_with_candidates"] for a in at3)
        assert at3[0]["dense"] and at3[0]["not_dense"] and at19[0]["dense"] and at19[0]["not_dense"]
        assert at19[0]["thread_with_16_flags"] and at19[0]["ring_all_sides"] and at19[0]["ring_all_corners"]
    else:
        assert any(a["merged_below_sum"] for a in at19) and any(a["one_half_with_candidates"] for a in at3)


# ---- the comparison with the oracle ----

def _triples(a):
    return np.stack([a["x"], a["y"], a["response"]], axis=1).astype(np.int64).reshape(-1, 3)


class _Reference:
    """the oracle's results for one image, computed once and left unchanged"""

    def __init__(self, oracle, img, p):
        h, w = img.shape
        g = oracle.geometry(p, w, h)
        self.levels = []
        for l, lv in enumerate(oracle.pyramid(img, p)):
            cand = oracle.candidates(lv, p.ini_th_fast, p.min_th_fast)
            self.levels.append({"shape": lv.shape, "blur": oracle.blur(lv).reshape(-1), "score": oracle.fast_score_map(lv, p.min_th_fast).reshape(-1),
                                "cand": _triples(cand), "quota": g.quota[l],
                                "sel": _triples(oracle.distribute(cand, lv.shape[1], lv.shape[0], g.quota[l])) + np.array([16, 16, 0])})
        self.kps, self.desc, self.counts = oracle.extract(img, p)


def _first_diff(got, want, w):
    bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    y, x = divmod(int(bad[0]), w)
    return f"{len(bad)} differ, first at (x={x}, y={y}): got {int(np.asarray(got).reshape(-1)[bad[0]])}, oracle {int(np.asarray(want).reshape(-1)[bad[0]])}"


def _check_final(ref, got, what):
    kps, desc, counts = got
    assert np.array_equal(counts, ref.counts), f"{what}: level counts {list(counts)} != {list(ref.counts)}"
    assert kps.tobytes() == ref.kps.tobytes(), f"{what}: keypoints"
    assert np.array_equal(desc, ref.desc), f"{what}: descriptors"


def _check_levels(ref, ctx, frame, what):
    for l, r in enumerate(ref.levels):
        lh, lw = r["shape"]
        where = f"{what}: level {l} ({lw}x{lh})"
        out = ctx.debug_fetch(1, frame, l, (lh, lw))
        assert np.array_equal(out, r["blur"]), f"{where} blurred level: {_first_diff(out, r['blur'], lw)}"
        out = ctx.debug_fetch(2, frame, l, (lh, lw))
        assert np.array_equal(out, r["score"]), f"{where} response map: {_first_diff(out, r['score'], lw)}"
        out = ctx.debug_fetch(3, frame, l, (lw * lh,), np.int32).reshape(-1, 3)
        assert out.shape == r["cand"].shape and np.array_equal(out, r["cand"]), f"{where} survivors per cell: {len(out)} against the oracle's {len(r['cand'])}"
        out = ctx.debug_fetch(4, frame, l, ((4 * r["quota"] + 64) * 3,), np.int32).reshape(-1, 3)
        assert out.shape == r["sel"].shape and np.array_equal(out, r["sel"]), f"{where} quadtree selection"


@functools.lru_cache(maxsize=None)
def _frames_for_pairs(tiles):
    """the smallest batch whose launch has more tiles than the chip has block slots (eight per CU): only such a launch is paired"""
    import torch
    slots = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert slots >= tiles
    return slots // tiles + 1


def _check(oracle, img, what, **params):
    """Two contexts.  The first never asks for the response map, so its kernel stops 19 px from the edges: the keypoints and
    descriptors of a single frame and of the first and last frame of a paired batch.  The second keeps the map (the bound at
    3 px): every level of the single frame and of the same two frames of the batch."""
    import torch
    from send_slam_amd import binding
    p = oracle.default_params(**params)
    h, w = img.shape
    g = oracle.geometry(p, w, h)
    n = _frames_for_pairs(sum(((g.w[l] + 63) // 64) * ((g.h[l] + 31) // 32) for l in range(g.n_levels)))
    ref = _Reference(oracle, img, p)
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (n, h, w)))).to(torch.device("cuda:0"))
    tag = f"{what} {w}x{h}"
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        _check_final(ref, ctx.extract(img), f"{tag}, single frame, bound 19")
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        for b in (0, n - 1):
            _check_final(ref, ctx.fetch_frame(b), f"{tag}, frame {b} of {n}, bound 19")
    with binding.OrbContext(0, max_batch=n, **params) as ctx:
        got = ctx.extract(img)
        _check_levels(ref, ctx, 0, f"{tag}, single frame")
        _check_final(ref, got, f"{tag}, single frame")
        ctx.extract_batch_device(d.data_ptr(), n, w, h)
        ctx.synchronize()
        for b in (0, n - 1):
            _check_levels(ref, ctx, b, f"{tag}, frame {b} of {n}")
            _check_final(ref, ctx.fetch_frame(b), f"{tag}, frame {b} of {n}")
    return ref.kps


@pytest.mark.gpu
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("content", list(NEEDS))
def test_one_level_vs_oracle(oracle, size, content):
    w, h = size
    img = image(content, w, h)
    _assert_paths(content, img)
    kps = _check(oracle, img, content, n_features=200, n_levels=1)
    assert (len(kps) == 0) == (content == "flat")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RING_DOTS)
def test_ring_entry_alone_vs_oracle(oracle, kind):
    _assert_ring_dot(kind)
    _check(oracle, ring_dot(kind)[0], f"dot on the ring ({kind})", n_features=200, n_levels=1)


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["noise", "dots_rows", "mixed_contrast"])
def test_pyramid_vs_oracle(oracle, content):
    w, h = PYRAMID
    _assert_pyramid_paths(oracle, content)
    kps = _check(oracle, image(content, w, h), content, n_features=500)
    assert len(kps) > 0
