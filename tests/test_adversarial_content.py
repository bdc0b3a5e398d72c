"""Extraction and matching on tie-heavy and corner-dense images (tests/patterns.py).

Every other image of the suite comes from send_slam_amd/synth.py, whose +-3 pixel noise breaks every tie and keeps corners
at 0.2 % of the pixels.  The kernels have paths only other content reaches: NMS between equal neighbours, a phase-2 queue
that holds every pixel of a tile, int8 extremes in the matrix-core Gaussian, contrasts exactly at iniThFAST / minThFAST,
one response for a whole level in the quadtree, angles at multiples of 45 degrees, tens of thousands of candidates per
level, whole clusters of equal descriptors in the matcher, and the tile / bucket / candidate capacities.

CPU part (no marker): each pattern has, by the oracle alone, the property it is there for -- a pattern that loses it
fails here instead of silently becoming an easy input -- and the oracle agrees with tests/pyref.py on crops of all of them.
GPU part: the HIP path against the oracle stage by stage, whole arrays, then the batch path and every matcher form.

That the GPU part can fail was tried once on an MI355X, with one-line variants of k_fast_score built outside lib/ (selected
by SENDSLAM_LIB; not committed):
  `sc >= m` for `sc > m` in the NMS       -> every 3-px checkerboard case ends in SS_ERR_OVERFLOW (tied neighbours all survive
                                             and a tile holds more than SS_TS_CAP of them); the lattice and the 35-px
                                             checkerboard get extra candidates from level 1 on.
  `R >= min_th` for `R > min_th`          -> ring7/8/20/21 and noise differ in the score map (6 where the oracle has 0).  The
                                             contrast-7 LATTICE does not notice: the compass pre-test (`> min_th` too) sees the
                                             same value as the arc search there and drops the dots first.  ring_dots exists for
                                             this.
  `sc > ini_th` for `sc >= ini_th`        -> both mixed_contrast cases get the minTh survivors of cells that hold an iniTh one
                                             (33 411 candidates against 9 156); the contrast-21 lattice alone does not notice
                                             (a cell without an iniTh survivor falls back to the same set).
"""
import os

import numpy as np
import pytest

import patterns
import pyref
from send_slam_amd import synth
from test_oracle_units import _cell_candidates_from_map

W0, H0 = 640, 480
SIZES = [(640, 480), (333, 517), (717, 403)]  # the last two: neither dimension a multiple of the 64 x 32 tile
BIG = (1280, 720)
SOAK = "SENDSLAM_SOAK_CASES" in os.environ  # the full phase x size cross product (by hand, on a GPU box)


# ---- the catalogue: name -> (w, h) -> image ------------------------------------------------------------------------
def _catalogue():
    c = {}
    for dx in range(2):
        for dy in range(4):
            c[f"dots_{dx}{dy}"] = lambda w, h, dx=dx, dy=dy: patterns.dots(w, h, dx, dy)
            c[f"ramp_dots_{dx}{dy}"] = lambda w, h, dx=dx, dy=dy: patterns.ramp_dots(w, h, dx, dy)
    for k in (1, 2, 3, 4, 5, 8, 35):
        for ph in range(k if SOAK else min(k, 8)):  # phase on the diagonal
            c[f"checker{k}_{ph}"] = lambda w, h, k=k, ph=ph: patterns.checker(w, h, k, ph, ph)
    for k in (2, 3, 5):
        c[f"blocks{k}_bw"] = lambda w, h, k=k: patterns.blocks(w, h, k, 11 + k, (0, 255))
        c[f"blocks{k}_4"] = lambda w, h, k=k: patterns.blocks(w, h, k, 17 + k, (0, 85, 170, 255))
    c["noise"] = lambda w, h: patterns.noise(w, h, 5)
    c["noise01"] = lambda w, h: patterns.noise01(w, h, 6)
    c["saturated"] = lambda w, h: patterns.saturated(3, w, h)
    c["mirrored"] = lambda w, h: patterns.mirrored(4, w, h)
    for v in (0, 1, 254, 255):
        c[f"flat{v}"] = lambda w, h, v=v: patterns.flat(w, h, v)
    for cc in (7, 8, 20, 21):
        c[f"contrast{cc}_mid"] = lambda w, h, cc=cc: patterns.contrast_dots(w, h, 100, cc)
        c[f"contrast{cc}_low"] = lambda w, h, cc=cc: patterns.contrast_dots(w, h, 0, cc, 1, 1)
        c[f"contrast{cc}_high"] = lambda w, h, cc=cc: patterns.contrast_dots(w, h, 255 - cc, cc, 0, 2)
        c[f"ring{cc}"] = lambda w, h, cc=cc: patterns.ring_dots(w, h, cc, cc % 3, cc % 5)
    c["mixed_contrast"] = lambda w, h: patterns.mixed_contrast(w, h)
    c["mixed_contrast_13"] = lambda w, h: patterns.mixed_contrast(w, h, 1, 3)
    return c


CATALOGUE = _catalogue()


def _is_phase(name):
    """a phase-shifted copy of a periodic pattern (the copy at phase 0 is the family's representative)"""
    head, _, tail = name.rpartition("_")
    return (head.startswith(("dots", "ramp_dots")) and tail != "00") or (head.startswith("checker") and tail != "0")


def _triples(a):
    return np.stack([a["x"], a["y"], a["response"]], axis=1).astype(np.int64).reshape(-1, 3)


def _compass_pass(img, th):
    """Phase 1 of k_fast_score from its definition: with the ring pairs (0, 8) and (4, 12), a pixel goes on to the arc search
    iff max(v - max(min(p0, p8), min(p4, p12)), min(max(p0, p8), max(p4, p12)) - v) > th.  -> bool map of the pixels FAST
    evaluates (3 px inside the image)."""
    v = img.astype(np.int64)
    h, w = v.shape
    c = v[3:h - 3, 3:w - 3]
    p0, p8 = v[6:h, 3:w - 3], v[0:h - 6, 3:w - 3]
    p4, p12 = v[3:h - 3, 6:w], v[3:h - 3, 0:w - 6]
    dark = c - np.maximum(np.minimum(p0, p8), np.minimum(p4, p12))
    bright = np.minimum(np.maximum(p0, p8), np.maximum(p4, p12)) - c
    return np.maximum(dark, bright) > th


def _compass_pass_rate(img, th):
    return float(_compass_pass(img, th).mean())


# =====================================================================================================================
# CPU: the inputs do what they are there for (floors: the oracle's figures at 640 x 480, with a little slack)
# =====================================================================================================================
def test_catalogue_is_deterministic_and_well_formed():
    for name, make in CATALOGUE.items():
        a, b = make(200, 150), make(200, 150)
        assert a.dtype == np.uint8 and a.shape == (150, 200) and a.flags.c_contiguous, name
        assert np.array_equal(a, b), name
    assert not np.array_equal(patterns.noise(64, 64, 1), patterns.noise(64, 64, 2))
    assert set(np.unique(patterns.noise01(64, 64, 1))) == {0, 255}
    assert set(np.unique(patterns.blocks(64, 64, 3, 1, (0, 85, 170, 255)))) == {0, 85, 170, 255}
    m = patterns.mirrored(4, 201, 100)
    assert np.array_equal(m[:, :100], m[:, 101:][:, ::-1])


@pytest.mark.parametrize("dx,dy", [(0, 0), (1, 3)])
def test_lattice_is_dense_with_one_response(oracle, dx, dy):
    img = patterns.dots(W0, H0, dx, dy)
    cand = oracle.candidates(img, 20, 7)
    assert len(cand) >= 0.10 * W0 * H0                      # measured 33 411 = 10.9 %; synth.frame gives 0.2 %
    assert set(cand["response"].tolist()) == {254}           # R = 255 for every dot: one distinct response
    assert 0.11 <= _compass_pass_rate(img, 7) <= 0.14        # every dot and nothing else: 1 / 8 of the pixels
    sc = oracle.fast_score_map(img, 7)
    assert (sc > 0).mean() >= 0.12


def test_ramp_lattice_is_dense_with_distinct_responses(oracle):
    cand = oracle.candidates(patterns.ramp_dots(W0, H0), 20, 7)
    assert len(cand) >= 0.10 * W0 * H0 and len(set(cand["response"].tolist())) >= 100  # measured 108


def test_one_pixel_checkerboard_passes_the_compass_test_everywhere_and_has_no_corner(oracle):
    img = patterns.checker(W0, H0, 1)
    assert _compass_pass_rate(img, 7) == 1.0                 # the dense queue path: every pixel is queued for the arc search
    assert (oracle.fast_score_map(img, 7) > 0).sum() == 0
    assert len(oracle.candidates(img, 20, 7)) == 0
    assert set(np.unique(oracle.blur(img)[8:-8, 8:-8])) == {127, 128}


@pytest.mark.parametrize("ph", [0, 1, 2])
def test_three_pixel_checkerboard_is_all_ties(oracle, ph):
    img = patterns.checker(W0, H0, 3, ph, ph)
    assert _compass_pass_rate(img, 7) == 1.0
    assert (oracle.fast_score_map(img, 7) > 0).mean() >= 0.40  # measured 43.5 %
    assert len(oracle.candidates(img, 20, 7)) == 0             # every score has an equal neighbour: `>` removes them all


def test_noise_is_dense(oracle):
    img = patterns.noise(W0, H0, 5)
    assert _compass_pass_rate(img, 7) >= 0.85                  # measured 90.9 %
    assert (oracle.fast_score_map(img, 7) > 0).mean() >= 0.30  # 34.2 %
    cand = oracle.candidates(img, 20, 7)
    assert len(cand) >= 0.08 * W0 * H0                         # 27 594 = 9.0 %
    # the busiest 64 x 32 tile (candidates are relative to the (16, 16) border origin)
    tiles = np.bincount(((cand["y"] + 16) // 32) * 16 + (cand["x"] + 16) // 64)
    assert tiles.max() >= 180                                  # measured 231; synth.frame: a few dozen


@pytest.mark.parametrize("base", ["mid", "low", "high"])
def test_contrast_dots_sit_exactly_on_the_thresholds(oracle, base):
    """R > minThFAST (7) makes a corner, R - 1 >= iniThFAST (20) makes it one at the first threshold.  On this lattice the
    kernel's compass pre-test sees the same value as the arc search (all 16 ring pixels are equal), so it is the pre-test's
    `> min_th` that the contrast-7 lattice pins; patterns.ring_dots pins the arc search's."""
    want = {7: (0, None), 8: (33000, 7), 20: (33000, 19), 21: (33000, 20)}
    for c, (floor, resp) in want.items():
        cand = oracle.candidates(CATALOGUE[f"contrast{c}_{base}"](W0, H0), 20, 7)
        if resp is None:
            assert len(cand) == 0, (c, len(cand))
        else:
            assert len(cand) >= floor and set(cand["response"].tolist()) == {resp}, (c, len(cand))


def test_ring_dots_leave_the_threshold_to_the_arc_search(oracle):
    """R == minThFAST exactly at pixels that pass the compass pre-test: `R > min_th` in the arc search decides alone."""
    want = {7: 0, 8: 7, 20: 19, 21: 20}
    for c, score in want.items():
        img = patterns.ring_dots(W0, H0, c)
        centres = (slice(8, H0 - 8, 8), slice(8, W0 - 8, 8))
        assert _compass_pass(img, 7)[5:H0 - 11:8, 5:W0 - 11:8].all(), c          # the same pixels in the map's coordinates (- 3)
        assert (pyref.fast_response(img)[centres] == c).all(), c
        assert (oracle.fast_score_map(img, 7)[centres] == score).all(), c
        assert (oracle.fast_score_map(img, 20)[centres] == (score if score >= 20 else 0)).all(), c


def test_mixed_contrast_has_both_kinds_of_cell(oracle):
    cand = oracle.candidates(patterns.mixed_contrast(W0, H0), 20, 7)
    resp = cand["response"]
    assert set(resp.tolist()) == {7, 19, 20}
    assert (resp == 20).sum() > 500 and (resp < 20).sum() > 5000
    # a cell keeps either its >= iniTh survivors or all its minTh ones, never both
    cell = ((cand["y"] - 3) // 38).astype(np.int64) * 1000 + (cand["x"] - 3) // 36   # 640 x 480: 17 x 12 cells of 36 x 38 px at (3, 3)
    strong = set(cell[resp == 20].tolist())
    weak = set(cell[resp < 20].tolist())
    assert strong and weak and not (strong & weak)


def test_lattice_keypoints_have_axis_angles_and_twins(oracle):
    kps, desc, counts = oracle.extract(patterns.dots(W0, H0), oracle.default_params())
    assert len(kps) >= 1200
    assert np.mean(np.mod(kps["angle"], np.float32(45)) == 0) >= 0.15   # measured 22 %
    idx, d1, d2 = oracle.match(desc, desc, exclude_self=True)
    assert np.mean(d1 == 0) >= 0.30                                      # measured 41 %
    assert len({bytes(r) for r in desc}) <= 0.8 * len(desc)


def test_one_pixel_checkerboard_descriptors_repeat(oracle):
    kps, desc, counts = oracle.extract(patterns.checker(W0, H0, 1), oracle.default_params())
    assert counts[0] == 0 and len(kps) >= 500                 # corners appear only where the pyramid's resize beats
    assert len({bytes(r) for r in desc}) <= len(desc) // 4    # measured 99 distinct among 731


def test_saturated_pins_large_areas_at_both_ends(oracle):
    img = patterns.saturated(3, W0, H0)
    assert (img == 0).mean() >= 0.05 and (img == 255).mean() >= 0.05
    assert len(oracle.candidates(img, 20, 7)) >= 300


@pytest.mark.parametrize("size", SIZES + [BIG])
def test_every_size_admits_eight_levels(oracle, size):
    kps, desc, counts = oracle.extract(patterns.dots(*size), oracle.default_params(n_features=1000))
    assert len(counts) == 8 and counts[0] > 0


CROP = (200, 150)


@pytest.mark.parametrize("name", [n for n in CATALOGUE if not _is_phase(n)] + ["dots_13", "checker3_2", "checker5_3"])
def test_oracle_agrees_with_rederivations_on_crops(oracle, name):
    """score map, blur, per-cell candidates, quadtree and match of the C oracle against the numpy / Python statements of the
    same algorithms, on 200 x 150 of every pattern: the reference handles this content consistently."""
    img = CATALOGUE[name](*CROP)
    w, h = CROP
    for t in (7, 20):
        assert np.array_equal(oracle.fast_score_map(img, t), pyref.fast_score_map(img, t)), f"score map at {t}"
    assert np.array_equal(oracle.blur(img), pyref.blur(img)), "blur"
    cand = oracle.candidates(img, 20, 7)
    tup = [tuple(r) for r in _triples(cand).tolist()]
    assert tup == _cell_candidates_from_map(img, 20, 7), "candidates"
    for n in (5, 60, 400):
        got = oracle.distribute(cand, w, h, n)
        want = pyref.distribute_array_form(tup, w, h, n, oracle.std_sort) if tup else []
        assert [tuple(r) for r in _triples(got).tolist()] == want, f"quadtree, quota {n}"
    kps, desc, _ = oracle.extract(img, oracle.default_params(n_features=300, n_levels=3))
    if len(desc):
        q = desc[:150]
        for kw in (dict(th=50, ratio_num=9), dict(th=256, ratio_num=10)):
            for a, b in zip(oracle.match(q, q, exclude_self=True, **kw), pyref.match(q, q, kw["th"], kw["ratio_num"], 10, exclude_self=True)):
                assert np.array_equal(a, b), "self-match"
            for a, b in zip(oracle.match(q, desc[::-1][:120], **kw), pyref.match(q, desc[::-1][:120], kw["th"], kw["ratio_num"], 10)):
                assert np.array_equal(a, b), "match"


# =====================================================================================================================
# GPU: stage by stage against the oracle, whole arrays
# =====================================================================================================================
def _first_diff(got, want, shape):
    bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    y, x = divmod(int(bad[0]), shape[1])
    return f"{len(bad)} pixels differ, first at (x={x}, y={y}): got {int(np.asarray(got).reshape(-1)[bad[0]])}, oracle {int(np.asarray(want).reshape(-1)[bad[0]])}"


def _first_row_diff(got, want):
    n = min(len(got), len(want))
    bad = np.nonzero((got[:n] != want[:n]).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        return f"{len(got)} against the oracle's {len(want)}, first difference at entry {i}: got {got[i].tolist()}, oracle {want[i].tolist()}"
    return f"{len(got)} entries against the oracle's {len(want)}"


def check_stages(oracle, binding, img, what, n_features=1000, ctx=None, **ctx_kw):
    """ctx.extract(img), then per level pyramid / blurred level / score map / candidates / quadtree selection against the
    oracle computed here -- whole arrays, border pixels included -- then counts, keypoints bit for bit and descriptors.
    A failure names the first stage and level that differs and the first differing coordinate.  -> (keypoints, descriptors)"""
    h, w = img.shape
    p = oracle.default_params(n_features=n_features)
    g = oracle.geometry(p, w, h)
    levels = oracle.pyramid(img, p)
    own = ctx is None
    if own:
        ctx = binding.OrbContext(0, n_features=n_features, **ctx_kw)
    try:
        kps, desc, counts = ctx.extract(img)  # SS_ERR_OVERFLOW raises here: the capacities suffice (geometry_sweep.cpp)
        for l, lv in enumerate(levels):
            lh, lw = lv.shape
            where = f"{what} {w}x{h} n={n_features}: level {l} ({lw}x{lh})"
            got = ctx.debug_fetch(0, 0, l, (lh, lw))
            assert np.array_equal(got, lv.reshape(-1)), f"{where} pyramid: {_first_diff(got, lv, lv.shape)}"
            got, want = ctx.debug_fetch(1, 0, l, (lh, lw)), oracle.blur(lv)
            assert np.array_equal(got, want.reshape(-1)), f"{where} blurred level: {_first_diff(got, want, lv.shape)}"
            got, want = ctx.debug_fetch(2, 0, l, (lh, lw)), oracle.fast_score_map(lv, p.min_th_fast)
            assert np.array_equal(got, want.reshape(-1)), f"{where} FAST score map: {_first_diff(got, want, lv.shape)}"
            ocand = oracle.candidates(lv, p.ini_th_fast, p.min_th_fast)
            got, want = ctx.debug_fetch(3, 0, l, (lw * lh,), np.int32).reshape(-1, 3), _triples(ocand)
            assert np.array_equal(got, want), f"{where} candidates: {_first_row_diff(got, want)}"
            osel = _triples(oracle.distribute(ocand, lw, lh, g.quota[l])) + np.array([16, 16, 0])
            got = ctx.debug_fetch(4, 0, l, ((4 * g.quota[l] + 64) * 3,), np.int32).reshape(-1, 3)
            assert np.array_equal(got, osel), f"{where} quadtree selection: {_first_row_diff(got, osel)}"
        okps, odesc, ocounts = oracle.extract(img, p)
        where = f"{what} {w}x{h} n={n_features}"
        assert np.array_equal(counts, ocounts), f"{where} level counts {list(counts)} != {list(ocounts)}"
        for f in ("octave", "response", "x", "y", "size", "angle"):
            bad = np.nonzero(kps[f].view(np.uint32) != okps[f].view(np.uint32))[0]
            assert len(bad) == 0, f"{where} keypoint field {f}: {len(bad)} differ, first {bad[:5]}: {kps[f][bad[:5]]} != {okps[f][bad[:5]]}"
        assert kps.tobytes() == okps.tobytes(), f"{where} keypoints"
        bad = np.nonzero((desc != odesc).any(axis=1))[0]
        assert len(bad) == 0, f"{where} descriptors: {len(bad)} differ, first {bad[:5]}"
        return kps, desc
    finally:
        if own:
            ctx.close()


def _stage_cases():
    """(pattern, (w, h), n_features).  Default: every pattern once, sizes and phases rotating so that each size meets each
    family and each phase of the lattice and of the small checkerboards occurs; the lattice's quota extremes; the large
    size for the four densest.  With SENDSLAM_SOAK_CASES set: every pattern x every size."""
    names = list(CATALOGUE)
    if SOAK:
        cases = [(n, s, 1000) for n in names for s in SIZES]
        cases += [(n, BIG, 1000) for n in names if n.startswith(("dots", "noise", "checker1_", "checker3_"))]
    else:
        cases = [(n, SIZES[i % 3], 1000) for i, n in enumerate(names)]
        cases += [("dots_00", s, 1000) for s in SIZES[1:]] + [("noise", s, 1000) for s in SIZES[:2]]
        cases += [("checker1_0", SIZES[1], 1000), ("checker3_1", SIZES[2], 1000), ("checker3_2", SIZES[0], 1000)]
        cases += [(n, BIG, 1000) for n in ("dots_00", "noise", "checker1_0", "checker3_0")]
    cases += [("dots_00", SIZES[0], 40), ("dots_13", SIZES[1], 40), ("dots_00", SIZES[0], 6250), ("dots_12", SIZES[2], 6250),
              ("ramp_dots_00", SIZES[0], 6250), ("noise", SIZES[0], 6250), ("checker3_0", SIZES[0], 40)]
    return list(dict.fromkeys(cases))


@pytest.mark.gpu
@pytest.mark.parametrize("name,size,nf", _stage_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_stage_by_stage_vs_oracle(oracle, name, size, nf):
    from send_slam_amd import binding
    img = CATALOGUE[name](*size)
    kps, desc = check_stages(oracle, binding, img, name, n_features=nf)
    if name.startswith("flat"):
        assert len(kps) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 255])
def test_flat_extremes_blur_to_themselves(value):
    """pixel - 128 at both ends of int8 in the matrix-core Gaussian: every blurred level of a flat 0 / 255 image is exactly
    0 / 255, rim included, and there is no keypoint."""
    from send_slam_amd import binding
    from oracle import orb_oracle as O
    for w, h in ((640, 480), (333, 517)):
        with binding.OrbContext(0) as ctx:
            kps, desc, counts = ctx.extract(patterns.flat(w, h, value))
            g = O.geometry(O.default_params(), w, h)
            for l in range(8):
                blr = ctx.debug_fetch(1, 0, l, (g.h[l], g.w[l]))
                assert len(blr) == g.h[l] * g.w[l] and (blr == value).all(), (w, h, l, np.unique(blr))
        assert len(kps) == 0 and counts.sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("dots_01", (640, 480)), ("noise", (717, 403))])
def test_stage_by_stage_with_two_levels_per_launch(oracle, monkeypatch, name, size):
    from send_slam_amd import binding
    monkeypatch.setenv("SENDSLAM_RESIZE_PAIRS", "1")  # read at ss_create
    check_stages(oracle, binding, CATALOGUE[name](*size), name + " (resize pairs)")


# =====================================================================================================================
# GPU: the batch path and the matcher on this content
# =====================================================================================================================
BATCH_NAMES = ["dots_00", "noise", "checker3_0", "checker1_0", "saturated", "synth", "flat0", "flat255"]  # densest first


def _batch_frame(name, w, h):
    return synth.frame(21, w, h) if name == "synth" else CATALOGUE[name](w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["densest_first", "densest_last"])
def test_batch_of_mixed_content_vs_oracle_and_single_frame_path(oracle, order):
    """A dense frame must not disturb its neighbours' tile or bucket slabs: eight frames in one extract_batch_device, every
    frame equal to the oracle's and to the single-frame path's result; then both batch matching modes."""
    import torch
    from send_slam_amd import binding
    w, h, nf = 640, 480, 1000
    names = BATCH_NAMES if order == "densest_first" else BATCH_NAMES[::-1]
    frames = np.stack([_batch_frame(n, w, h) for n in names])
    B = len(frames)
    dev = torch.device("cuda:0")
    d = torch.from_numpy(frames).to(dev)
    with binding.OrbContext(0, n_features=nf, max_batch=B) as ctx:
        ctx.extract_batch_device(d.data_ptr(), B, w, h)
        ctx.synchronize()
        kcap = ctx.batch_view().kp_capacity
        outs = [torch.empty((B, kcap), dtype=t, device=dev) for t in (torch.int32, torch.int16, torch.int16)]
        res = {}
        for mode in (0, 1):
            ctx.match_batch_device(mode, *[o.data_ptr() for o in outs])
            ctx.synchronize()
            res[mode] = (outs[0].cpu().numpy().copy(), outs[1].cpu().numpy().view(np.uint16).copy(), outs[2].cpu().numpy().view(np.uint16).copy())
        fetched = [ctx.fetch_frame(b) for b in range(B)]
        single = [ctx.extract(frames[b]) for b in range(B)]
    p = oracle.default_params(n_features=nf)
    prev = None
    for b, name in enumerate(names):
        okps, odesc, ocounts = oracle.extract(frames[b], p)
        for path, (k, dsc, cnt) in (("batch", fetched[b]), ("single", single[b])):
            assert np.array_equal(cnt, ocounts), f"{order} frame {b} ({name}), {path} path: counts {list(cnt)} != {list(ocounts)}"
            assert k.tobytes() == okps.tobytes(), f"{order} frame {b} ({name}), {path} path: keypoints"
            assert np.array_equal(dsc, odesc), f"{order} frame {b} ({name}), {path} path: descriptors"
        n = len(okps)
        want0 = oracle.match(odesc, odesc, exclude_self=True)
        want1 = want0 if b == 0 else oracle.match(odesc, prev)
        for mode, want in ((0, want0), (1, want1)):
            for a, ww, nm in zip(res[mode], want, ("idx", "d1", "d2")):
                assert np.array_equal(a[b, :n], ww), f"{order} frame {b} ({name}) mode {mode}: {nm}"
            assert (res[mode][0][b, n:] == -1).all()
        prev = odesc
    assert len(fetched[names.index("flat0")][0]) == 0 and len(fetched[names.index("flat255")][0]) == 0


MATCHER_FORMS = [("default", {}), ("compact", {"SENDSLAM_MX_FORM": "compact"}), ("pipelined", {"SENDSLAM_MX_FORM": "pipelined"}),
                 ("one_chunk", {"SENDSLAM_MX_CHUNKS": "1"}), ("packed", {"SENDSLAM_MATCH_PACKED": "1"})]
_DESC_SETS = {}


def _descriptor_sets(oracle):
    """Descriptor sets with whole clusters of equal rows, from the oracle (the extraction is checked above):
    (name, set, set of the phase-shifted frame)."""
    if not _DESC_SETS:
        for name, a, b, size, nf in (("lattice_640x480", "dots_00", "dots_12", (640, 480), 1250),
                                     ("lattice_1280x720", "dots_00", "dots_11", (1280, 720), 2000),
                                     ("checker1_640x480", "checker1_0", "checker1_0", (640, 480), 1250)):
            p = oracle.default_params(n_features=nf)
            da = oracle.extract(CATALOGUE[a](*size), p)[1]
            # the 1-px checkerboard has one other phase: shifted by one pixel along x (its negative)
            db = oracle.extract(CATALOGUE[b](*size), p)[1] if a != b else oracle.extract(patterns.checker(size[0], size[1], 1, 1, 0), p)[1]
            _DESC_SETS[name] = (da, db)
    return _DESC_SETS


def test_descriptor_sets_are_tie_heavy(oracle):
    sets = _descriptor_sets(oracle)
    for name, (da, db) in sets.items():
        assert len(da) >= 700 and len(db) >= 700, (name, len(da), len(db))
        idx, d1, d2 = oracle.match(da, da, th=-1, exclude_self=True)
        assert np.mean(d1 == 0) >= 0.30, (name, float(np.mean(d1 == 0)))          # 41 % / 57 % / most of checker 1
        assert np.mean((d1 == 0) & (d2 == 0)) >= 0.10, name                        # clusters of three and more equal rows
    assert len({bytes(r) for r in sets["checker1_640x480"][0]}) <= len(sets["checker1_640x480"][0]) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("form,env", MATCHER_FORMS, ids=[f for f, _ in MATCHER_FORMS])
def test_matcher_forms_on_duplicate_heavy_sets(oracle, monkeypatch, form, env):
    """Group-minimum selection with an exact second pass: lowest-index ties and d2 == d1 == 0 for whole clusters of equal
    rows, under every matcher form a host can select; bit-exact idx, d1, d2."""
    from send_slam_amd import binding
    for k in ("SENDSLAM_MX_FORM", "SENDSLAM_MX_CHUNKS", "SENDSLAM_MATCH_PACKED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # before the context is created
    with binding.OrbContext(0) as ctx:
        for name, (da, db) in _descriptor_sets(oracle).items():
            small = np.ascontiguousarray(da[::max(1, len(da) // 100)][:120])  # < 128 rows: the VALU kernel
            assert len(small) < 128
            for th in (50, 256, -1):
                for ratio_num in (7, 9, 10):
                    kw = dict(th=th, ratio_num=ratio_num, ratio_den=10)
                    runs = [("self", da, da, True), ("shifted", da, db, False), ("shifted back", db, da, False),
                            ("small self", small, small, True), ("small vs set", small, db, False)]
                    for what, q, t, ex in runs:
                        got = ctx.match(q, t, exclude_self=ex, **kw)
                        want = oracle.match(q, t, exclude_self=ex, **kw)
                        for a, b, nm in zip(got, want, ("idx", "d1", "d2")):
                            bad = np.nonzero(a != b)[0]
                            assert len(bad) == 0, (f"{form} / {name} / {what} / {kw}: {nm} differs for {len(bad)} of {len(q)} queries, "
                                                   f"first {bad[:5]}: {a[bad[:5]]} != {b[bad[:5]]}")
