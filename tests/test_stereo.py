"""GPU parity of the stereo depth path (ss_stereo_batch_device, ss_extract_stereo) against tests/stereo_ref.py: bit for bit,
no tolerance -- right_idx / orb_dist / sad equal, u_right and depth compared as raw 32-bit patterns, every summary field equal.

That the median select can fail was tried once on an MI355X with a one-line variant of k_stereo_cut built outside lib/ (selected
by SENDSLAM_LIB; not committed):
  rank `(n_ref - 1) / 2` for `n_ref / 2`       -> test_tiny_counts_through_the_median_select fails on the two-point pair: the
                                                 smaller SAD becomes the median and the other point loses its depth (u_right
                                                 -1 for 39.0 at row 1); the one- and three-point pairs agree, as they must.
                                                 Pairs with an even count of a few hundred notice too, by a median one step
                                                 lower (335 for 338 on 333 x 247, 289 for 290 at scale 1.5) or one point cut
                                                 more: 7 of the 14 tests of this file fail, the other 7 have odd counts or
                                                 equal middle SADs.
"""
from collections import Counter

import numpy as np
import pytest

import patterns
import stereo_ref as R
from send_slam_amd import synth

pytestmark = pytest.mark.gpu

BASELINE, TH_DEPTH = 0.1, 35.0


def _params(oracle, nf, scale=1.2, levels=8):
    """the stereo setting: lapping area {0, 0}"""
    return oracle.default_params(n_features=nf, lapping_x0=0, lapping_x1=0, scale_factor=scale, n_levels=levels)


def _ctx(binding, nf, scale=1.2, levels=8, max_batch=2):
    return binding.OrbContext(0, n_features=nf, lapping_x0=0, lapping_x1=0, scale_factor=scale, n_levels=levels, max_batch=max_batch)


def _parallax_pair(w, h, t, seed):
    sc = synth.scene(seed, w, h)
    return synth.parallax_frame(seed, w, h, t, sc=sc), synth.parallax_frame(seed, w, h, 0, sc=sc)


def _pattern_pairs(w, h):
    """tie-heavy content shifted horizontally: equal Hamming distances and equal SADs decide by lowest index"""
    P = patterns
    return {"checker16_dx6": (P.checker(w, h, 16, dx=6), P.checker(w, h, 16)),
            "checker8_dx3": (P.checker(w, h, 8, dx=3), P.checker(w, h, 8)),
            "dots_dx2": (P.dots(w, h, dx=2), P.dots(w, h)),
            "blocks_roll7": (np.roll(P.blocks(w, h, 12, 5), 7, axis=1), P.blocks(w, h, 12, 5)),
            "noise_roll9": (np.roll(P.noise(w, h, 3), 9, axis=1), P.noise(w, h, 3)),
            "mixed_dx5": (P.mixed_contrast(w, h, dx=5), P.mixed_contrast(w, h))}


def _ingests(ctx):
    return sum(s["launches"] for s in ctx.stats() if s["name"] == "ingest")


def _stereo_batch(ctx, frames, fx_list, row_stride=None, ingest=None):
    """frames [2 * pairs, h, w] through ss_extract_batch_device, then one ss_stereo_batch_device per fx on the same batch.
    -> {fx: (points [pairs, kcap], summaries [pairs])}.  row_stride: rows that far apart, the padding filled with 0x5C;
    ingest: when given, whether level 0 must have been copied into the pyramid block (False: read in place)"""
    import torch
    from send_slam_amd import binding
    dev = torch.device("cuda:0")
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape
    rs = w if row_stride is None else row_stride
    padded = np.full((n, h, rs), 0x5C, np.uint8)
    padded[:, :, :w] = frames
    d = torch.from_numpy(padded).to(dev)
    if ingest is not None:
        assert ((d.data_ptr() | rs | (rs * h)) % 16 != 0) == ingest, "the buffer does not take the route this case is there for"
        ctx.profile(True)
        ctx.profile_reset()
    ctx.extract_batch_device(d.data_ptr(), n, w, h, row_stride=rs, frame_stride=rs * h)
    if ingest is not None:
        ctx.synchronize()
        assert _ingests(ctx) == int(ingest)
        ctx.profile(False)
    kcap = ctx.batch_view().kp_capacity
    out = {}
    for fx in fx_list:
        d_pts = torch.full((n // 2, kcap, binding.STEREO_POINT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device=dev)
        d_sum = torch.full((n // 2, binding.STEREO_SUMMARY_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device=dev)
        ctx.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), fx, BASELINE, TH_DEPTH)
        ctx.synchronize()
        out[fx] = (d_pts.cpu().numpy().copy().view(binding.STEREO_POINT_DTYPE).reshape(n // 2, kcap),
                   d_sum.cpu().numpy().copy().view(binding.STEREO_SUMMARY_DTYPE).reshape(n // 2))
    return out


def _check(tag, got_pts, got_sum, want_pts, want_sum):
    """got_pts may hold more rows than the left eye has keypoints: the rest must be "none" """
    n = len(want_pts)
    got = {k: int(got_sum[k]) for k in R.SUMMARY_FIELDS} if not isinstance(got_sum, dict) else got_sum
    print(tag, got)
    assert got["n_left"] == want_sum["n_left"] and got["n_right"] == want_sum["n_right"], f"{tag}: extraction differs {got} {want_sum}"
    for f in ("right_idx", "orb_dist", "sad"):
        bad = np.flatnonzero(got_pts[f][:n] != want_pts[f])
        assert len(bad) == 0, f"{tag}: {f} differs at rows {bad[:8]}: {got_pts[f][:n][bad[:8]]} != {want_pts[f][bad[:8]]}"
    for f in ("u_right", "depth"):
        a, b = np.ascontiguousarray(got_pts[f][:n]).view(np.uint32), np.ascontiguousarray(want_pts[f]).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{tag}: {f} differs at rows {bad[:8]}: {got_pts[f][:n][bad[:8]]} != {want_pts[f][bad[:8]]}"
    assert got_pts[n:].tobytes() == R.none_points(len(got_pts) - n).tobytes(), f"{tag}: rows past the left keypoints are not 'none'"
    assert got == want_sum, f"{tag}: summary {got} != {want_sum}"


def _reference(oracle, left, right, p, fx):
    st = Counter()
    res = R.stereo_pair(left, right, p, fx, BASELINE, TH_DEPTH, st)
    assert st["guard"] == 0, "the window guard fired: the deviation from upstream is no longer theoretical on this input"
    return res, st


PARALLAX = [(640, 480, 1000, 4, 7, 1.2, 8), (1280, 720, 2000, 6, 3, 1.2, 8), (640, 480, 1000, 4, 7, 1.5, 5)]


@pytest.mark.parametrize("w,h,nf,t,seed,scale,levels", PARALLAX)
def test_parallax_pairs_bit_exact(oracle, w, h, nf, t, seed, scale, levels):
    """fx = 500: the whole disparity range is admitted.  fx = 20: maxD = bf / mb = 20 px, so the bands whose disparity is
    larger (three of six at t = 4, four at t = 6) cannot match: the minU filter bites."""
    from send_slam_amd import binding
    left, right = _parallax_pair(w, h, t, seed)
    p = _params(oracle, nf, scale, levels)
    with _ctx(binding, nf, scale, levels) as ctx:
        got = _stereo_batch(ctx, np.stack([left, right]), [500.0, 20.0])
    matched = {}
    for fx in (500.0, 20.0):
        (kL, dL, kR, dR, pts, summ), st = _reference(oracle, left, right, p, fx)
        print(fx, summ, dict(st))
        # no vacuous pass: asserted on the REFERENCE
        assert st["median_cut"] >= 1
        if fx == 500.0:
            assert summ["n_depth"] >= 0.4 * summ["n_left"], summ
        matched[fx] = summ["n_matched"]
        _check(f"parallax {w}x{h} scale {scale} fx {fx}", got[fx][0][0], got[fx][1][0], pts, summ)
    assert 0 < matched[20.0] < matched[500.0]


ODD_PAIRS = [(330, 250, 3, 11), (333, 247, 3, 5)]  # widths that are no multiple of 16, nor of 4: level 0 cannot be read in place


@pytest.mark.parametrize("w,h,t,seed", ODD_PAIRS)
def test_level_0_in_the_pyramid_block_and_in_place_with_a_pitch(oracle, w, h, t, seed):
    """The same pair by three routes, each against the reference: dense device rows (the ingest copy: k_stereo_refine reads
    level 0 from the pyramid block, whose pitch is not the width), rows padded to 336 bytes (in place, pitch != width) and
    ss_extract_stereo from host pixels."""
    from send_slam_amd import binding
    nf = 500
    left, right = _parallax_pair(w, h, t, seed)
    p = _params(oracle, nf)
    want = {fx: _reference(oracle, left, right, p, fx)[0] for fx in (500.0, 20.0)}
    assert 0 < want[20.0][5]["n_matched"] < want[500.0][5]["n_matched"] and want[500.0][5]["n_depth"] > 200
    with _ctx(binding, nf) as ctx:
        for route, rs, ingest in (("ingest", w, True), ("in place, pitch 336", 336, False)):
            got = _stereo_batch(ctx, np.stack([left, right]), [500.0, 20.0], row_stride=rs, ingest=ingest)
            for fx in (500.0, 20.0):
                _check(f"{w}x{h} {route} fx {fx}", got[fx][0][0], got[fx][1][0], want[fx][4], want[fx][5])
        for cam_id, fx in ((3, 500.0), (4, 20.0)):
            cam = binding.Camera(type=b"PinHole", fx=fx, fy=fx, cx=w / 2, cy=h / 2, width=w, height=h, fps=30.0, th_depth=TH_DEPTH,
                                 baseline=BASELINE)
            ctx.set_calibration(cam_id, cam)
            kL, dL, kR, dR, pts, summ = ctx.extract_stereo(left, right, camera_id=cam_id)
            okL, odL, okR, odR, opts, osumm = want[fx]
            assert kL.tobytes() == okL.tobytes() and np.array_equal(dL, odL) and kR.tobytes() == okR.tobytes() and np.array_equal(dR, odR)
            assert len(pts) == len(okL)
            _check(f"{w}x{h} host pixels fx {fx}", pts, summ, opts, osumm)


TINY_SIZES = (22, 26, 28)  # the side of the textured patch: 1, 2 and 3 refined points (tests/test_stereo_ref.py)


def tiny_pairs():
    """pairs with a handful of keypoints: the 320 x 240 pair of seed 11, t = 3, flat except for a patch of s x s px in the left
    eye and of (s + 16) x s px, starting 8 px further left, in the right one; a flat pair sits between them"""
    from test_orient_split import patch_of
    left, right = _parallax_pair(320, 240, 3, 11)
    pairs = [(f"patch{s}", (patch_of(left, 40, 40, s, s), patch_of(right, 32, 40, s + 16, s))) for s in TINY_SIZES]
    pairs.insert(2, ("flat", (patterns.flat(320, 240, 100), patterns.flat(320, 240, 100))))
    return pairs


def test_tiny_counts_through_the_median_select(oracle):
    """1, 2 and 3 refined points per pair, one batch: element [n / 2] of one, two and three SADs.  With two the median is the
    larger one and neither point is cut; a rank of (n - 1) / 2 would take the smaller and cut the other."""
    from send_slam_amd import binding
    nf = 500
    pairs = tiny_pairs()
    p = _params(oracle, nf)
    with _ctx(binding, nf, max_batch=2 * len(pairs)) as ctx:
        got = _stereo_batch(ctx, np.stack([e for _, pr in pairs for e in pr]), [500.0], ingest=False)[500.0]
    for i, (name, (l, r)) in enumerate(pairs):
        (kL, dL, kR, dR, pts, summ), st = _reference(oracle, l, r, p, 500.0)
        _check(f"pair {i} ({name})", got[0][i], got[1][i], pts, summ)


PYRAMIDS = [(800, 600, 600, 4, 7, 2.0, 4), (640, 480, 1000, 4, 7, 1.2, 1), (640, 480, 1000, 4, 7, 1.1, 8)]


@pytest.mark.parametrize("w,h,nf,t,seed,scale,levels", PYRAMIDS)
def test_pyramid_shapes(oracle, w, h, nf, t, seed, scale, levels):
    """scale factor 2.0 (every level half the one below), a pyramid of ONE level (the packed octave test of k_stereo_search
    runs with octL - 1 == 0xFFFF for every keypoint) and scale factor 1.1 (eight levels of nearly one size)"""
    from send_slam_amd import binding
    left, right = _parallax_pair(w, h, t, seed)
    (kL, dL, kR, dR, pts, summ), st = _reference(oracle, left, right, _params(oracle, nf, scale, levels), 500.0)
    print(summ, dict(st))
    assert st["median_cut"] >= 1 and summ["n_depth"] > 300
    assert set(kL["octave"].tolist()) == set(range(levels))
    with _ctx(binding, nf, scale, levels) as ctx:
        got = _stereo_batch(ctx, np.stack([left, right]), [500.0], ingest=False)[500.0]
    _check(f"{w}x{h} scale {scale} levels {levels}", got[0][0], got[1][0], pts, summ)


def test_identical_pair_cuts_everything(oracle):
    """left == right: every SAD is 0, the median is 0, stage C cuts every point; the disparity is negative or lands on the
    0.01 clamp"""
    from send_slam_amd import binding
    w, h, nf = 640, 480, 1000
    img = synth.frame(5, w, h)
    p = _params(oracle, nf)
    (kL, dL, kR, dR, pts, summ), st = _reference(oracle, img, img, p, 500.0)
    print(summ, dict(st))
    assert summ["n_refined"] > 100 and summ["sad_median"] == 0 and summ["n_depth"] == 0 and st["median_cut"] == summ["n_refined"]
    assert st["disp_negative"] > 0 and st["disp_clamped"] > 0
    with _ctx(binding, nf) as ctx:
        got = _stereo_batch(ctx, np.stack([img, img]), [500.0])
    _check("identical pair", got[500.0][0][0], got[500.0][1][0], pts, summ)


def _mixed_batch(w, h):
    """ten pairs of different content: the six tie-heavy ones, a parallax pair, a pair with a flat LEFT eye, one with a flat
    RIGHT eye (zero keypoints), an identical pair"""
    pairs = list(_pattern_pairs(w, h).items())
    pl, pr = _parallax_pair(w, h, 3, 11)
    pairs += [("parallax", (pl, pr)), ("flat_left", (patterns.flat(w, h, 90), pr)), ("flat_right", (pl, patterns.flat(w, h, 255))),
              ("identical", (pr, pr))]
    return pairs


def test_batch_of_mixed_pairs_then_a_second_call(oracle):
    """>= 8 pairs in one call, two of them with an eye without keypoints: every pair equals the reference, the neighbours of
    the empty pairs included; then the same context takes other frames (the pairs in reverse order, eyes swapped):
    nothing of the first call leaks into the second."""
    from send_slam_amd import binding
    w, h, nf = 320, 240, 500
    pairs = _mixed_batch(w, h)
    p = _params(oracle, nf)
    second = [(name + "_swapped", (r, l)) for name, (l, r) in pairs[::-1]]
    seen = Counter()
    with _ctx(binding, nf, max_batch=2 * len(pairs)) as ctx:
        for call, batch in enumerate((pairs, second)):
            frames = np.stack([np.ascontiguousarray(e) for _, (l, r) in batch for e in (l, r)])
            got = _stereo_batch(ctx, frames, [500.0, 12.0])
            for fx in (500.0, 12.0):
                for i, (name, (l, r)) in enumerate(batch):
                    (kL, dL, kR, dR, pts, summ), st = _reference(oracle, l, r, p, fx)
                    _check(f"call {call} pair {i} ({name}) fx {fx}", got[fx][0][i], got[fx][1][i], pts, summ)
                    if name.startswith("flat"):
                        assert summ["n_left"] == 0 or summ["n_right"] == 0
                        assert summ["n_matched"] == 0 and summ["sad_median"] == -1 and summ["status"] == 0
                    if call == 0 and fx == 500.0:
                        seen.update(st)
                        seen["depth"] += summ["n_depth"]
    print(dict(seen))
    # the tie-heavy content reaches the branches the parallax pairs do not
    assert seen["slide_end"] > 0 and seen["median_cut"] > 0 and seen["depth"] > 100 and seen["disp_negative"] + seen["disp_reject"] > 0


def test_a_flagged_eye_voids_its_pair_only(oracle, monkeypatch):
    """A frame the kernels flag (frame_error -> SS_ERR_OVERFLOW) in either eye voids its pair: status, all rows "none", zero
    counts; the neighbours are untouched.  The flags come from the test hook SENDSLAM_TEST_STEREO_FLAG (nothing overflows on
    the device)."""
    from send_slam_amd import binding
    w, h, nf = 320, 240, 500
    monkeypatch.setenv("SENDSLAM_TEST_STEREO_FLAG", "2,7")  # the left eye of pair 1, the right eye of pair 3
    pairs = [_parallax_pair(w, h, 3, 11), _parallax_pair(w, h, 2, 12), _parallax_pair(w, h, 4, 13), _parallax_pair(w, h, 3, 14)]
    p = _params(oracle, nf)
    with _ctx(binding, nf, max_batch=8) as ctx:
        got = _stereo_batch(ctx, np.stack([e for pr in pairs for e in pr]), [500.0])[500.0]
    for i, (l, r) in enumerate(pairs):
        (kL, dL, kR, dR, pts, summ), st = _reference(oracle, l, r, p, 500.0)
        assert summ["n_depth"] > 50
        if i in (1, 3):
            want = dict.fromkeys(R.SUMMARY_FIELDS, 0)
            want.update(status=binding.SS_ERR_OVERFLOW, sad_median=-1)
            assert {k: int(got[1][i][k]) for k in R.SUMMARY_FIELDS} == want
            assert got[0][i].tobytes() == R.none_points(len(got[0][i])).tobytes()
        else:
            _check(f"pair {i} next to a voided one", got[0][i], got[1][i], pts, summ)


def test_extract_stereo_host_path(oracle):
    """host pixels in, both eyes' features and the points out: features equal the oracle's, points the reference's; a second
    pair on the same context; fx / baseline / th_depth come from the camera's calibration"""
    from send_slam_amd import binding
    w, h, nf = 640, 480, 1000
    p = _params(oracle, nf)
    cases = [_parallax_pair(w, h, 4, 7), tuple(np.ascontiguousarray(e) for e in _pattern_pairs(w, h)["checker16_dx6"]), _parallax_pair(w, h, 2, 9)]
    with _ctx(binding, nf) as ctx:
        cam = binding.Camera(type=b"PinHole", fx=500.0, fy=500.0, cx=w / 2, cy=h / 2, width=w, height=h, fps=30.0, th_depth=TH_DEPTH,
                             baseline=BASELINE)
        ctx.set_calibration(3, cam)
        for i, (left, right) in enumerate(cases):
            kL, dL, kR, dR, pts, summ = ctx.extract_stereo(left, right, camera_id=3, timestamp=float(i))
            (okL, odL, okR, odR, opts, osumm), st = _reference(oracle, left, right, p, 500.0)
            assert kL.tobytes() == okL.tobytes() and np.array_equal(dL, odL), f"pair {i}: left features"
            assert kR.tobytes() == okR.tobytes() and np.array_equal(dR, odR), f"pair {i}: right features"
            assert len(pts) == len(okL)
            _check(f"extract_stereo pair {i}", pts, summ, opts, osumm)
            assert osumm["n_depth"] > 50


def test_argument_checks_leave_the_context_usable(oracle):
    import torch
    from send_slam_amd import binding
    w, h, nf = 320, 240, 500
    left, right = _parallax_pair(w, h, 3, 11)
    dev = torch.device("cuda:0")

    def fails(code, fn):
        with pytest.raises(binding.OrbError) as e:
            fn()
        assert e.value.code == code and e.value.message, (e.value.code, e.value.message)

    with _ctx(binding, nf, max_batch=3) as ctx:
        fails(binding.SS_ERR_NOT_CALIBRATED, lambda: ctx.extract_stereo(left, right, camera_id=1))
        d = torch.from_numpy(np.stack([left, right, left])).to(dev)
        ctx.extract_batch_device(d.data_ptr(), 3, w, h)
        kcap = ctx.batch_view().kp_capacity
        d_pts = torch.zeros((2, kcap, 16), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
        fails(binding.SS_ERR_INVALID_ARG, lambda: ctx.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), 500.0, BASELINE))  # odd batch
        ctx.extract_batch_device(d.data_ptr(), 2, w, h)
        for fx, b, th in ((500.0, 0.0, 35.0), (0.0, 0.1, 35.0), (-1.0, 0.1, 35.0), (float("nan"), 0.1, 35.0), (500.0, float("inf"), 35.0),
                          (500.0, 0.1, float("nan"))):
            fails(binding.SS_ERR_INVALID_ARG, lambda: ctx.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), fx, b, th))
        cam = binding.Camera(type=b"PinHole", fx=500.0, fy=500.0, cx=w / 2, cy=h / 2, width=w, height=h, fps=30.0, th_depth=TH_DEPTH, baseline=0.0)
        ctx.set_calibration(1, cam)
        fails(binding.SS_ERR_INVALID_ARG, lambda: ctx.extract_stereo(left, right, camera_id=1))  # a monocular calibration
        cam.baseline = BASELINE
        ctx.set_calibration(1, cam)
        fails(binding.SS_ERR_NOT_CALIBRATED, lambda: ctx.extract_stereo(left, right, camera_id=2))  # another camera has none
        # still usable, and right
        kL, dL, kR, dR, pts, summ = ctx.extract_stereo(left, right, camera_id=1)
        (okL, odL, okR, odR, opts, osumm), st = _reference(oracle, left, right, _params(oracle, nf), 500.0)
        _check("after the failed calls", pts, summ, opts, osumm)
    with _ctx(binding, nf, max_batch=1) as ctx:
        cam = binding.Camera(type=b"PinHole", fx=500.0, fy=500.0, cx=w / 2, cy=h / 2, width=w, height=h, fps=30.0, th_depth=TH_DEPTH,
                             baseline=BASELINE)
        ctx.set_calibration(1, cam)
        fails(binding.SS_ERR_INVALID_ARG, lambda: ctx.extract_stereo(left, right, camera_id=1))  # both eyes are one batch
        kps, desc, counts = ctx.extract(left)
        assert len(kps) > 100
