"""GPU parity of the rectification stage (ss_rectify_set_map, ss_rectify_batch_device, ss_extract_stereo_raw) against
tests/rectify_ref.py: every remapped byte equal, no tolerance; the chain into extraction and stereo depth against
tests/stereo_ref.py on the reference-rectified pair, bit for bit.

That the rotated maps can fail was tried once on an MI355X with a one-line variant of k_rectify built outside lib/ (selected by
SENDSLAM_LIB; not committed):
  the third chunk register is never stored     -> the three cases of test_rotated_maps_mix_every_form_of_the_staging alone fail,
  (no `box[16 * (tid + 512)] = st2`)              in their staged runs, in the tiles whose box is above 8192 B: 1919 bytes of
                                                 frame 0 differ on 640 x 484 gray (first at row 67, column 255), 80 with 3
                                                 channels, 1255 with 4; the other 12 tests of this file pass, as no box of
                                                 theirs is above 6144 B.
"""
import functools
from collections import Counter

import numpy as np
import pytest

import rectify_ref as R
import stereo_ref

pytestmark = pytest.mark.gpu

FILL = 0xAB
BASELINE, TH_DEPTH, FX = 0.1, 35.0, 500.0


@functools.lru_cache(maxsize=None)
def _maps(name):
    """the reference's float maps of the named test model, computed once"""
    m = {"A": R.model_a, "E": R.model_e, "I": lambda: R.identity(320, 240), "A_small": lambda: R.scaled(R.model_a(), 97, 61),
         "A_hd": lambda: R.scaled(R.model_a(), 1280, 720, focal=4.0), "I_hd": lambda: R.identity(1280, 720)}[name]()
    return m, R.build_map(m)


def _random(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=shape, dtype=np.uint8)


def _ctx(binding, max_batch=8, nf=500):
    return binding.OrbContext(0, n_features=nf, lapping_x0=0, lapping_x1=0, max_batch=max_batch)


def _set_model(ctx, binding, map_id, name):
    ctx.set_rectify_model(map_id, binding.rectify_model(**_maps(name)[0]))


def _remap(ctx, frames, ids, row_stride=None, dst_row_stride=None, dst_offset=0, staged=None):
    """frames [n, h, w] or [n, h, w, c] -> (result [n, h, w(, c)], the whole destination buffer as the device left it);
    staged: when given, whether the source must meet the alignment rule of the kernel's LDS form"""
    import torch
    dev = torch.device("cuda:0")
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else frames.shape[3]
    rs = w * ch if row_stride is None else row_stride
    drs = w * ch if dst_row_stride is None else dst_row_stride
    src = np.full((n, h, rs), 0x5C, np.uint8)
    src[:, :, :w * ch] = frames.reshape(n, h, w * ch)
    d_src = torch.from_numpy(src).to(dev)
    if staged is not None:
        assert ((d_src.data_ptr() | rs | (rs * h) | (w * ch)) % 16 == 0) == staged
    d_dst = torch.full((dst_offset + n * h * drs,), FILL, dtype=torch.uint8, device=dev)
    ctx.rectify_batch_device(d_src.data_ptr(), n, w, h, ids, d_dst.data_ptr() + dst_offset, channels=ch, row_stride=rs, frame_stride=rs * h,
                             dst_row_stride=drs, dst_frame_stride=drs * h)
    ctx.synchronize()
    whole = d_dst.cpu().numpy()
    rows = whole[dst_offset:].reshape(n, h, drs)
    assert (whole[:dst_offset] == FILL).all() and (rows[:, :, w * ch:] == FILL).all(), "bytes outside the destination rows were written"
    return rows[:, :, :w * ch].reshape(frames.shape).copy(), whole


def _same(tag, got, want):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{tag}: {len(bad)} bytes differ, first at {bad[:4].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def test_batch_with_shared_maps():
    """five frames on three maps, the maps built by the library: every frame equals the reference, the padding of the
    destination rows is untouched, the stage reports its algorithmic bytes"""
    from send_slam_amd import binding
    w, h, ids = 320, 240, [0, 1, 0, 2, 1]
    names = {0: "A", 1: "I", 2: "E"}
    frames = _random((5, h, w), 21)
    with _ctx(binding) as ctx:
        for i, name in names.items():
            _set_model(ctx, binding, i, name)
        ctx.profile(True)
        got, _ = _remap(ctx, frames, ids, dst_row_stride=336)
        row = [s for s in ctx.stats() if s["name"] == "rectify"]
    for f, i in enumerate(ids):
        _same(f"frame {f} map {names[i]}", got[f], R.remap(frames[f], *_maps(names[i])[1]))
    _same("identity", got[1], frames[1])
    assert len(row) == 1 and row[0]["launches"] == 1 and row[0]["algorithmic_bytes"] == 5 * w * h * 2 + 3 * w * h * 6


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_odd_shapes_and_channels(ch):
    """97 x 61: narrower than a tile, no multiple of four either way; padded source rows, an unaligned destination stride
    (rows start at every alignment) and an unaligned destination base"""
    from send_slam_amd import binding
    w, h = 97, 61
    frames = _random((3, h, w) if ch == 1 else (3, h, w, ch), 30 + ch)
    mx, my = _maps("A_small")[1]
    with _ctx(binding) as ctx:
        ctx.set_rectify_map(3, mx, my)
        got, _ = _remap(ctx, frames, [3, 3, 3], row_stride=101 * ch, dst_row_stride=w * ch + 3)
        got1, _ = _remap(ctx, frames, [3, 3, 3], row_stride=101 * ch, dst_row_stride=w * ch + 4, dst_offset=1)
    cls = R.tap_classes(mx, my)
    assert (cls == 0).any() and (cls == 4).any() and ((cls > 0) & (cls < 4)).any()
    for f in range(3):
        want = R.remap(frames[f], mx, my)
        _same(f"channels {ch} frame {f}", got[f], want)
        _same(f"channels {ch} frame {f}, unaligned base", got1[f], want)


def _crafted_weights_map(w, h):
    """pixel (b, a) of the top-left 32 x 32 block maps to (3 + a / 32, 5 + b / 32): each of the 1024 (a, b) pairs once.  A map has
    the size of its frames, so the block sits in a map of the source's size; the rest of it is the identity"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    a, b = np.meshgrid(np.arange(32, dtype=np.float32), np.arange(32, dtype=np.float32))
    x[:32, :32] = np.float32(3) + a / np.float32(32)
    y[:32, :32] = np.float32(5) + b / np.float32(32)
    return x, y


def _crafted_edge_map(w, h):
    """the values of the CPU conversion test along all four edges and in the corners"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))

    def vals(n):
        return np.array([-1, -1 + 1 / 32, n - 1, n - 1 + 1 / 64, n, np.nan, np.inf, -np.inf, 1e30, -1e30, 40000, -0.0, 0.5], np.float32)

    k = len(vals(w))
    for row in (0, 1, h - 2, h - 1):  # x runs through the values on the top and bottom rows ...
        x[row, :k] = vals(w)
        x[row, w - k:] = vals(w)[::-1]
    for col in (0, 1, w - 2, w - 1):  # ... y down the left and right columns, so the corners get both
        y[:k, col] = vals(h)
        y[h - k:, col] = vals(h)[::-1]
    return x, y


@pytest.mark.parametrize("ch,size", [(1, 40), (3, 40), (1, 48), (3, 48)])
def test_every_weight_and_every_edge(ch, size):
    """40 x 40: rows of 40 (120) bytes, which the kernel gathers tap by tap; 48 x 48: rows of whole 16-byte chunks, which it
    stages in LDS"""
    from send_slam_amd import binding
    w = h = size
    frames = _random((2, h, w) if ch == 1 else (2, h, w, ch), 40 + ch) | 1  # no zero byte: a tap wrongly taken as border shows
    wx, wy = _crafted_weights_map(w, h)
    _, a = R.to_fixed(wx[:32, :32])
    _, b = R.to_fixed(wy[:32, :32])
    assert len(set((a * 32 + b).ravel().tolist())) == 1024
    ex, ey = _crafted_edge_map(w, h)
    cls = R.tap_classes(ex, ey)
    assert {0, 1, 2, 4} <= set(cls.ravel().tolist())
    with _ctx(binding) as ctx:
        ctx.set_rectify_map(0, wx, wy)
        ctx.set_rectify_map(15, ex, ey)
        got, _ = _remap(ctx, frames, [0, 15])
    _same("every weight", got[0], R.remap(frames[0], wx, wy))
    _same("every edge", got[1], R.remap(frames[1], ex, ey))


def test_a_map_without_any_smoothness():
    """every destination pixel reads a random source position, a tenth of them outside the image: the taps of a tile span the
    whole frame (the box a workgroup would stage does not fit), and neighbouring lanes read unrelated bytes"""
    from send_slam_amd import binding
    w, h = 320, 240
    rng = np.random.Generator(np.random.PCG64(70))
    mx = rng.uniform(-20, w + 20, size=(h, w)).astype(np.float32)
    my = rng.uniform(-20, h + 20, size=(h, w)).astype(np.float32)
    frames = _random((2, h, w), 71)
    with _ctx(binding) as ctx:
        ctx.set_rectify_map(0, mx, my)
        ctx.set_rectify_map(1, *_maps("E")[1])
        got, _ = _remap(ctx, frames, [0, 1])
    cls = R.tap_classes(mx, my)
    assert (cls == 0).mean() > 0.05 and (cls == 4).mean() > 0.5
    _same("scrambled", got[0], R.remap(frames[0], mx, my))
    _same("its neighbour", got[1], R.remap(frames[1], *_maps("E")[1]))


@pytest.mark.parametrize("w,h,degrees,ch", [(640, 484, 45, 1), (336, 61, 8, 3), (336, 61, 8, 4)])
def test_rotated_maps_mix_every_form_of_the_staging(w, h, degrees, ch):
    """A rotation about the centre (45 degrees on 640 x 484 gray, 8 degrees on 336 x 61 with 3 and 4 channels): in ONE staged
    launch tiles without a tap, tiles of two chunks per lane, tiles that fill the third chunk register (8193 - 10240 B) and
    tiles that fall back to the gather loop (tests/test_rectify_ref.py counts them), a height that is no multiple of 8 and,
    with colour, a width that is no multiple of 128, so lanes without a pixel take part in the staging.  Three frames: the
    frame loop and the prefetch of the next box run; the gray batch has an identity frame in the middle.  Then the same
    frames onto a destination of stride w * ch + 3 at base offset 1, and with source rows 4 bytes longer, which takes the
    gather form: the same bytes."""
    from send_slam_amd import binding
    mx, my = R.rotation_map(w, h, degrees)
    maps = {0: (mx, my), 1: R.identity_map(w, h)}
    ids = [0, 1, 0] if ch == 1 else [0, 0, 0]
    frames = _random((3, h, w) if ch == 1 else (3, h, w, ch), 80 + ch) | 1  # no zero byte: a tap wrongly taken as border shows
    want = [R.remap(frames[f], *maps[i]) for f, i in enumerate(ids)]
    with _ctx(binding) as ctx:
        for i, m in maps.items():
            ctx.set_rectify_map(i, *m)
        runs = {"staged": _remap(ctx, frames, ids, staged=True)[0],
                "staged, unaligned destination": _remap(ctx, frames, ids, dst_row_stride=w * ch + 3, dst_offset=1, staged=True)[0],
                "gathered": _remap(ctx, frames, ids, row_stride=w * ch + 4, staged=False)[0],
                "gathered, unaligned destination": _remap(ctx, frames, ids, row_stride=w * ch + 4, dst_row_stride=w * ch + 3, dst_offset=1,
                                                          staged=False)[0]}
    for tag, got in runs.items():
        for f in range(3):
            _same(f"{w} x {h} x {ch} frame {f}, {tag}", got[f], want[f])
    assert not np.array_equal(want[0], frames[0]) and (ch > 1 or np.array_equal(want[1], frames[1]))


def test_state_and_argument_checks():
    import torch
    from send_slam_amd import binding
    dev = torch.device("cuda:0")
    big, small = _random((2, 240, 320), 50), _random((2, 61, 97), 51)
    (_, (ax, ay)), (_, (sx, sy)) = _maps("A"), _maps("A_small")

    def fails(fn):
        with pytest.raises(binding.OrbError) as e:
            fn()
        assert e.value.code == binding.SS_ERR_INVALID_ARG and e.value.message, (e.value.code, e.value.message)

    with _ctx(binding, max_batch=2) as ctx:
        ctx.set_rectify_map(5, ax, ay)
        got, _ = _remap(ctx, big, [5, 5])
        _same("first map", got[1], R.remap(big[1], ax, ay))
        ctx.set_rectify_map(5, sx, sy)  # replaced by a map of another size: the next call follows the new one
        got, _ = _remap(ctx, small, [5, 5])
        _same("replaced map", got[0], R.remap(small[0], sx, sy))
        ctx.set_rectify_map(6, ax, ay)

        w, h = 320, 240
        d_src = torch.from_numpy(np.concatenate([big, big])).to(dev)  # four frames: room for an overlapping destination
        d_dst = torch.full((3 * h * w,), FILL, dtype=torch.uint8, device=dev)

        def call(n=2, ids=(6, 6), dst=None, drs=w, dfs=w * h, width=w, height=h):
            ctx.rectify_batch_device(d_src.data_ptr(), n, width, height, list(ids), d_dst.data_ptr() if dst is None else dst,
                                     dst_row_stride=drs, dst_frame_stride=dfs)

        fails(lambda: call(ids=(6, 16)))                         # an id out of range
        fails(lambda: call(ids=(-1, 6)))
        fails(lambda: call(ids=(6, 7)))                          # an unset map
        fails(lambda: call(ids=(6, 5)))                          # map 5 is 97 x 61 now
        fails(lambda: call(dst=d_src.data_ptr()))                # in place
        fails(lambda: call(dst=d_src.data_ptr() + 2 * w * h - 1))  # the last source byte is the first destination byte
        fails(lambda: call(dst=d_src.data_ptr() + w))             # shifted by one row
        fails(lambda: call(drs=w - 1))                           # a destination row stride smaller than a row
        fails(lambda: call(dfs=w * h - 1))                       # a destination frame stride smaller than a frame
        fails(lambda: call(n=3, ids=(6, 6, 6)))                  # n_frames > max_batch
        ctx.set_rectify_map(6, None, None)                       # dropped
        fails(lambda: call())
        fails(lambda: ctx.set_rectify_map(16, ax, ay))
        ctx.synchronize()
        assert (d_dst.cpu().numpy() == FILL).all() and np.array_equal(d_src.cpu().numpy()[:2], big), "a refused call wrote something"
        # the destination right behind the source is no overlap; the context is still usable, and right
        ctx.set_rectify_map(6, ax, ay)
        call(dst=d_src.data_ptr() + 2 * w * h)
        ctx.synchronize()
        out = d_src.cpu().numpy()
        _same("after the refused calls", out[2], R.remap(big[0], ax, ay))
        left, right = R.end_to_end_pair()
        fails(lambda: ctx.extract_stereo_raw(left, right, 6, 9, FX, BASELINE))   # map 9 is unset
        fails(lambda: ctx.extract_stereo_raw(left, right, 6, 6, FX, 0.0))        # the stereo parameters are checked
    with _ctx(binding, max_batch=1) as ctx:
        ctx.set_rectify_map(0, ax, ay)
        left, right = R.end_to_end_pair()
        fails(lambda: ctx.extract_stereo_raw(left, right, 0, 0, FX, BASELINE))   # both eyes are one batch


def _check(tag, got_pts, got_sum, want_pts, want_sum):
    """the comparison of tests/test_stereo.py: got_pts may hold more rows than the left eye has keypoints, the rest is "none" """
    n = len(want_pts)
    got = {k: int(got_sum[k]) for k in stereo_ref.SUMMARY_FIELDS} if not isinstance(got_sum, dict) else got_sum
    print(tag, got)
    assert got["n_left"] == want_sum["n_left"] and got["n_right"] == want_sum["n_right"], f"{tag}: extraction differs {got} {want_sum}"
    for f in ("right_idx", "orb_dist", "sad"):
        bad = np.flatnonzero(got_pts[f][:n] != want_pts[f])
        assert len(bad) == 0, f"{tag}: {f} differs at rows {bad[:8]}: {got_pts[f][:n][bad[:8]]} != {want_pts[f][bad[:8]]}"
    for f in ("u_right", "depth"):
        a, b = np.ascontiguousarray(got_pts[f][:n]).view(np.uint32), np.ascontiguousarray(want_pts[f]).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{tag}: {f} differs at rows {bad[:8]}: {got_pts[f][:n][bad[:8]]} != {want_pts[f][bad[:8]]}"
    assert got_pts[n:].tobytes() == stereo_ref.none_points(len(got_pts) - n).tobytes(), f"{tag}: rows past the left keypoints are not 'none'"
    assert got == want_sum, f"{tag}: summary {got} != {want_sum}"


def test_chain_into_extraction_and_stereo(oracle):
    """raw pair -> remap into a 16-byte aligned device buffer -> ss_extract_batch_device (level 0 in place) ->
    ss_stereo_batch_device, against the reference on the reference-rectified pair; then ss_extract_stereo_raw on the same host
    pixels, gray (no calibration) and as a 3-channel copy (against ss_extract_stereo on the reference-rectified colour pair)"""
    import torch
    from send_slam_amd import binding
    dev = torch.device("cuda:0")
    w, h, nf = 320, 240, 500
    left, right = R.end_to_end_pair(w, h)
    mx, my = _maps("E")[1]
    rl, rr = R.remap(left, mx, my), R.remap(right, mx, my)
    p = oracle.default_params(n_features=nf, lapping_x0=0, lapping_x1=0)
    st = Counter()
    okL, odL, okR, odR, opts, osumm = stereo_ref.stereo_pair(rl, rr, p, FX, BASELINE, TH_DEPTH, st)
    assert st["guard"] == 0 and osumm["n_depth"] >= 0.4 * osumm["n_left"] > 0
    with _ctx(binding, max_batch=2, nf=nf) as ctx:
        _set_model(ctx, binding, 2, "E")
        _set_model(ctx, binding, 3, "E")
        d_raw = torch.from_numpy(np.stack([left, right])).to(dev)
        d_rect = torch.full((2, h, w), FILL, dtype=torch.uint8, device=dev)
        assert d_rect.data_ptr() % 16 == 0 and w % 16 == 0
        ctx.rectify_batch_device(d_raw.data_ptr(), 2, w, h, [2, 3], d_rect.data_ptr())
        ctx.extract_batch_device(d_rect.data_ptr(), 2, w, h)
        kcap = ctx.batch_view().kp_capacity
        d_pts = torch.full((kcap, binding.STEREO_POINT_DTYPE.itemsize), FILL, dtype=torch.uint8, device=dev)
        d_sum = torch.full((binding.STEREO_SUMMARY_DTYPE.itemsize,), FILL, dtype=torch.uint8, device=dev)
        ctx.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), FX, BASELINE, TH_DEPTH)
        ctx.synchronize()
        rect = d_rect.cpu().numpy()
        _same("rectified left", rect[0], rl)
        _same("rectified right", rect[1], rr)
        kL, dL, _ = ctx.fetch_frame(0)
        assert kL.tobytes() == okL.tobytes() and np.array_equal(dL, odL)
        _check("chain", d_pts.cpu().numpy().copy().view(binding.STEREO_POINT_DTYPE).reshape(kcap),
               d_sum.cpu().numpy().copy().view(binding.STEREO_SUMMARY_DTYPE)[0], opts, osumm)

        # one call, gray: no calibration has been set on this context
        kL, dL, kR, dR, pts, summ = ctx.extract_stereo_raw(left, right, 2, 3, FX, BASELINE, TH_DEPTH, camera_id=4, timestamp=1.0)
        assert kL.tobytes() == okL.tobytes() and np.array_equal(dL, odL), "left features"
        assert kR.tobytes() == okR.tobytes() and np.array_equal(dR, odR), "right features"
        assert len(pts) == len(okL)
        _check("extract_stereo_raw", pts, summ, opts, osumm)

        # colour: remapped before the gray conversion, as upstream does
        left3, right3 = (np.ascontiguousarray(np.repeat(e[:, :, None], 3, axis=2)) for e in (left, right))
        with pytest.raises(binding.OrbError) as e:
            ctx.extract_stereo_raw(left3, right3, 2, 3, FX, BASELINE, TH_DEPTH, camera_id=4)
        assert e.value.code == binding.SS_ERR_NOT_CALIBRATED  # ss_extract's rule for colour frames
        cam = binding.Camera(type=b"PinHole", fx=FX, fy=FX, cx=w / 2, cy=h / 2, width=w, height=h, fps=30.0, rgb=1, th_depth=TH_DEPTH,
                             baseline=BASELINE)
        ctx.set_calibration(4, cam)
        raw3 = ctx.extract_stereo_raw(left3, right3, 2, 3, FX, BASELINE, TH_DEPTH, camera_id=4)
        want3 = ctx.extract_stereo(R.remap(left3, mx, my), R.remap(right3, mx, my), camera_id=4)
        for i, (g, wnt) in enumerate(zip(raw3[:5], want3[:5])):
            assert g.tobytes() == wnt.tobytes(), f"3-channel pair: output {i} differs"
        assert raw3[5] == want3[5] and raw3[5]["n_depth"] > 50


def test_one_full_size_batch():
    """1280 x 720, four frames on two maps: many tiles per row, many blocks, the frame loop of each map longer than one"""
    from send_slam_amd import binding
    w, h, ids = 1280, 720, [0, 1, 1, 0]
    frames = _random((4, h, w), 60)
    with _ctx(binding) as ctx:
        _set_model(ctx, binding, 0, "A_hd")
        _set_model(ctx, binding, 1, "I_hd")
        got, _ = _remap(ctx, frames, ids)
    want_a = [R.remap(frames[f], *_maps("A_hd")[1]) for f in (0, 3)]
    _same("frame 0", got[0], want_a[0])
    _same("frame 3", got[3], want_a[1])
    _same("frame 1", got[1], frames[1])
    _same("frame 2", got[2], frames[2])
    assert not np.array_equal(want_a[0], frames[0])
