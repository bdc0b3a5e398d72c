"""GPU parity of Frame's keypoint post-processing (ss_undistort_pairs_device, ss_undistort_batch_device, ss_get_batch_raw_xy,
ss_depth_pairs_device, ss_depth_batch_device) against the host twins, bit for bit (non-finite positions by value), and of the batch
searches on a batch that was undistorted in place against the pairs forms and tests/guided_ref.py on host-undistorted keypoints."""
import numpy as np
import pytest

import guided_cases as G
import guided_ref as R
import proj_cases as PC
import proj_ref as P
import undistort_cases as UC
import undistort_ref as UR

pytestmark = pytest.mark.gpu

BATCH = ["synth_t0", "synth_t1", "synth_t2"]
KP_BYTES = 24


def _torch():
    import torch
    return torch


def _to_dev(a):
    a = np.ascontiguousarray(a)
    t = _torch().from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to("cuda:0")
    _torch().cuda.synchronize()  # the library's stream does not wait for torch's
    return t


def _filled(shape, dtype=None):
    """a device array of UC.PATTERN bytes"""
    torch = _torch()
    t = torch.full(shape, UC.PATTERN, dtype=torch.uint8 if dtype is None else dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _kp_of(t, n, rows):
    from send_slam_amd import binding
    return t.cpu().numpy().copy().view(binding.KP_DTYPE).reshape(n, rows)


def dev_bytes(ptr, nbytes):
    """host copy of `nbytes` of device memory at the raw address `ptr`"""
    class _Wrap:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return _torch().as_tensor(_Wrap(), device="cuda:0").cpu().numpy().copy()


def same_kp(tag, got, want):
    """x and y bit for bit where finite, by value (NaN equals NaN) where not; every other field, and every row, by its bytes"""
    got, want = got.reshape(-1), want.reshape(-1)
    assert len(got) == len(want), tag
    for f in ("x", "y"):
        g, w = got[f], want[f]
        odd = ~np.isfinite(w)
        assert np.array_equal(g[odd], w[odd], equal_nan=True), f"{tag}: non-finite {f} differs"
        bad = np.flatnonzero(g[~odd].view(np.int32) != w[~odd].view(np.int32))
        assert len(bad) == 0, f"{tag}: {f} differs at {len(bad)} rows, first {bad[:6]}: {g[~odd][bad[:6]]} != {w[~odd][bad[:6]]}"
    for f in ("size", "angle", "response", "octave"):
        assert got[f].tobytes() == want[f].tobytes(), f"{tag}: {f} was touched"


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(BATCH)) as c:
        yield c


def _cams(names):
    return [UC.camera(n) for n in names]


# ---- the pairs form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_names", [UC.FRAME_CAMERAS, ["D"], ["P"]], ids=["camera_per_frame", "one_camera", "pincushion"])
@pytest.mark.parametrize("counts", [UC.COUNTS, [200, -3, 69]], ids=["counts_70_1_0", "counts_past_the_rows_and_below_0"])
def test_pairs_form(ctx, cam_names, counts):
    """3 frames x 70 rows (one wave plus six lanes): rows below the clamped count are the twin's, the rest keep the prefill"""
    kp, cams = UC.frames_case(), _cams(cam_names)
    d_kp, d_n = _to_dev(kp), _to_dev(np.array(counts, np.int32))
    d_out = _filled((UC.F, UC.ROWS * KP_BYTES))
    ctx.undistort_pairs_device(d_kp.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS, cams if len(cams) > 1 else cams[0], d_out.data_ptr())
    ctx.synchronize()
    got = _kp_of(d_out, UC.F, UC.ROWS)
    pattern = np.frombuffer(bytes([UC.PATTERN]) * (UC.F * UC.ROWS * KP_BYTES), got.dtype).reshape(UC.F, UC.ROWS)
    want = UC.twin_frames(kp, counts, cams, pattern)
    for b in range(UC.F):
        n = UC.clamp(counts[b])
        same_kp(f"frame {b}", got[b, :n], want[b, :n])
        assert got[b, n:].tobytes() == pattern[b, n:].tobytes(), f"frame {b}: rows past the count were written"
    assert _kp_of(d_kp, UC.F, UC.ROWS).tobytes() == kp.tobytes(), "the input was written"
    moved = np.abs(got[0]["x"][:20] - kp[0]["x"][:20]).max()
    assert moved > 5.0, moved  # cameras D and P move the corners by tens of pixels


def test_pairs_form_in_place(ctx):
    """d_kp_out == d_kp: x and y of the live rows only"""
    kp, cams = UC.frames_case(), _cams(UC.FRAME_CAMERAS)
    d_kp, d_n = _to_dev(kp), _to_dev(np.array(UC.COUNTS, np.int32))
    ctx.undistort_pairs_device(d_kp.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS, cams, d_kp.data_ptr())
    ctx.synchronize()
    got, want = _kp_of(d_kp, UC.F, UC.ROWS), UC.twin_frames(kp, UC.COUNTS, cams)
    for b in range(UC.F):
        n = UC.clamp(UC.COUNTS[b])
        same_kp(f"frame {b}", got[b, :n], want[b, :n])
        assert got[b, n:].tobytes() == kp[b, n:].tobytes()


def test_pairs_form_refusals(ctx):
    from send_slam_amd import binding
    kp = UC.frames_case()
    d_kp, d_n = _to_dev(kp), _to_dev(np.array(UC.COUNTS, np.int32))
    d_out = _filled((UC.F, UC.ROWS * KP_BYTES))
    before = d_out.cpu().numpy().copy()
    a = (d_kp.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS)
    for cams, word in ((_cams(["D", "Z"]), "n_cams"), (UC.camera("D", fx=0.0), "fx and fy"), (UC.camera("D", fy=float("nan")), "fx and fy"), (None, "cams is NULL")):
        with pytest.raises(binding.OrbError) as e:
            ctx.undistort_pairs_device(*a, cams, d_out.data_ptr())
        assert e.value.code == binding.SS_ERR_INVALID_ARG and word in e.value.message, e.value.message
    with pytest.raises(binding.OrbError) as e:
        ctx.undistort_pairs_device(d_kp.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS, UC.camera("D"), 0)
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    ctx.undistort_pairs_device(d_kp.data_ptr(), d_n.data_ptr(), 0, UC.ROWS, UC.camera("D"), d_out.data_ptr())  # no frames: nothing to do
    ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), before)


# ---- the batch form ----------------------------------------------------------------------------------------------------------------
def _extract(c, names):
    """the named frames as one batch -> (pixels kept alive, kcap, [(kp, desc)] as fetched)"""
    frames = np.stack([G.frame(n) for n in names])
    d = _to_dev(frames)
    c.extract_batch_device(d.data_ptr(), len(names), G.W, G.H)
    c.synchronize()
    return d, c.batch_view().kp_capacity, [c.fetch_frame(b)[:2] for b in range(len(names))]


def _raw_batch(c, n):
    v = c.batch_view()
    from send_slam_amd import binding
    return dev_bytes(v.keypoints, n * v.kp_capacity * KP_BYTES).view(binding.KP_DTYPE).reshape(n, v.kp_capacity)


@pytest.mark.parametrize("names", [BATCH, ["synth_t0", "flat", "synth_t1"]], ids=["three_frames", "an_empty_frame"])
def test_batch_form(names):
    from send_slam_amd import binding
    cam, n = UC.camera("D"), len(names)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        with pytest.raises(binding.OrbError) as e:  # no batch yet
            c.undistort_batch_device(cam)
        assert e.value.code == binding.SS_ERR_STATE
        pixels, kcap, raw = _extract(c, names)
        counts = [len(k) for k, _ in raw]
        assert counts[0] > 300 and (names[1] != "flat" or counts[1] == 0)
        with pytest.raises(binding.OrbError) as e:
            c.undistort_batch_device()  # cams NULL and no calibration
        assert e.value.code == binding.SS_ERR_NOT_CALIBRATED
        with pytest.raises(binding.OrbError) as e:
            c.batch_raw_xy()
        assert e.value.code == binding.SS_ERR_STATE
        all_rows_before = _raw_batch(c, n)
        twin = [binding.undistort_host(cam, k) for k, _ in raw]
        # out of place: the twin on the fetched keypoints, the batch as it was
        d_out = _filled((n, kcap * KP_BYTES))
        c.undistort_batch_device(cam, d_out.data_ptr())
        c.synchronize()
        got = _kp_of(d_out, n, kcap)
        for b in range(n):
            same_kp(f"out of place, frame {b}", got[b, :counts[b]], twin[b])
            assert (got[b, counts[b]:].view(np.uint8) == UC.PATTERN).all()
        assert _raw_batch(c, n).tobytes() == all_rows_before.tobytes()
        with pytest.raises(binding.OrbError) as e:
            c.batch_raw_xy()  # an out-of-place call saves nothing
        assert e.value.code == binding.SS_ERR_STATE
        # in place, through the calibration set last
        c.set_calibration(1, cam)
        c.undistort_batch_device()
        c.synchronize()
        for b in range(n):
            k, d = c.fetch_frame(b)[:2]
            same_kp(f"in place, frame {b}", k, twin[b])
            assert d.tobytes() == raw[b][1].tobytes(), "descriptors changed"
        all_rows_after = _raw_batch(c, n)
        for b in range(n):
            assert all_rows_after[b, counts[b]:].tobytes() == all_rows_before[b, counts[b]:].tobytes(), "rows past the count were written"
        xy = dev_bytes(c.batch_raw_xy(), n * kcap * 8).view(np.float32).reshape(n, kcap, 2)
        for b in range(n):
            assert xy[b, :counts[b], 0].tobytes() == raw[b][0]["x"].tobytes() and xy[b, :counts[b], 1].tobytes() == raw[b][0]["y"].tobytes()
        moved = np.concatenate([np.hypot(t["x"] - k["x"], t["y"] - k["y"]) for t, (k, _) in zip(twin, raw)])
        print("largest shift of a keypoint:", moved.max())
        assert moved.max() > 20.0
        # a second in-place call: refused, nothing written
        with pytest.raises(binding.OrbError) as e:
            c.undistort_batch_device(cam)
        assert e.value.code == binding.SS_ERR_STATE
        c.synchronize()
        assert _raw_batch(c, n).tobytes() == all_rows_after.tobytes()
        assert dev_bytes(c.batch_raw_xy(), n * kcap * 8).tobytes() == xy.tobytes()
        # a new extraction clears the state
        pixels2, _, raw2 = _extract(c, names)
        assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(raw, raw2))
        with pytest.raises(binding.OrbError) as e:
            c.batch_raw_xy()
        assert e.value.code == binding.SS_ERR_STATE
        c.undistort_batch_device([cam] * n)  # a camera per frame
        c.synchronize()
        for b in range(n):
            same_kp(f"in place again, frame {b}", c.fetch_frame(b)[0], twin[b])
        with pytest.raises(binding.OrbError) as e:
            c.undistort_batch_device([cam] * 2, d_out.data_ptr())
        assert e.value.code == binding.SS_ERR_INVALID_ARG
        del pixels, pixels2


def test_zero_coefficients_are_a_bit_copy_in_place():
    """what ss_stereo_batch_device relies on: rectified pairs have zero coefficients"""
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=2) as c:
        pixels, kcap, raw = _extract(c, BATCH[:2])
        before = _raw_batch(c, 2)
        c.undistort_batch_device(UC.camera("Z"))
        c.synchronize()
        assert _raw_batch(c, 2).tobytes() == before.tobytes()
        xy = dev_bytes(c.batch_raw_xy(), 2 * kcap * 8).view(np.float32).reshape(2, kcap, 2)
        for b in range(2):
            n = len(raw[b][0])
            assert xy[b, :n, 0].tobytes() == raw[b][0]["x"].tobytes()
        del pixels


def test_a_flagged_frame_counts_as_no_rows(monkeypatch):
    """SENDSLAM_TEST_FLAG_BATCH=1: frame 1 keeps its raw keypoints in place, and has no depth"""
    from send_slam_amd import binding
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1")
    cam = UC.camera("D")
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        pixels, kcap, raw = _extract(c, BATCH)
        before = _raw_batch(c, 3)
        c.undistort_batch_device(cam)
        c.synchronize()
        after = _raw_batch(c, 3)
        assert after[1].tobytes() == before[1].tobytes()
        for b in (0, 2):
            same_kp(f"frame {b}", after[b, :len(raw[b][0])], binding.undistort_host(cam, raw[b][0]))
        depth = np.full((3, G.H, G.W), 2.0, np.float32)
        d_depth, out = _to_dev(depth), DepthOutputs(3, kcap)
        c.depth_batch_device(binding.depth_params(26.0, 1.0, 3.0, 0), d_depth.data_ptr(), G.W, G.H, G.W * 4, G.W * G.H * 4, *out.ptrs())
        c.synchronize()
        right, dep, summ = out.host()
        assert (dep[1] == -1).all() and (right[1] == -1).all()
        assert [int(summ[1][f]) for f in UR.SUMMARY_FIELDS] == [binding.SS_ERR_OVERFLOW, 0, 0, 0]
        assert int(summ[0]["status"]) == 0 and int(summ[0]["n_kp"]) == len(raw[0][0]) and int(summ[0]["n_depth"]) > 300
        del pixels


# ---- the searches read mvKeysUn ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["D", "W"])
def undistorted_batch(request):
    """BATCH extracted and undistorted in place under camera D or W (UC.search_camera) -> (ctx, kcap, raw features,
    host-undistorted keypoints, camera, whether a good part of the keypoints has left the image)"""
    from send_slam_amd import binding
    cam = UC.search_camera(request.param)
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(BATCH)) as c:
        pixels, kcap, raw = _extract(c, BATCH)
        for b, name in enumerate(BATCH):  # the references are computed on the oracle's features
            okp, odesc = G.features(name)
            assert raw[b][0].tobytes() == okp.tobytes() and np.array_equal(raw[b][1], odesc)
        c.undistort_batch_device(cam)
        c.synchronize()
        un = [binding.undistort_host(cam, k) for k, _ in raw]
        outside = np.concatenate([(t["x"] < 0) | (t["x"] >= G.W) | (t["y"] < 0) | (t["y"] >= G.H) for t in un])
        print("keypoints outside the image after undistortion:", outside.mean())
        assert (outside.mean() > 0.1) == (request.param == "W")
        yield c, kcap, raw, un, cam, request.param == "W"
        del pixels


def test_projection_search_on_the_undistorted_batch(undistorted_batch):
    """ss_match_proj_batch_device after the in-place undistortion returns the bytes of ss_match_proj_pairs_device fed the
    host-undistorted keypoints; the bounds are ss_proj_view_set_bounds's, so points of the undistorted margin are in view"""
    from send_slam_amd import binding
    c, kcap, raw, un, cam, wide = undistorted_batch
    n = len(BATCH)
    rng = np.random.Generator(np.random.PCG64(0x0D15))
    # the map: frame 0's undistorted keypoints back-projected under the camera's intrinsics, seen by all three frames
    pts, _ = PC.back_project(rng, un[0], PC.scale(), cam.fx, cam.fy, cam.cx, cam.cy)
    pd = PC.desc_near(rng, raw[0][1])
    point_rows = len(pts) + 3
    views = [binding.proj_view_set_bounds(binding.proj_view(cam, r, t, bf=26.0), cam) for r, t in PC.POSES]
    narrow = [binding.proj_view(cam, r, t, bf=26.0) for r, t in PC.POSES]
    points = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE)
    p_desc = np.zeros((1, point_rows, 32), np.uint8)
    points[0, :len(pts)], p_desc[0, :len(pts)] = pts, pd
    t_kp, t_desc = np.zeros((n, kcap), binding.KP_DTYPE), np.zeros((n, kcap, 32), np.uint8)
    for b in range(n):
        t_kp[b, :len(un[b])], t_desc[b, :len(un[b])] = un[b], raw[b][1]
    d_pts, d_pd, d_np = _to_dev(points), _to_dev(p_desc), _to_dev(np.array([len(pts)], np.int32))
    d_tkp, d_td, d_nt = _to_dev(t_kp), _to_dev(t_desc), _to_dev(np.array([len(k) for k in un], np.int32))
    params = binding.proj_params(th=3.0, one_to_one=True, extent_w=G.W, extent_h=G.H)

    def outputs():
        o = [_filled((n, point_rows * k)) for k in (4, 2, 2, 32)] + [_filled((n, 32))]
        return o, [t.data_ptr() for t in o]

    pairs, pairs_ptrs = outputs()
    c.match_proj_pairs_device(d_pts.data_ptr(), d_pd.data_ptr(), d_np.data_ptr(), 1, point_rows, d_td.data_ptr(), d_tkp.data_ptr(), d_nt.data_ptr(), n, kcap,
                              views, params, *pairs_ptrs, point_src=[0] * n)
    batch, batch_ptrs = outputs()
    c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_np.data_ptr(), 1, point_rows, views, params, *batch_ptrs, point_src=[0] * n)
    inside, inside_ptrs = outputs()
    c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_np.data_ptr(), 1, point_rows, narrow, params, *inside_ptrs, point_src=[0] * n)
    c.synchronize()
    for name, a, b in zip(("idx", "d1", "d2", "proj", "summary"), pairs, batch):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{name}: the batch form differs from the pairs form on the host-undistorted keypoints"
    summ = batch[4].cpu().numpy().copy().view(binding.PROJ_SUMMARY_DTYPE).reshape(n)
    proj = batch[3].cpu().numpy().copy().view(binding.PROJ_POINT_DTYPE).reshape(n, point_rows)
    idx = batch[0].cpu().numpy().copy().view(np.int32).reshape(n, point_rows)
    print(summ)
    assert int(summ[0]["n_accepted"]) > 100 and int(summ[0]["status"]) == 0
    # points that project into the undistorted margin are in view, and some of them find their keypoint there
    margin = (proj[0]["state"] == 0) & ((proj[0]["u"] < 0) | (proj[0]["u"] > G.W) | (proj[0]["v"] < 0) | (proj[0]["v"] > G.H))
    narrow_summ = inside[4].cpu().numpy().copy().view(binding.PROJ_SUMMARY_DTYPE).reshape(n)
    print("in the margin:", int(margin.sum()), "matched there:", int((idx[0][margin] >= 0).sum()))
    assert int(narrow_summ[0]["n_in_view"]) == int(summ[0]["n_in_view"]) - int(margin.sum())
    if wide:
        assert margin.sum() > 20 and (idx[0][margin] >= 0).sum() > 10
    # against the reference on the undistorted keypoints
    ref_view = P.view_init(cam.fx, cam.fy, cam.cx, cam.cy, G.W, G.H, PC.POSES[0][0], PC.POSES[0][1], 26.0)
    ref_view["min_x"], ref_view["max_x"], ref_view["min_y"], ref_view["max_y"] = UR.bounds(cam, G.W, G.H)
    want = P.match(ref_view, pts, pd, un[0], raw[0][1], PC.scale(), th=3.0, one_to_one=True)
    assert np.array_equal(idx[0][:len(pts)], want[0]) and proj[0][:len(pts)].tobytes() == want[3].tobytes()


def test_guided_search_on_the_undistorted_batch(undistorted_batch):
    """ss_match_guided_batch_device (windows NULL, radius 20) after the in-place undistortion returns the bytes of
    tests/guided_ref.py on the undistorted keypoints; under camera W a sixth of them lie outside 0 .. width, in the grid index's
    border cells"""
    from send_slam_amd import binding
    c, kcap, raw, un, cam, wide = undistorted_batch
    n = len(BATCH)
    combo = dict(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1)
    params = binding.guided_params(radius=20.0, radius_by_octave=True, octave_span=1, **combo)
    idx, d1, d2, summ = _filled((n, kcap * 4)), _filled((n, kcap * 2)), _filled((n, kcap * 2)), _filled((n, 32))
    c.match_guided_batch_device(params, idx.data_ptr(), d1.data_ptr(), d2.data_ptr(), summ.data_ptr())
    c.synchronize()
    idx = idx.cpu().numpy().copy().view(np.int32).reshape(n, kcap)
    d1, d2 = (t.cpu().numpy().copy().view(np.uint16).reshape(n, kcap) for t in (d1, d2))
    summ = summ.cpu().numpy().copy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(n)
    accepted_outside, differ = 0, 0
    for b in range(n):
        windows = R.own_windows(un[b], 20.0, True, 1, G.scales())
        t_kp, t_desc = (un[b - 1], raw[b - 1][1]) if b else (None, None)
        widx, wd1, wd2, wsumm = R.match(un[b], raw[b][1], t_kp, t_desc, windows, **combo)[:4]
        k = len(un[b])
        assert {f: int(summ[b][f]) for f in R.SUMMARY_FIELDS} == wsumm, f"frame {b}: summary"
        assert np.array_equal(idx[b, :k], widx) and np.array_equal(d1[b, :k], wd1) and np.array_equal(d2[b, :k], wd2), f"frame {b}"
        assert (idx[b, k:] == -1).all() and (d1[b, k:] == R.NONE).all()
        out = (un[b]["x"] < 0) | (un[b]["x"] >= G.W) | (un[b]["y"] < 0) | (un[b]["y"] >= G.H)
        accepted_outside += int((widx[out] >= 0).sum())
        if b:
            # under W the same search on the raw keypoints gives other matches: the batch really reads mvKeysUn
            ridx = R.match(raw[b][0], raw[b][1], raw[b - 1][0], raw[b - 1][1], R.own_windows(raw[b][0], 20.0, True, 1, G.scales()), **combo)[0]
            differ += not np.array_equal(ridx, widx)
    print("accepted matches of keypoints outside the image:", accepted_outside, "frames whose raw search differs:", differ)
    if wide:
        assert accepted_outside > 10 and differ > 0


# ---- depth ---------------------------------------------------------------------------------------------------------------------------
class DepthOutputs:
    def __init__(self, n, rows):
        self.n, self.rows = n, rows
        self.right, self.depth, self.summary = _filled((n, rows * 4)), _filled((n, rows * 4)), _filled((n, 16))

    def ptrs(self):
        return self.right.data_ptr(), self.depth.data_ptr(), self.summary.data_ptr()

    def host(self):
        from send_slam_amd import binding
        f = lambda t: t.cpu().numpy().copy().view(np.float32).reshape(self.n, self.rows)  # noqa: E731
        return f(self.right), f(self.depth), self.summary.cpu().numpy().copy().view(binding.DEPTH_SUMMARY_DTYPE).reshape(self.n)


def _check_depth(tag, got, b, want, n):
    right, depth, summ = got
    w_right, w_depth, w_summ = want
    assert depth[b, :n].tobytes() == w_depth.tobytes(), f"{tag}: depth"
    assert right[b, :n].tobytes() == w_right.tobytes(), f"{tag}: right"
    assert (depth[b, n:] == -1).all() and (right[b, n:] == -1).all(), f"{tag}: rows past the count"
    assert summ[b].tobytes() == w_summ.tobytes(), f"{tag}: summary {summ[b]} != {w_summ}"


@pytest.mark.parametrize("kind,factor", [("u16", 5000.0), ("f32", 1.0), ("f32", 0.5)], ids=["uint16_5000", "float32_pitched", "float32_scaled"])
@pytest.mark.parametrize("counts", [UC.COUNTS, [200, -3, 69]], ids=["counts_70_1_0", "counts_past_the_rows_and_below_0"])
def test_depth_pairs_form(ctx, kind, factor, counts):
    from send_slam_amd import binding
    img, kp = UC.depth_frames(kind), UC.depth_kp()
    cam = UC.camera("D", width=UC.DEPTH_W, height=UC.DEPTH_H, cx=31.0, cy=25.0, fx=60.0, fy=58.0)
    un = np.stack([binding.undistort_host(cam, kp[b]) for b in range(UC.F)])
    p = binding.depth_params(26.0, factor, 3.0, 1 if kind == "u16" else 0)
    d_img, d_raw, d_un, d_n = _to_dev(img.reshape(UC.F, -1)), _to_dev(kp), _to_dev(un), _to_dev(np.array(counts, np.int32))
    for d_kp_un, kp_un in ((d_un.data_ptr(), un), (0, kp)):
        out = DepthOutputs(UC.F, UC.ROWS)
        ctx.depth_pairs_device(p, d_img.data_ptr(), UC.DEPTH_W, UC.DEPTH_H, img.strides[1], img.strides[0], d_raw.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS,
                               *out.ptrs(), d_kp_un=d_kp_un)
        ctx.synchronize()
        got = out.host()
        for b in range(UC.F):
            n = UC.clamp(counts[b])
            want = binding.depth_host(p, img[b], kp[b, :n], kp_un[b, :n], width=UC.DEPTH_W)
            _check_depth(f"frame {b}", got, b, want, n)
            if n == UC.ROWS:
                assert 0 < int(want[2]["n_close"]) < int(want[2]["n_depth"]) < n
    with pytest.raises(binding.OrbError) as e:  # a row stride below the width
        ctx.depth_pairs_device(p, d_img.data_ptr(), UC.DEPTH_W, UC.DEPTH_H, UC.DEPTH_W, img.strides[0], d_raw.data_ptr(), d_n.data_ptr(), UC.F, UC.ROWS, *out.ptrs())
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "strides" in e.value.message


def test_depth_batch_form_before_and_after_the_undistortion():
    """before: the batch's keypoints serve as both; after the in-place undistortion: the saved raw pairs give the pixel, the
    undistorted x the right coordinate"""
    from send_slam_amd import binding
    cam, n = UC.camera("D"), len(BATCH)
    rng = np.random.Generator(np.random.PCG64(0xDE9704))
    img = rng.integers(0, 40000, (n, G.H, G.W)).astype(np.uint16)  # every pixel another depth: a wrong pixel shows
    p = binding.depth_params_from_camera(cam, 1)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        pixels, kcap, raw = _extract(c, BATCH)
        d_img = _to_dev(img.reshape(n, -1))
        a = (p, d_img.data_ptr(), G.W, G.H, G.W * 2, G.W * G.H * 2)
        out = DepthOutputs(n, kcap)
        c.depth_batch_device(*a, *out.ptrs())
        c.synchronize()
        before = out.host()
        for b in range(n):
            _check_depth(f"before, frame {b}", before, b, binding.depth_host(p, img[b], raw[b][0]), len(raw[b][0]))
        c.undistort_batch_device(cam)
        out = DepthOutputs(n, kcap)
        c.depth_batch_device(*a, *out.ptrs())
        c.synchronize()
        after = out.host()
        for b in range(n):
            k = len(raw[b][0])
            un = binding.undistort_host(cam, raw[b][0])
            want = binding.depth_host(p, img[b], raw[b][0], un)
            _check_depth(f"after, frame {b}", after, b, want, k)
            # the pixels are the raw ones: the depth plane is unchanged; the right coordinates follow the undistorted x
            assert after[1][b].tobytes() == before[1][b].tobytes() and after[0][b].tobytes() != before[0][b].tobytes()
            wrong = binding.depth_host(p, img[b], un, un)  # the lookup at the undistorted position: another plane
            assert wrong[1].tobytes() != want[1].tobytes()
            assert int(want[2]["n_depth"]) > 300
        del pixels
