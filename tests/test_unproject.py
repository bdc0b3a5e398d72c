"""GPU parity of the map points from depth (ss_unproject_pairs_device, ss_unproject_batch_device, ss_unproject) against the host twin
ss_unproject_host, bit for bit: the pairs form on caller arrays, the selection at SS_GUIDED_MAX_ROWS rows, the batch form after
ss_stereo_batch_device and after ss_depth_batch_device on a batch undistorted in place, and the chain into the projection search."""
import os

import numpy as np
import pytest

import camera_cases as CC
import guided_cases as G
import proj_cases as PC
import undistort_cases as UC
import unproject_cases as K
import unproject_ref as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_BYTES = 24


def _torch():
    import torch
    return torch


def _to_dev(a):
    a = np.ascontiguousarray(a)
    t = _torch().from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to("cuda:0")
    _torch().cuda.synchronize()  # the library's stream does not wait for torch's
    return t


def _filled(shape):
    """a device array of K.PATTERN bytes"""
    torch = _torch()
    t = torch.full(shape, K.PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


class Outputs:
    """the six output arrays of a call of n frames, prefilled"""

    def __init__(self, n, rows):
        self.n, self.rows = n, rows
        self.arrays = [_filled((n, rows * k)) for k in (4, 32, 32, 8)] + [_filled((n, 4)), _filled((n, 40))]

    def ptrs(self):
        return [t.data_ptr() for t in self.arrays]

    def host(self):
        from send_slam_amd import binding
        info, pts, pd, pr, n_pts, summ = (t.cpu().numpy().copy() for t in self.arrays)
        return dict(state=info.view(np.int32).reshape(self.n, self.rows), points=pts.view(binding.MAP_POINT_DTYPE).reshape(self.n, self.rows),
                    desc=pd.reshape(self.n, self.rows, 32), rows=pr.view(np.int32).reshape(self.n, self.rows, 2), n_points=n_pts.view(np.int32).reshape(self.n),
                    summary=summ.view(binding.UNPROJECT_SUMMARY_DTYPE).reshape(self.n))


def check_frame(tag, got, b, want, status=0):
    """frame b of a device call against a result in the shape of unproject_ref.frame; rows from n_points on keep the prefill"""
    m = int(got["n_points"][b])
    mine = dict(state=got["state"][b], points=got["points"][b, :m], desc=got["desc"][b, :m], rows=got["rows"][b, :m],
                summary={f: int(got["summary"][b][f]) for f in U.SUMMARY_FIELDS})
    K.same_frame(tag, mine, dict(want, summary=dict(want["summary"], status=status)))
    assert m == want["summary"]["n_created"], tag
    for name in ("points", "desc", "rows"):
        assert (got[name][b, m:].view(np.uint8) == K.PATTERN).all(), f"{tag}: {name} was written from n_points on"


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


# ---- the pairs form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [U.ALL, U.CLOSE], ids=["all", "close"])
@pytest.mark.parametrize("stride", [4, 16], ids=["float_plane", "stereo_points"])
@pytest.mark.parametrize("counts", K.COUNTS, ids=["counts_70_1_0", "counts_past_the_rows_and_below_0"])
def test_pairs_form(ctx, counts, stride, mode):
    """3 frames x 70 rows (one wave plus six lanes), a view per frame, max_points 5"""
    from send_slam_amd import binding
    f, views = K.frames_case(), K.twin_views()
    plane = f["depth"] if stride == 4 else K.stereo_points(f["depth"])
    inputs = [f["kp"], f["desc"].reshape(K.F, -1), np.array(counts, np.int32), plane, f["has_point"], f["outlier"]]
    d_kp, d_desc, d_n, d_plane, d_hp, d_ol = dev = [_to_dev(a) for a in inputs]
    d_depth = d_plane.data_ptr() + (0 if stride == 4 else binding.STEREO_POINT_DTYPE.fields["depth"][1])
    p = binding.unproject_params(mode, K.MAX_POINTS, K.CLOSE_LIMIT)
    out = Outputs(K.F, K.ROWS)
    ctx.unproject_pairs_device(d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth, stride, K.F, K.ROWS, views, p, *out.ptrs(),
                               d_has_point=d_hp.data_ptr(), d_outlier=d_ol.data_ptr())
    ctx.synchronize()
    got = out.host()
    for b in range(K.F):
        want = K.twin_frame(views[b], mode, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][b], f["desc"][b], f["depth"][b], n=counts[b], has_point=f["has_point"][b],
                            outlier=f["outlier"][b])
        check_frame(f"frame {b}", got, b, want)
    for t, a in zip(dev, inputs):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input was written"
    first = got["summary"][0] if counts[0] >= K.ROWS else got["summary"][2]
    print(first)
    assert int(first["n_created"]) > 0 and int(first["n_kept"]) > 0
    if mode == U.CLOSE:
        assert int(first["n_processed"]) == max(int(first["n_not_far"]), K.MAX_POINTS) + 1 < int(first["n_depth"]) - 2


def test_pairs_form_without_flags_and_with_a_frame_without_depth(ctx):
    """has_point and outlier NULL; depth_src: frame 1 reads block 0, frame 0 has no depth plane, frame 2 reads block 1"""
    from send_slam_amd import binding
    f, views = K.frames_case(), K.twin_views()
    d_kp, d_desc, d_n, d_depth = (_to_dev(a) for a in (f["kp"], f["desc"].reshape(K.F, -1), np.array([K.ROWS] * K.F, np.int32), f["depth"][:2]))
    p = binding.unproject_params(U.CLOSE, K.MAX_POINTS, K.CLOSE_LIMIT)
    out = Outputs(K.F, K.ROWS)
    src = [-1, 0, 1]
    ctx.unproject_pairs_device(d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 4, K.F, K.ROWS, views, p, *out.ptrs(), depth_src=src)
    ctx.synchronize()
    got = out.host()
    for b in range(K.F):
        depth = f["depth"][src[b]] if src[b] >= 0 else np.full(K.ROWS, -1.0, np.float32)
        check_frame(f"frame {b}", got, b, K.twin_frame(views[b], U.CLOSE, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][b], f["desc"][b], depth))
    assert (got["state"][0] == U.NO_DEPTH).all() and int(got["summary"][0]["n_depth"]) == 0 and int(got["n_points"][1]) > 0


@pytest.mark.parametrize("which", ["above", "below"])
def test_selection_at_the_largest_row_count(ctx, which):
    """two frames of SS_GUIDED_MAX_ROWS rows, max_points 100, depths drawn from 64 values: n_not_far far above max_points, and 0 with the
    cut inside the 230-odd rows of the lowest value"""
    from send_slam_amd import binding
    s = K.size_case()
    limit, rows = s["limits"][which], K.SIZE_ROWS
    views = K.twin_views()[:2]
    d_kp, d_desc, d_n, d_depth, d_hp = (_to_dev(a) for a in (s["kp"], s["desc"].reshape(2, -1), np.array([rows, rows - 1000], np.int32), s["depth"], s["has_point"]))
    p = binding.unproject_params(U.CLOSE, K.SIZE_MAX_POINTS, limit)
    out = Outputs(2, rows)
    ctx.unproject_pairs_device(d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 4, 2, rows, views, p, *out.ptrs(), d_has_point=d_hp.data_ptr())
    ctx.synchronize()
    got = out.host()
    for b, n in enumerate((rows, rows - 1000)):
        want = K.twin_frame(views[b], U.CLOSE, K.SIZE_MAX_POINTS, limit, s["kp"][b], s["desc"][b], s["depth"][b], n=n, has_point=s["has_point"][b])
        check_frame(f"{which}, frame {b}", got, b, want)
        summ = want["summary"]
        print(which, summ)
        if which == "above":
            assert summ["n_not_far"] > 6000 and summ["n_processed"] == summ["n_not_far"] + 1
        else:
            assert summ["n_not_far"] == 0 and summ["n_processed"] == K.SIZE_MAX_POINTS + 1
            low = np.flatnonzero((s["depth"][b][:n] == 0.25) & (s["kp"][b]["octave"][:n] < 8))
            assert len(low) > 150 and np.array_equal(np.flatnonzero((got["state"][b] >= 0) & (got["state"][b] <= U.KEPT)), low[:K.SIZE_MAX_POINTS + 1]), "the lowest rows of the tie win"


def test_host_pointer_form(ctx):
    f, v = K.frames_case(), K.twin_views()[1]
    from send_slam_amd import binding
    for mode in (U.ALL, U.CLOSE):
        p = binding.unproject_params(mode, K.MAX_POINTS, K.CLOSE_LIMIT)
        for depth in (f["depth"][1], K.stereo_points(f["depth"][1])):
            info, pts, pd, pr, summ = ctx.unproject(v, p, f["kp"][1], f["desc"][1], depth, has_point=f["has_point"][1], outlier=f["outlier"][1])
            got = dict(state=info["state"], points=pts, desc=pd, rows=pr, summary={k: int(summ[k]) for k in U.SUMMARY_FIELDS})
            K.same_frame("ss_unproject", got, K.twin_frame(v, mode, K.MAX_POINTS, K.CLOSE_LIMIT, f["kp"][1], f["desc"][1], f["depth"][1],
                                                           has_point=f["has_point"][1], outlier=f["outlier"][1]))
    info, pts, _, _, summ = ctx.unproject(v, p, f["kp"][1][:0], f["desc"][1][:0], f["depth"][1][:0])
    assert len(info) == 0 and len(pts) == 0 and int(summ["n_kp"]) == 0


def test_refusals_leave_the_context_usable(ctx):
    from send_slam_amd import binding
    f, views = K.frames_case(), K.twin_views()
    d_kp, d_desc, d_n, d_depth = (_to_dev(a) for a in (f["kp"], f["desc"].reshape(K.F, -1), np.array(K.COUNTS[0], np.int32), f["depth"]))
    out = Outputs(K.F, K.ROWS)
    before = [t.cpu().numpy().copy() for t in out.arrays]
    ok = dict(mode=1, max_points=5, close_limit=3.0, reserved=0)

    def call(params=ok, kp=d_kp.data_ptr(), depth=d_depth.data_ptr(), stride=4, n_frames=K.F, rows=K.ROWS, ptrs=None, **kw):
        ctx.unproject_pairs_device(kp, d_desc.data_ptr(), d_n.data_ptr(), depth, stride, n_frames, rows, views[:max(n_frames, 0)] if n_frames != K.F else views,
                                   binding.UnprojectParams(**params), *(ptrs or out.ptrs()), **kw)
    cases = [dict(params=dict(ok, mode=2)), dict(params=dict(ok, max_points=-1)), dict(params=dict(ok, close_limit=float("nan"))),
             dict(params=dict(ok, close_limit=float("-inf"))), dict(params=dict(ok, reserved=3)), dict(stride=0), dict(stride=-4), dict(stride=10),
             dict(depth=d_depth.data_ptr() + 1), dict(depth=0), dict(kp=0), dict(rows=0), dict(rows=binding.SS_GUIDED_MAX_ROWS + 1),
             dict(ptrs=out.ptrs()[:5] + [0]), dict(ptrs=[0] + out.ptrs()[1:]), dict(depth_src=[0, 1, 3], n_depth_blocks=3), dict(depth_src=[0, -2, 1], n_depth_blocks=3),
             dict(n_depth_blocks=2), dict(n_depth_blocks=0, depth_src=[-1, -1, -1])]
    for kw in cases:
        with pytest.raises(binding.OrbError) as e:
            call(**kw)
            pytest.fail(f"not refused: {kw}")
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    with pytest.raises(ValueError):
        call(n_frames=-1)
    ctx.synchronize()
    for t, a in zip(out.arrays, before):
        assert np.array_equal(t.cpu().numpy(), a), "a refused call wrote"
    ctx.unproject_pairs_device(d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 4, 0, K.ROWS, [], binding.UnprojectParams(**ok), *out.ptrs())
    call()  # the context is usable
    ctx.synchronize()
    assert int(out.host()["n_points"][0]) > 0


# ---- the batch form ------------------------------------------------------------------------------------------------------------------
def _extract(c, frames):
    d = _to_dev(np.ascontiguousarray(frames))
    c.extract_batch_device(d.data_ptr(), len(frames), frames.shape[2], frames.shape[1])
    c.synchronize()
    return d, c.batch_view().kp_capacity, [c.fetch_frame(b)[:2] for b in range(len(frames))]


def test_batch_form_after_the_stereo_depth():
    """a golden rectified pair: the left eye reads ss_stereo_point in place (stride 16, block 0), the right eye has no depth plane"""
    from send_slam_amd import binding
    z = np.load(os.path.join(ROOT, "tests", "golden", "stereo", "parallax_t3_s11_fx500.npz"))
    assert float(z["scale_factor"]) == np.float32(1.2) and int(z["n_levels"]) == 8
    fx, baseline, th_depth = float(z["fx"]), float(z["baseline"]), float(z["th_depth"])
    cam = binding.Camera(fx=fx, fy=fx, cx=160.0, cy=120.0, width=320, height=240)
    views = [binding.unproject_view(cam, *K.POSES[0]), binding.unproject_view(cam, *K.POSES[1])]
    limit = np.float32(baseline * th_depth)
    with binding.OrbContext(0, n_features=int(z["n_features"]), lapping_x0=0, lapping_x1=0, max_batch=2) as c:
        with pytest.raises(binding.OrbError) as e:  # no batch yet
            c.unproject_batch_device(0, 4, views, binding.unproject_params(), 0, 0, 0, 0, 0, 0)
        assert e.value.code == binding.SS_ERR_STATE
        pixels, kcap, raw = _extract(c, np.stack([z["left"], z["right"]]))
        d_pts, d_sum = _filled((1, kcap * 16)), _filled((1, 32))
        c.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), fx, baseline, th_depth)
        c.synchronize()
        pts = d_pts.cpu().numpy().copy().view(binding.STEREO_POINT_DTYPE).reshape(kcap)
        n_left = len(raw[0][0])
        assert pts[:n_left].tobytes() == z["points"].tobytes()
        for mode, mp in ((U.ALL, 0), (U.CLOSE, 100), (U.CLOSE, 20)):
            out = Outputs(2, kcap)
            c.unproject_batch_device(d_pts.data_ptr() + binding.STEREO_POINT_DTYPE.fields["depth"][1], 16, views, binding.unproject_params(mode, mp, limit),
                                     *out.ptrs(), depth_src=[0, -1])
            c.synchronize()
            got = out.host()
            pad = lambda a: np.concatenate([a, np.zeros((kcap - n_left,) + a.shape[1:], a.dtype)])  # noqa: E731
            want = K.twin_frame(views[0], mode, mp, limit, pad(raw[0][0]), pad(raw[0][1]), pts, n=n_left)
            check_frame(f"left eye, mode {mode}, max_points {mp}", got, 0, want)
            print(mode, mp, want["summary"])
            assert want["summary"]["n_created"] > 50
            right = got
            n_right = len(raw[1][0])
            assert (right["state"][1, :n_right] == U.NO_DEPTH).all() and (right["state"][1, n_right:] == -1).all() and int(right["n_points"][1]) == 0
            assert int(right["summary"][1]["n_kp"]) == n_right and int(right["summary"][1]["n_depth"]) == 0
        del pixels


def _depth_image(n):
    """float32 metres over the 320 x 240 frames: every pixel another depth between 0.5 and 6.3, holes of 0 and NaN"""
    rng = np.random.Generator(np.random.PCG64(0xDE9705))
    img = (0.5 + rng.integers(0, 58000, (n, G.H, G.W)) / 10000.0).astype(np.float32)
    hole = rng.random(img.shape)
    img[hole < 0.05], img[(hole >= 0.05) & (hole < 0.1)] = 0.0, np.nan
    return img


@pytest.mark.parametrize("flag", [False, True], ids=["an_empty_frame", "a_flagged_frame"])
def test_batch_form_after_the_rgbd_depth_on_an_undistorted_batch(monkeypatch, flag):
    """extraction, in-place undistortion, ss_depth_batch_device, ss_unproject_batch_device: the twin on the host-undistorted keypoints"""
    from send_slam_amd import binding
    if flag:
        monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "2")
    names = ["synth_t0", "flat", "synth_t1"]
    cam, n = UC.camera("D"), len(names)
    img = _depth_image(n)
    dp = binding.depth_params(26.0, 1.0, K.CLOSE_LIMIT, 0)
    views = [binding.unproject_view(cam, *pose) for pose in K.POSES]
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        pixels, kcap, raw = _extract(c, np.stack([G.frame(name) for name in names]))
        assert len(raw[0][0]) > 300 and len(raw[1][0]) == 0
        c.undistort_batch_device(cam)
        d_img, d_right, d_depth, d_dsum = _to_dev(img.reshape(n, -1)), _filled((n, kcap * 4)), _filled((n, kcap * 4)), _filled((n, 16))
        c.depth_batch_device(dp, d_img.data_ptr(), G.W, G.H, G.W * 4, G.W * G.H * 4, d_right.data_ptr(), d_depth.data_ptr(), d_dsum.data_ptr())
        rng = np.random.Generator(np.random.PCG64(0x4A5))
        has_point = (rng.random((n, kcap)) < 0.5).astype(np.uint8)
        d_hp = _to_dev(has_point)
        for mode, mp in ((U.ALL, 0), (U.CLOSE, 100)):
            out = Outputs(n, kcap)
            c.unproject_batch_device(d_depth.data_ptr(), 4, views, binding.unproject_params(mode, mp, K.CLOSE_LIMIT), *out.ptrs(), d_has_point=d_hp.data_ptr())
            c.synchronize()
            got = out.host()
            for b in range(n):
                k = len(raw[b][0])
                un = binding.undistort_host(cam, raw[b][0])
                depth = binding.depth_host(dp, img[b], raw[b][0], un)[1]
                pad = lambda a, fill=0: np.concatenate([a, np.full((kcap - k,) + a.shape[1:], fill, a.dtype)])  # noqa: E731
                voided = flag and b == 2
                want = K.twin_frame(views[b], mode, mp, K.CLOSE_LIMIT, pad(un), pad(raw[b][1]), pad(depth, -1), n=0 if voided else k, has_point=has_point[b])
                check_frame(f"mode {mode}, frame {b}", got, b, want, status=binding.SS_ERR_OVERFLOW if voided else 0)
                if b == 0:
                    print(mode, want["summary"])
                    assert want["summary"]["n_created"] > 50 and want["summary"]["n_kept"] > 50
                    # the raw keypoints give other points: the batch form reads mvKeysUn
                    other = K.twin_frame(views[b], mode, mp, K.CLOSE_LIMIT, pad(raw[b][0]), pad(raw[b][1]), pad(depth, -1), n=k, has_point=has_point[b])
                    assert other["points"].tobytes() != want["points"].tobytes()
        del pixels


def test_the_unprojected_block_feeds_the_projection_search():
    """frame 0's block into ss_match_proj_batch_device on frame 1 with check_right: the bytes of the pairs form fed with the twin's
    points.  Both frames show the same image under the same pose, so every point projects onto its own keypoint"""
    from send_slam_amd import binding
    cam, n = UC.camera("D"), 2
    img = np.repeat(_depth_image(1), 2, axis=0)
    dp = binding.depth_params(26.0, 1.0, K.CLOSE_LIMIT, 0)
    pose = PC.POSES[0]
    views = [binding.unproject_view(cam, *pose)] * n
    proj_views = [binding.proj_view_set_bounds(binding.proj_view(cam, pose[0], pose[1], bf=26.0), cam)] * n
    params = binding.proj_params(th=3.0, one_to_one=True, check_right=True, extent_w=G.W, extent_h=G.H)
    up = binding.unproject_params(U.CLOSE, 100, K.CLOSE_LIMIT)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        pixels, kcap, raw = _extract(c, np.stack([G.frame("synth_t0")] * n))
        c.undistort_batch_device(cam)
        d_img, d_right, d_depth, d_dsum = _to_dev(img.reshape(n, -1)), _filled((n, kcap * 4)), _filled((n, kcap * 4)), _filled((n, 16))
        c.depth_batch_device(dp, d_img.data_ptr(), G.W, G.H, G.W * 4, G.W * G.H * 4, d_right.data_ptr(), d_depth.data_ptr(), d_dsum.data_ptr())
        out = Outputs(n, kcap)
        c.unproject_batch_device(d_depth.data_ptr(), 4, views, up, *out.ptrs())

        def outputs():
            o = [_filled((n, kcap * k)) for k in (4, 2, 2, 32)] + [_filled((n, 32))]
            return o, [t.data_ptr() for t in o]
        d_points, d_pdesc, d_n_points = out.arrays[1], out.arrays[2], out.arrays[4]
        batch, batch_ptrs = outputs()
        c.match_proj_batch_device(d_points.data_ptr(), d_pdesc.data_ptr(), d_n_points.data_ptr(), n, kcap, proj_views, params, *batch_ptrs, point_src=[0, 0],
                                  d_train_right=d_right.data_ptr())
        c.synchronize()
        # the twin's side: host-undistorted keypoints, the host depth lookup, the host unprojection
        k = len(raw[0][0])
        un = binding.undistort_host(cam, raw[0][0])
        right, depth, _ = binding.depth_host(dp, img[0], raw[0][0], un)
        twin = K.twin_frame(views[0], U.CLOSE, 100, K.CLOSE_LIMIT, un, raw[0][1], depth)
        m = twin["summary"]["n_created"]
        points, p_desc = np.zeros((n, kcap), binding.MAP_POINT_DTYPE), np.zeros((n, kcap, 32), np.uint8)
        t_kp, t_desc, t_right = np.zeros((n, kcap), binding.KP_DTYPE), np.zeros((n, kcap, 32), np.uint8), np.full((n, kcap), -1.0, np.float32)
        for b in range(n):
            points[b, :m], p_desc[b, :m] = twin["points"], twin["desc"]
            t_kp[b, :k], t_desc[b, :k], t_right[b, :k] = un, raw[0][1], right
        dev = [_to_dev(a) for a in (points, p_desc, np.array([m, m], np.int32), t_desc, t_kp, np.array([k, k], np.int32), t_right)]
        pairs, pairs_ptrs = outputs()
        c.match_proj_pairs_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n, kcap, dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), n, kcap,
                                  proj_views, params, *pairs_ptrs, point_src=[0, 0], d_train_right=dev[6].data_ptr())
        c.synchronize()
        for name, a, b in zip(("idx", "d1", "d2", "proj", "summary"), pairs, batch):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"{name}: the chain differs from the pairs form on the twin's points"
        summ = batch[4].cpu().numpy().copy().view(binding.PROJ_SUMMARY_DTYPE).reshape(n)
        idx = batch[0].cpu().numpy().copy().view(np.int32).reshape(n, kcap)
        print(summ, m)
        assert m > 100 and int(summ[1]["n_accepted"]) > 0 and int(summ[0]["n_accepted"]) > 0
        # an accepted point has found the keypoint it was made from
        own, found = twin["rows"][:, 0], idx[1, :m] >= 0
        print("accepted", int(found.sum()), "of", m, "own keypoint", float((idx[1, :m][found] == own[found]).mean()))
        assert (idx[1, :m][found] == own[found]).mean() > 0.9
        del pixels
