"""GPU parity of the stereo form of the triangulation (ss_triangulate_stereo_pairs_device, ss_triangulate_stereo_batch_device) against the
host twin ss_triangulate_stereo_host, bit for bit; all planes -1 against ss_triangulate_pairs_device byte for byte; the compact block
into the projection search."""
import numpy as np
import pytest

import camera_cases as CC
import guided_cases as G
import proj_cases as PC
import tri_stereo_cases as K
import undistort_cases as UC

pytestmark = pytest.mark.gpu
PATTERN = 0x5A


def _torch():
    import torch
    return torch


def _to_dev(a):
    a = np.ascontiguousarray(a)
    t = _torch().from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to("cuda:0")
    _torch().cuda.synchronize()  # the library's stream does not wait for torch's
    return t


def _filled(shape):
    torch = _torch()
    t = torch.full(shape, PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


class Outputs:
    def __init__(self, n, rows, info_bytes, summary_bytes):
        self.n, self.rows, self.info_bytes = n, rows, info_bytes
        self.arrays = [_filled((n, rows * k)) for k in (info_bytes, 32, 32, 8)] + [_filled((n, 4)), _filled((n, summary_bytes))]

    def ptrs(self):
        return [t.data_ptr() for t in self.arrays]

    def host(self):
        from send_slam_amd import binding
        info, pts, pd, pr, n_pts, summ = (t.cpu().numpy().copy() for t in self.arrays)
        stereo = self.info_bytes == 32
        return dict(info=info.view(binding.TRI_STEREO_INFO_DTYPE if stereo else binding.TRI_INFO_DTYPE).reshape(self.n, self.rows),
                    points=pts.view(binding.MAP_POINT_DTYPE).reshape(self.n, self.rows), desc=pd.reshape(self.n, self.rows, 32),
                    rows=pr.view(np.int32).reshape(self.n, self.rows, 2), n_points=n_pts.view(np.int32).reshape(self.n),
                    summary=summ.view(binding.TRI_STEREO_SUMMARY_DTYPE if stereo else binding.TRI_SUMMARY_DTYPE).reshape(self.n))


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


def _call_arrays():
    cases = [K.pair_case(k) for k in range(K.F)]
    stack = lambda name: np.stack([c[name] for c in cases])  # noqa: E731
    return cases, {n: stack(n) for n in ("q_kp", "t_kp", "q_desc", "idx", "depth1", "right1", "depth2", "right2")}


def _stereo_points(depth, right):
    from send_slam_amd import binding
    pts = np.zeros(depth.shape, binding.STEREO_POINT_DTYPE)
    pts["right_idx"], pts["orb_dist"], pts["sad"] = 123456, 4321, 54321
    pts["depth"], pts["u_right"] = depth, right
    return pts


def _run_pairs(ctx, a, planes, counts=(K.ROWS,) * K.F):
    """planes: ((address, stride),) * 4"""
    from send_slam_amd import binding
    dev = [_to_dev(x) for x in (a["q_desc"].reshape(K.F, -1), a["q_kp"], np.array(counts, np.int32), a["t_kp"], a["idx"])]
    out = Outputs(K.F, K.ROWS, 32, 80)
    ctx.triangulate_stereo_pairs_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[2].data_ptr(), dev[4].data_ptr(), K.F,
                                        K.ROWS, [K.twin_pair(k) for k in range(K.F)], [K.twin_rig(K.pair_case(k)["rig"]) for k in range(K.F)], planes,
                                        K.twin_params(), *out.ptrs())
    ctx.synchronize()
    return out.host(), dev


def _check_against_the_twin(got, mono=False):
    modes = np.zeros(3, int)
    for k in range(K.F):
        info, pts = K.twin_rows(k, mono=mono)
        c = K.pair_case(k)
        assert got["info"][k].tobytes() == info.tobytes(), f"pair {k}: info differs at rows {np.flatnonzero(got['info'][k] != info)[:6]}"
        rows = np.flatnonzero(info["state"] == 0)
        m = int(got["n_points"][k])
        assert m == len(rows)
        assert got["points"][k, :m].tobytes() == pts[rows].tobytes() and got["desc"][k, :m].tobytes() == c["q_desc"][rows].tobytes()
        assert np.array_equal(got["rows"][k, :m], np.stack([rows, c["idx"][rows]], 1))
        for name in ("points", "desc", "rows"):
            assert (got[name][k, m:].view(np.uint8) == PATTERN).all(), f"pair {k}: {name} was written from n_points on"
        want = K.summary_of(info)
        s = got["summary"][k]
        mine = dict(status=int(s["status"]), n_query=int(s["n_query"]), n_train=int(s["n_train"]), n_matches=int(s["n_matches"]), n_points=int(s["n_points"]),
                    n_state=s["n_state"].tolist(), n_mode=s["n_mode"].tolist())
        assert mine == want and int(s["reserved"]) == 0, (mine, want)
        modes += np.array(want["n_mode"])
    return modes


@pytest.mark.parametrize("layout", ["float_planes", "stereo_points"])
def test_three_pairs_under_three_cameras_with_mixed_rows(ctx, layout):
    """one call: 3 pairs x 70 rows, a camera pair and a rig per pair, mono and stereo rows on both sides; all three modes in the summaries"""
    from send_slam_amd import binding
    cases, a = _call_arrays()
    if layout == "float_planes":
        d = [_to_dev(a[n]) for n in ("depth1", "right1", "depth2", "right2")]
        planes = [(t.data_ptr(), 4) for t in d]
    else:
        d = [_to_dev(_stereo_points(a["depth1"], a["right1"])), _to_dev(_stereo_points(a["depth2"], a["right2"]))]
        off = binding.STEREO_POINT_DTYPE.fields
        planes = [(d[0].data_ptr() + off["depth"][1], 16), (d[0].data_ptr() + off["u_right"][1], 16), (d[1].data_ptr() + off["depth"][1], 16),
                  (d[1].data_ptr() + off["u_right"][1], 16)]
    got, _ = _run_pairs(ctx, a, planes)
    modes = _check_against_the_twin(got)
    print("rows per mode", modes)
    assert (modes > 5).all()


def test_all_planes_minus_one_is_the_mono_form_byte_for_byte(ctx):
    from send_slam_amd import binding
    cases, a = _call_arrays()
    minus = _to_dev(np.full((K.F, K.ROWS), -1.0, np.float32))
    got, dev = _run_pairs(ctx, a, [(minus.data_ptr(), 4)] * 4)
    _check_against_the_twin(got, mono=True)
    mono = Outputs(K.F, K.ROWS, 16, 64)
    tp = binding.tri_params(**{n: K.TP[n] for n in ("cos_parallax_max", "chi2", "ratio_factor", "far_limit")})
    ctx.triangulate_pairs_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[2].data_ptr(), dev[4].data_ptr(), K.F, K.ROWS,
                                 [K.twin_pair(k) for k in range(K.F)], tp, *mono.ptrs())
    ctx.synchronize()
    want = mono.host()
    assert got["info"]["state"].tobytes() == want["info"]["state"].tobytes()
    for name in ("points", "desc", "rows", "n_points"):
        assert got[name].tobytes() == want[name].tobytes(), name
    for f in binding.TRI_SUMMARY_DTYPE.names:
        assert got["summary"][f].tobytes() == want["summary"][f].tobytes(), f
    assert int(want["n_points"][0]) > 20


def test_refusals_leave_the_context_usable(ctx):
    from send_slam_amd import binding
    cases, a = _call_arrays()
    d = [_to_dev(a[n]) for n in ("depth1", "right1", "depth2", "right2")]
    good = [(t.data_ptr(), 4) for t in d]
    for bad in ([(0, 4)] + good[1:], good[:3] + [(d[3].data_ptr(), 6)], good[:2] + [(d[2].data_ptr() + 2, 4)] + good[3:], [(d[0].data_ptr(), 0)] + good[1:]):
        with pytest.raises(binding.OrbError) as e:
            _run_pairs(ctx, a, bad)
        assert e.value.code == binding.SS_ERR_INVALID_ARG
    _check_against_the_twin(_run_pairs(ctx, a, good)[0])


def test_the_compact_block_feeds_the_projection_search(ctx):
    """the stereo triangulation's block of pair 0 searched in its own query frame: the bytes of the same search on the twin's points"""
    from send_slam_amd import binding
    cases, a = _call_arrays()
    d = [_to_dev(a[n]) for n in ("depth1", "right1", "depth2", "right2")]
    got_dev = Outputs(K.F, K.ROWS, 32, 80)
    dev = [_to_dev(x) for x in (a["q_desc"].reshape(K.F, -1), a["q_kp"], np.array([K.ROWS] * K.F, np.int32), a["t_kp"], a["idx"])]
    ctx.triangulate_stereo_pairs_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[2].data_ptr(), dev[4].data_ptr(), K.F,
                                        K.ROWS, [K.twin_pair(k) for k in range(K.F)], [K.twin_rig(c["rig"]) for c in cases], [(t.data_ptr(), 4) for t in d],
                                        K.twin_params(), *got_dev.ptrs())
    views = []
    for k in range(K.F):
        cam = K.binding_camera(CC.PAIR_CAMERAS[k][0])
        (r1, t1), _ = K.poses(k)
        views.append(binding.proj_view(cam, r1, t1, bf=K.B * CC.PAIR_CAMERAS[k][0][0]))
    params = binding.proj_params(th=3.0, one_to_one=True, extent_w=G.W, extent_h=G.H)

    def search(d_points, d_pdesc, d_np):
        o = [_filled((K.F, K.ROWS * k)) for k in (4, 2, 2, 32)] + [_filled((K.F, 32))]
        ctx.match_proj_pairs_device(d_points, d_pdesc, d_np, K.F, K.ROWS, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), K.F, K.ROWS, views, params,
                                    *[t.data_ptr() for t in o])
        ctx.synchronize()
        return [t.cpu().numpy().copy() for t in o]
    mine = search(got_dev.arrays[1].data_ptr(), got_dev.arrays[2].data_ptr(), got_dev.arrays[4].data_ptr())
    points, p_desc, n_pts = np.zeros((K.F, K.ROWS), binding.MAP_POINT_DTYPE), np.zeros((K.F, K.ROWS, 32), np.uint8), np.zeros(K.F, np.int32)
    for k in range(K.F):
        info, pts = K.twin_rows(k)
        rows = np.flatnonzero(info["state"] == 0)
        points[k, :len(rows)], p_desc[k, :len(rows)], n_pts[k] = pts[rows], cases[k]["q_desc"][rows], len(rows)
    twin_dev = [_to_dev(x) for x in (points, p_desc, n_pts)]
    want = search(twin_dev[0].data_ptr(), twin_dev[1].data_ptr(), twin_dev[2].data_ptr())
    for name, x, y in zip(("idx", "d1", "d2", "proj", "summary"), mine, want):
        assert x.tobytes() == y.tobytes(), name
    summ = mine[4].view(binding.PROJ_SUMMARY_DTYPE).reshape(K.F)
    print(summ)
    assert all(int(s["n_accepted"]) > 0 for s in summ)


def test_batch_form_equals_the_pairs_form_on_the_batch_arrays():
    """frame 1 against frame 0 of a batch that shows one image and one depth frame twice, a millimetre apart, matches idx[i] = i, the
    planes of ss_depth_batch_device: the rows with a depth are unprojected (mode 1), the others fail the parallax test"""
    from send_slam_amd import binding
    cam, n = UC.camera("Z"), 2
    poses = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([-0.001, 0.0, 0.0]))]
    rng = np.random.Generator(np.random.PCG64(0xBA7C))
    one = rng.uniform(0.5, 6.0, (G.H, G.W)).astype(np.float32)
    one[rng.random(one.shape) < 0.3] = 0.0  # mono rows
    img = np.stack([one] * n)
    dp = binding.depth_params(cam.fx * 0.1, 1.0, 3.0, 0)
    pairs = [binding.epi_pair(cam, *poses[b], cam, *poses[b - 1]) for b in range(n)]
    rigs = [binding.TriStereoRig(bf1=0.1 * cam.fx, b1=0.1, bf2=0.1 * cam.fx, b2=0.1)] * n
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        frames = np.stack([G.frame("synth_t0")] * n)
        d_pix = _to_dev(frames)
        c.extract_batch_device(d_pix.data_ptr(), n, G.W, G.H)
        kcap = c.batch_view().kp_capacity
        d_img, d_right, d_depth, d_dsum = _to_dev(img.reshape(n, -1)), _filled((n, kcap * 4)), _filled((n, kcap * 4)), _filled((n, 16))
        c.depth_batch_device(dp, d_img.data_ptr(), G.W, G.H, G.W * 4, G.W * G.H * 4, d_right.data_ptr(), d_depth.data_ptr(), d_dsum.data_ptr())
        d_idx = _to_dev(np.tile(np.arange(kcap, dtype=np.int32), (n, 1)))
        batch = Outputs(n, kcap, 32, 80)
        c.triangulate_stereo_batch_device(d_idx.data_ptr(), pairs, rigs, d_depth.data_ptr(), 4, d_right.data_ptr(), 4, K.twin_params(), *batch.ptrs())
        c.synchronize()
        got = batch.host()
        # the twin on the fetched arrays: frame 1 (query) against frame 0 (train)
        (kq, dq, _), (kt, _, _) = c.fetch_frame(1), c.fetch_frame(0)
        depth, right = d_depth.cpu().numpy().view(np.float32).reshape(n, kcap), d_right.cpu().numpy().view(np.float32).reshape(n, kcap)
        m = len(kq)
        assert m == len(kt) > 300
        pts, info = binding.triangulate_stereo_host(pairs[1], rigs[1], K.twin_params(), K.scale(), kq, kt, depth[1, :m], right[1, :m], depth[0, :m], right[0, :m])
        assert got["info"][1, :m].tobytes() == info.tobytes() and (got["info"][1, m:]["state"] == -1).all()
        rows = np.flatnonzero(info["state"] == 0)
        assert int(got["n_points"][1]) == len(rows) > 50 and got["points"][1, :len(rows)].tobytes() == pts[rows].tobytes()
        assert got["desc"][1, :len(rows)].tobytes() == dq[rows].tobytes()
        assert got["summary"][1]["n_mode"].tolist() == [int(((info["state"] == 0) & (info["mode"] == k)).sum()) for k in range(3)]
        print(got["summary"])
        assert (got["info"][0]["state"] == -1).all() and int(got["n_points"][0]) == 0  # frame 0 has no train
        del d_pix
