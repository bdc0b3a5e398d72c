"""GPU parity of map-point fusion (ss_match_fuse_pairs_device, ss_match_fuse_batch_device, ss_match_fuse) against tests/fuse_ref.py:
bit for bit, no tolerance -- idx, d1, the ss_fuse_action and the ss_fuse_point of every row, every summary field.  Every output
starts prefilled with a pattern no result has; rows past the points must be "none".  tests/test_fuse_ref.py asserts on the
reference that the shared cases are live."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as F
import guided_cases as G
import proj_cases as PC
import proj_ref as P

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()  # the library's stream does not wait for torch's


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to(_dev())


class Outputs:
    """device idx / d1 / fuse / point [n, rows] and summaries [n], prefilled with a pattern no result has"""

    def __init__(self, n, rows):
        import torch
        self.n, self.rows = n, rows
        self.idx = torch.full((n, rows), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        self.d1 = torch.full((n, rows), 0x5A5A, dtype=torch.int16, device=_dev())
        self.fuse = torch.full((n, rows * 8), 0x5A, dtype=torch.uint8, device=_dev())
        self.point = torch.full((n, rows * 32), 0x5A, dtype=torch.uint8, device=_dev())
        self.summary = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=_dev())
        _sync()

    def ptrs(self):
        return self.idx.data_ptr(), self.d1.data_ptr(), self.fuse.data_ptr(), self.point.data_ptr(), self.summary.data_ptr()

    def host(self):
        from send_slam_amd import binding
        summ = self.summary.cpu().numpy().copy().view(binding.FUSE_SUMMARY_DTYPE).reshape(self.n)
        fuse = self.fuse.cpu().numpy().copy().view(binding.FUSE_ACTION_DTYPE).reshape(self.n, self.rows)
        point = self.point.cpu().numpy().copy().view(binding.FUSE_POINT_DTYPE).reshape(self.n, self.rows)
        return (self.idx.cpu().numpy(), self.d1.cpu().numpy().view(np.uint16), fuse, point, [{f: int(s[f]) for f in F.SUMMARY_FIELDS} for s in summ])


def _check(tag, got, b, want):
    """frame b of a call's host outputs against a reference result (idx, d1, actions, points, summary, ...)"""
    idx, d1, fuse, point, summ = got
    widx, wd1, wact, wpts, wsumm = want[:5]
    n = len(widx)
    assert summ[b] == wsumm, f"{tag}: summary {summ[b]} != {wsumm}"
    for name, g, w in (("idx", idx[b], widx), ("d1", d1[b], wd1), ("action", fuse[b]["action"], wact["action"]), ("other", fuse[b]["other"], wact["other"])):
        bad = np.flatnonzero(g[:n] != w)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {g[:n][bad[:8]]} != {w[bad[:8]]}"
    for name in F.POINT_DTYPE.names:  # bit for bit
        bad = np.flatnonzero(point[b][name][:n].view(np.int32) != wpts[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {point[b][name][:n][bad[:8]]} != {wpts[name][bad[:8]]}"
    assert (idx[b][n:] == -1).all() and (d1[b][n:] == F.NONE).all(), f"{tag}: rows past the points are not 'none'"
    assert fuse[b][n:].tobytes() == F.none_actions(len(fuse[b]) - n).tobytes(), f"{tag}: rows past the points are not 'none'"
    assert point[b][n:].tobytes() == F.none_points(len(point[b]) - n).tobytes(), f"{tag}: rows past the points are not 'none'"


def _upload(frames, point_rows, rows):
    """frames: dicts view points p_desc t_kp t_desc [skip] [right] [taken] [train_point] -> device arrays of the pairs form, block b =
    frame b; [n_points] [n_train]: the counts the device is told, where they are not the lengths of the arrays"""
    from send_slam_amd import binding
    n = len(frames)
    host = {"points": np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), "p_desc": np.zeros((n, point_rows, 32), np.uint8),
            "skip": np.zeros((n, point_rows), np.uint8), "t_desc": np.zeros((n, rows, 32), np.uint8), "t_kp": np.zeros((n, rows), binding.KP_DTYPE),
            "right": np.full((n, rows), -1, np.float32), "taken": np.zeros((n, rows), np.uint8), "train_point": np.full((n, rows), -1, np.int32),
            "np": np.zeros(n, np.int32), "nt": np.zeros(n, np.int32)}
    for b, f in enumerate(frames):
        k, nt = len(f["points"]), len(f["t_kp"])
        host["np"][b], host["nt"][b] = f.get("n_points", k), f.get("n_train", nt)
        host["points"][b, :k], host["p_desc"][b, :k] = f["points"], f["p_desc"]
        host["t_desc"][b, :nt], host["t_kp"][b, :nt] = f["t_desc"], f["t_kp"]
        if f.get("skip") is not None:
            host["skip"][b, :k] = f["skip"]
        for name in ("right", "taken", "train_point"):
            if f.get(name) is not None:
                host[name][b, :nt] = f[name]
    # past the counts: rows that would match anything if they were read (no flag, free, right -1, all-zero descriptors)
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["views"] = np.concatenate([np.asarray(f["view"]).reshape(1) for f in frames])
    _sync()
    return dev


def _run_pairs(ctx, dev, n, point_rows, rows, params, skip=True, right=True, taken=True, train_point=True, point_src=None, n_blocks=None):
    out = Outputs(n, point_rows)
    ctx.match_fuse_pairs_device(dev["points"].data_ptr(), dev["p_desc"].data_ptr(), dev["np"].data_ptr(), n if n_blocks is None else n_blocks, point_rows,
                                dev["t_desc"].data_ptr(), dev["t_kp"].data_ptr(), dev["nt"].data_ptr(), n, rows, dev["views"][:n], params, *out.ptrs(),
                                point_src=point_src, d_point_skip=dev["skip"].data_ptr() if skip else 0,
                                d_train_right=dev["right"].data_ptr() if right else 0, d_train_taken=dev["taken"].data_ptr() if taken else 0,
                                d_train_point=dev["train_point"].data_ptr() if train_point else 0)
    ctx.synchronize()
    return out.host()


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


def _tables_on(c, sc, tag):
    """the boundary table of a pyramid table through the pairs form, the host form and the twin of a context that holds that table"""
    from send_slam_amd import binding
    view, points, skip, groups, tk, td, pd = FC.boundary_table(sc)
    want = FC.boundary_reference(sc)
    frame = {"view": view, "points": points, "p_desc": pd, "skip": skip, "t_kp": tk, "t_desc": td}
    point_rows, rows = len(points) + 3, len(tk) + 1
    dev = _upload([frame], point_rows, rows)
    kw = dict(chi2_mono=0.0, th_low=256, **FC.B_LIMITS)
    p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **kw)
    _check(tag, _run_pairs(c, dev, 1, point_rows, rows, p, right=False, taken=False, train_point=False), 0, want)
    idx, d1, act, pts, summ = c.match_fuse(view, points, pd, td, tk, p, skip=skip)
    _check(tag + ", host form", (idx[None], d1[None], act[None], pts[None], [summ]), 0, want)
    assert binding.fuse_points_host(view, p, sc, points, skip).tobytes() == want[3].tobytes(), tag
    return want


@pytest.mark.parametrize("name", list(PC.PYRAMIDS))
def test_tables_under_other_pyramid_tables(name):
    """contexts with one level, two levels, a scale factor of 2 and SS_MAX_LEVELS levels: the boundary table with the ratio on
    every scale[n]"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        want = _tables_on(c, sc, name)
    assert set(int(v) for v in want[3]["level"][want[3]["state"] == 0]) == set(range(n_levels))


def test_boundary_table(ctx):
    """identity pose, exact products: every test of step 1 with np.nextafter on both sides, u on max_x and v on max_y rejected, the
    ratio on every scale[n], NaN and infinite coordinates, skip flags of 1 and 255"""
    want = _tables_on(ctx, PC.scale(), "boundary table")
    assert want[4]["n_candidates"] > 20


@pytest.mark.parametrize("name", ["default"] + list(PC.PYRAMIDS))
def test_candidate_table(name):
    """one point at (160, 120), u_right 130: octaves level - 2 .. level + 1 and -1 at level 0, |x - u| on the radius, e2 on both
    chi-square limits, right coordinates of -1, -0.0, 0.0 and just above, chi2_mono of 0, negative and NaN, a taken row, d1 on th_low,
    a distance of 256, equal distances; through the pairs form, the host form and the twins, in contexts of 8, 1, 2, 4 and 16 levels"""
    from send_slam_amd import binding
    factor, n_levels = (1.2, 8) if name == "default" else PC.PYRAMIDS[name]
    sc = PC.scale() if name == "default" else PC.scale_table(factor, n_levels)
    view = FC.candidate_view()
    cases = FC.candidate_cases(None if name == "default" else sc)
    point_rows, rows = 3, max(len(c["t_kp"]) for c in cases) + 2
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as ctx:
        for c in cases:
            want = FC.case_reference(c)
            dev = _upload([dict(c, view=view)], point_rows, rows)
            p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **c["params"])
            got = _run_pairs(ctx, dev, 1, point_rows, rows, p, skip=False)
            _check(c["name"], got, 0, want)
            if c["expect"] is not None:
                assert got[0][0][0] == c["expect"], c["name"]
            if c["cands"] is not None:
                assert got[4][0]["n_candidates"] == len(c["cands"]), c["name"]
            idx, d1, act, pts, summ = ctx.match_fuse(view, c["points"], c["p_desc"], c["t_desc"], c["t_kp"], p, right=c["right"], taken=c["taken"],
                                                     train_point=c["train_point"])
            _check(c["name"] + ", host form", (idx[None], d1[None], act[None], pts[None], [summ]), 0, want)
            checks = binding.fuse_check_host(p, sc, np.repeat(want[3], len(c["t_kp"])), c["t_kp"], c["right"], c["taken"])
            assert list(np.flatnonzero(checks == 0)) == want[5][2][0], c["name"]


def test_outcome_frames(ctx):
    """one free row named by three points at distances 9, 8 and 8: the lower row of the two eights adds, the others are its
    duplicates; the same row occupied: three REPLACE with the id; no ids at all; ids of 0, -1 and INT32_MIN"""
    from send_slam_amd import binding
    view = FC.candidate_view()
    p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **F.LOCAL_MAPPING)
    for f in FC.outcome_frames():
        want = F.match(view, f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), train_point=f["train_point"], **F.LOCAL_MAPPING)
        dev = _upload([dict(f, view=view)], 4, 3)
        got = _run_pairs(ctx, dev, 1, 4, 3, p, skip=False, right=False, taken=False, train_point=f["train_point"] is not None)
        _check(f["name"], got, 0, want)
        assert [(int(a), int(o)) for a, o in got[2][0][:3]] == f["expect"], f["name"]


@pytest.fixture(scope="module")
def scene_arrays():
    frames = FC.scenes()
    point_rows, rows = 470, 483  # no multiple of the 64 points of a workgroup
    assert all(len(f["points"]) <= point_rows and len(f["t_kp"]) <= rows for f in frames)
    return _upload(frames, point_rows, rows), point_rows, rows


@pytest.mark.parametrize("pset", FC.PARAM_SETS, ids=FC.SET_NAMES)
def test_scenes(ctx, scene_arrays, pset):
    """the three proj_cases scenes with a 10 % skip mask and ids on 40 % of the train rows, under upstream's local-mapping
    parameters (right coordinates on and off), th 1 and 2, and the Sim3 forms at th 4 and 8, th_low 50 and 37, taken on and off"""
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    got = _run_pairs(ctx, dev, n, point_rows, rows, FC.set_params(binding, pset, extent_w=G.W, extent_h=G.H), taken=pset["taken"])
    for k in range(n):
        _check(f"scene {k} {pset['name']}", got, k, FC.scene_reference(k, pset))
    assert sum(s["n_add"] for s in got[4]) > 10


def test_host_form_equals_the_pairs_form(ctx, scene_arrays):
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    for pset in (FC.PARAM_SETS[1], FC.PARAM_SETS[-1]):
        p = FC.set_params(binding, pset, extent_w=G.W, extent_h=G.H)
        pairs = _run_pairs(ctx, dev, len(PC.SCENES), point_rows, rows, p, taken=pset["taken"])
        for k, f in enumerate(FC.scenes()):
            idx, d1, act, pts, summ = ctx.match_fuse(f["view"], f["points"], f["p_desc"], f["t_desc"], f["t_kp"], p, skip=f["skip"], right=f["right"],
                                                     taken=f["taken"] if pset["taken"] else None, train_point=f["train_point"])
            n = len(idx)
            assert np.array_equal(idx, pairs[0][k][:n]) and np.array_equal(d1, pairs[1][k][:n]) and act.tobytes() == pairs[2][k][:n].tobytes()
            assert pts.tobytes() == pairs[3][k][:n].tobytes() and summ == pairs[4][k]
            _check(f"host form, scene {k} {pset['name']}", (idx[None], d1[None], act[None], pts[None], [summ]), 0, FC.scene_reference(k, pset))
    # empty sides, and no optional array at all
    f = FC.scenes()[0]
    p = binding.fuse_params(extent_w=G.W, extent_h=G.H)
    idx, d1, act, pts, summ = ctx.match_fuse(f["view"], f["points"], f["p_desc"], f["t_desc"][:0], f["t_kp"][:0], p)
    assert (idx == -1).all() and (d1 == F.NONE).all() and act.tobytes() == F.none_actions(len(idx)).tobytes()
    assert summ["n_train"] == 0 and summ["n_points"] == len(idx) and summ["n_candidates"] == 0
    assert pts.tobytes() == F.eval_points(f["view"], f["points"], None, 0.5, 3.0, PC.scale()).tobytes() and summ["n_in_view"] > 0
    idx, d1, act, pts, summ = ctx.match_fuse(f["view"], f["points"][:0], f["p_desc"][:0], f["t_desc"], f["t_kp"], p)
    assert len(idx) == 0 and summ["n_points"] == 0 and summ["n_train"] == len(f["t_kp"]) and summ["n_in_view"] == 0
    want = F.match(f["view"], f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), **F.LOCAL_MAPPING)
    idx, d1, act, pts, summ = ctx.match_fuse(f["view"], f["points"], f["p_desc"], f["t_desc"], f["t_kp"], p)
    _check("no optional array", (idx[None], d1[None], act[None], pts[None], [summ]), 0, want)
    assert summ["n_replace"] == 0 and summ["n_add"] > 100


def test_one_block_searched_by_several_frames(ctx, scene_arrays):
    """point_src: every frame searches the points of block 2 under its own view, skip flags and train rows; NULL: block b"""
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    pset = FC.PARAM_SETS[-2]
    p = FC.set_params(binding, pset, extent_w=G.W, extent_h=G.H)
    got = _run_pairs(ctx, dev, n, point_rows, rows, p, taken=pset["taken"], point_src=[2, 2, 2])
    _check("point_src, frame 2", got, 2, FC.scene_reference(2, pset))
    f = FC.scenes()[2]
    for b in (0, 1):
        s = FC.scenes()[b]
        skip = np.zeros(len(f["points"]), np.uint8)
        m = min(len(skip), len(s["skip"]))
        skip[:m] = s["skip"][:m]  # the flags are the frame's, not the block's
        want = F.match(s["view"], f["points"], f["p_desc"], s["t_kp"], s["t_desc"], PC.scale(), skip=skip, right=s["right"],
                       taken=s["taken"] if pset["taken"] else None, train_point=s["train_point"], **pset["params"])
        _check(f"point_src, frame {b} on block 2", got, b, want)
    assert sum(s["n_replace"] for s in got[4]) > 5


# ---- odd cameras, per frame ----------------------------------------------------------------------------------------------------------------
CAMERA_FORMS = [(w, sh) for w in FC.CAMERA_SETS for sh in (False, True)]
CAMERA_IDS = [f"{w}_{'one_shared_block' if sh else 'own_blocks'}" for w, sh in CAMERA_FORMS]


def _camera_frames(binding, which, shared):
    """the camera scenes with the library's own views and the skip flags of the form"""
    frames = [dict(f, view=np.frombuffer(bytes(FC.library_view(binding, k, which)), P.VIEW_DTYPE)[0], skip=FC.camera_skip(k, shared))
              for k, f in enumerate(FC.camera_scenes())]
    assert len({f["view"].tobytes() for f in frames}) == 3
    return frames


@pytest.mark.parametrize("which,shared", CAMERA_FORMS, ids=CAMERA_IDS)
def test_three_cameras_per_call(ctx, which, shared):
    """one call whose frames are seen by camera A, camera B and the square camera (fx != fy, principal points off the centre, three
    values of bf), each on its own block of points and all on block 0 (point_src [0, 0, 0]): Fuse with the right coordinates under
    views of ss_proj_view_init, and the Sim3 projection search under views of ss_fuse_view_sim3 and ss_sim3_to_view; the pairs form
    and the host form.  tests/test_fuse_ref.py shows that a kernel which exchanged fx and fy or cx and cy, or read another frame's
    view or bf, would give other bytes"""
    from send_slam_amd import binding
    frames = _camera_frames(binding, which, shared)
    point_rows, rows = 470, 483
    blocks = [dict(f, skip=None) for f in frames]
    dev = _upload(blocks, point_rows, rows)
    skips = np.zeros((3, point_rows), np.uint8)
    for k, f in enumerate(frames):
        skips[k, :len(f["skip"])] = f["skip"]
    dev["skip"] = _to_dev(skips)
    _sync()
    p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **FC.CAMERA_SETS[which])
    got = _run_pairs(ctx, dev, 3, point_rows, rows, p, point_src=[0, 0, 0] if shared else None, n_blocks=1 if shared else None)
    for k, f in enumerate(frames):
        want = FC.camera_reference(k, which, shared)
        _check(f"cameras, {which}, frame {k}", got, k, want)
        b = frames[0] if shared else f
        idx, d1, act, pts, summ = ctx.match_fuse(f["view"], b["points"], b["p_desc"], f["t_desc"], f["t_kp"], p, skip=f["skip"], right=f["right"],
                                                 taken=f["taken"], train_point=f["train_point"])
        _check(f"cameras, {which}, host form, frame {k}", (idx[None], d1[None], act[None], pts[None], [summ]), 0, want)
    assert sum(s["n_add"] for s in got[4]) > 100


@pytest.mark.parametrize("shared", [False, True], ids=["own_blocks", "one_shared_block"])
def test_batch_form_under_a_camera_per_frame(shared):
    """ss_match_fuse_batch_device on three extracted frames (the train frames of the camera scenes) under three cameras"""
    from send_slam_amd import binding
    from test_guided import _extract
    which = "fuse"
    frames = _camera_frames(binding, which, shared)
    n, point_rows = 3, 500
    views = np.concatenate([np.asarray(f["view"]).reshape(1) for f in frames])
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, [train for _, train in PC.SCENES])
        pts, pd = np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), np.zeros((n, point_rows, 32), np.uint8)
        skip = np.zeros((n, point_rows), np.uint8)
        right, taken, ids = np.full((n, kcap), -1, np.float32), np.zeros((n, kcap), np.uint8), np.full((n, kcap), -1, np.int32)
        for b, f in enumerate(frames):
            k, m = len(f["points"]), len(f["t_kp"])
            pts[b, :k], pd[b, :k], skip[b, :len(f["skip"])] = f["points"], f["p_desc"], f["skip"]
            right[b, :m], taken[b, :m], ids[b, :m] = f["right"], f["taken"], f["train_point"]
        counts = np.array([len(f["points"]) for f in frames], np.int32)
        d_pts, d_pd, d_n, d_skip, d_right, d_taken, d_ids = (_to_dev(a) for a in (pts, pd, counts, skip, right, taken, ids))
        out = Outputs(n, point_rows)
        _sync()
        c.match_fuse_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1 if shared else n, point_rows, views,
                                  binding.fuse_params(**FC.CAMERA_SETS[which]), *out.ptrs(), point_src=[0, 0, 0] if shared else None,
                                  d_point_skip=d_skip.data_ptr(), d_train_right=d_right.data_ptr(), d_train_taken=d_taken.data_ptr(),
                                  d_train_point=d_ids.data_ptr())
        c.synchronize()
        got = out.host()
    for k in range(n):
        _check(f"cameras, batch form, frame {k}", got, k, FC.camera_reference(k, which, shared))


BATCH = ["synth_t0", "synth_t1", "flat", "synth_t1"]
BATCH_SRC = [0, 0, 0, 1]


def _batch_run(binding, pset, flagged=False):
    """four extracted frames, point_src [0, 0, 0, 1], block 1 empty: frames 0 and 1 search the same map points under their own views;
    flat, which has no keypoints, searches them too; the last frame has keypoints and an empty block"""
    import torch
    frames = np.stack([G.frame(n) for n in BATCH])
    s0, s1 = FC.scenes()[0], FC.scenes()[1]
    views = np.concatenate([np.asarray(v).reshape(1) for v in (s0["view"], s1["view"], s1["view"], s1["view"])])
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(BATCH)) as c:
        point_rows, n_blocks = 500, 2
        pts = np.zeros((n_blocks, point_rows), binding.MAP_POINT_DTYPE)
        pd = np.zeros((n_blocks, point_rows, 32), np.uint8)
        k = len(s0["points"])
        pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
        pts[1], pd[1] = s0["points"][0], s0["p_desc"][0]  # block 1 is empty by its count, not by its content
        counts = np.array([k, 0], np.int32)
        d_pts, d_pd, d_n = (_to_dev(a) for a in (pts, pd, counts))
        out = Outputs(len(BATCH), point_rows)
        p = FC.set_params(binding, pset)
        with pytest.raises(binding.OrbError) as e:  # no batch yet
            c.match_fuse_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, p, *out.ptrs(), point_src=BATCH_SRC)
        assert e.value.code == binding.SS_ERR_STATE and "ss_match_fuse_batch_device: no batch has been extracted" in e.value.message
        d = torch.from_numpy(frames).to(_dev())
        _sync()
        c.extract_batch_device(d.data_ptr(), len(BATCH), G.W, G.H)
        c.synchronize()
        for b, n in enumerate(BATCH):  # the references are computed on the oracle's features
            kp, desc, _ = c.fetch_frame(b)
            okp, odesc = G.features(n)
            assert kp.tobytes() == okp.tobytes() and np.array_equal(desc, odesc), f"frame {b} ({n}): extraction differs from the oracle"
        kcap = c.batch_view().kp_capacity
        skip = np.zeros((len(BATCH), point_rows), np.uint8)
        right, taken = np.full((len(BATCH), kcap), -1, np.float32), np.zeros((len(BATCH), kcap), np.uint8)
        ids = np.full((len(BATCH), kcap), -1, np.int32)
        for b, s in enumerate((s0, s1)):
            skip[b, :k] = s0["skip"]
            m = len(G.features(BATCH[b])[0])
            right[b, :m], taken[b, :m], ids[b, :m] = np.resize(s["right"], m), np.resize(s["taken"], m), np.resize(s["train_point"], m)
        d_skip, d_right, d_taken, d_ids = (_to_dev(a) for a in (skip, right, taken, ids))
        _sync()
        c.match_fuse_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, p, *out.ptrs(), point_src=BATCH_SRC,
                                  d_point_skip=d_skip.data_ptr(), d_train_right=d_right.data_ptr(), d_train_taken=d_taken.data_ptr() if pset["taken"] else 0,
                                  d_train_point=d_ids.data_ptr())
        c.synchronize()
        got = out.host()
        with pytest.raises(binding.OrbError) as e:
            c.match_fuse_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, p, *out.ptrs(), point_src=[0, 2, 0, 1])
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "point_src[1] = 2 names no block of points (2)" in e.value.message
    want = []
    for b, s in enumerate((s0, s1)):
        tk, td = G.features(BATCH[b])
        m = len(tk)
        want.append(F.match(s["view"], s0["points"], s0["p_desc"], tk, td, PC.scale(), skip=s0["skip"], right=np.resize(s["right"], m),
                            taken=np.resize(s["taken"], m) if pset["taken"] else None, train_point=np.resize(s["train_point"], m), **pset["params"]))
    return got, want


@pytest.mark.parametrize("pset", [FC.PARAM_SETS[1], FC.PARAM_SETS[-1]], ids=lambda s: s["name"])
def test_batch_form(pset, monkeypatch):
    """SS_ERR_STATE before a batch; then frames 0 and 1 against the reference, the same block against a frame without keypoints, an
    empty block against a frame with keypoints, a bad point_src"""
    from send_slam_amd import binding
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    got, want = _batch_run(binding, pset)
    _check("batch frame 0", got, 0, want[0])
    _check("batch frame 1", got, 1, want[1])
    assert want[0][4]["n_add"] > 50 and want[1][4]["n_add"] > 10 and want[1][4]["n_replace"] > 5
    s0, s1 = FC.scenes()[0], FC.scenes()[1]
    assert len(G.features("flat")[0]) == 0
    no_train = F.match(s1["view"], s0["points"], s0["p_desc"], None, None, PC.scale(), skip=np.zeros(len(s0["points"]), np.uint8), **pset["params"])
    _check("batch frame 2 (block 0, no keypoints)", got, 2, no_train)
    assert no_train[4]["n_in_view"] > 100 and no_train[4]["n_train"] == 0
    tk, td = G.features(BATCH[3])
    _check("batch frame 3 (empty block)", got, 3, F.match(s1["view"], s0["points"][:0], s0["p_desc"][:0], tk, td, PC.scale(), **pset["params"]))


def test_flagged_frames_are_voided_in_the_batch_form(monkeypatch):
    """SENDSLAM_TEST_FLAG_BATCH=1: frame 1 is flagged although it has keypoints: status, zero counts, every row "none"; frame 0 is
    what the unflagged run and the reference give"""
    from send_slam_amd import binding
    pset = FC.PARAM_SETS[1]
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1")
    got, want = _batch_run(binding, pset)
    _check("flagged run, frame 0", got, 0, want[0])
    s1 = FC.scenes()[1]
    none = F.match(s1["view"], s1["points"][:0], s1["p_desc"][:0], None, None, PC.scale())
    _check("frame 1 flagged", got, 1, none[:4] + (dict(none[4], status=binding.SS_ERR_OVERFLOW),))
    assert want[1][4]["n_train"] > 100 and want[1][4]["n_in_view"] > 100


def test_counts_at_zero_one_a_workgroup_and_above_the_rows(ctx):
    """one call, every frame holds the same 65 live points and train rows; only the counts differ: 0, 1, 63, 64, 65, above the row
    counts (clamped) and negative (0)"""
    from send_slam_amd import binding
    base, counts = FC.count_frames()
    frames = [dict(base, n_points=k, n_train=nt) for k, nt in counts]
    rows = FC.COUNT_ROWS
    dev = _upload(frames, rows, rows)
    got = _run_pairs(ctx, dev, len(frames), rows, rows, FC.set_params(binding, FC.COUNT_SET, extent_w=G.W, extent_h=G.H))
    for b, (k, nt) in enumerate(counts):
        _check(f"counts {k} / {nt}", got, b, FC.count_reference(k, nt))
    full = FC.count_reference(65, 65)[4]
    assert full["n_add"] > 10 and full["n_replace"] > 5, full


def test_full_capacity(ctx):
    """two frames with point_rows = rows_per_frame = SS_GUIDED_MAX_ROWS: free rows contested on both sides of the 8192-row pass of
    the conflict table, about half of the rows occupied"""
    from send_slam_amd import binding
    frames = FC.capacity_frames()
    rows = FC.CAP_ROWS
    assert rows == binding.SS_GUIDED_MAX_ROWS
    dev = _upload(frames, rows, rows)
    p = binding.fuse_params(extent_w=PC.CAP_W, extent_h=PC.CAP_H, **FC.CAP_PARAMS)
    got = _run_pairs(ctx, dev, 2, rows, rows, p)
    for b in range(2):
        want = FC.capacity_reference(b)
        _check(f"capacity frame {b}", got, b, want)
        dup = want[2]["action"] == F.ACT_DUPLICATE
        assert (want[0][dup] >= 8192).sum() > 20 and want[4]["n_replace"] > 500 and want[4]["n_add"] > 300
    assert (FC.capacity_reference(0)[0][FC.capacity_reference(0)[2]["action"] == F.ACT_DUPLICATE] < 8192).sum() > 20


@pytest.mark.parametrize("pset", FC.EXTENT_SETS, ids=lambda s: s["name"])
@pytest.mark.parametrize("extent", PC.EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_scenes_on_other_grids(ctx, scene_arrays, extent, pset):
    """the extent sizes the index and never the answer"""
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    got = _run_pairs(ctx, dev, n, point_rows, rows, FC.set_params(binding, pset, extent_w=extent[0], extent_h=extent[1]), taken=pset["taken"])
    for k in range(n):
        _check(f"scene {k} {pset['name']} on {extent}", got, k, FC.scene_reference(k, pset))


def test_search_then_triangulate_then_fuse(ctx):
    """end to end on the device: ss_match_epi_pairs_device -> ss_triangulate_pairs_device -> ss_match_fuse_pairs_device of the
    produced block, as it was written (point_rows = rows), into a third keyframe whose train_point marks the rows the first two
    keyframes matched; the block equals epi_ref's and the result fuse_ref.match on it (tests/test_fuse_ref.py asserts on the
    reference that the chain replaces and adds)"""
    import epi_cases as EC
    import torch
    from send_slam_amd import binding
    n, rows = len(EC.SCENES), 483  # no multiple of the 64 rows of a workgroup
    host = {name: np.zeros((n, rows) + shape, dtype) for name, shape, dtype in (
        ("q_desc", (32,), np.uint8), ("t_desc", (32,), np.uint8), ("q_kp", (), binding.KP_DTYPE), ("t_kp", (), binding.KP_DTYPE),
        ("q_node", (), np.int32), ("t_node", (), np.int32), ("q_taken", (), np.uint8), ("t_taken", (), np.uint8))}
    counts = np.zeros((2, n), np.int32)
    for k, s in enumerate(EC.scenes()):
        counts[:, k] = len(s["q_kp"]), len(s["t_kp"])
        for name in host:
            host[name][k, :len(s[name])] = s[name]
    d = {name: _to_dev(a) for name, a in host.items()}
    d_nq, d_nt = _to_dev(counts[0]), _to_dev(counts[1])
    pairs = np.concatenate([np.asarray(s["pair"]).reshape(1) for s in EC.scenes()])
    fill = lambda *shape: torch.full(shape, 0x5A, dtype=torch.uint8, device=_dev())  # noqa: E731
    e_idx, e_d1, e_sum = fill(n, rows * 4), fill(n, rows * 2), fill(n, 40)
    info, points, desc, prows, npts, t_sum = fill(n, rows * 16), fill(n, rows * 32), fill(n, rows * 32), fill(n, rows * 8), fill(n * 4), fill(n, 64)
    third = _upload(FC.end_to_end_thirds(), rows, rows)
    out = Outputs(n, rows)
    ctx.match_epi_pairs_device(d["q_desc"].data_ptr(), d["q_kp"].data_ptr(), d["q_node"].data_ptr(), d_nq.data_ptr(), d["t_desc"].data_ptr(),
                               d["t_kp"].data_ptr(), d["t_node"].data_ptr(), d_nt.data_ptr(), n, rows, pairs, EC.combo_params(binding, FC.END_TO_END_COMBO),
                               e_idx.data_ptr(), e_d1.data_ptr(), e_sum.data_ptr(), d_q_taken=d["q_taken"].data_ptr(), d_t_taken=d["t_taken"].data_ptr())
    ctx.triangulate_pairs_device(d["q_desc"].data_ptr(), d["q_kp"].data_ptr(), d_nq.data_ptr(), d["t_kp"].data_ptr(), d_nt.data_ptr(), e_idx.data_ptr(), n, rows,
                                 pairs, binding.tri_params(**EC.TRI), *(t.data_ptr() for t in (info, points, desc, prows, npts, t_sum)))
    p = binding.fuse_params(extent_w=G.W, extent_h=G.H, **FC.END_TO_END)
    ctx.match_fuse_pairs_device(points.data_ptr(), desc.data_ptr(), npts.data_ptr(), n, rows, third["t_desc"].data_ptr(), third["t_kp"].data_ptr(),
                                third["nt"].data_ptr(), n, rows, third["views"], p, *out.ptrs(), d_train_point=third["train_point"].data_ptr())
    ctx.synchronize()
    got = out.host()
    h_points = points.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(n, rows)
    h_desc, h_n = desc.cpu().numpy().reshape(n, rows, 32), npts.cpu().numpy().copy().view(np.int32)
    for k in range(n):
        tri, w = FC.end_to_end_reference(k)
        m = len(tri[1])
        assert h_n[k] == m and h_points[k][:m].tobytes() == tri[1].tobytes() and np.array_equal(h_desc[k][:m], tri[2]), f"scene {k}: the block differs"
        _check(f"scene {k}", got, k, w)
    assert sum(s["n_replace"] for s in got[4]) >= 1 and sum(s["n_add"] for s in got[4]) >= 1, got[4]


def test_refused_arguments_leave_the_context_usable(ctx, scene_arrays):
    """every refused argument with its message, then a good call on the same context"""
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    good = dict(extent_w=G.W, extent_h=G.H)
    big = binding.SS_GUIDED_MAX_ROWS + 1
    nan, inf = float("nan"), float("inf")
    run = lambda *a, **kw: _run_pairs(ctx, dev, *a, **kw)  # noqa: E731
    P_ = binding.fuse_params
    cases = [(lambda: run(1, big, rows, P_(**good)), f"fusion: point_rows {big} / rows_per_frame {rows} exceed SS_GUIDED_MAX_ROWS (16384)"),
             (lambda: run(1, point_rows, big, P_(**good)), f"fusion: point_rows {point_rows} / rows_per_frame {big} exceed SS_GUIDED_MAX_ROWS (16384)"),
             (lambda: run(1, 0, rows, P_(**good)), "fusion: bad frame, block or row count"),
             (lambda: run(n, point_rows, rows, P_(**good), point_src=[0, n, 1]), f"point_src[1] = {n} names no block of points ({n})"),
             (lambda: run(n, point_rows, rows, P_(**good), point_src=[0, -1, 1]), f"point_src[1] = -1 names no block of points ({n})"),
             (lambda: run(n, point_rows, rows, P_(**good), n_blocks=2), "frame [2] = 2 names no block of points (2)"),
             (lambda: run(n, point_rows, rows, P_(extent_w=0, extent_h=G.H)), "fusion: extent_w and extent_h must be > 0"),
             (lambda: run(n, point_rows, rows, P_(check_right=True, **good), right=False), "fusion: check_right needs the right coordinates of the train rows")]
    for kw, msg in ((dict(th=0.0), "fusion: th must be finite and > 0"), (dict(th=nan), "fusion: th must be finite and > 0"),
                    (dict(th=inf), "fusion: th must be finite and > 0"), (dict(view_cos_limit=nan), "fusion: view_cos_limit is NaN"),
                    (dict(th_low=257), "fusion: th_low must be 0 .. 256"), (dict(th_low=-1), "fusion: th_low must be 0 .. 256"),
                    (dict(check_right=True, chi2_stereo=nan), "fusion: chi2_stereo must be finite and > 0 when chi2_mono > 0 and check_right is set"),
                    (dict(check_right=True, chi2_stereo=0.0), "fusion: chi2_stereo must be finite and > 0 when chi2_mono > 0 and check_right is set"),
                    (dict(reserved=(0, 7)), "fusion: the reserved fields must be 0")):
        cases.append((lambda kw=kw: run(n, point_rows, rows, P_(**dict(good, **kw))), msg))
    # a NULL buffer: the points, then an output
    out = Outputs(n, point_rows)
    args = lambda: [dev["points"].data_ptr(), dev["p_desc"].data_ptr(), dev["np"].data_ptr(), n, point_rows, dev["t_desc"].data_ptr(),  # noqa: E731
                    dev["t_kp"].data_ptr(), dev["nt"].data_ptr(), n, rows, dev["views"][:n], P_(**good)]
    cases.append((lambda: ctx.match_fuse_pairs_device(*([0] + args()[1:]), *out.ptrs()), "fusion: NULL buffer"))
    cases.append((lambda: ctx.match_fuse_pairs_device(*args(), *((0,) + out.ptrs()[1:])), "fusion: NULL buffer"))
    for k, (call, msg) in enumerate(cases):
        with pytest.raises(binding.OrbError) as e:
            call()
        assert e.value.code == binding.SS_ERR_INVALID_ARG and e.value.message == msg, (k, e.value.message, msg)
    f = FC.scenes()[0]
    with pytest.raises(binding.OrbError) as e:
        ctx.match_fuse(f["view"], f["points"], f["p_desc"], f["t_desc"], f["t_kp"], P_(check_right=True, **good))
    assert e.value.message == "fusion: check_right needs the right coordinates of the train rows"
    pset = FC.PARAM_SETS[1]
    got = _run_pairs(ctx, dev, n, point_rows, rows, FC.set_params(binding, pset, **good), taken=pset["taken"])
    for k in range(n):
        _check(f"scene {k} after the refused calls", got, k, FC.scene_reference(k, pset))
