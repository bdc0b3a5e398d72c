"""GPU parity of the map-point projection search (ss_match_proj_pairs_device, ss_match_proj_batch_device, ss_match_proj) against
tests/proj_ref.py: bit for bit, no tolerance -- idx, d1, d2 and the ss_proj_point of every row, every summary field.  Every output
starts prefilled with a pattern no result has; rows past the points must be "none".  tests/test_proj_ref.py asserts on the
reference that the shared cases are live."""
import numpy as np
import pytest

import guided_cases as G
import proj_cases as PC
import proj_ref as P

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).to(_dev())


class Outputs:
    """device idx / d1 / d2 / proj [n, rows] and summaries [n], prefilled with a pattern no result has"""

    def __init__(self, n, rows):
        import torch
        self.n, self.rows = n, rows
        self.idx = torch.full((n, rows), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        self.d1 = torch.full((n, rows), 0x5A5A, dtype=torch.int16, device=_dev())
        self.d2 = torch.full((n, rows), 0x5A5A, dtype=torch.int16, device=_dev())
        self.proj = torch.full((n, rows * 32), 0x5A, dtype=torch.uint8, device=_dev())
        self.summary = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=_dev())

    def ptrs(self):
        return self.idx.data_ptr(), self.d1.data_ptr(), self.d2.data_ptr(), self.proj.data_ptr(), self.summary.data_ptr()

    def host(self):
        from send_slam_amd import binding
        summ = self.summary.cpu().numpy().copy().view(binding.PROJ_SUMMARY_DTYPE).reshape(self.n)
        proj = self.proj.cpu().numpy().copy().view(binding.PROJ_POINT_DTYPE).reshape(self.n, self.rows)
        return (self.idx.cpu().numpy(), self.d1.cpu().numpy().view(np.uint16), self.d2.cpu().numpy().view(np.uint16), proj,
                [{f: int(s[f]) for f in P.SUMMARY_FIELDS} for s in summ])


def _check(tag, got, b, want):
    """frame b of a call's host outputs against a reference result (idx, d1, d2, proj, summary, ...)"""
    idx, d1, d2, proj, summ = got
    widx, wd1, wd2, wproj, wsumm = want[:5]
    n = len(widx)
    assert summ[b] == wsumm, f"{tag}: summary {summ[b]} != {wsumm}"
    for name, g, w in (("idx", idx[b], widx), ("d1", d1[b], wd1), ("d2", d2[b], wd2)):
        bad = np.flatnonzero(g[:n] != w)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {g[:n][bad[:8]]} != {w[bad[:8]]}"
    for name in P.POINT_DTYPE.names:  # bit for bit
        bad = np.flatnonzero(proj[b][name][:n].view(np.int32) != wproj[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {proj[b][name][:n][bad[:8]]} != {wproj[name][bad[:8]]}"
    assert (idx[b][n:] == -1).all() and (d1[b][n:] == P.NONE).all() and (d2[b][n:] == P.NONE).all(), f"{tag}: rows past the points are not 'none'"
    assert proj[b][n:].tobytes() == P.none_points(len(proj[b]) - n).tobytes(), f"{tag}: rows past the points are not 'none'"


def _upload(frames, point_rows, rows):
    """frames: dicts view points p_desc t_kp t_desc [right] [taken] -> device arrays of the pairs form, block b = frame b;
    [n_points] [n_train]: the counts the device is told, where they are not the lengths of the arrays"""
    from send_slam_amd import binding
    n = len(frames)
    host = {"points": np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), "p_desc": np.zeros((n, point_rows, 32), np.uint8),
            "t_desc": np.zeros((n, rows, 32), np.uint8), "t_kp": np.zeros((n, rows), binding.KP_DTYPE), "right": np.full((n, rows), -1, np.float32),
            "taken": np.zeros((n, rows), np.uint8), "np": np.zeros(n, np.int32), "nt": np.zeros(n, np.int32)}
    for b, f in enumerate(frames):
        k, nt = len(f["points"]), len(f["t_kp"])
        host["np"][b], host["nt"][b] = f.get("n_points", k), f.get("n_train", nt)
        host["points"][b, :k], host["p_desc"][b, :k] = f["points"], f["p_desc"]
        host["t_desc"][b, :nt], host["t_kp"][b, :nt] = f["t_desc"], f["t_kp"]
        if "right" in f:
            host["right"][b, :nt] = f["right"]
        if "taken" in f:
            host["taken"][b, :nt] = f["taken"]
    # past the counts: rows that would match anything if they were read (taken 0, right -1 = unchecked, all-zero descriptors)
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["views"] = np.concatenate([np.asarray(f["view"]).reshape(1) for f in frames])
    return dev


def _run_pairs(ctx, dev, n, point_rows, rows, params, taken=True, right=True, point_src=None, n_blocks=None):
    out = Outputs(n, point_rows)
    ctx.match_proj_pairs_device(dev["points"].data_ptr(), dev["p_desc"].data_ptr(), dev["np"].data_ptr(), n if n_blocks is None else n_blocks, point_rows,
                                dev["t_desc"].data_ptr(), dev["t_kp"].data_ptr(), dev["nt"].data_ptr(), n, rows, dev["views"][:n], params, *out.ptrs(),
                                point_src=point_src, d_train_right=dev["right"].data_ptr() if right else 0,
                                d_train_taken=dev["taken"].data_ptr() if taken else 0)
    ctx.synchronize()
    return out.host()


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


def _boundary_table_on(c, sc, tag):
    """the boundary table of a pyramid table through the pairs form and the host twin of a context that holds that table"""
    from send_slam_amd import binding
    view, points, groups, tk, td, pd = PC.boundary_table(sc)
    want = P.match(view, points, pd, tk, td, sc, th_high=256, ratio_num=0, ratio_den=0, **PC.B_LIMITS)
    proj = want[3]
    for name, a, live in groups:  # every case is live, on the reference
        rows = {(int(proj["state"][i]), int(proj["level"][i]), float(proj["radius"][i])) for i in range(a, a + 3)}
        assert (len(rows) > 1) == live, (tag, name, rows)
    frame = {"view": view, "points": points, "p_desc": pd, "t_kp": tk, "t_desc": td}
    point_rows, rows = len(points) + 3, len(tk) + 1
    dev = _upload([frame], point_rows, rows)
    p = binding.proj_params(th_high=256, ratio_num=0, ratio_den=0, extent_w=G.W, extent_h=G.H, **PC.B_LIMITS)
    _check(tag, _run_pairs(c, dev, 1, point_rows, rows, p, taken=False, right=False), 0, want)
    got = binding.proj_points_host(view, p, sc, points)
    assert got.tobytes() == proj.tobytes(), tag
    return want


@pytest.mark.parametrize("name", list(PC.PYRAMIDS))
def test_boundary_table_under_other_pyramid_tables(name):
    """contexts with one level (octaves -1 .. 0 only), two levels, a scale factor of 2 and SS_MAX_LEVELS levels: the ratio on
    every scale[n] with np.nextafter on both sides, ratios below scale[0] and above the last entry"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        want = _boundary_table_on(c, sc, name)
    levels = set(int(v) for v in want[3]["level"][want[3]["state"] == 0])
    assert levels == set(range(n_levels)) and want[4]["n_accepted"] > 10, (name, levels)


def test_boundary_table(ctx):
    """identity pose, exact products: z at 0, u / v on each image bound, dist on 0.8f * min_dist, 1.2f * max_dist and far_limit,
    view_cos on the limit and on 0.998, the ratio on every scale[n], each with np.nextafter on both sides; NaN and infinite
    coordinates; ratios below 1 and above the last entry"""
    want = _boundary_table_on(ctx, PC.scale(), "boundary table")
    assert want[4]["n_candidates"] > 20 and want[4]["n_accepted"] > 10


def test_level_aware_ratio_taken_row_and_right_eye(ctx):
    """under 8 / 10: at one level 8 against 9 is rejected, 8 against 10 accepted (equality accepts), 8 against 11 accepted; at
    different levels the ratio does not count; d1 == d2; a single candidate; predicted level 0 (octaves -1 .. 0); a taken row and
    a right-eye rejection that change the winner"""
    from send_slam_amd import binding
    view, frames = PC.ratio_frames()
    frames = [dict(f, view=view) for f in frames]
    point_rows, rows = 3, 5
    dev = _upload(frames, point_rows, rows)
    got = _run_pairs(ctx, dev, len(frames), point_rows, rows, binding.proj_params(extent_w=G.W, extent_h=G.H, **PC.RATIO_PARAMS))
    for b, f in enumerate(frames):
        want = P.match(view, f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), right=f["right"], taken=f["taken"], **PC.RATIO_PARAMS)
        assert want[0][0] == f["expect"], f["name"]
        _check(f["name"], got, b, want)
        assert got[0][b][0] == f["expect"], f["name"]


@pytest.fixture(scope="module")
def scene_arrays():
    frames = PC.scenes()
    point_rows, rows = 470, 483  # no multiple of the 64 points of a workgroup
    assert all(len(f["points"]) <= point_rows and len(f["t_kp"]) <= rows for f in frames)
    return _upload(frames, point_rows, rows), point_rows, rows


@pytest.mark.parametrize("combo", PC.COMBOS, ids=PC.combo_name)
def test_reprojected_scenes(ctx, scene_arrays, combo):
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    got = _run_pairs(ctx, dev, n, point_rows, rows, PC.combo_params(binding, combo, extent_w=G.W, extent_h=G.H), taken=combo["taken"],
                     right=combo["check_right"])
    for k in range(n):
        want = PC.scene_reference(k, combo)
        _check(f"scene {k} {PC.combo_name(combo)}", got, k, want)
    assert sum(s["n_accepted"] for s in got[4]) > 100


def test_host_form_equals_the_pairs_form(ctx, scene_arrays):
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    for combo in (PC.COMBOS[0], PC.COMBOS[-1], dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=True, taken=False)):
        p = PC.combo_params(binding, combo, extent_w=G.W, extent_h=G.H)
        pairs = _run_pairs(ctx, dev, len(PC.SCENES), point_rows, rows, p, taken=combo["taken"], right=combo["check_right"])
        for k, f in enumerate(PC.scenes()):
            idx, d1, d2, proj, summ = ctx.match_proj(f["view"], f["points"], f["p_desc"], f["t_desc"], f["t_kp"], p,
                                                     right=f["right"] if combo["check_right"] else None, taken=f["taken"] if combo["taken"] else None)
            n = len(idx)
            assert np.array_equal(idx, pairs[0][k][:n]) and np.array_equal(d1, pairs[1][k][:n]) and np.array_equal(d2, pairs[2][k][:n])
            assert proj.tobytes() == pairs[3][k][:n].tobytes() and summ == pairs[4][k]
            _check(f"host form, scene {k} {PC.combo_name(combo)}", (idx[None], d1[None], d2[None], proj[None], [summ]), 0, PC.scene_reference(k, combo))
    # empty sides
    f = PC.scenes()[0]
    p = binding.proj_params(extent_w=G.W, extent_h=G.H)
    idx, d1, d2, proj, summ = ctx.match_proj(f["view"], f["points"], f["p_desc"], f["t_desc"][:0], f["t_kp"][:0], p)
    assert (idx == -1).all() and (d1 == P.NONE).all() and summ["n_train"] == 0 and summ["n_points"] == len(idx) and summ["n_candidates"] == 0
    assert proj.tobytes() == PC.scene_proj(0, 1.0).tobytes() and summ["n_in_view"] == int((proj["state"] == 0).sum()) > 0
    idx, d1, d2, proj, summ = ctx.match_proj(f["view"], f["points"][:0], f["p_desc"][:0], f["t_desc"], f["t_kp"], p)
    assert len(idx) == 0 and summ["n_points"] == 0 and summ["n_train"] == len(f["t_kp"]) and summ["n_in_view"] == 0


def test_refused_arguments_leave_the_context_usable(ctx, scene_arrays):
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    good = dict(extent_w=G.W, extent_h=G.H)
    big = binding.SS_GUIDED_MAX_ROWS + 1
    calls = [lambda: _run_pairs(ctx, dev, 1, big, rows, binding.proj_params(**good)),
             lambda: _run_pairs(ctx, dev, 1, point_rows, big, binding.proj_params(**good)),
             lambda: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(**good), point_src=[0, n, 1]),
             lambda: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(**good), point_src=[0, -1, 1]),
             lambda: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(**good), n_blocks=2),  # frame 2 reads block 2
             lambda: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(extent_w=0, extent_h=G.H)),
             lambda: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(check_right=True, **good), right=False)]
    for kw in (dict(th=0.0), dict(th=float("nan")), dict(th=float("inf")), dict(view_cos_limit=float("nan")), dict(th_high=257), dict(th_high=-1),
               dict(ratio_num=32768), dict(ratio_den=-1)):
        calls.append(lambda kw=kw: _run_pairs(ctx, dev, n, point_rows, rows, binding.proj_params(**dict(good, **kw))))
    for k, call in enumerate(calls):
        with pytest.raises(binding.OrbError) as e:
            call()
        assert e.value.code == binding.SS_ERR_INVALID_ARG, k
        if k < 2:
            assert "SS_GUIDED_MAX_ROWS" in e.value.message
        if k in (2, 3):
            assert "point_src[1]" in e.value.message
    combo = PC.COMBOS[3]
    got = _run_pairs(ctx, dev, n, point_rows, rows, PC.combo_params(binding, combo, **good), taken=combo["taken"], right=combo["check_right"])
    for k in range(n):
        _check(f"scene {k} after the refused calls", got, k, PC.scene_reference(k, combo))
    # point_src: every frame searches the points of block 2; a frame's own train rows stay its own
    got = _run_pairs(ctx, dev, n, point_rows, rows, PC.combo_params(binding, combo, **good), taken=combo["taken"], right=combo["check_right"],
                     point_src=[2, 2, 2])
    _check("point_src, frame 2", got, 2, PC.scene_reference(2, combo))
    f, s = PC.scenes()[2], PC.scenes()[0]
    want = P.match(s["view"], f["points"], f["p_desc"], s["t_kp"], s["t_desc"], PC.scale(), th=combo["th"], ratio_num=combo["ratio"][0],
                   ratio_den=combo["ratio"][1], one_to_one=combo["one_to_one"], check_right=combo["check_right"], right=s["right"],
                   taken=s["taken"] if combo["taken"] else None)
    _check("point_src, frame 0 on block 2", got, 0, want)


BATCH = ["synth_t0", "synth_t1", "checker_shift"]


def test_batch_form():
    """three extracted frames, point_src [0, 0, 1], block 1 empty: frames 0 and 1 search the same map points under their own
    views, frame 2 has none"""
    import torch
    from send_slam_amd import binding
    frames = np.stack([G.frame(n) for n in BATCH])
    s0, s1 = PC.scenes()[0], PC.scenes()[1]
    views = np.concatenate([np.asarray(v).reshape(1) for v in (s0["view"], s1["view"], s1["view"])])
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(BATCH)) as c:
        d = torch.from_numpy(frames).to(_dev())
        c.extract_batch_device(d.data_ptr(), len(BATCH), G.W, G.H)
        c.synchronize()
        for b, n in enumerate(BATCH):  # the references are computed on the oracle's features
            kp, desc, _ = c.fetch_frame(b)
            okp, odesc = G.features(n)
            assert kp.tobytes() == okp.tobytes() and np.array_equal(desc, odesc), f"frame {b} ({n}): extraction differs from the oracle"
        kcap = c.batch_view().kp_capacity
        point_rows, n_blocks = 500, 2
        pts = np.zeros((n_blocks, point_rows), binding.MAP_POINT_DTYPE)
        pd = np.zeros((n_blocks, point_rows, 32), np.uint8)
        k = len(s0["points"])
        pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
        pts[1], pd[1] = s0["points"][0], s0["p_desc"][0]  # block 1 is empty by its count, not by its content
        counts = np.array([k, 0], np.int32)
        right, taken = np.full((len(BATCH), kcap), -1, np.float32), np.zeros((len(BATCH), kcap), np.uint8)
        for b, s in enumerate((s0, s1)):
            right[b, :len(s["right"])], taken[b, :len(s["taken"])] = s["right"], s["taken"]
        d_pts, d_pd, d_n, d_right, d_taken = (_to_dev(a) for a in (pts, pd, counts, right, taken))
        for combo in (dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=True, taken=True), PC.COMBOS[0]):
            out = Outputs(len(BATCH), point_rows)
            c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, PC.combo_params(binding, combo),
                                      *out.ptrs(), point_src=[0, 0, 1], d_train_right=d_right.data_ptr() if combo["check_right"] else 0,
                                      d_train_taken=d_taken.data_ptr() if combo["taken"] else 0)
            c.synchronize()
            got = out.host()
            _check("batch frame 0", got, 0, PC.scene_reference(0, combo))
            tk, td = G.features(BATCH[1])
            want = P.match(s1["view"], s0["points"], s0["p_desc"], tk, td, PC.scale(), th=combo["th"], ratio_num=combo["ratio"][0],
                           ratio_den=combo["ratio"][1], one_to_one=combo["one_to_one"], check_right=combo["check_right"], right=s1["right"],
                           taken=s1["taken"] if combo["taken"] else None)
            _check("batch frame 1", got, 1, want)
            assert want[4]["n_accepted"] > 50
            tk2, td2 = G.features(BATCH[2])
            none = P.match(s1["view"], s0["points"][:0], s0["p_desc"][:0], tk2, td2, PC.scale())
            _check("batch frame 2 (empty block)", got, 2, none)
            assert got[4][2]["n_train"] == len(tk2) > 100
        with pytest.raises(binding.OrbError) as e:
            c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, binding.proj_params(), *out.ptrs(),
                                      point_src=[0, 2, 1])
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "point_src[1]" in e.value.message
    with binding.OrbContext(0, n_features=G.NF) as c:  # no batch
        with pytest.raises(binding.OrbError) as e:
            c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_blocks, point_rows, views, binding.proj_params(), *out.ptrs())
        assert e.value.code == binding.SS_ERR_STATE


# ---- odd cameras, per frame ----------------------------------------------------------------------------------------------------------------
CAMERA_ROWS = (470, 483)  # no multiple of the 64 points of a workgroup


@pytest.mark.parametrize("shared", [False, True], ids=["own_blocks", "one_shared_block"])
def test_three_cameras_per_call(ctx, shared):
    """one call whose frames are seen by camera A, camera B and the square camera (fx != fy, principal points off the centre, three
    values of bf, check_right on), each on its own block of points and all on block 0 (point_src [0, 0, 0]); the pairs form and the
    host form.  tests/test_proj_ref.py shows that a kernel which exchanged fx and fy or cx and cy, or read another frame's view or
    bf, would give other bytes"""
    from send_slam_amd import binding
    frames, combo = PC.camera_scenes(), PC.CAMERA_COMBO
    point_rows, rows = CAMERA_ROWS
    assert len({f["view"].tobytes() for f in frames}) == 3
    dev = _upload(frames, point_rows, rows)
    p = PC.combo_params(binding, combo, extent_w=G.W, extent_h=G.H)
    got = _run_pairs(ctx, dev, 3, point_rows, rows, p, point_src=[0, 0, 0] if shared else None, n_blocks=1 if shared else None)
    for k, f in enumerate(frames):
        want = PC.camera_reference(k, shared)
        _check(f"cameras, frame {k}", got, k, want)
        b = frames[0] if shared else f
        idx, d1, d2, proj, summ = ctx.match_proj(f["view"], b["points"], b["p_desc"], f["t_desc"], f["t_kp"], p, right=f["right"], taken=f["taken"])
        _check(f"cameras, host form, frame {k}", (idx[None], d1[None], d2[None], proj[None], [summ]), 0, want)
    assert sum(s["n_unique"] for s in got[4]) > 200


@pytest.mark.parametrize("shared", [False, True], ids=["own_blocks", "one_shared_block"])
def test_batch_form_under_a_camera_per_frame(shared):
    """ss_match_proj_batch_device on three extracted frames (the train frames of the camera scenes) under three cameras"""
    from send_slam_amd import binding
    from test_guided import _extract
    frames, combo = PC.camera_scenes(), PC.CAMERA_COMBO
    n, point_rows = 3, 500
    views = np.concatenate([np.asarray(f["view"]).reshape(1) for f in frames])
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, [train for _, train in PC.SCENES])
        pts, pd = np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), np.zeros((n, point_rows, 32), np.uint8)
        right, taken = np.full((n, kcap), -1, np.float32), np.zeros((n, kcap), np.uint8)
        for b, f in enumerate(frames):
            pts[b, :len(f["points"])], pd[b, :len(f["points"])] = f["points"], f["p_desc"]
            right[b, :len(f["right"])], taken[b, :len(f["taken"])] = f["right"], f["taken"]
        counts = np.array([len(f["points"]) for f in frames], np.int32)
        d_pts, d_pd, d_n, d_right, d_taken = (_to_dev(a) for a in (pts, pd, counts, right, taken))
        out = Outputs(n, point_rows)
        import torch
        torch.cuda.synchronize()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1 if shared else n, point_rows, views, PC.combo_params(binding, combo),
                                  *out.ptrs(), point_src=[0, 0, 0] if shared else None, d_train_right=d_right.data_ptr(), d_train_taken=d_taken.data_ptr())
        c.synchronize()
        got = out.host()
    for k in range(n):
        _check(f"cameras, batch form, frame {k}", got, k, PC.camera_reference(k, shared))


def test_full_capacity(ctx):
    """two frames with point_rows = rows_per_frame = SS_GUIDED_MAX_ROWS, one_to_one on, dense coordinates: contested train rows on
    both sides of the 8192-row pass of the conflict table (tests/test_proj_ref.py counts them), 64 px cells"""
    from send_slam_amd import binding
    frames = PC.capacity_frames()
    rows = PC.CAP_ROWS
    assert rows == binding.SS_GUIDED_MAX_ROWS
    dev = _upload(frames, rows, rows)
    p = binding.proj_params(extent_w=PC.CAP_W, extent_h=PC.CAP_H, **PC.CAP_PARAMS)
    got = _run_pairs(ctx, dev, 2, rows, rows, p)
    for b in range(2):
        want = PC.capacity_reference(b)
        print(b, want[4])
        _check(f"capacity frame {b}", got, b, want)
        assert (want[0] >= 8192).sum() > 1000


# ---- other grids, the image's edge, counts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", PC.EXTENT_COMBOS, ids=PC.combo_name)
@pytest.mark.parametrize("extent", PC.EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_scenes_on_other_grids(ctx, scene_arrays, extent, combo):
    """the extent sizes the index and never the answer: 256 px cells, 4096 x 1 cells, an extent beyond 2^24, 157 x 2 cells, one
    cell, extents smaller than the keypoints' spread"""
    from send_slam_amd import binding
    dev, point_rows, rows = scene_arrays
    n = len(PC.SCENES)
    got = _run_pairs(ctx, dev, n, point_rows, rows, PC.combo_params(binding, combo, extent_w=extent[0], extent_h=extent[1]), taken=combo["taken"],
                     right=combo["check_right"])
    for k in range(n):
        _check(f"scene {k} {PC.combo_name(combo)} on {extent}", got, k, PC.scene_reference(k, combo))
    assert sum(s["n_accepted"] for s in got[4]) > 100


@pytest.mark.parametrize("extent", [(PC.E_W, PC.E_H), (64, 64), (1 << 25, 1 << 25)], ids=lambda e: f"{e[0]}x{e[1]}")
def test_windows_at_the_edge_of_the_image_and_beyond(ctx, extent):
    """projections on each image bound and one float32 step inside and outside it, radii from 4 px to 4e30 px, train rows in the
    border cells, on the last pixel, on the bound and outside the extent"""
    from send_slam_amd import binding
    view, points, pd, tk, td = PC.edge_table()
    frame = {"view": view, "points": points, "p_desc": pd, "t_kp": tk, "t_desc": td}
    point_rows, rows = len(points) + 2, len(tk) + 5
    dev = _upload([frame], point_rows, rows)
    for th in PC.E_THS:
        want = PC.edge_reference(th)
        p = binding.proj_params(extent_w=extent[0], extent_h=extent[1], **dict(PC.E_PARAMS, th=th))
        got = _run_pairs(ctx, dev, 1, point_rows, rows, p, taken=False, right=False)
        print(th, want[4])
        _check(f"edge table, th {th}, extent {extent}", got, 0, want)
        assert binding.proj_points_host(view, p, PC.scale(), points).tobytes() == want[3].tobytes()


def test_a_distance_of_256_is_accepted_at_th_high_256_only(ctx):
    from send_slam_amd import binding
    f = PC.far_descriptor_frame()
    dev = _upload([f], 2, 3)
    for th_high, idx in ((256, 0), (255, -1)):
        kw = dict(PC.RATIO_PARAMS, th_high=th_high, check_right=False)
        want = P.match(f["view"], f["points"], f["p_desc"], f["t_kp"], f["t_desc"], PC.scale(), **kw)
        assert want[0][0] == idx and want[1][0] == 256 and want[4]["n_candidates"] == 1
        got = _run_pairs(ctx, dev, 1, 2, 3, binding.proj_params(extent_w=G.W, extent_h=G.H, **kw), taken=False, right=False)
        _check(f"th_high {th_high}", got, 0, want)
        assert got[0][0][0] == idx and got[1][0][0] == 256


def test_counts_at_zero_one_a_workgroup_and_above_the_rows(ctx):
    """one call, every frame holds the same 65 live points and train rows; only the counts differ: 0, 1, 63, 64, 65, above the row
    counts (clamped) and negative (0)"""
    from send_slam_amd import binding
    base, counts = PC.count_frames()
    frames = [dict(base, n_points=k, n_train=nt) for k, nt in counts]
    rows = PC.COUNT_ROWS
    dev = _upload(frames, rows, rows)
    got = _run_pairs(ctx, dev, len(frames), rows, rows, binding.proj_params(extent_w=G.W, extent_h=G.H, **PC.COUNT_PARAMS))
    for b, (k, nt) in enumerate(counts):
        _check(f"counts {k} / {nt}", got, b, PC.count_reference(k, nt))
    assert PC.count_reference(65, 65)[4]["n_unique"] > 30


FLAG_BATCH = ["synth_t0", "synth_t1", "synth_t2", "synth_t3"]


def _flag_run(binding, combo):
    """the batch form on FLAG_BATCH: every frame searches the map points of scene 0 under scene 0's view"""
    import torch
    s0 = PC.scenes()[0]
    frames = np.stack([G.frame(n) for n in FLAG_BATCH])
    n = len(FLAG_BATCH)
    views = np.concatenate([np.asarray(s0["view"]).reshape(1)] * n)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        d = torch.from_numpy(frames).to(_dev())
        c.extract_batch_device(d.data_ptr(), n, G.W, G.H)
        c.synchronize()
        for b, name in enumerate(FLAG_BATCH):  # the references are computed on the oracle's features
            kp, desc, _ = c.fetch_frame(b)
            okp, odesc = G.features(name)
            assert kp.tobytes() == okp.tobytes() and np.array_equal(desc, odesc), f"frame {b} ({name}): extraction differs from the oracle"
        point_rows = 470
        dev = _upload([dict(s0, t_kp=s0["t_kp"][:0], t_desc=s0["t_desc"][:0], right=s0["right"][:0], taken=s0["taken"][:0])], point_rows, 1)
        out = Outputs(n, point_rows)
        torch.cuda.synchronize()
        c.match_proj_batch_device(dev["points"].data_ptr(), dev["p_desc"].data_ptr(), dev["np"].data_ptr(), 1, point_rows, views,
                                  PC.combo_params(binding, combo), *out.ptrs(), point_src=[0] * n)
        c.synchronize()  # raises nothing: the extraction's own frame_error is clean
        return out.host()


def test_flagged_frames_are_voided_in_the_batch_form(monkeypatch):
    """SENDSLAM_TEST_FLAG_BATCH=1,2: frames 1 and 2 are flagged although they have keypoints: status, zero counts, every row "none";
    frames 0 and 3 are what the unflagged run and the reference give"""
    from send_slam_amd import binding
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    plain = _flag_run(binding, combo)
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1,2")
    flagged = _flag_run(binding, combo)
    s0 = PC.scenes()[0]
    kw = dict(th=combo["th"], ratio_num=combo["ratio"][0], ratio_den=combo["ratio"][1], one_to_one=True)
    for b, name in enumerate(FLAG_BATCH):
        tk, td = G.features(name)
        want = P.match(s0["view"], s0["points"], s0["p_desc"], tk, td, PC.scale(), **kw)
        _check(f"unflagged, frame {b}", plain, b, want)
        assert want[4]["n_train"] > 100 and want[4]["n_in_view"] > 100
        if b in (1, 2):
            none = P.match(s0["view"], s0["points"][:0], s0["p_desc"][:0], tk[:0], td[:0], PC.scale(), **kw)
            _check(f"frame {b} flagged", flagged, b, none[:4] + (dict(none[4], status=binding.SS_ERR_OVERFLOW),))
        else:
            _check(f"flagged run, frame {b}", flagged, b, want)
            assert all(np.array_equal(flagged[j][b], plain[j][b]) for j in range(3)) and flagged[3][b].tobytes() == plain[3][b].tobytes()
            assert want[4]["n_unique"] > (50 if b == 0 else 0)
