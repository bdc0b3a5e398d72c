"""GPU parity of the covisibility family (ss_covis_set_map, ss_covis_kf_device, ss_covis_frames_device, ss_covis) against
tests/covis_ref.py (the shared cases, the calls) and the host twin through the C ABI (the ladders): exactly, no tolerance -- every entry
of every neighbour list and every field of every ss_covis_row.  Every output starts prefilled with a pattern no result has.
tests/test_covis_ref.py asserts on the reference that the cases are live and holds the host twin to the reference at the ladders' sizes."""
import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
import guided_cases as G

pytestmark = pytest.mark.gpu

FILL = 0x5A
SHARED, LADDERS = CC.shared_cases(), CC.ladder_cases()


def _dev():
    import torch
    return torch.device("cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()  # the library's stream does not wait for torch's


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


class Out:
    """device neighbour lists [n_rows][cap][2] and rows [n_rows], prefilled with a pattern no result has"""

    def __init__(self, n_rows, cap):
        import torch
        self.n_rows, self.cap = n_rows, cap
        self.nb = torch.full((max(n_rows, 1), cap * 8), FILL, dtype=torch.uint8, device=_dev())
        self.row = torch.full((max(n_rows, 1), 32), FILL, dtype=torch.uint8, device=_dev())
        _sync()

    def ptrs(self):
        return self.nb.data_ptr(), self.row.data_ptr()

    def raw(self):
        return self.nb.cpu().numpy().copy(), self.row.cpu().numpy().copy()

    def host(self):
        nb, row = self.raw()
        return nb.view(np.int32).reshape(-1, self.cap, 2)[:self.n_rows], row.view(CR.ROW_DTYPE).reshape(-1)[:self.n_rows]


def _params(p):
    from send_slam_amd import binding
    return binding.covis_params(**p)


def set_map(ctx, call):
    ctx.covis_set_map(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], cull_skip=call["skip"], check_right=call["check_right"])


def run_kf(ctx, call, params, cap, rows=None, n_rows=None, out=None):
    if call is not None:
        set_map(ctx, call)
    n_rows = (len(rows) if rows is not None else call["n_kf"]) if n_rows is None else n_rows
    out = out or Out(n_rows, cap)
    ctx.covis_kf_device(rows, n_rows, _params(params), cap, *out.ptrs())
    ctx.synchronize()
    return out.host()


def run_frames(ctx, call, idx, n_points, point_src, params, cap):
    if call is not None:
        set_map(ctx, call)
    d_idx, d_np = _to_dev(np.asarray(idx, np.int32)), _to_dev(np.asarray(n_points, np.int32))
    out = Out(len(point_src), cap)
    ctx.covis_frames_device(d_idx.data_ptr(), d_np.data_ptr(), point_src, _params(params), cap, *out.ptrs())
    ctx.synchronize()
    return out.host()


def twin_kf(call, params, cap, rows=None):
    from send_slam_amd import binding
    return binding.covis_kf_host(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], CC.N_LEVELS, _params(params), cap, rows=rows,
                                 cull_skip=call["skip"], check_right=call["check_right"])


def same(tag, got, want):
    nb, row = got
    wnb, wrow = want
    assert nb.shape == wnb.shape and len(row) == len(wrow), tag
    for name in CR.ROW_DTYPE.names:
        assert np.array_equal(row[name], wrow[name]), f"{tag}: row.{name} {row[name][:8]} != {wrow[name][:8]} at rows {np.flatnonzero(row[name] != wrow[name])[:8]}"
    assert np.array_equal(nb, wnb), f"{tag}: neighbour lists differ in rows {np.flatnonzero((nb != wnb).any(axis=(1, 2)))[:8]}"


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        assert CC.N_LEVELS == 8
        yield c


@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_cases_against_the_reference(ctx, name):
    c = SHARED[name]
    call = CC.single(c)
    same(name, run_kf(ctx, call, c["params"], c["cap"], c["rows"]), CR.kf_rows(CC.ref_map(call), c["rows"], c["params"], c["cap"]))


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladders_against_the_host_twin(ctx, name):
    c = LADDERS[name]
    call = CC.single(c)
    same(name, run_kf(ctx, call, c["params"], c["cap"], c["rows"]), twin_kf(call, c["params"], c["cap"], c["rows"]))


def test_two_problems_in_either_order_with_gaps_junk_shuffled_records_and_rows_in_any_order(ctx):
    cases = [LADDERS["kf_65"], dict(LADDERS["items_257"], check_right=True)]
    params = cases[0]["params"]
    for order, lead, gap, seed in (([0, 1], 0, 0, None), ([1, 0], 2, 3, 5)):
        call = CC.stack(cases, 100, lead=lead, gap=gap, order=order, shuffle_seed=seed)
        whole = run_kf(ctx, call, params, 48)
        same(f"order {order}: rows NULL", whole, CR.kf_rows(CC.ref_map(call), None, params, 48))
        rows = np.array([call["n_kf"] - 1, 0, 3, 3, 1] + list(range(call["n_kf"] - 1, -1, -1)), np.int32)
        explicit = run_kf(ctx, None, params, 48, rows)  # the map stays
        same(f"order {order}: explicit rows, duplicates, reversed", explicit, (whole[0][rows], whole[1][rows]))
        same(f"order {order}: the same call twice", run_kf(ctx, None, params, 48, rows), explicit)


def test_a_small_map_after_a_large_one_then_no_map(ctx):
    from send_slam_amd import binding
    big, small = LADDERS["kf_1025"], SHARED["lonely"]
    call = CC.single(big)
    same("large", run_kf(ctx, call, dict(min_weight=1), 1024, [0, 1024]), twin_kf(call, dict(min_weight=1), 1024, [0, 1024]))
    call = CC.single(small)
    same("small after large", run_kf(ctx, call, dict(min_weight=1), 1024), CR.kf_rows(CC.ref_map(call), None, dict(min_weight=1), 1024))
    out = Out(3, 4)
    ctx.covis_kf_device(None, 0, _params({}), 4, *out.ptrs())  # no row: SS_OK, nothing written
    ctx.covis_set_map(np.zeros(0, binding.GBA_PROBLEM_DTYPE), 0, 0, 6, call["obs"][:0])  # no problem: the map is cleared
    for query in (lambda: ctx.covis_kf_device(None, 3, _params({}), 4, *out.ptrs()), lambda: ctx.covis_kf_device([0], 1, _params({}), 4, *out.ptrs()),
                  lambda: ctx.covis_frames_device(out.nb.data_ptr(), out.nb.data_ptr(), [0], _params({}), 4, *out.ptrs())):
        with pytest.raises(binding.OrbError) as e:
            query()
        assert e.value.code == binding.SS_ERR_STATE and "no map (ss_covis_set_map)" in e.value.message
    ctx.synchronize()
    assert all((a == FILL).all() for a in out.raw())


def test_frame_rows(ctx):
    call, idx, n_points, point_src = CC.frames_case()
    m = CC.ref_map(call)
    for params, cap in ((dict(min_weight=1), 64), (dict(min_weight=3, fallback=0), 5)):
        same(f"frames {params}", run_frames(ctx, call, idx, n_points, point_src, params, cap), CR.frame_rows(m, idx, n_points, point_src, params, cap))
    same("keyframe rows of the same map", run_kf(ctx, None, {}, 8, n_rows=call["n_kf"]), CR.kf_rows(m, None, {}, 8))


def test_two_frames_of_the_largest_row_count(ctx):
    rows = 16384  # SS_GUIDED_MAX_ROWS
    rng = np.random.default_rng(21)
    kfs = rng.integers(0, 300, (rows, 3)).astype(np.int32)
    kfs[:, 1] = (kfs[:, 0] + 1 + kfs[:, 1] % 299) % 300  # two distinct keyframes per point, and keyframe 300 on every one
    obs = np.concatenate([CR.obs_records(kfs[:, 0], np.arange(rows, dtype=np.int32)), CR.obs_records(kfs[:, 1], np.arange(rows, dtype=np.int32)),
                          CR.obs_records(np.full(rows, 300, np.int32), np.arange(rows, dtype=np.int32))])
    call = CC.single(CC.case(301, rows, [obs]), rows)
    idx = np.stack([np.zeros(rows, np.int32), np.where(rng.random(rows) < 0.5, 7, -1).astype(np.int32)])
    got = run_frames(ctx, call, idx, [rows], [0, 0], dict(min_weight=40), 1024)
    same("two frames of SS_GUIDED_MAX_ROWS rows", got, CR.frame_rows(CC.ref_map(call), idx, [rows], [0, 0], dict(min_weight=40), 1024))
    assert got[0][0][0].tolist() == [300, rows] and got[1]["n_shared"].tolist() == [301, 301]


def test_the_host_pointer_form(ctx):
    for name in ("culling", "planted", "items_513"):
        c = dict(SHARED, **LADDERS)[name]
        nb, row = ctx.covis(c["n_kf"], c["n_points"], c["obs"], _params(c["params"]), c["cap"], cull_skip=c["skip"], check_right=c["check_right"])
        same(name, (nb, row), CR.kf_rows(CC.ref_map(CC.single(c)), None, c["params"], c["cap"]))
    big = LADDERS["key_ends"]  # 16 383 points: one block; one more point than a block holds: two blocks
    obs = np.concatenate([big["obs"], CR.obs_records([0, 16383, 0, 16383], [16383, 16383, 16384, 16384])])
    nb, row = ctx.covis(16384, 16385, obs, _params(dict(min_weight=1)), 2)
    assert nb[0].tolist() == [[16383, 16385], [5, 3]] and nb[16383].tolist() == [[0, 16385], [5, 3]] and nb[5].tolist() == [[0, 3], [16383, 3]] and row["n_shared"][1] == 0


def test_stats_stages_and_their_bytes():
    from send_slam_amd import binding
    call, idx, n_points, point_src = CC.frames_case()
    with binding.OrbContext(0, n_features=G.NF) as c:
        c.profile(True)
        run_kf(c, call, {}, 8)
        run_kf(c, None, {}, 8, [1, 2, 3])
        run_frames(c, None, idx, n_points, point_src, {}, 16)
        stats = {s["name"]: (s["launches"], s["algorithmic_bytes"]) for s in c.stats()}
    items, K = int(call["table"]["n_obs"].sum()), call["n_kf"]
    assert stats["covis_kf"] == (2, items * 20 * 3 // K + 3 * (8 * 8 + 36)) and stats["covis_frames"] == (1, len(point_src) * (call["point_rows"] * 12 + 16 * 8 + 36))
    assert stats["covis_upload"][0] == 1 and stats["covis_upload"][1] >= items * 12 + call["n_blocks"] * call["point_rows"] * 8 + K * 12


def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    c = SHARED["planted"]
    call = CC.single(c)
    want = CR.kf_rows(CC.ref_map(call), None, {}, 4)
    same("before the refusals", run_kf(ctx, call, {}, 4), want)
    t = lambda *rows: np.array([r + ((0, 0),) if len(r) == 6 else r for r in rows], binding.GBA_PROBLEM_DTYPE)  # noqa: E731
    n_o, P = len(call["obs"]), call["point_rows"]
    good = dict(problems=call["table"], n_kf=41, n_blocks=1, point_rows=P, obs=call["obs"])
    kf_out, pt_out, twice = call["obs"].copy(), call["obs"].copy(), call["obs"].copy()
    kf_out["kf"][5], pt_out["point"][6], twice[8] = 41, P, twice[2]
    heavy = CR.obs_records(np.zeros(CR.MAX_ROW_ITEMS + 1, np.int32), np.arange(CR.MAX_ROW_ITEMS + 1, dtype=np.int32))
    bad = [(dict(problems=t((0, 0, 0, 1, 0, n_o))), "n_kf 0 outside 1 .. SS_GBA_MAX_KF (16384)"), (dict(problems=t((0, 16385, 0, 1, 0, n_o)), n_kf=16385), "n_kf 16385 outside 1 .. SS_GBA_MAX_KF"),
           (dict(problems=t((0, 41, 0, 65, 0, n_o)), n_blocks=65, point_rows=16384), "n_blocks 65 of 16384 rows outside 0 .. SS_GBA_MAX_POINTS (1048576) points"),
           (dict(problems=t((0, 41, 0, 1, 0, -1))), "n_obs -1 outside 0 .. SS_GBA_MAX_OBS (4194304)"),
           (dict(problems=t((1, 41, 0, 1, 0, n_o))), "keyframes 1 .. + 41 lie outside the call's 41"), (dict(problems=t((0, 41, 1, 1, 0, n_o))), "blocks 1 .. + 1 lie outside the call's 1"),
           (dict(problems=t((0, 41, 0, 1, 1, n_o))), f"records 1 .. + {n_o} lie outside the call's {n_o}"),
           (dict(problems=t((0, 41, 0, 1, 0, n_o, (0, 1)))), "problem 0: the reserved fields must be 0"),
           (dict(problems=t((0, 2, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0))), "problem 1: keyframe 1 belongs to problem 0 already"),
           (dict(problems=t((0, 2, 0, 1, 0, 0), (2, 2, 0, 1, 0, 0))), "problem 1: block 0 belongs to problem 0 already"),
           (dict(problems=t((0, 2, 0, 0, 0, 3), (2, 2, 0, 0, 2, 3))), "problem 1: record 2 belongs to problem 0 already"),
           (dict(obs=kf_out), "covis: problem 0: record 5: kf 41 outside 0 .. 40"), (dict(obs=pt_out), f"problem 0: record 6: point {P} outside 0 .. {P - 1}"),
           (dict(obs=twice), f"record 8: the pair (kf {twice['kf'][2]}, point {twice['point'][2]}) has a record already"),
           (dict(n_blocks=-1), "bad keyframe, problem, block, row or record count"), (dict(point_rows=0), "bad keyframe, problem, block, row or record count"),
           (dict(point_rows=16385), "point_rows 16385 exceeds SS_GUIDED_MAX_ROWS (16384)"),
           (dict(n_kf=1048577), "n_kf 1048577 exceeds SS_COVIS_MAX_MAP_KF (1048576) keyframes in one call"),
           (dict(problems=t((0, 2, 0, 17, 0, len(heavy))), n_kf=2, n_blocks=17, point_rows=16384, obs=heavy), "keyframe 0 has more than SS_COVIS_MAX_ROW_ITEMS (262143) records")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.covis_set_map(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    out = Out(41, 4)
    cp = binding.covis_params
    queries = [(dict(rows=[0, 41], n_rows=2), "ss_covis_kf_device: row 1: keyframe 41 lies outside the map's 41"), (dict(rows=[-1], n_rows=1), "row 0: keyframe -1 lies outside"),
               (dict(n_rows=40), "rows is NULL, so n_rows must be the map's 41 keyframes, not 40"), (dict(n_rows=-1), "bad row count"),
               (dict(rows=np.zeros(65536, np.int32), n_rows=65536), "more than 65535 rows in one call"),
               (dict(cap=0), "cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)"), (dict(cap=1025), "cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)"),
               (dict(params=cp(min_weight=0)), "min_weight must be >= 1"), (dict(params=cp(fallback=2)), "fallback must be 0 or 1"), (dict(params=cp(cull_obs=-1)), "cull_obs must be >= 0"),
               (dict(params=cp(cull_slack=17)), "cull_slack must be 0 .. SS_MAX_LEVELS"), (dict(params=cp(redundant_th=float("nan"))), "redundant_th must be finite and 0 .. 1"),
               (dict(params=cp(redundant_th=1.25)), "redundant_th must be finite and 0 .. 1"), (dict(params=cp(reserved=(1, 0, 0))), "the reserved fields must be 0"),
               (dict(d_nb=0), "ss_covis_kf_device: NULL buffer"), (dict(d_row=0), "ss_covis_kf_device: NULL buffer")]
    ok = dict(rows=None, n_rows=41, params=cp(), cap=4, d_nb=out.ptrs()[0], d_row=out.ptrs()[1])
    for kw, msg in queries:
        with pytest.raises(binding.OrbError) as e:
            ctx.covis_kf_device(**dict(ok, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    d_idx, d_np = _to_dev(np.zeros((1, P), np.int32)), _to_dev(np.array([P], np.int32))
    fok = dict(d_idx=d_idx.data_ptr(), d_n_points=d_np.data_ptr(), point_src=[0], params=cp(), cap=4, d_nb=out.ptrs()[0], d_row=out.ptrs()[1])
    for kw, msg in [(dict(point_src=[1]), "ss_covis_frames_device: row 0: block 1 lies outside the map's 1"), (dict(point_src=[-1]), "block -1 lies outside"),
                    (dict(d_idx=0), "ss_covis_frames_device: NULL buffer"), (dict(d_n_points=0), "NULL buffer"), (dict(d_nb=0), "NULL buffer"), (dict(d_row=0), "NULL buffer"),
                    (dict(cap=2000), "cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)")]:
        with pytest.raises(binding.OrbError) as e:
            ctx.covis_frames_device(**dict(fok, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    with pytest.raises(binding.OrbError) as e:
        ctx.covis(41, P, kf_out, cp(), 4)
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "record 5: kf 41 outside 0 .. 40" in e.value.message
    ctx.synchronize()
    assert all((a == FILL).all() for a in out.raw())  # nothing was written
    same("after the refusals: the map a refused ss_covis_set_map found is still there", run_kf(ctx, None, {}, 4, out=out, n_rows=41), want)


# ---- the chains ----------------------------------------------------------------------------------------------------------------------
CHAIN = ["synth_t0", "synth_t1", "checker_shift"]


def test_chains_from_a_projection_search_to_the_global_ba_and_the_pose_graph():
    """three extracted keyframes -> ss_match_proj_batch_device -> ss_covis_frames_device on its d_idx as it lies on the device, against
    the reference on the downloaded idx; ss_global_ba_obs_from_idx_host -> ss_covis_set_map, ss_covis_kf_device and
    ss_global_ba_device on the same tables; ss_covis_edges_host -> ss_pose_graph_device, which accepts the edges"""
    import torch
    import pose_cases as PO
    import proj_cases as PC
    from send_slam_amd import binding
    from test_gba import Out as GbaOut
    from test_graph import Out as GraphOut
    from test_proj import Outputs as ProjOut
    s0 = PC.scenes()[0]
    n = len(CHAIN)
    cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    feats = [G.features(name) for name in CHAIN]
    kp_rows = max(len(f[0]) for f in feats)
    kp, n_kp = np.zeros((n, kp_rows), binding.KP_DTYPE), np.array([len(f[0]) for f in feats], np.int32)
    for b, f in enumerate(feats):
        kp[b, :len(f[0])] = f[0]
    k, point_rows = len(s0["points"]), len(s0["points"]) + 7
    pts, pd = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE), np.zeros((1, point_rows, 32), np.uint8)
    pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
    poses = np.array([np.concatenate([np.asarray(PC.POSES[b][0], np.float64).reshape(-1), np.asarray(PC.POSES[b][1], np.float64).reshape(-1)]) for b in range(n)])
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        d = torch.from_numpy(np.stack([G.frame(name) for name in CHAIN])).to(_dev())
        c.extract_batch_device(d.data_ptr(), n, G.W, G.H)
        d_pts, d_pd, d_n = _to_dev(pts.view(np.uint8).reshape(1, -1)), _to_dev(pd), _to_dev(np.array([k], np.int32))
        views = [binding.proj_view(cam, poses[b][:9], poses[b][9:], PC.BF) for b in range(n)]
        m = ProjOut(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, PC.combo_params(binding, combo), *m.ptrs(), point_src=[0, 0, 0])
        c.synchronize()
        idx = m.host()[0]
        obs = binding.global_ba_obs_from_idx(kp, idx[:, :k], n_kp)
        assert len(obs) > 100
        table = np.array([(0, n, 0, 1, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE)
        c.covis_set_map(table, n, 1, point_rows, obs)
        ref_map = CR.Map(table, n, 1, point_rows, obs, CC.N_LEVELS)
        # 1. the frames' rows from d_idx as the search left it
        fout, kout = Out(n, 8), Out(n, 8)
        c.covis_frames_device(m.idx.data_ptr(), d_n.data_ptr(), [0, 0, 0], _params(dict(min_weight=1)), 8, *fout.ptrs())
        c.covis_kf_device(None, n, _params(dict(min_weight=1)), 8, *kout.ptrs())
        # 2. the global bundle adjustment on the same tables
        gout = GbaOut(n, 1, point_rows, len(obs), 1)
        d_start, d_fixed = _to_dev(poses), _to_dev(np.array([1, 0, 0], np.uint8))
        _sync()
        c.global_ba_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, d_start.data_ptr(), d_fixed.data_ptr(), n, table, obs,
                           np.array([PO.view(cam=(PC.FX, PC.FY, PC.CX, PC.CY, PC.BF))] * n), binding.gba_params(iterations=(2, 0, 0, 0)), *gout.ptrs())
        c.synchronize()
        frames, kfs = fout.host(), kout.host()
        same("frame rows on the search's d_idx", frames, CR.frame_rows(ref_map, idx, [k], [0, 0, 0], dict(min_weight=1), 8))
        same("keyframe rows of the map the search gave", kfs, CR.kf_rows(ref_map, None, dict(min_weight=1), 8))
        hits = (idx[:, :k] >= 0).sum(axis=1)
        assert frames[1]["n_shared"].min() >= 2 and [dict(frames[0][b][:frames[1][b]["n_written"]].tolist())[b] for b in range(n)] == hits.tolist()  # no self exclusion
        assert gout.host()[4][0]["status"] == binding.SS_OK and gout.host()[4][0]["n_obs"] == len(obs)
        # 3. the covisibility edges into the essential graph
        low = int(kfs[0][:, :, 1].max())
        edges = binding.covis_edges(kfs[0], kfs[1], np.arange(n, dtype=np.int32), min(low, 2))
        assert len(edges) >= 2 and np.array_equal(edges, CR.edges(kfs[0], kfs[1], np.arange(n), min(low, 2))) and (edges[:, 0] < edges[:, 1]).all()
        nc = np.concatenate([poses, np.ones((n, 1))], axis=1)
        d_nc, d_s = _to_dev(nc), _to_dev(nc.copy())
        graph = GraphOut(n, 1)
        _sync()
        c.pose_graph_device(d_nc.data_ptr(), d_s.data_ptr(), d_fixed.data_ptr(), n, np.array([(0, n, 0, len(edges))], binding.GRAPH_PROBLEM_DTYPE), edges,
                            binding.graph_params(), *graph.ptrs())
        c.synchronize()
        assert np.isfinite(graph.host()[1]).all()
