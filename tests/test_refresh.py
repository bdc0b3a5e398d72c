"""GPU parity of the map-point refresh (ss_covis_set_map_rows, ss_refresh_device, ss_refresh) against tests/refresh_ref.py (the shared
cases, the calls) and the host twin through the C ABI (the ladder, the longest list): exactly, no tolerance -- the bytes of the map
blocks and every field of every ss_refresh_info and ss_refresh_summary.  Every output starts prefilled with a pattern no result has.
tests/test_refresh_ref.py asserts on the reference that the cases are live and holds the host twin to the reference."""
import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
import guided_cases as G
import refresh_cases as RC
import refresh_ref as RR
from test_refresh_ref import ref, same, twin

pytestmark = pytest.mark.gpu

FILL = 0x5A
SHARED, LADDERS = RC.shared_cases(), RC.ladder_cases(extra=(4097,))


def _dev():
    import torch
    return torch.device("cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()  # the library's stream does not wait for torch's


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


class Dev:
    """the device arrays of a call; info and summary prefilled with a pattern no result has"""

    def __init__(self, call):
        import torch
        self.B, self.R = call["n_blocks"], call["point_rows"]
        self.pts = _to_dev(np.ascontiguousarray(call["points"]).view(np.uint8).reshape(-1))
        self.pd = _to_dev(call["point_desc"]) if call["point_desc"] is not None else None
        self.np = _to_dev(np.asarray(call["n_points"], np.int32))
        self.ref = None if call["ref_kf"] is None else _to_dev(np.asarray(call["ref_kf"], np.int32))
        self.sel = None if call["select"] is None else _to_dev(np.asarray(call["select"], np.uint8))
        self.desc = None if call["desc"] is None else _to_dev(call["desc"])
        self.info = torch.full((max(self.B * self.R, 1), 32), FILL, dtype=torch.uint8, device=_dev())
        self.summary = torch.full((max(self.B, 1), 32), FILL, dtype=torch.uint8, device=_dev())
        _sync()

    def run(self, ctx, call, geometry=1, descriptor=1, **over):
        from send_slam_amd import binding
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        kw = dict(d_points=ptr(self.pts), d_point_desc=ptr(self.pd), d_n_points=ptr(self.np), d_desc=ptr(self.desc), rows_per_frame=call["rows_per_frame"],
                  views=call["views"], params=binding.refresh_params(geometry, descriptor), d_info=ptr(self.info), d_summary=ptr(self.summary), d_ref_kf=ptr(self.ref),
                  d_select=ptr(self.sel))
        ctx.refresh_device(**dict(kw, **over))
        ctx.synchronize()
        return self.host()

    def raw(self):
        return self.info.cpu().numpy().copy(), self.summary.cpu().numpy().copy()

    def host(self):
        info, summary = self.raw()
        return (self.pts.cpu().numpy().view(RR.MAP_POINT_DTYPE).reshape(self.B, self.R), None if self.pd is None else self.pd.cpu().numpy().reshape(self.B, self.R, 32),
                info.view(RR.INFO_DTYPE).reshape(-1)[:self.B * self.R].reshape(self.B, self.R), summary.view(RR.SUMMARY_DTYPE).reshape(-1)[:self.B])


def set_map(ctx, call, rows=True):
    ctx.covis_set_map(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], check_right=call["check_right"],
                      obs_row=call["obs_row"] if rows else None)


def run(ctx, call, geometry=1, descriptor=1, rows=True):
    set_map(ctx, call, rows)
    return Dev(call).run(ctx, call, geometry, descriptor)


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        assert RC.N_LEVELS == 8
        yield c


@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_cases_against_the_reference(ctx, name):
    call = RC.single(SHARED[name])
    for g, d in ((1, 1), (1, 0), (0, 1)):
        same(f"{name} geometry {g} descriptor {d}", run(ctx, call, g, d), ref(call, g, d))


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder_against_the_host_twin(ctx, name):
    call = RC.single(LADDERS[name])
    got = run(ctx, call)
    same(name, got, twin(call))
    assert got[2][0, 0]["n_obs"] == int(name.split("_")[1])


def test_one_point_seen_by_all_of_16384_keyframes(ctx):
    call = RC.single(RC.ladder_case(16384))
    got = run(ctx, call)
    same("16 384 observations", got, twin(call))
    assert got[2][0, 0]["n_obs"] == 16384 and got[2][0, 0]["state"] == 0 and 0 < got[2][0, 0]["best_median"] < 256


def test_two_problems_in_either_order_with_gaps_and_the_same_call_twice(ctx):
    cases = [LADDERS["len_65"], SHARED["random_12"], LADDERS["len_5"], LADDERS["len_129"]]
    for order, lead, gap, seed in (([0, 1, 2, 3], 0, 0, None), ([2, 0, 3, 1], 2, 3, 5)):
        call = RC.stack(cases, 16, lead=lead, gap=gap, order=order, shuffle_seed=seed)
        set_map(ctx, call)
        for g, d in ((1, 1), (1, 0), (0, 1)):
            dev = Dev(call)
            first = dev.run(ctx, call, g, d)
            same(f"order {order} {g} {d}", first, ref(call, g, d))
            same(f"order {order} {g} {d}: the same call twice", dev.run(ctx, call, g, d), first)


def test_flags_alone_leave_the_other_half_and_need_no_buffer_for_it(ctx):
    call = RC.single(SHARED["random_70"])
    set_map(ctx, call)
    geo, des = Dev(call).run(ctx, call, 1, 0), Dev(call).run(ctx, call, 0, 1)
    same("geometry alone", geo, ref(call, 1, 0))
    same("descriptor alone", des, ref(call, 0, 1))
    assert np.array_equal(geo[1], call["point_desc"]) and des[0].tobytes() == call["points"].tobytes() and (geo[2]["state"] == 0).sum() > 10
    bare = Dev(dict(call, point_desc=None, desc=None))
    got = bare.run(ctx, call, 1, 0)
    assert got[0].tobytes() == geo[0].tobytes() and np.array_equal(got[2], geo[2])
    set_map(ctx, call, rows=False)  # a geometry-only call needs no rows
    again = Dev(call).run(ctx, call, 1, 0)
    same("a map without rows", again, geo)


def test_a_small_map_after_a_large_one_then_no_map_and_a_map_without_rows(ctx):
    from send_slam_amd import binding
    big, small = RC.single(LADDERS["len_1025"]), RC.single(SHARED["one_row_frames"])
    same("large", run(ctx, big), twin(big))
    same("small after large", run(ctx, small), ref(small))
    dev = Dev(small)
    set_map(ctx, small, rows=False)
    with pytest.raises(binding.OrbError) as e:
        dev.run(ctx, small)
    assert e.value.code == binding.SS_ERR_STATE and "the map was set without rows" in e.value.message
    ctx.covis_set_map(np.zeros(0, binding.GBA_PROBLEM_DTYPE), 0, 0, 6, small["obs"][:0])  # no problem: the map is cleared
    for g, d in ((1, 1), (1, 0)):
        with pytest.raises(binding.OrbError) as e:
            dev.run(ctx, small, g, d)
        assert e.value.code == binding.SS_ERR_STATE and "no map (ss_covis_set_map_rows)" in e.value.message
    ctx.synchronize()
    assert all((a == FILL).all() for a in dev.raw()) and dev.host()[0].tobytes() == small["points"].tobytes() and np.array_equal(dev.host()[1], small["point_desc"])


def test_refused_arguments_and_their_messages_leave_the_map(ctx):
    from send_slam_amd import binding
    c = CC.shared_cases()["planted"]
    cov = CC.single(c)
    rows = np.arange(len(cov["obs"]), dtype=np.int32) % 7
    want = CR.kf_rows(CC.ref_map(cov), None, {}, 4)
    ctx.covis_set_map(cov["table"], cov["n_kf"], cov["n_blocks"], cov["point_rows"], cov["obs"], obs_row=rows)
    for where, value in ((3, -1), (11, 16384)):
        bad = rows.copy()
        bad[where] = value
        with pytest.raises(binding.OrbError) as e:
            ctx.covis_set_map(cov["table"], cov["n_kf"], cov["n_blocks"], cov["point_rows"], cov["obs"], obs_row=bad)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and f"covis: problem 0: record {where}: row {value} outside 0 .. SS_GUIDED_MAX_ROWS - 1 (16383)" in e.value.message
    P = cov["point_rows"]
    call = dict(n_blocks=1, point_rows=P, points=np.zeros(P, RR.MAP_POINT_DTYPE), point_desc=np.full((P, 32), 0xC3, np.uint8), n_points=[P], ref_kf=None, select=None,
                desc=np.zeros((cov["n_kf"], 7, 32), np.uint8), rows_per_frame=7, views=RC.views_of(np.ones((cov["n_kf"], 3), np.float32)))
    dev = Dev(call)
    rp = binding.refresh_params
    for over, msg in ((dict(rows_per_frame=6), "ss_refresh_device: rows_per_frame 6 is not above the map's largest row 6"),
                      (dict(rows_per_frame=16385), "rows_per_frame 16385 exceeds SS_GUIDED_MAX_ROWS (16384)"), (dict(params=rp(0, 0)), "geometry or descriptor must be set"),
                      (dict(params=rp(1, 3)), "descriptor must be 0 or 1"), (dict(params=rp(-1, 1)), "geometry must be 0 or 1"),
                      (dict(params=rp(reserved=(1, 0, 0, 0, 0, 0))), "the reserved fields must be 0"), (dict(d_points=0), "NULL buffer"), (dict(d_n_points=0), "NULL buffer"),
                      (dict(d_info=0), "NULL buffer"), (dict(d_summary=0), "NULL buffer"), (dict(d_desc=0), "NULL buffer"), (dict(d_point_desc=0), "ss_refresh_device: NULL buffer")):
        with pytest.raises(binding.OrbError) as e:
            dev.run(ctx, call, **over)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (over, e.value.message)
    ctx.synchronize()
    assert all((a == FILL).all() for a in dev.raw())  # nothing was written
    from test_covis import Out, same as same_rows
    out = Out(cov["n_kf"], 4)
    ctx.covis_kf_device(None, cov["n_kf"], binding.covis_params(), 4, *out.ptrs())
    ctx.synchronize()
    same_rows("the map with rows answers the covisibility queries as the map without", out.host(), want)
    got = dev.run(ctx, call)  # and the refresh
    assert (got[2]["state"] >= 0).all() and got[3][0]["n_selected"] == P


def test_the_host_pointer_form(ctx):
    for name, c in (("random_12", SHARED["random_12"]), ("len_257", LADDERS["len_257"])):
        call = RC.single(c)
        for g, d in ((1, 1), (1, 0)):
            from send_slam_amd import binding
            got = ctx.refresh(call["views"], c["points"], c["point_desc"], c["obs"], c["obs_row"] if d else None, c["desc"], binding.refresh_params(g, d), ref_kf=c["ref_kf"],
                              select=c["select"], check_right=c["check_right"])
            want = ref(call, g, d)
            same(f"{name} {g} {d}", (got[0].reshape(1, -1), got[1].reshape(1, -1, 32), got[2].reshape(1, -1), got[3]), want)


def test_stats_stage_and_its_bytes():
    from send_slam_amd import binding
    call = RC.single(SHARED["random_12"])
    with binding.OrbContext(0, n_features=G.NF) as c:
        c.profile(True)
        run(c, call)
        Dev(call).run(c, call, 1, 0)
        stats = {s["name"]: (s["launches"], s["algorithmic_bytes"]) for s in c.stats()}
    items, NP = len(call["obs"]), call["n_blocks"] * call["point_rows"]
    assert stats["refresh"] == (2, items * (4 + 12) + NP * (8 + 32 + 32 + 20) + call["n_blocks"] * 36)  # the bytes of the last call: geometry alone


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
CHAIN = ["synth_t0", "synth_t1", "checker_shift"]


def test_chain_search_adjust_refresh_search():
    """three extracted keyframes -> ss_match_proj_batch_device -> ss_global_ba_obs_from_idx_host + ss_global_ba_rows_from_idx_host ->
    ss_covis_set_map_rows -> ss_global_ba_device -> ss_local_ba_points_to_block -> ss_refresh_device with d_point_flags as d_select and the
    extraction's own descriptor block as d_desc -> ss_proj_view_init -> ss_match_proj_batch_device on the refreshed blocks; every stage
    against the references chained the same way"""
    import torch
    import pose_cases as PO
    import proj_cases as PC
    import proj_ref as P
    from send_slam_amd import binding
    from test_gba import Out as GbaOut
    from test_proj import Outputs as ProjOut
    from test_proj import _check as check_proj
    s0 = PC.scenes()[0]
    n = len(CHAIN)
    cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    k, point_rows = len(s0["points"]), len(s0["points"]) + 7
    pts, pd = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE), np.zeros((1, point_rows, 32), np.uint8)
    pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
    poses = np.array([np.concatenate([np.asarray(PC.POSES[b][0], np.float64).reshape(-1), np.asarray(PC.POSES[b][1], np.float64).reshape(-1)]) for b in range(n)])
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        d = torch.from_numpy(np.stack([G.frame(name) for name in CHAIN])).to(_dev())
        c.extract_batch_device(d.data_ptr(), n, G.W, G.H)
        c.synchronize()
        feats = [c.fetch_frame(b)[:2] for b in range(n)]
        for b, name in enumerate(CHAIN):  # the references are computed on the oracle's features
            assert feats[b][0].tobytes() == G.features(name)[0].tobytes() and np.array_equal(feats[b][1], G.features(name)[1])
        bv = c.batch_view()
        kcap = bv.kp_capacity
        kp, n_kp, desc = np.zeros((n, kcap), binding.KP_DTYPE), np.array([len(f[0]) for f in feats], np.int32), np.zeros((n, kcap, 32), np.uint8)
        for b, f in enumerate(feats):
            kp[b, :len(f[0])], desc[b, :len(f[0])] = f
        d_pts, d_pd, d_n = _to_dev(pts.view(np.uint8).reshape(1, -1)), _to_dev(pd), _to_dev(np.array([k], np.int32))
        views = [binding.proj_view(cam, poses[b][:9], poses[b][9:], PC.BF) for b in range(n)]
        params = PC.combo_params(binding, combo)

        def search(tag, views, block, block_desc):
            m = ProjOut(n, point_rows)
            _sync()
            c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, params, *m.ptrs(), point_src=[0, 0, 0])
            c.synchronize()
            got = m.host()
            for b in range(n):
                v = np.frombuffer(bytes(views[b]), P.VIEW_DTYPE)[0]
                want = P.match(v, block[:k], block_desc[:k], feats[b][0], feats[b][1], PC.scale(), th=combo["th"], ratio_num=combo["ratio"][0], ratio_den=combo["ratio"][1],
                               one_to_one=combo["one_to_one"])
                check_proj(f"{tag}, frame {b}", got, b, want)
            return got
        first = search("the first search", views, pts[0], pd[0])
        idx = first[0]
        # the map: the records and their rows from the search's idx
        obs, rows = binding.global_ba_obs_from_idx(kp, idx[:, :k], n_kp), binding.global_ba_rows_from_idx(idx[:, :k], n_kp, kcap)
        assert len(obs) == len(rows) > 100 and np.array_equal(obs["u"], kp["x"][obs["kf"], rows]) and np.array_equal(rows, idx[obs["kf"], obs["point"]])
        table = np.array([(0, n, 0, 1, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE)
        c.covis_set_map(table, n, 1, point_rows, obs, obs_row=rows)
        # the global bundle adjustment, rounded back into the block
        gviews, gp = np.array([PO.view(cam=(PC.FX, PC.FY, PC.CX, PC.CY, PC.BF))] * n), binding.gba_params(iterations=(2, 0, 0, 0))
        gout = GbaOut(n, 1, point_rows, len(obs), 1)
        d_start, d_fixed = _to_dev(poses), _to_dev(np.array([1, 0, 0], np.uint8))
        _sync()
        c.global_ba_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, d_start.data_ptr(), d_fixed.data_ptr(), n, table, obs, gviews, gp, *gout.ptrs())
        c.local_ba_points_to_block(gout.xyz.data_ptr(), gout.pflag.data_ptr(), 1, point_rows, d_pts.data_ptr(), 1)
        c.synchronize()
        g_poses, g_xyz, g_pflag, _, g_res = gout.host()
        w_poses, w_xyz, w_pflag, _, w_res = binding.global_ba_host(gviews, poses, np.array([1, 0, 0], np.uint8), PC.scale(), pts[0, :k], obs, gp)
        assert g_res[0]["state"] == 0 and g_poses.tobytes() == w_poses.tobytes() and g_xyz[0, :k].tobytes() == w_xyz.tobytes() and np.array_equal(g_pflag[0, :k], w_pflag)
        assert (g_pflag[0, k:] == 2).all() and (w_pflag == 0).sum() > 50
        block = pts[0].copy()
        moved = np.flatnonzero(w_pflag != 2)
        block["x"][moved], block["y"][moved], block["z"][moved] = w_xyz[moved].astype(np.float32).T
        assert d_pts.cpu().numpy().tobytes() == block.tobytes()
        # the refresh of the optimised points: d_point_flags is d_select as it lies, the extraction's own descriptor block is d_desc
        new_views = [binding.proj_view(cam, g_poses[b][:9], g_poses[b][9:], PC.BF) for b in range(n)]
        call = dict(table=table, n_kf=n, n_blocks=1, point_rows=point_rows, obs=obs, obs_row=rows, points=block, point_desc=pd[0], n_points=[k], ref_kf=None,
                    select=g_pflag[:1], desc=desc, rows_per_frame=kcap, views=np.frombuffer(b"".join(bytes(v) for v in new_views), RC.VIEW_DTYPE), check_right=False)
        info = torch.full((point_rows, 32), FILL, dtype=torch.uint8, device=_dev())
        summary = torch.full((1, 32), FILL, dtype=torch.uint8, device=_dev())
        _sync()
        c.refresh_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), bv.descriptors, kcap, new_views, binding.refresh_params(), info.data_ptr(), summary.data_ptr(),
                         d_select=gout.pflag.data_ptr())
        c.synchronize()
        want = ref(call)
        got = (d_pts.cpu().numpy().view(RR.MAP_POINT_DTYPE).reshape(1, -1), d_pd.cpu().numpy(), info.cpu().numpy().view(RR.INFO_DTYPE).reshape(1, -1),
               summary.cpu().numpy().view(RR.SUMMARY_DTYPE).reshape(-1))
        same("the refresh", got, want)
        same("the refresh, host twin", twin(call), want)
        assert want[3][0]["n_refreshed"] == (w_pflag == 0).sum() and (want[2][0]["n_obs"][:k][w_pflag == 0] >= 2).all() and want[3][0]["n_rows"] == k
        assert (want[0]["min_dist"][0, :k][w_pflag == 0] != pts["min_dist"][0, :k][w_pflag == 0]).any()
        # the narrower search on the refreshed blocks under the adjusted poses
        second = search("the second search", new_views, want[0][0], want[1][0])
        assert (second[0][:, :k] >= 0).sum() > 100
