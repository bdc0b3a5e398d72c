"""GPU parity of the essential-graph optimisation (ss_pose_graph_device, ss_pose_graph, ss_pose_graph_points_device) against
tests/graph_ref.py through the C ABI: bit for bit, no tolerance -- every Sim3, every pose and every byte of every ss_graph_result.
Every output starts prefilled with a pattern no result has.  tests/test_graph_ref.py asserts on the reference that the shared cases are
live, and that the host twin, which stands in for the reference at the sizes of the ladders, equals it there."""
import numpy as np
import pytest

import graph_cases as GC
import graph_ref as GR
import guided_cases as G

pytestmark = pytest.mark.gpu

FILL = 0x5A
SHORT = dict(iterations=3, pcg_iterations=12)


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


class Out:
    """device sim3 [n_kf][13], poses [n_kf][12] and results [n_problems], prefilled with a pattern no result has"""

    def __init__(self, n_kf, n_problems):
        import torch
        self.shape = (n_kf, n_problems)
        fill = lambda *s: torch.full(s, FILL, dtype=torch.uint8, device=_dev())  # noqa: E731
        self.sim3, self.poses, self.result = fill(n_kf, 104), fill(n_kf, 96), fill(max(n_problems, 1), 48)
        _sync()

    def ptrs(self):
        return tuple(t.data_ptr() for t in (self.sim3, self.poses, self.result))

    def host(self):
        from send_slam_amd import binding
        n_kf, nq = self.shape
        return (self.sim3.cpu().numpy().copy().view(np.float64).reshape(n_kf, 13), self.poses.cpu().numpy().copy().view(np.float64).reshape(n_kf, 12),
                self.result.cpu().numpy().copy().view(binding.GRAPH_RESULT_DTYPE).reshape(-1)[:nq])


def _params(binding, p):
    return binding.graph_params(**{k: v for k, v in dict(GR.DEFAULTS, **p).items()})


def _run(ctx, call, params, table=None):
    """a stacked call (graph_cases.stack) -> (sim3, poses, results in table order)"""
    from send_slam_amd import binding
    nc, start, fixed, edges, tab, _ = call
    tab = np.array(tab if table is None else table, binding.GRAPH_PROBLEM_DTYPE)
    d = [_to_dev(nc), _to_dev(start), _to_dev(fixed)]
    out = Out(len(nc), len(tab))
    ctx.pose_graph_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(nc), tab, edges, _params(binding, params), *out.ptrs())
    ctx.synchronize()
    return out.host()


def _check(tag, got, q, k0, want):
    """problem q of a call, whose keyframes start at k0, against a result of graph_ref.optimise or of the host twin"""
    sim3, poses, results = got
    wsim3, wposes, wres = want[:3]
    n_kf = len(wsim3)
    for name in GR.RESULT_DTYPE.names:
        assert results[q][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[q][name]} != {wres[name]}"
    assert sim3[k0:k0 + n_kf].tobytes() == wsim3.tobytes(), f"{tag}: Sim3s differ in keyframes {np.flatnonzero((sim3[k0:k0 + n_kf] != wsim3).any(axis=1))[:8]}"
    assert poses[k0:k0 + n_kf].tobytes() == wposes.tobytes(), f"{tag}: poses differ in keyframes {np.flatnonzero((poses[k0:k0 + n_kf] != wposes).any(axis=1))[:8]}"


def _twin(pr, params):
    from send_slam_amd import binding
    return binding.pose_graph_host(pr["nc"], pr["start"], pr["fixed"], pr["edges"], _params(binding, params))


def _against(ctx, problems, params, tag, wants=None, **kw):
    call = GC.stack(problems, **kw)
    got = _run(ctx, call, params)
    wants = [_twin(pr, params) for pr in problems] if wants is None else wants
    for q, k in enumerate(call[5]):
        _check(f"{tag}, problem {q}", got, q, call[4][q][0], wants[k])
    return call, got, wants


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as c:
        yield c


@pytest.mark.parametrize("k", range(len(GC.CASES)), ids=GC.CASE_NAMES)
def test_cases_as_the_first_of_three_problems(ctx, k):
    p = GC.CASES[k]["params"]
    others = [GC.vertex_ladder(3), GC.edge_ladder(17)]
    wants = [GC.reference(k)[:3]] + [_twin(pr, p) for pr in others]
    _against(ctx, [GC.case_problem(k)] + others, p, GC.CASE_NAMES[k], wants=wants)


def test_the_vertex_ladder_in_one_call(ctx):
    _, got, wants = _against(ctx, [GC.vertex_ladder(n) for n in (2, 3, 36, 37, 257)], SHORT, "vertex ladder")
    assert all(w[2]["state"] == 0 and w[2]["accepted"] > 0 for w in wants)


def test_the_edge_ladder_in_one_call(ctx):
    _, got, wants = _against(ctx, [GC.edge_ladder(n) for n in (1, 15, 16, 17, 255, 256, 257, 513)], SHORT, "edge ladder")
    assert all(w[2]["state"] == 0 and w[2]["accepted"] > 0 for w in wants)


def test_the_star_and_a_lone_free_keyframe(ctx):
    lone = GC.make_problem(11, 9, GC.ring(8), drift=0.01)  # keyframe 8 has no edge: it does not move
    _, got, wants = _against(ctx, [GC.star(300), lone], SHORT, "star")
    assert wants[0][2]["state"] == 0 and wants[0][2]["accepted"] > 0
    assert wants[1][0][8].tobytes() == lone["start"][8].tobytes() and wants[1][2]["accepted"] > 0


def test_failures(ctx):
    cases = GC.failure_cases()
    names = list(cases)
    p = dict(iterations=4, pcg_iterations=30)
    call, got, wants = _against(ctx, [cases[n] for n in names], p, "failures")
    state = {n: int(w[2]["state"]) for n, w in zip(names, wants)}
    assert state["all_fixed"] == 1 and state["no_edges"] == 1 and state["nan_start"] == 2 and state["bad_scale"] == 2, state
    assert state["two_fixed"] == 0 and state["duplicate_edges"] == 0 and state["half_turn"] == 0 and state["far_start"] == 4, state
    for n, w in zip(names, wants):
        if state[n] in (1, 2):
            assert w[0].tobytes() == cases[n]["start"].tobytes() and w[2]["steps"] == 0, n
        else:
            assert np.isfinite(w[0]).all(), n
    one = _against(ctx, [cases["duplicate_edges"]], dict(p, pcg_iterations=1), "pcg_iterations 1")[2][0]
    assert one[2]["pcg_iterations"] == one[2]["steps"] == 4


def test_the_same_call_twice_and_the_problems_permuted(ctx):
    problems = [GC.vertex_ladder(36), GC.edge_ladder(17), GC.case_problem(3), GC.vertex_ladder(3)]
    params = dict(SHORT, fix_scale=False)
    call = GC.stack(problems)
    first, second = _run(ctx, call, params), _run(ctx, call, params)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    order = [2, 0, 3, 1]
    permuted = _run(ctx, call, params, table=[call[4][k] for k in order])
    assert permuted[0].tobytes() == first[0].tobytes() and permuted[1].tobytes() == first[1].tobytes()
    assert permuted[2].tobytes() == first[2][order].tobytes()
    for q, pr in enumerate(problems):
        _check(f"problem {q}", first, q, call[4][q][0], _twin(pr, params))


def test_a_small_call_after_a_large_one_and_keyframes_of_no_problem(ctx):
    _against(ctx, [GC.vertex_ladder(257), GC.edge_ladder(513)], SHORT, "large")
    call, got, _ = _against(ctx, [GC.vertex_ladder(3), GC.edge_ladder(15)], SHORT, "small, with gaps", gaps=2)
    nc, start = call[0], call[1]
    owned = np.zeros(len(nc), bool)
    for k0, n_kf, _, _ in call[4]:
        owned[k0:k0 + n_kf] = True
    assert (~owned).sum() == 4
    assert got[0][~owned].tobytes() == start[~owned].tobytes() and got[1][~owned].tobytes() == GR.pose(GR.cols(start[~owned])).tobytes()
    # no problem at all: every keyframe passes through
    got = _run(ctx, call, SHORT, table=[])
    assert got[0].tobytes() == start.tobytes() and got[1].tobytes() == GR.pose(GR.cols(start)).tobytes()


def test_the_host_pointer_form(ctx):
    from send_slam_amd import binding
    for k in (0, 3):
        pr, p = GC.case_problem(k), GC.CASES[k]["params"]
        got = ctx.pose_graph(pr["nc"], pr["start"], pr["fixed"], pr["edges"], _params(binding, p))
        want = GC.reference(k)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want[:3])), GC.CASE_NAMES[k]


def test_stats_stages_and_their_bytes():
    from send_slam_amd import binding
    problems = [GC.vertex_ladder(36), GC.edge_ladder(17)]
    nc, start, fixed, edges, tab, _ = GC.stack(problems)
    K, E, nq, its, pcg = len(nc), len(edges), 2, 3, 12
    d = [_to_dev(nc), _to_dev(start), _to_dev(fixed)]
    pts = _to_dev(np.zeros((1, 300), binding.MAP_POINT_DTYPE))
    ref = _to_dev(np.zeros((1, 300), np.int32))
    with binding.OrbContext(0, n_features=G.NF) as c:
        c.profile(True)
        out = Out(K, nq)
        c.pose_graph_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), K, np.array(tab, binding.GRAPH_PROBLEM_DTYPE), edges, _params(binding, SHORT), *out.ptrs())
        c.pose_graph_points_device(pts.data_ptr(), ref.data_ptr(), 1, 300, d[0].data_ptr(), out.sim3.data_ptr(), K)
        c.synchronize()
        got = {(s["name"], s["launches"], s["algorithmic_bytes"]) for s in c.stats()}
    state_bytes = 3 * 8 + 8 * 4
    assert got == {("graph_gather", 1, K * 418 + E * 320 + nq * state_bytes), ("graph_lin", its, E * 16 * 320 + E * 840),
                   ("graph_blocks", its, 2 * E * 452 + K * 505), ("graph_solve", its, pcg * (E * (952 + 904) + K * 952) + K * 264),
                   ("graph_cost", its + 1, E * 320 + nq * state_bytes), ("graph_finish", 1, K * 308 + nq * (state_bytes + 48)),
                   ("graph_points", 1, 300 * 236)}


def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    pr = GC.vertex_ladder(36)
    nc, start, fixed, edges, tab, _ = GC.stack([pr])
    d = [_to_dev(nc), _to_dev(start), _to_dev(fixed)]
    out = Out(36, 1)
    ptrs = out.ptrs()
    t = lambda *rows: np.array(list(rows), binding.GRAPH_PROBLEM_DTYPE)  # noqa: E731
    good = dict(d_nc=d[0].data_ptr(), d_start=d[1].data_ptr(), d_fixed=d[2].data_ptr(), n_kf=36, problems=t(*tab), edges=edges, params=binding.graph_params(),
                d_sim3=ptrs[0], d_poses=ptrs[1], d_result=ptrs[2])
    n_e = len(edges)
    gp = binding.graph_params
    nan, inf = float("nan"), float("inf")
    outside, loop = edges.copy(), edges.copy()
    outside[5, 1], loop[7] = 36, (4, 4)
    bad = [(dict(problems=t((0, 0, 0, n_e))), "n_kf 0 outside 1 .. SS_GRAPH_MAX_KF (16384)"), (dict(problems=t((0, 16385, 0, n_e))), "n_kf 16385 outside 1 .. SS_GRAPH_MAX_KF"),
           (dict(problems=t((0, 36, 0, -1))), "n_edges -1 outside 0 .. SS_GRAPH_MAX_EDGES (131072)"),
           (dict(problems=t((0, 36, 0, 131073))), "n_edges 131073 outside 0 .. SS_GRAPH_MAX_EDGES (131072)"),
           (dict(problems=np.zeros(65536, binding.GRAPH_PROBLEM_DTYPE)), "more than 65535 problems in one call"),
           (dict(problems=t((1, 36, 0, n_e))), "keyframes 1 .. + 36 lie outside the call's 36"), (dict(problems=t((0, 36, 1, n_e))), f"edges 1 .. + {n_e} lie outside the call's {n_e}"),
           (dict(problems=t((0, 35, 0, n_e))), "names a keyframe outside the problem"), (dict(edges=outside), "edge 5 (5, 36) names a keyframe outside the problem"),
           (dict(edges=loop), "edge 7 joins keyframe 4 to itself"),
           (dict(problems=t((0, 36, 0, n_e), (20, 16, 0, 0))), "problem 1: keyframe 20 belongs to problem 0 already"),
           (dict(problems=t((0, 36, 0, n_e), (0, 36, 3, 2))), "problem 1: keyframe 0 belongs to problem 0 already"),
           (dict(n_kf=-1), "bad keyframe, problem or edge count"),
           (dict(params=gp(lambda_=-1.0)), "lambda must be finite and >= 0"), (dict(params=gp(lambda_=nan)), "lambda must be finite and >= 0"),
           (dict(params=gp(lambda_factor=1.0)), "lambda_factor must be finite and > 1"), (dict(params=gp(lambda_min=inf)), "lambda_min must be finite and >= 0"),
           (dict(params=gp(pcg_tol=-1e-3)), "pcg_tol must be finite and >= 0"), (dict(params=gp(iterations=0)), "iterations must be 1 .. 64"),
           (dict(params=gp(iterations=65)), "iterations must be 1 .. 64"), (dict(params=gp(pcg_iterations=0)), "pcg_iterations must be 1 .. 4096"),
           (dict(params=gp(pcg_iterations=4097)), "pcg_iterations must be 1 .. 4096"), (dict(params=gp(reserved=1)), "reserved field must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.pose_graph_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    # edges that overlap between two problems over disjoint keyframes
    two = GC.stack([GC.vertex_ladder(3), GC.vertex_ladder(3)])
    d2 = [_to_dev(two[0]), _to_dev(two[1]), _to_dev(two[2])]
    with pytest.raises(binding.OrbError) as e:
        ctx.pose_graph_device(d2[0].data_ptr(), d2[1].data_ptr(), d2[2].data_ptr(), 6, t((0, 3, 0, 3), (3, 3, 2, 1)), two[3], binding.graph_params(), *ptrs)
    assert e.value.code == binding.SS_ERR_INVALID_ARG and ("names a keyframe outside the problem" in e.value.message or "belongs to problem 0 already" in e.value.message)
    pts, ref = _to_dev(np.zeros((1, 8), binding.MAP_POINT_DTYPE)), _to_dev(np.zeros((1, 8), np.int32))
    gpts = dict(d_points=pts.data_ptr(), d_ref=ref.data_ptr(), n_blocks=1, point_rows=8, d_nc=d[0].data_ptr(), d_sim3=ptrs[0], n_kf=36)
    for kw, msg in ((dict(point_rows=0), "bad block, row or keyframe count"), (dict(point_rows=16385), "bad block, row or keyframe count"), (dict(d_ref=0), "NULL buffer"),
                    (dict(n_blocks=65536), "more than 65535 blocks in one call"), (dict(n_blocks=-1), "bad block, row or keyframe count"),
                    (dict(d_sim3=0), "NULL buffer")):
        with pytest.raises(binding.OrbError) as e:
            ctx.pose_graph_points_device(**dict(gpts, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    ctx.pose_graph_device(**dict(good, n_kf=0, problems=t(), edges=edges[:0]))  # nothing to do, nothing written
    ctx.synchronize()
    assert out.host()[0].tobytes() == bytes([FILL]) * (36 * 104)
    ctx.pose_graph_device(**good)  # the context is usable after the refusals
    ctx.synchronize()
    _check("after the refusals", out.host(), 0, 0, _twin(pr, {}))


def test_the_points_against_the_reference(ctx):
    """rows of -1 and of numbers outside the call, a block whose rows name keyframes of two problems, point_rows no multiple of 256"""
    from send_slam_amd import binding
    problems = [GC.vertex_ladder(36), GC.edge_ladder(17)]
    call = GC.stack(problems)
    got = _run(ctx, call, SHORT)
    n_kf, rows = len(call[0]), 300
    rng = np.random.default_rng(31)
    blocks = np.zeros((3, rows), binding.MAP_POINT_DTYPE)
    for name in blocks.dtype.names:
        blocks[name] = rng.uniform(-3, 3, blocks.shape).astype(np.float32)
    ref = rng.integers(0, n_kf, (3, rows)).astype(np.int32)  # every block names keyframes of both problems
    ref[0, ::7], ref[1, ::5], ref[2, 3::11], ref[2, 280:] = -1, n_kf, -2 ** 31, -1
    d_blocks, d_ref, d_nc, d_sim3 = _to_dev(blocks), _to_dev(ref), _to_dev(call[0]), _to_dev(got[0])
    _sync()
    ctx.pose_graph_points_device(d_blocks.data_ptr(), d_ref.data_ptr(), 3, rows, d_nc.data_ptr(), d_sim3.data_ptr(), n_kf)
    ctx.synchronize()
    after = d_blocks.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(3, rows)
    want = blocks.copy()
    for b in range(3):
        xyz = GR.points(np.stack([blocks[n][b] for n in "xyz"], axis=1), ref[b], call[0], got[0])
        for e, name in enumerate("xyz"):
            want[name][b] = xyz[:, e]
    assert after.tobytes() == want.tobytes()
    moved = (after["x"] != blocks["x"]) | (after["y"] != blocks["y"])
    assert moved.sum() > 500 and not moved[0, ::7].any() and not moved[2, 280:].any() and not moved[1, ::5].any()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
CHAIN = ["synth_t0", "synth_t1", "checker_shift"]


def test_chain_from_the_pose_graph_to_a_projection_search_on_the_corrected_map():
    """ss_pose_graph_device -> ss_pose_graph_points_device -> ss_proj_view_init from d_poses -> ss_match_proj_batch_device on three
    extracted keyframes: keyframe 2 is fixed at a start that a Sim3 of scale 1.05 separates from its non-corrected pose, the loop
    (0, 1), (1, 2), (2, 0) carries that correction to the others, the points of keyframe 0 move with it, and the search under the
    corrected poses equals the projection reference on the corrected map"""
    import torch
    import proj_cases as PC
    import proj_ref as P
    from send_slam_amd import binding
    from test_proj import Outputs as ProjOut
    from test_proj import _check as _check_proj
    s0 = PC.scenes()[0]
    n = len(CHAIN)
    nc = np.stack([np.concatenate([np.asarray(PC.POSES[k][0], np.float64).reshape(-1), np.asarray(PC.POSES[k][1], np.float64).reshape(-1), [1.0]]) for k in (0, 1)] +
                  [GC.sim3((0.02, -0.3, 0.1), (0.5, -0.2, 0.3), 1.0)])
    shift = GR.cols(GC.sim3((0.01, -0.02, 0.015), (0.05, -0.03, 0.02), 1.05))
    start = nc.copy()
    start[2] = GR.mul(GR.cols(nc[2]), shift)[:, 0]
    fixed, edges = np.array([0, 0, 1], np.uint8), np.array([(0, 1), (1, 2), (2, 0)], np.int32)
    want = GR.optimise(nc, start, fixed, edges)
    assert want[2]["state"] == 0 and want[2]["cost_after"] < 1e-20 and abs(want[0][0][12] - 1.05) < 1e-9
    cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        d = torch.from_numpy(np.stack([G.frame(name) for name in CHAIN])).to(_dev())
        c.extract_batch_device(d.data_ptr(), n, G.W, G.H)
        k, point_rows = len(s0["points"]), len(s0["points"]) + 7
        pts, pd = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE), np.zeros((1, point_rows, 32), np.uint8)
        pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
        ref = np.zeros((1, point_rows), np.int32)  # every point's reference keyframe is keyframe 0; a few stay where they are
        ref[0, 5::17], ref[0, k:] = -1, -1
        d_pts, d_pd, d_n, d_ref = _to_dev(pts), _to_dev(pd), _to_dev(np.array([k], np.int32)), _to_dev(ref)
        d_nc, d_start, d_fixed = _to_dev(nc), _to_dev(start), _to_dev(fixed)
        out = Out(n, 1)
        _sync()
        c.pose_graph_device(d_nc.data_ptr(), d_start.data_ptr(), d_fixed.data_ptr(), n, np.array([(0, n, 0, 3)], binding.GRAPH_PROBLEM_DTYPE), edges,
                            binding.graph_params(), *out.ptrs())
        c.pose_graph_points_device(d_pts.data_ptr(), d_ref.data_ptr(), 1, point_rows, d_nc.data_ptr(), out.sim3.data_ptr(), n)
        c.synchronize()
        got = out.host()
        _check("chain", got, 0, 0, want)
        moved = pts[0].copy()
        xyz = GR.points(np.stack([pts[0][name] for name in "xyz"], axis=1), ref[0], nc, want[0])
        for e, name in enumerate("xyz"):
            moved[name] = xyz[:, e]
        assert d_pts.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(point_rows).tobytes() == moved.tobytes()
        views = [binding.proj_view(cam, got[1][b][:9], got[1][b][9:], PC.BF) for b in range(n)]  # d_poses feeds ss_proj_view_init unchanged
        m = ProjOut(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, PC.combo_params(binding, combo), *m.ptrs(),
                                  point_src=[0, 0, 0])
        c.synchronize()
        found = m.host()
        for b in range(n):
            tk, td = G.features(CHAIN[b])
            wv = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, want[1][b][:9], want[1][b][9:], PC.BF)
            second = P.match(wv, moved[:k], s0["p_desc"], tk, td, PC.scale(), th=3.0, ratio_num=8, ratio_den=10, one_to_one=True)
            _check_proj(f"chain, search, frame {b}", found, b, second)
            if b == 0:
                assert second[4]["n_accepted"] > 50
