"""GPU parity of the global bundle adjustment (ss_global_ba_device, ss_global_ba) against tests/gba_ref.py and the host twin through the
C ABI: bit for bit, no tolerance -- every pose, point, flag and every byte of every ss_gba_result.  Every output starts prefilled with
a pattern no result has.  tests/test_gba_ref.py asserts on the reference that the shared cases are live, and holds the host twin,
which stands in for the reference in the ladders, to the reference at those sizes."""
import numpy as np
import pytest

import ba_cases as BC
import camera_cases as CC
import gba_cases as GC
import gba_ref as GR
import guided_cases as G
import pose_cases as PO
import proj_cases as PC

pytestmark = pytest.mark.gpu

FILL = 0x5A
STATE_BYTES = 5 * 8 + 20 * 4  # ssk_gba_state


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
    """device poses [n_kf][12], xyz [n_blocks][rows][3], point flags [n_blocks][rows], observation flags [n_obs] and results
    [n_problems], prefilled with a pattern no result has"""

    def __init__(self, n_kf, n_blocks, rows, n_obs, n_problems):
        import torch
        self.shape = (n_kf, n_blocks, rows, n_obs, n_problems)
        fill = lambda *s: torch.full(s, FILL, dtype=torch.uint8, device=_dev())  # noqa: E731
        self.poses, self.xyz, self.pflag = fill(max(n_kf, 1), 96), fill(max(n_blocks, 1), rows * 24), fill(max(n_blocks, 1), rows)
        self.oflag, self.result = fill(max(n_obs, 1)), fill(max(n_problems, 1), 104)
        _sync()

    def ptrs(self):
        return tuple(t.data_ptr() for t in (self.poses, self.xyz, self.pflag, self.oflag, self.result))

    def raw(self):
        return tuple(t.cpu().numpy().copy() for t in (self.poses, self.xyz, self.pflag, self.oflag, self.result))

    def host(self):
        from send_slam_amd import binding
        n_kf, n_blocks, rows, n_obs, nq = self.shape
        poses, xyz, pflag, oflag, result = self.raw()
        return (poses.view(np.float64).reshape(-1, 12)[:n_kf], xyz.view(np.float64).reshape(-1, rows, 3)[:n_blocks], pflag[:n_blocks], oflag[:n_obs],
                result.view(binding.GBA_RESULT_DTYPE).reshape(-1)[:nq])


def _stack(problems, rows, lead_kf=0, lead_blocks=0, lead_obs=0, gap=0, order=None):
    """the problems of one call, each with blocks of `rows` point rows of its own (the last one short): keyframes, blocks and records
    one problem after the other in the order `order`, after lead_* keyframes, blocks and records of no problem and with `gap` of each
    between two problems -> a dict of host arrays and the table (in the problems' order)"""
    from send_slam_amd import binding
    order = list(range(len(problems))) if order is None else order
    at_kf, at_blk, at_obs, table = lead_kf, lead_blocks, lead_obs, [None] * len(problems)
    for q in order:
        pr = problems[q]
        nb = -(-len(pr["points"]) // rows)
        table[q] = (at_kf, len(pr["views"]), at_blk, nb, at_obs, len(pr["obs"]), (0, 0))
        at_kf, at_blk, at_obs = at_kf + len(pr["views"]) + gap, at_blk + nb + gap, at_obs + len(pr["obs"]) + gap
    n_kf, n_blocks, n_obs = at_kf, at_blk, at_obs
    rng = np.random.default_rng(5)
    host = {"points": np.zeros((max(n_blocks, 1), rows), binding.MAP_POINT_DTYPE), "skip": np.zeros((max(n_blocks, 1), rows), np.uint8),
            "np": np.full(max(n_blocks, 1), rows // 2, np.int32), "start": np.tile(PO.start_of(np.eye(3) * 2.0, np.array([1.0, 2.0, 3.0])), (max(n_kf, 1), 1)),
            "fixed": np.zeros(max(n_kf, 1), np.uint8), "views": np.array([PO.view()] * max(n_kf, 1)), "obs": np.zeros(n_obs, GR.OBS_DTYPE)}
    for name in ("x", "y", "z"):  # the blocks of no problem hold points: nobody reads them
        host["points"][name] = rng.uniform(1, 9, host["points"].shape).astype(np.float32)
    host["obs"]["kf"], host["obs"]["point"] = -3, 1 << 30  # the records of no problem hold junk: nobody reads them
    for q, pr in enumerate(problems):
        k0, nk, b0, nb, s0, ns, _ = table[q]
        P_ = len(pr["points"])
        flat = host["points"][b0:b0 + nb].reshape(-1)
        flat[:P_] = pr["points"]
        flat[P_:] = pr["points"][0] if P_ else 0  # live-looking rows past the count
        host["np"][b0:b0 + nb] = [min(rows, P_ - b * rows) for b in range(nb)]
        if pr.get("skip") is not None:
            host["skip"][b0:b0 + nb].reshape(-1)[:P_] = pr["skip"]
        host["start"][k0:k0 + nk], host["fixed"][k0:k0 + nk], host["views"][k0:k0 + nk] = pr["start"], pr["fixed"], pr["views"]
        host["obs"][s0:s0 + ns] = pr["obs"]
    host.update(table=np.array(table, binding.GBA_PROBLEM_DTYPE), n_kf=n_kf, n_blocks=n_blocks, n_obs=n_obs, rows=rows)
    return host


def _params(binding, p):
    return binding.gba_params(**{k: p[k] for k in GR.DEFAULTS if k in p})


def _run(ctx, call, params, skip=False, table=None, out=None):
    from send_slam_amd import binding
    table = call["table"] if table is None else table
    dev = {k: _to_dev(call[k]) for k in ("points", "skip", "np", "start", "fixed")}
    out = out or Out(call["n_kf"], call["n_blocks"], call["rows"], call["n_obs"], len(table))
    _sync()
    ctx.global_ba_device(dev["points"].data_ptr(), dev["np"].data_ptr(), call["n_blocks"], call["rows"], dev["start"].data_ptr(), dev["fixed"].data_ptr(), call["n_kf"],
                         table, call["obs"], call["views"][:call["n_kf"]], _params(binding, params), *out.ptrs(), d_point_skip=dev["skip"].data_ptr() if skip else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, call, q, want):
    """problem q of a call against a reference result of its points, in one block"""
    poses, xyz, pflag, oflag, results = got
    wposes, wxyz, wpflag, woflag, wres = want[:5]
    k0, nk, b0, nb, s0, ns, _ = call["table"][q].tolist()
    P_, rows = len(wxyz), call["rows"]
    for name in GR.RESULT_DTYPE.names:
        assert results[q][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[q][name]} != {wres[name]}"
    assert poses[k0:k0 + nk].tobytes() == wposes.tobytes(), f"{tag}: poses differ in keyframes {np.flatnonzero((poses[k0:k0 + nk] != wposes).any(axis=1))[:8]}"
    fx, ff = xyz[b0:b0 + nb].reshape(-1, 3), pflag[b0:b0 + nb].reshape(-1)
    assert fx[:P_].tobytes() == wxyz.tobytes(), f"{tag}: points differ at rows {np.flatnonzero((fx[:P_] != wxyz).any(axis=1))[:8]}"
    assert np.array_equal(ff[:P_], wpflag), f"{tag}: point flags differ at rows {np.flatnonzero(ff[:P_] != wpflag)[:8]}"
    assert np.array_equal(oflag[s0:s0 + ns], woflag), f"{tag}: observation flags differ at {np.flatnonzero(oflag[s0:s0 + ns] != woflag)[:8]}"
    assert (ff[P_:] == 2).all() and fx[P_:].tobytes() == bytes(24 * (nb * rows - P_)), f"{tag}: rows past the points"
    assert np.isfinite(poses[k0:k0 + nk]).all() and np.isfinite(fx).all() and all(np.isfinite(results[q][n]) for n in ("lambda_", "cost_before", "cost_after")), f"{tag}: not finite"


def _twin(pr, params):
    from send_slam_amd import binding
    return binding.global_ba_host(pr["views"], pr["start"], pr["fixed"], PC.scale(), pr["points"], pr["obs"], _params(binding, dict(GR.DEFAULTS, **params)), pr.get("skip"))


def _no_problem_parts(got, call, tag):
    """keyframes of no problem return their orthonormalised start, blocks of no problem flag 2 and +0.0, records of no problem 2"""
    poses, xyz, pflag, oflag, _ = got
    kf, blk, rec = np.ones(call["n_kf"], bool), np.ones(call["n_blocks"], bool), np.ones(call["n_obs"], bool)
    for k0, nk, b0, nb, s0, ns, _ in call["table"].tolist():
        kf[k0:k0 + nk], blk[b0:b0 + nb], rec[s0:s0 + ns] = False, False, False
    want = np.array([list(R) + list(t) for R, t in (GR.PR.start_pose(s)[:2] for s in call["start"][:call["n_kf"]])]).reshape(-1, 12)
    assert poses[kf].tobytes() == want[kf].tobytes(), tag
    assert (pflag[blk] == 2).all() and xyz[blk].tobytes() == bytes(24 * call["rows"] * int(blk.sum())) and (oflag[rec] == 2).all(), tag
    return int(kf.sum()), int(blk.sum()), int(rec.sum())


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


@pytest.mark.parametrize("k", range(len(GC.CASES)), ids=GC.CASE_NAMES)
def test_cases_as_the_first_of_three_problems(ctx, k):
    """against the reference; blocks of 100 rows, so the case's points span several; the default-schedule case is noise_free"""
    params = GC.CASES[k]["params"]
    others = [GC.point_ladder_problem(2), GC.kf_ladder_problem(3)]
    call = _stack([GC.case_problem(k)] + others, rows=100)
    got = _run(ctx, call, params, skip=True)
    _check(GC.CASE_NAMES[k], got, call, 0, GC.reference(k))
    for q, pr in enumerate(others):
        _check(f"{GC.CASE_NAMES[k]}, problem {q + 1}", got, call, q + 1, _twin(pr, params))


def test_the_keyframe_ladder_in_one_call(ctx):
    problems = [GC.kf_ladder_problem(n) for n in GC.KF_LADDER]
    call = _stack(problems, rows=64)
    got = _run(ctx, call, GC.LADDER)
    for q, pr in enumerate(problems):
        _check(f"{GC.KF_LADDER[q]} free keyframes", got, call, q, _twin(pr, GC.LADDER))


def test_the_point_and_list_ladders_in_one_call(ctx):
    problems = [GC.point_ladder_problem(n) for n in GC.POINT_LADDER] + [GC.list_ladder_problem(n) for n in GC.LIST_LADDER]
    call = _stack(problems, rows=257)
    assert call["table"]["n_blocks"].tolist()[:7] == [0, 1, 1, 1, 1, 1, 2]
    got = _run(ctx, call, GC.LADDER)
    for q, pr in enumerate(problems):
        _check(f"ladder problem {q}", got, call, q, _twin(pr, GC.LADDER))


def test_seen_by_one_two_and_sixty_five_and_beyond_the_local_limits(ctx):
    problems = [GC.seen_by_problem(), GC.beyond_local_problem(), GC.lonely_problem()]
    call = _stack(problems, rows=300)
    got = _run(ctx, call, GC.LADDER)
    for q, pr in enumerate(problems):
        _check(f"problem {q}", got, call, q, _twin(pr, GC.LADDER))
    assert got[4]["state"].tolist() == [0, 0, 0] and got[2][0][:3].tolist() == [1, 0, 0]


def test_two_problems_with_the_table_permuted_and_the_same_call_twice(ctx):
    """problems over disjoint keyframes, blocks and records, laid out in the other order and listed in the other order: the same
    bytes per problem; the same call twice: the same bytes"""
    a, b = GC.case_problem(GC.CASE_NAMES.index("stereo_mixed")), GC.case_problem(GC.CASE_NAMES.index("no_fixed"))
    params = dict(GC.SHORT, check_right=True)
    wants = [_twin(a, params), _twin(b, params)]
    call = _stack([a, b], rows=128)
    first = _run(ctx, call, params)
    again = _run(ctx, call, params)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    other = _stack([a, b], rows=128, order=[1, 0])
    assert other["table"]["first_kf"].tolist() == [5, 0]
    laid = _run(ctx, other, params)
    swapped = dict(call, table=call["table"][::-1].copy())
    listed = _run(ctx, swapped, params)
    for q in range(2):
        _check(f"problem {q}", first, call, q, wants[q])
        _check(f"problem {q}, laid out second", laid, other, q, wants[q])
        _check(f"problem {q}, listed second", listed, swapped, 1 - q, wants[q])
    shuffled = np.random.default_rng(9).permutation(len(a["obs"]))
    mixed = _stack([dict(a, obs=a["obs"][shuffled]), b], rows=128)
    got = _run(ctx, mixed, params)
    _check("records shuffled", got, mixed, 0, wants[0][:3] + (wants[0][3][shuffled],) + wants[0][4:])


def test_a_small_call_after_a_large_one_and_parts_of_no_problem(ctx):
    large = _stack([GC.kf_ladder_problem(257), GC.list_ladder_problem(513)], rows=300)
    got = _run(ctx, large, GC.LADDER)
    _check("large", got, large, 0, _twin(GC.kf_ladder_problem(257), GC.LADDER))
    pr = GC.point_ladder_problem(2)
    small = _stack([pr, GC.kf_ladder_problem(2)], rows=7, lead_kf=3, lead_blocks=2, lead_obs=5, gap=1)
    got = _run(ctx, small, GC.LADDER)
    _check("small", got, small, 0, _twin(pr, GC.LADDER))
    _check("small, second", got, small, 1, _twin(GC.kf_ladder_problem(2), GC.LADDER))
    assert _no_problem_parts(got, small, "small") == (5, 4, 7)


def test_a_call_without_a_problem_or_a_keyframe_writes_nothing(ctx):
    from send_slam_amd import binding
    call = _stack([GC.point_ladder_problem(2)], rows=8)
    for kw in (dict(table=np.zeros(0, binding.GBA_PROBLEM_DTYPE)), dict(n_kf=0)):
        c = dict(call, **{k: v for k, v in kw.items() if k != "table"})
        out = Out(call["n_kf"], call["n_blocks"], 8, call["n_obs"], 1)
        if "n_kf" in kw:
            c["table"] = np.zeros(0, binding.GBA_PROBLEM_DTYPE)
        _run(ctx, c, GC.LADDER, table=kw.get("table"), out=out)
        assert all((a == FILL).all() for a in out.raw()), kw


def test_failure_states(ctx):
    k = GC.CASE_NAMES.index("noisy_outliers")
    base, params = GC.case_problem(k), GC.CASES[k]["params"]
    all_fixed = dict(base, fixed=np.ones(8, np.uint8))
    nan_point = dict(base, points=base["points"].copy())
    nan_point["points"]["y"][33] = np.nan
    nan_start = dict(base, start=base["start"].copy())
    nan_start["start"][3, 4] = np.nan
    rolled = dict(base, start=base["start"].copy())
    rolled["start"][0] = PO.start_of(PC.rot(0.0, 0.0, 3.0) @ base["start"][0][:9].reshape(3, 3), base["start"][0][9:])
    behind = dict(base, points=base["points"].copy())
    behind["points"]["z"][5:15] = -behind["points"]["z"][5:15]
    lonely = GC.lonely_problem()
    problems = [all_fixed, nan_point, nan_start, rolled, behind, lonely, dict(lonely, fixed=np.array([0, 1, 1, 1, 1, 1], np.uint8))]
    call = _stack(problems, rows=150)
    for p in (params, dict(params, lambda_=0.0, lambda_min=0.0), dict(params, pcg_iterations=1)):
        got = _run(ctx, call, p)
        wants = [_twin(pr, p) for pr in problems]
        for q, w in enumerate(wants):
            _check(f"problem {q}, lambda {p['lambda_']}", got, call, q, w)
        assert got[4]["state"].tolist()[:5] == [1, 0, 2, 4, 0] and got[4]["state"][5] == (0 if p["lambda_"] else 2)
    frozen = BC.frozen_problem()
    g = dict(views=frozen["views"], start=frozen["start"], fixed=np.array([0, 1, 1], np.uint8), points=frozen["points"],
             obs=GR.obs_from_idx(frozen["kp"], frozen["idx"], frozen["n_kp"]), skip=None)
    fp = dict(lambda_=0.0, lambda_min=0.0, n_rounds=1, iterations=(3, 0, 0, 0), pcg_iterations=16)
    call = _stack([g], rows=64)
    got = _run(ctx, call, fp)
    _check("frozen", got, call, 0, _twin(g, fp))
    assert got[4]["n_frozen_max"][0] == 1


def test_cameras_a_b_and_the_square_one_in_one_problem(ctx):
    cams = [CC.A, CC.B, CC.SQUARE]
    pr = GC.make_problem(seed=1600, n_kf=6, n_free=4, n_points=120, n_out=10, stereo_every=2, cams=cams)
    assert len({tuple(float(v[n]) for n in ("fx", "fy", "cx", "cy", "bf")) for v in pr["views"]}) == 3
    params = dict(GC.SHORT, check_right=True)
    want = GC.solve(pr, params)
    assert want[4]["state"] == 0 and want[4]["n_stereo"] > 0 and want[4]["accepted"].sum() > 0
    call = _stack([pr, GC.point_ladder_problem(2)], rows=50)
    _check("three cameras", _run(ctx, call, params), call, 0, want)
    mixed = dict(pr, views=pr["views"][[1, 2, 0, 4, 5, 3]])
    assert GC.solve(mixed, params)[0].tobytes() != want[0].tobytes()  # the cameras count


def test_the_host_pointer_form(ctx):
    from send_slam_amd import binding
    for k in (GC.CASE_NAMES.index("stereo_mixed"), GC.CASE_NAMES.index("no_fixed")):
        pr, params = GC.case_problem(k), GC.CASES[k]["params"]
        got = ctx.global_ba(pr["views"], pr["start"], pr["fixed"], pr["points"], pr["obs"], _params(binding, params), pr.get("skip"))
        want = GC.reference(k)
        for name, g, w in zip(("poses", "xyz", "point flags", "observation flags"), got[:4], want[:4]):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (GC.CASE_NAMES[k], name)
        assert got[4].tobytes() == want[4].tobytes()
    pr = GC.point_ladder_problem(0)
    got = ctx.global_ba(pr["views"], pr["start"], pr["fixed"], pr["points"], pr["obs"], _params(binding, GC.LADDER))
    assert got[4].tobytes() == _twin(pr, GC.LADDER)[4].tobytes() and got[4]["state"] == 1 and len(got[1]) == 0


def test_stats_stages_and_their_bytes():
    from send_slam_amd import binding
    problems = [GC.kf_ladder_problem(3), GC.point_ladder_problem(257)]
    call = _stack(problems, rows=100)
    params = dict(GC.LADDER, pcg_iterations=4)
    K, NP, S, nq, T, rounds, cap = call["n_kf"], call["n_blocks"] * 100, call["n_obs"], 2, 3, 2, 4
    groups = call["n_blocks"] * 1
    with binding.OrbContext(0, n_features=G.NF) as c:
        c.profile(True)
        got = _run(c, call, params)
        stats = {(s["name"], s["launches"], s["algorithmic_bytes"]) for s in c.stats()}
    for q, pr in enumerate(problems):
        _check(f"problem {q}", got, call, q, _twin(pr, params))
    st = nq * STATE_BYTES
    assert stats == {("gba_gather", 1, K * 289 + NP * 90 + S * 33 + groups * 32 + st), ("gba_points", T, NP * 106 + S * 323 + groups * 4),
                     ("gba_blocks", T, S * 278 + K * 898 + groups * 4 + 2 * st), ("gba_pcg", T * cap, S * 432 + NP * 81 + K * 849 + 2 * st),
                     ("gba_update", T, K * 242 + NP * 130 + S * 226 + groups * 8), ("gba_cost", T + rounds, K * 169 + S * 62 + groups * 8 + 2 * st),
                     ("gba_classify", rounds, NP * 34 + S * 178), ("gba_finish", 1, NP * 58 + S * 35 + K * 196 + groups * 16 + nq * 104 + st)}


def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    pr = GC.kf_ladder_problem(3)
    call = _stack([pr], rows=64)
    dev = {k: _to_dev(call[k]) for k in ("points", "skip", "np", "start", "fixed")}
    out = Out(4, 1, 64, call["n_obs"], 1)
    ptrs = out.ptrs()
    n_o = call["n_obs"]
    t = lambda *rows: np.array([r + ((0, 0),) if len(r) == 6 else r for r in rows], binding.GBA_PROBLEM_DTYPE)  # noqa: E731
    good = dict(d_points=dev["points"].data_ptr(), d_n_points=dev["np"].data_ptr(), n_blocks=1, point_rows=64, d_start=dev["start"].data_ptr(), d_fixed=dev["fixed"].data_ptr(),
                n_kf=4, problems=call["table"], obs=call["obs"], views=call["views"], params=binding.gba_params(), d_poses=ptrs[0], d_xyz=ptrs[1], d_point_flags=ptrs[2],
                d_obs_flags=ptrs[3], d_result=ptrs[4])
    gp = binding.gba_params
    nan, inf = float("nan"), float("inf")
    kf_out, pt_out, twice = call["obs"].copy(), call["obs"].copy(), call["obs"].copy()
    kf_out["kf"][5], pt_out["point"][6], twice[8] = 4, 64, twice[2]
    bad = [(dict(problems=t((0, 0, 0, 1, 0, n_o))), "n_kf 0 outside 1 .. SS_GBA_MAX_KF (16384)"), (dict(problems=t((0, 16385, 0, 1, 0, n_o))), "n_kf 16385 outside 1 .. SS_GBA_MAX_KF"),
           (dict(problems=t((0, 4, 0, -1, 0, n_o))), "n_blocks -1 of 64 rows outside 0 .. SS_GBA_MAX_POINTS (1048576) points"),
           (dict(problems=t((0, 4, 0, 16385, 0, n_o))), "n_blocks 16385 of 64 rows outside 0 .. SS_GBA_MAX_POINTS"),
           (dict(problems=t((0, 4, 0, 1, 0, -1))), "n_obs -1 outside 0 .. SS_GBA_MAX_OBS (4194304)"), (dict(problems=t((0, 4, 0, 1, 0, 4194305))), "n_obs 4194305 outside 0 .. SS_GBA_MAX_OBS"),
           (dict(problems=np.zeros(65536, binding.GBA_PROBLEM_DTYPE)), "more than 65535 problems in one call"),
           (dict(problems=t((1, 4, 0, 1, 0, n_o))), "keyframes 1 .. + 4 lie outside the call's 4"), (dict(problems=t((0, 4, 1, 1, 0, n_o))), "blocks 1 .. + 1 lie outside the call's 1"),
           (dict(problems=t((0, 4, 0, 1, 1, n_o))), f"records 1 .. + {n_o} lie outside the call's {n_o}"),
           (dict(problems=t((0, 4, 0, 1, 0, n_o, (0, 1)))), "problem 0: the reserved fields must be 0"),
           (dict(problems=t((0, 2, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0))), "problem 1: keyframe 1 belongs to problem 0 already"),
           (dict(problems=t((0, 2, 0, 1, 0, 0), (2, 2, 0, 1, 0, 0))), "problem 1: block 0 belongs to problem 0 already"),
           (dict(problems=t((0, 2, 0, 0, 0, 3), (2, 2, 0, 0, 2, 3))), "problem 1: record 2 belongs to problem 0 already"),
           (dict(obs=kf_out), "problem 0: record 5: kf 4 outside 0 .. 3"), (dict(obs=pt_out), "problem 0: record 6: point 64 outside 0 .. 63"),
           (dict(obs=twice), f"record 8: the pair (kf {twice['kf'][2]}, point {twice['point'][2]}) has a record already"),
           (dict(n_blocks=-1), "bad keyframe, problem, block, row or record count"), (dict(point_rows=0), "bad keyframe, problem, block, row or record count"),
           (dict(point_rows=16385), "point_rows 16385 exceeds SS_GUIDED_MAX_ROWS (16384)"),
           (dict(params=gp(chi2_mono=0.0)), "chi2_mono must be finite and > 0"), (dict(params=gp(chi2_stereo=nan)), "chi2_stereo must be finite and > 0"),
           (dict(params=gp(lambda_=-1.0)), "lambda must be finite and >= 0"), (dict(params=gp(lambda_factor=1.0)), "lambda_factor must be finite and > 1"),
           (dict(params=gp(lambda_min=inf)), "lambda_min must be finite and >= 0"), (dict(params=gp(step_eps=-1.0)), "step_eps must be finite and >= 0"),
           (dict(params=gp(pcg_tol=-1e-3)), "pcg_tol must be finite and >= 0"), (dict(params=gp(n_rounds=5)), "n_rounds must be 1 .. 4"),
           (dict(params=gp(iterations=(33, 0, 0, 0))), "iterations must be 1 .. 32 in every round"), (dict(params=gp(robust_rounds=5)), "robust_rounds must be 0 .. 4"),
           (dict(params=gp(min_point_obs=0)), "min_point_obs must be >= 1"), (dict(params=gp(pcg_iterations=0)), "pcg_iterations must be 1 .. 256"),
           (dict(params=gp(pcg_iterations=257)), "pcg_iterations must be 1 .. 256"), (dict(params=gp(reserved=(0, 1, 0))), "the reserved fields must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.global_ba_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    with pytest.raises(binding.OrbError) as e:
        ctx.global_ba(pr["views"], pr["start"], pr["fixed"], pr["points"], kf_out, gp())
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "record 5: kf 4 outside 0 .. 3" in e.value.message
    assert all((a == FILL).all() for a in out.raw())  # nothing was written
    ctx.global_ba_device(**dict(good, params=_params(binding, GC.LADDER)))  # the context is usable after the refusals
    ctx.synchronize()
    _check("after the refusals", out.host(), call, 0, _twin(pr, GC.LADDER))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
CHAIN = ["synth_t0", "synth_t1", "checker_shift"]


def test_chain_from_the_pose_graph_through_the_global_ba_to_a_projection_search():
    """ss_pose_graph_device -> ss_pose_graph_points_device -> (a projection search gives the observations) -> ss_global_ba_device
    with d_start = the graph's d_poses -> ss_local_ba_points_to_block -> ss_proj_view_init from the new poses ->
    ss_match_proj_batch_device, on three extracted keyframes, against the same chain on the references"""
    import torch
    import graph_cases as QC
    import graph_ref as QR
    import proj_ref as P
    from send_slam_amd import binding
    from test_graph import Out as GraphOut
    from test_proj import Outputs as ProjOut
    from test_proj import _check as _check_proj
    s0 = PC.scenes()[0]
    n = len(CHAIN)
    nc = np.stack([np.concatenate([np.asarray(PC.POSES[k][0], np.float64).reshape(-1), np.asarray(PC.POSES[k][1], np.float64).reshape(-1), [1.0]]) for k in (0, 1)] +
                  [QC.sim3((0.02, -0.3, 0.1), (0.5, -0.2, 0.3), 1.0)])
    start = nc.copy()
    start[2] = QR.mul(QR.cols(nc[2]), QR.cols(QC.sim3((0.01, -0.02, 0.015), (0.05, -0.03, 0.02), 1.05)))[:, 0]
    fixed, edges = np.array([0, 0, 1], np.uint8), np.array([(0, 1), (1, 2), (2, 0)], np.int32)
    graph = QR.optimise(nc, start, fixed, edges)
    cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    search = dict(th=3.0, ratio_num=8, ratio_den=10, one_to_one=True)
    params = dict(GC.SHORT, iterations=(3, 1, 0, 0))
    feats = [G.features(name) for name in CHAIN]
    kp_rows = max(len(f[0]) for f in feats)
    kp, n_kp = np.zeros((n, kp_rows), binding.KP_DTYPE), np.array([len(f[0]) for f in feats], np.int32)
    for b, f in enumerate(feats):
        kp[b, :len(f[0])] = f[0]
    k, point_rows = len(s0["points"]), len(s0["points"]) + 7
    pts, pd = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE), np.zeros((1, point_rows, 32), np.uint8)
    pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
    ref = np.zeros((1, point_rows), np.int32)
    ref[0, 5::17], ref[0, k:] = -1, -1
    # the chain on the references
    moved = pts[0].copy()
    xyz = QR.points(np.stack([pts[0][name] for name in "xyz"], axis=1), ref[0], nc, graph[0])
    for e, name in enumerate("xyz"):
        moved[name] = xyz[:, e]
    wviews = [P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, graph[1][b][:9], graph[1][b][9:], PC.BF) for b in range(n)]
    first = [P.match(wviews[b], moved[:k], s0["p_desc"], feats[b][0], feats[b][1], PC.scale(), **search) for b in range(n)]
    widx = np.stack([f[0] for f in first])
    wobs = GR.obs_from_idx(kp, widx, n_kp)
    assert len(wobs) > 100 and (np.bincount(wobs["point"], minlength=k) >= 2).sum() > 30
    gviews = np.array([PO.view(cam=(PC.FX, PC.FY, PC.CX, PC.CY, PC.BF))] * n)
    wgba = GR.optimise(gviews, graph[1], fixed, PC.scale(), moved[:k], wobs, dict(GR.DEFAULTS, **params))
    assert wgba[4]["state"] == 0 and wgba[4]["accepted"].sum() > 0 and np.abs(wgba[0][:2] - graph[1][:2]).max() > 1e-6
    assert wgba[0][2].tolist() == [float(v) for part in GR.PR.start_pose(graph[1][2])[:2] for v in part]  # the fixed keyframe: its start, orthonormalised
    refined = moved.copy()
    for e, name in enumerate("xyz"):
        refined[name][:k] = np.where(wgba[2] == 2, moved[name][:k], wgba[1][:, e].astype(np.float32))
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        d = torch.from_numpy(np.stack([G.frame(name) for name in CHAIN])).to(_dev())
        c.extract_batch_device(d.data_ptr(), n, G.W, G.H)
        d_pts, d_pd, d_n, d_ref = _to_dev(pts), _to_dev(pd), _to_dev(np.array([k], np.int32)), _to_dev(ref)
        d_nc, d_start, d_fixed = _to_dev(nc), _to_dev(start), _to_dev(fixed)
        gout = GraphOut(n, 1)
        _sync()
        c.pose_graph_device(d_nc.data_ptr(), d_start.data_ptr(), d_fixed.data_ptr(), n, np.array([(0, n, 0, 3)], binding.GRAPH_PROBLEM_DTYPE), edges,
                            binding.graph_params(), *gout.ptrs())
        c.pose_graph_points_device(d_pts.data_ptr(), d_ref.data_ptr(), 1, point_rows, d_nc.data_ptr(), gout.sim3.data_ptr(), n)
        c.synchronize()
        poses = gout.host()[1]
        assert poses.tobytes() == graph[1].tobytes()
        views = [binding.proj_view(cam, poses[b][:9], poses[b][9:], PC.BF) for b in range(n)]
        m = ProjOut(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, PC.combo_params(binding, combo), *m.ptrs(), point_src=[0, 0, 0])
        c.synchronize()
        obs = binding.global_ba_obs_from_idx(kp, m.host()[0][:, :k], n_kp)  # the stack the search left, downloaded
        assert obs.tobytes() == wobs.tobytes()
        out = Out(n, 1, point_rows, len(obs), 1)
        c.global_ba_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, gout.poses.data_ptr(), d_fixed.data_ptr(), n,
                           np.array([(0, n, 0, 1, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE), obs, views, _params(binding, params), *out.ptrs())
        c.local_ba_points_to_block(out.xyz.data_ptr(), out.pflag.data_ptr(), 1, point_rows, d_pts.data_ptr(), 1)
        c.synchronize()
        got = out.host()
        call = dict(table=np.array([(0, n, 0, 1, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE), rows=point_rows)
        _check("chain", got, call, 0, wgba)
        assert d_pts.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(point_rows).tobytes() == refined.tobytes()
        views = [binding.proj_view(cam, got[0][b][:9], got[0][b][9:], PC.BF) for b in range(n)]  # d_poses feeds ss_proj_view_init unchanged
        m = ProjOut(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, PC.combo_params(binding, combo), *m.ptrs(), point_src=[0, 0, 0])
        c.synchronize()
        found = m.host()
        for b in range(n):
            wv = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, wgba[0][b][:9], wgba[0][b][9:], PC.BF)
            second = P.match(wv, refined[:k], s0["p_desc"], feats[b][0], feats[b][1], PC.scale(), **search)
            _check_proj(f"chain, search, frame {b}", found, b, second)
            if b == 0:
                assert second[4]["n_accepted"] > 50
