"""GPU parity of the local bundle adjustment (ss_local_ba_pairs_device, ss_local_ba_batch_device, ss_local_ba,
ss_local_ba_points_to_block) against tests/ba_ref.py through the C ABI: bit for bit, no tolerance -- every pose, point, flag and every
byte of every ss_ba_result.  Every output starts prefilled with a pattern no result has.  tests/test_ba_ref.py asserts on the
reference that the shared cases are live, and that the host twin, which stands in for the reference in the one case too large for
numpy, equals it."""
import numpy as np
import pytest

import ba_cases as BC
import ba_ref as BR
import camera_cases as CC
import guided_cases as G
import pose_cases as PO
import proj_cases as PC
import proj_ref as P

pytestmark = pytest.mark.gpu

MAX_ROWS = 16384  # SS_GUIDED_MAX_ROWS
FILL = 0x5A
SHORT = dict(n_rounds=2, iterations=(2, 1, 0, 0))


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
    """device poses [n_frames][12], xyz [n_problems][P][3], point flags [n_problems][P], observation flags [n_frames][P] and results
    [n_problems], prefilled with a pattern no result has"""

    def __init__(self, n_frames, n_problems, P_):
        import torch
        self.shape = (n_frames, n_problems, P_)
        fill = lambda *s: torch.full(s, FILL, dtype=torch.uint8, device=_dev())  # noqa: E731
        self.poses, self.xyz, self.pflag = fill(n_frames, 96), fill(n_problems, P_ * 24), fill(n_problems, P_)
        self.oflag, self.result = fill(n_frames, P_), fill(n_problems, 88)
        _sync()

    def ptrs(self):
        return tuple(t.data_ptr() for t in (self.poses, self.xyz, self.pflag, self.oflag, self.result))

    def host(self):
        from send_slam_amd import binding
        nf, nq, P_ = self.shape
        return (self.poses.cpu().numpy().copy().view(np.float64).reshape(nf, 12), self.xyz.cpu().numpy().copy().view(np.float64).reshape(nq, P_, 3),
                self.pflag.cpu().numpy().copy(), self.oflag.cpu().numpy().copy(), self.result.cpu().numpy().copy().view(binding.BA_RESULT_DTYPE).reshape(nq))


def _upload(problems, point_rows, rows, blocks=None):
    """the problems' keyframes one after the other; problem q reads block blocks[q] (None: q), which holds the points of the first
    problem that names it"""
    from send_slam_amd import binding
    blocks = list(range(len(problems))) if blocks is None else blocks
    n_frames, n_blocks = sum(len(pr["views"]) for pr in problems), max(blocks) + 1
    host = {"points": np.zeros((n_blocks, point_rows), binding.MAP_POINT_DTYPE), "skip": np.zeros((n_blocks, point_rows), np.uint8), "np": np.zeros(n_blocks, np.int32),
            "kp": np.zeros((n_frames, rows), binding.KP_DTYPE), "right": np.full((n_frames, rows), 5.0, np.float32), "nk": np.zeros(n_frames, np.int32),
            "idx": np.full((n_frames, point_rows), 7, np.int32)}
    table, f0, seen = [], 0, set()
    for pr, b in zip(problems, blocks):
        n_kf, n_p, r = len(pr["views"]), len(pr["points"]), pr["kp"].shape[1]
        if b not in seen:
            host["points"][b, :n_p], host["np"][b] = pr["points"], n_p
            if pr.get("skip") is not None:
                host["skip"][b, :n_p] = pr["skip"]
            seen.add(b)
        host["kp"][f0:f0 + n_kf, :r], host["nk"][f0:f0 + n_kf], host["idx"][f0:f0 + n_kf, :n_p] = pr["kp"], pr["n_kp"], pr["idx"]
        if pr.get("right") is not None:
            host["right"][f0:f0 + n_kf, :r] = pr["right"]
        table.append((f0, n_kf, pr["n_free"], b))
        f0 += n_kf
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev.update(table=np.array(table, binding.BA_PROBLEM_DTYPE), views=np.concatenate([np.asarray(pr["views"]).reshape(-1) for pr in problems]),
               start=np.concatenate([pr["start"] for pr in problems]), n_frames=n_frames, n_blocks=n_blocks)
    _sync()
    return dev


def _params(binding, p):
    return binding.ba_params(**{k: p[k] for k in BR.DEFAULTS if k in p})


def _run(ctx, dev, point_rows, rows, params, skip=False, right=False, table=None):
    from send_slam_amd import binding
    table = dev["table"] if table is None else table
    out = Out(dev["n_frames"], len(table), point_rows)
    ctx.local_ba_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), dev["n_blocks"], point_rows, dev["kp"].data_ptr(), dev["nk"].data_ptr(), dev["n_frames"],
                              rows, dev["idx"].data_ptr(), table, dev["views"], dev["start"], _params(binding, params), *out.ptrs(),
                              d_point_skip=dev["skip"].data_ptr() if skip else 0, d_right=dev["right"].data_ptr() if right else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, q, f0, want, point_rows):
    """problem q of a call, whose keyframes start at frame f0, against a reference result of its n_points rows"""
    poses, xyz, pflag, oflag, results = got
    wposes, wxyz, wpflag, woflag, wres = want[:5]
    n_kf, n_p = len(wposes), len(wxyz)
    for name in BR.RESULT_DTYPE.names:
        assert results[q][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[q][name]} != {wres[name]}"
    assert poses[f0:f0 + n_kf].tobytes() == wposes.tobytes(), f"{tag}: poses differ in keyframes {np.flatnonzero((poses[f0:f0 + n_kf] != wposes).any(axis=1))[:8]}"
    assert xyz[q][:n_p].tobytes() == wxyz.tobytes(), f"{tag}: points differ at rows {np.flatnonzero((xyz[q][:n_p] != wxyz).any(axis=1))[:8]}"
    assert np.array_equal(pflag[q][:n_p], wpflag), f"{tag}: point flags differ at rows {np.flatnonzero(pflag[q][:n_p] != wpflag)[:8]}"
    assert np.array_equal(oflag[f0:f0 + n_kf, :n_p], woflag), f"{tag}: observation flags differ at {np.argwhere(oflag[f0:f0 + n_kf, :n_p] != woflag)[:8].tolist()}"
    assert (pflag[q][n_p:] == 2).all() and (oflag[f0:f0 + n_kf, n_p:] == 2).all() and xyz[q][n_p:].tobytes() == bytes(24 * (point_rows - n_p)), f"{tag}: rows past the points"
    assert np.isfinite(poses[f0:f0 + n_kf]).all() and np.isfinite(xyz[q]).all(), f"{tag}: not finite"
    for name in ("lambda_", "cost_before", "cost_after"):
        assert np.isfinite(results[q][name]), f"{tag}: result.{name} is not finite"


def _against_reference(ctx, problems, params, tag, blocks=None, wants=None, **kw):
    point_rows, rows = max(len(pr["points"]) for pr in problems) + 3, max(pr["kp"].shape[1] for pr in problems) + 5
    dev = _upload(problems, point_rows, rows, blocks)
    got = _run(ctx, dev, point_rows, rows, params, **kw)
    if wants is None:
        wants = [BC.solve(dict(pr, skip=pr.get("skip") if kw.get("skip") else None, right=pr.get("right") if kw.get("right") else None), params) for pr in problems]
    for q, w in enumerate(wants):
        _check(f"{tag}, problem {q}", got, q, int(dev["table"]["first_frame"][q]), w, point_rows)
    return wants, got, dev, (point_rows, rows)


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


def _no_matches(pr):
    return dict(pr, idx=np.full_like(pr["idx"], -1))


def _from_truth(pr):
    return dict(pr, start=pr["truth"][0].copy())


@pytest.mark.parametrize("k", range(len(BC.CASES)), ids=BC.CASE_NAMES)
def test_cases_as_the_first_of_three_problems(ctx, k):
    """case k, the same problem started at the truth, and one without matches, in one call under case k's parameters"""
    pr, p = BC.case_problem(k), BC.CASES[k]["params"]
    wants, _, _, _ = _against_reference(ctx, [pr, _from_truth(pr), _no_matches(pr)], p, BC.CASE_NAMES[k], skip=pr["skip"] is not None, right=pr["right"] is not None)
    ref = BC.reference(k)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(wants[0][:5], ref[:5]))
    assert [int(w[4]["state"]) for w in wants] == [0, 0, 1] and wants[2][4]["n_obs"] == 0 and (wants[2][2] != 0).all()
    assert wants[1][0].tobytes() != wants[0][0].tobytes()
    if BC.CASE_NAMES[k] == "stereo_mixed_6kf_257":  # cameras A, B and the square one in one problem
        assert len({(float(v["fx"]), float(v["fy"])) for v in pr["views"]}) == 3 and [tuple(c) for c in CC.FRAME_CAMERAS] == [CC.A, CC.B, CC.SQUARE]


def test_the_point_ladder_in_one_call(ctx):
    counts = [0, 1, 2, 255, 256, 257, 513]
    problems = [BC.make_problem(seed=200 + n, n_kf=4, n_free=2, n_points=n, rows=max(n, 3) + 5, n_out=min(n // 16, 8)) for n in counts]
    wants, _, _, _ = _against_reference(ctx, problems, SHORT, "point ladder")
    assert [int(w[4]["state"]) for w in wants] == [1, 0, 0, 0, 0, 0, 0]


def test_the_keyframe_ladder_in_one_call(ctx):
    """n_free 1, 2, 3, 32 and n_kf 2, 3, 4, 33, 64: the last two have a reduced system of order 192"""
    shapes = [(2, 1), (3, 2), (4, 3), (33, 32), (64, 32), (64, 1)]
    problems = [BC.make_problem(seed=100 + n_kf + n_free, n_kf=n_kf, n_free=n_free, n_points=70, p_obs=0.5 if n_kf > 8 else 0.9, n_out=6 if n_kf > 2 else 0, stereo_every=3)
                for n_kf, n_free in shapes]
    wants, _, _, _ = _against_reference(ctx, problems, dict(SHORT, check_right=True), "keyframe ladder", right=True)
    assert all(w[4]["state"] == 0 and w[4]["n_stereo"] > 0 and w[4]["steps"][:2].tolist() == [2, 1] for w in wants)


def test_two_problems_of_the_row_limit_sharing_a_block():
    """SS_GUIDED_MAX_ROWS points, 33 keyframes of which 32 are free, twice over one block of points (the second problem starts at the
    truth).  The host twin stands in for the reference here: numpy would take minutes, and tests/test_ba_ref.py holds the twin to the
    reference at this row count and at this order"""
    from send_slam_amd import binding
    pr = BC.make_problem(seed=700, n_kf=33, n_free=32, n_points=MAX_ROWS, p_obs=0.12, n_out=200, skip_every=9, rows=MAX_ROWS)
    p = dict(BR.DEFAULTS, n_rounds=1, iterations=(2, 0, 0, 0))
    problems = [pr, _from_truth(pr)]
    wants = [binding.local_ba_host(q["views"], q["start"], q["n_free"], PC.scale(), q["points"], q["kp"], q["idx"], _params(binding, p), q["n_kp"], q["skip"]) for q in problems]
    assert all(w[4]["state"] == 0 and w[4]["n_points_active"] > 8000 for w in wants) and wants[0][0].tobytes() != wants[1][0].tobytes()
    dev = _upload(problems, MAX_ROWS, MAX_ROWS, blocks=[0, 0])
    with binding.OrbContext(0, n_features=G.NF) as c:
        got = _run(c, dev, MAX_ROWS, MAX_ROWS, p, skip=True)
    for q, w in enumerate(wants):
        _check(f"row limit, problem {q}", got, q, 33 * q, w, MAX_ROWS)


def test_two_small_problems_sharing_a_block_against_the_reference(ctx):
    """two problems over one block of points, each with its own keyframes, observations and start; the block's skip bytes hold for both"""
    a = BC.make_problem(seed=710, n_kf=5, n_free=2, n_points=300, n_out=20, skip_every=6, stereo_every=3)
    b = BC.make_problem(seed=711, n_kf=4, n_free=3, n_points=300, n_out=10, stereo_every=2)
    b = dict(b, points=a["points"], skip=a["skip"])  # b's keyframes look at a's points: its matches are gross outliers or no points
    wants, got, _, _ = _against_reference(ctx, [a, b, _from_truth(a)], dict(SHORT, check_right=True), "shared block", blocks=[0, 0, 0], skip=True, right=True)
    assert wants[0][4]["state"] == 0 and wants[0][4]["n_points_active"] > 200 and wants[1][4]["n_stereo"] > 0
    assert got[1][0].tobytes() != got[1][2].tobytes() and (got[2][:, 1::6][:, :50] == 2).all()


def test_failures(ctx):
    """points behind the cameras, a NaN keypoint (state 2 with the start returned, no NaN byte), a NaN point (no point), a rolled start
    (state 4), a start that is not finite (state 2), in one call"""
    base = BC.make_problem(seed=400, n_kf=4, n_free=2, n_points=90, p_obs=1.0, n_out=8)
    behind = dict(base, points=base["points"].copy())
    behind["points"]["z"][5:15] = -behind["points"]["z"][5:15]
    nan_kp = dict(base, kp=base["kp"].copy())
    nan_kp["kp"]["y"][0, base["idx"][0, 20]] = np.nan
    nan_point = dict(base, points=base["points"].copy())
    nan_point["points"]["y"][33] = np.nan
    rolled = dict(base, start=base["start"].copy())
    rolled["start"][0] = PO.start_of(PC.rot(0.0, 0.0, 3.0) @ base["start"][0][:9].reshape(3, 3), base["start"][0][9:])
    nan_start = dict(base, start=base["start"].copy())
    nan_start["start"][3, 4] = np.nan
    wants, got, _, _ = _against_reference(ctx, [behind, nan_kp, nan_point, rolled, nan_start, base], {}, "failures")
    assert [int(w[4]["state"]) for w in wants] == [0, 2, 0, 4, 2, 0]
    for a in got[:2]:
        assert not np.isnan(a).any()
    assert not any(np.isnan(got[4][name]).any() for name in ("lambda_", "cost_before", "cost_after"))


def test_the_same_call_twice_and_the_problems_permuted(ctx):
    problems = [BC.case_problem(0), BC.case_problem(2), BC.case_problem(4)]
    p = BC.CASES[0]["params"]
    wants, got, dev, (point_rows, rows) = _against_reference(ctx, problems, p, "first call")
    again = _run(ctx, dev, point_rows, rows, p)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    order = [2, 0, 1]
    perm = _run(ctx, dev, point_rows, rows, p, table=dev["table"][order])
    assert perm[0].tobytes() == got[0].tobytes() and perm[3].tobytes() == got[3].tobytes()  # per frame: the frames stay where they are
    for q, src in enumerate(order):  # per problem: they follow the table
        assert perm[1][q].tobytes() == got[1][src].tobytes() and perm[2][q].tobytes() == got[2][src].tobytes() and perm[4][q].tobytes() == got[4][src].tobytes()


def test_frames_of_no_problem_and_the_frozen_point(ctx):
    """a call whose table leaves two frames out: they get their orthonormalised start and flag 2 in every row; the frozen point of
    tests/ba_cases.py freezes on the device as well"""
    import pose_ref as PR
    pr = BC.frozen_problem()
    wants, got, dev, (point_rows, rows) = _against_reference(ctx, [BC.case_problem(3), pr], BC.FROZEN_PARAMS, "frozen")
    assert wants[1][4]["n_frozen_max"] == 1 and wants[0][4]["n_frozen_max"] == 0
    only = _run(ctx, dev, point_rows, rows, BC.FROZEN_PARAMS, table=dev["table"][1:])
    f0 = int(dev["table"]["first_frame"][1])
    _check("the second problem alone", only, 0, f0, wants[1], point_rows)
    start = np.array([list(R) + list(t) for R, t in (PR.start_pose(s)[:2] for s in dev["start"][:f0])])
    assert only[0][:f0].tobytes() == start.tobytes() and (only[3][:f0] == 2).all()


def test_three_problems_with_rotated_camera_rows(ctx):
    """BC.camera_problems(): first frames 0, 4 and 8, and keyframe k of problem q under camera (k + q) % 3, so views[k] for
    views[first_frame + k] in the staging, the blocks or the cost gives problems 1 and 2 other cameras (tests/test_ba_ref.py shows
    on the reference that their bytes change).  Then the table's rows permuted: the frames stay, the problems follow the table"""
    problems, p = BC.camera_problems(), BC.CAMERA_PARAMS
    wants, got, dev, (point_rows, rows) = _against_reference(ctx, problems, p, "rotated camera rows", right=True)
    assert dev["table"]["first_frame"].tolist() == [0, 4, 8] and [int(w[4]["n_obs"]) for w in wants] == [178, 182, 167]
    assert all(w[4]["state"] == 0 and w[4]["n_stereo"] > 80 and w[4]["accepted"].tolist() == [2, 1, 0, 0] for w in wants)
    order = [2, 0, 1]
    perm = _run(ctx, dev, point_rows, rows, p, right=True, table=dev["table"][order])
    assert perm[0].tobytes() == got[0].tobytes() and perm[3].tobytes() == got[3].tobytes()
    for q, src in enumerate(order):
        _check(f"rotated camera rows, permuted, problem {q}", perm, q, int(dev["table"]["first_frame"][src]), wants[src], point_rows)
        assert perm[1][q].tobytes() == got[1][src].tobytes() and perm[2][q].tobytes() == got[2][src].tobytes() and perm[4][q].tobytes() == got[4][src].tobytes()


@pytest.mark.parametrize("name", BC.PYRAMID_NAMES)
def test_other_pyramid_tables(name):
    """the octave test of the gather and the weights read the context's table: 1, 4 and 16 levels, with octaves -1, n_levels and
    n_levels - 1 among the observations"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    pr, table = BC.pyramid_problem(name)
    p = BC.PYRAMID_PARAMS
    want = BC.solve(pr, p, scale=table)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        _against_reference(c, [pr, _from_truth(pr)], p, name, wants=[want, BC.solve(_from_truth(pr), p, scale=table)])
    outside = [(k, i) for k, i, octave in pr["edited"] if octave in (-1, n_levels)]
    assert len(table) == n_levels and len(outside) == 6 and want[4]["n_obs"] == (pr["idx"] >= 0).sum() - 6 and want[4]["state"] == 0
    assert BC.solve(pr, p)[0].tobytes() != want[0].tobytes()  # the default table gives other poses


def test_row_counts_and_junk_idx(ctx):
    """n_kp = (100, 91, 0, 64, 100) over 100 rows with idx entries at n_kp[k], past it, at 1 << 30 and at -7; then the same with one
    count told as rows + 9 and one as -3; and a second problem whose block is told n_points = point_rows + 5"""
    pr, p = BC.row_count_problem(), BC.ROW_COUNT_PARAMS
    second = BC.make_problem(seed=841, n_kf=3, n_free=1, n_points=90, n_out=4, rows=100)
    problems = [pr, second]
    point_rows, rows = 90, 100  # the arrays' own lengths: a count past them has nothing to hide behind
    wants = [BC.solve(q, p) for q in problems]
    assert wants[0][4]["state"] == 0 and (wants[0][3][2] == 2).all() and all(wants[0][3][k, i] == 2 for k, i, _ in pr["junk"])
    dev = _upload(problems, point_rows, rows)
    got = _run(ctx, dev, point_rows, rows, p)
    for q, w in enumerate(wants):
        _check(f"row counts, problem {q}", got, q, 5 * q, w, point_rows)
    told = dict(pr, n_kp=np.array([rows + 9, 91, -3, 64, 100], np.int32))
    dev = _upload([told, second], point_rows, rows)
    dev["np"] = _to_dev(np.array([90, point_rows + 5], np.int32))
    _sync()
    assert dev["nk"].cpu().numpy()[:5].tolist() == [rows + 9, 91, -3, 64, 100]
    again = _run(ctx, dev, point_rows, rows, p)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))


def test_a_free_keyframe_without_observations(ctx):
    """a free keyframe nobody observes: its block of the reduced system is lambda alone.  lambda is a call's, so two calls of two
    problems each, an ordinary problem behind it: under the default lambda state 0, under lambda 0 state 2 with every byte finite
    (_check demands it) and the problem behind it solved"""
    pr = BC.unobserved_free_problem()
    a, b = BC.UNOBSERVED_PARAMS
    for p, state in ((a, 0), (b, 2)):
        wants, got, _, _ = _against_reference(ctx, [pr, BC.camera_problems()[1]], p, f"unobserved free keyframe, lambda {p['lambda_']}", right=True)
        assert wants[0][4]["state"] == state and wants[1][4]["state"] == 0 and (got[3][0] == 2).all()
        assert got[0][0].tobytes() == wants[0][0][0].tobytes()


def test_host_pointer_form_and_points_to_block(ctx):
    import torch
    from send_slam_amd import binding
    k = 1
    pr, p = BC.case_problem(k), BC.CASES[k]["params"]
    got = ctx.local_ba(pr["views"], pr["start"], pr["n_free"], pr["points"], pr["kp"], pr["idx"], _params(binding, p), pr["n_kp"], pr["skip"], pr["right"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, BC.reference(k)[:5]))
    empty = ctx.local_ba(pr["views"], pr["start"], pr["n_free"], pr["points"][:0], pr["kp"], pr["idx"][:, :0], _params(binding, p), pr["n_kp"])
    assert empty[4]["state"] == 1 and empty[1].shape == (0, 3) and empty[0].tobytes() == BC.solve(_no_matches(pr), p)[0].tobytes()
    # the points of two problems back into blocks 2 and 0 of three
    n_p, rows = len(pr["points"]), len(pr["points"]) + 3
    xyz, flags = np.zeros((2, rows, 3)), np.full((2, rows), 2, np.uint8)
    xyz[0, :n_p], flags[0, :n_p] = got[1], got[2]
    xyz[1, :n_p], flags[1, :n_p] = got[1][::-1], got[2][::-1]
    blocks = np.zeros((3, rows), binding.MAP_POINT_DTYPE)
    for name in blocks.dtype.names:
        blocks[name] = np.random.Generator(np.random.PCG64(9)).uniform(1, 2, blocks.shape).astype(np.float32)
    d_blocks, d_xyz, d_flags = _to_dev(blocks), _to_dev(xyz), _to_dev(flags)
    _sync()
    ctx.local_ba_points_to_block(d_xyz.data_ptr(), d_flags.data_ptr(), 2, rows, d_blocks.data_ptr(), 3, block_of=[2, 0])
    ctx.synchronize()
    after = d_blocks.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(3, rows)
    want = blocks.copy()
    for q, b in enumerate((2, 0)):
        move = flags[q] != 2
        for e, name in enumerate("xyz"):
            want[name][b][move] = xyz[q][move][:, e].astype(np.float32)
    assert after.tobytes() == want.tobytes() and (flags[0] != 2).sum() > 200 and (after["x"][1] == blocks["x"][1]).all()
    del torch


def test_stats_stages_and_their_bytes(ctx):
    from send_slam_amd import binding
    pr, p = BC.case_problem(3), BC.CASES[3]["params"]  # one round of ten
    point_rows, rows = len(pr["points"]) + 3, pr["kp"].shape[1] + 5
    dev = _upload([pr, _from_truth(pr)], point_rows, rows)
    with binding.OrbContext(0, n_features=G.NF) as c:
        c.profile(True)
        out = Out(dev["n_frames"], 2, point_rows)
        c.local_ba_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), 2, point_rows, dev["kp"].data_ptr(), dev["nk"].data_ptr(), dev["n_frames"], rows,
                                dev["idx"].data_ptr(), dev["table"], dev["views"], dev["start"], _params(binding, p), *out.ptrs(), d_point_skip=dev["skip"].data_ptr())
        c.local_ba_points_to_block(out.xyz.data_ptr(), out.pflag.data_ptr(), 2, point_rows, dev["points"].data_ptr(), 2)
        c.synchronize()
        got = {(s["name"], s["launches"], s["algorithmic_bytes"]) for s in c.stats()}
    nf, nq, P_, F, K, its = dev["n_frames"], 2, point_rows, pr["n_free"], len(pr["views"]), 10
    nfP, nqP = nf * P_, nq * P_
    state_bytes = 3 * 8 + 18 * 4
    assert got == {("ba_gather", 1, nfP * 21 + nqP * 81 + nqP), ("ba_points", its, nqP * (K * 18 + 24 + F * 288 + 72 + 2)),
                   ("ba_blocks", its, nq * (F * (F + 1) // 2) * P_ * 291 + nq * 36 * F * F * 8), ("ba_solve", its, nq * (36 * F * F * 8 + 6 * F * 16 + F * 192)),
                   ("ba_update", its, nqP * (2 + 48 + 72 + F * 145)), ("ba_cost", its + 1, nq * K * P_ * 42 + nq * K * 8),
                   ("ba_accept", its + 1, nq * (K * 8 + state_bytes)), ("ba_classify", 1, nqP * (1 + K * 17 + 24)),
                   ("ba_finish", 1, nqP * (49 + K) + nf * 96 + nq * 88), ("ba_points_to_block", 1, nqP * 37)}


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
CHAIN = ["parallax_t0", "parallax_t4", "parallax_t8"]  # a camera that moves sideways in front of strips at six depths (synth.parallax_frame)
CHAIN_STEP = 0.1  # the camera's step per frame number: with fx = 300 the strips lie 3.75 .. 15 away


def test_chain_from_the_epipolar_search_to_a_narrower_projection_search(monkeypatch):
    """ss_match_epi_batch_device -> ss_triangulate_batch_device -> ss_match_proj_batch_device on three keyframes ->
    ss_local_ba_batch_device on the device's own points and idx -> ss_local_ba_points_to_block -> a narrower ss_match_proj_batch_device
    under the adjusted poses.  The adjustment equals the reference on what the stages before it left on the device; the batch, pairs
    and host-pointer forms give the same bytes; the last search equals the projection reference on the adjusted map"""
    import bow_cases as BWC
    import epi_cases as EC
    from send_slam_amd import binding
    from test_bow import Transformed, _set
    from test_epi import SearchOut, TriOut
    from test_guided import _extract
    from test_proj import Outputs as ProjOut
    from test_proj import _check as _check_proj
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    n, src = len(CHAIN), [-1, 0, 0]
    poses = [(np.eye(3), (int(name[10:]) * CHAIN_STEP, 0.0, 0.0)) for name in CHAIN]
    pairs = [EC.make_pair(poses[b], poses[src[b]] if src[b] >= 0 else poses[(b + 1) % n]) for b in range(n)]
    cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
    views = [binding.proj_view(cam, np.asarray(r, np.float64), np.asarray(t, np.float64), PC.BF) for r, t in poses]
    start = np.stack([PO.start_of(r, t) for r, t in poses])
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    table = np.array([(0, 3, 1, 1)], binding.BA_PROBLEM_DTYPE)  # keyframes 1 and 2 hold the gauge; the points of pair 1 (frame 1 against frame 0)
    p = dict(BR.DEFAULTS)
    kps = [G.features(name)[0] for name in CHAIN]
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, CHAIN)
        _set(c, BWC.vocab(EC.VOC))
        tr, found, tri = Transformed(n, kcap), SearchOut(n, kcap), TriOut(n, kcap)
        c.bow_transform_batch_device(EC.LEVELSUP, *tr.ptrs())
        c.match_epi_batch_device(pairs, EC.combo_params(binding, dict(coarse=False, one_to_one=True, orientation=1, taken=False)), *found.ptrs(), train_src=src)
        c.triangulate_batch_device(found.idx.data_ptr(), pairs, binding.tri_params(**EC.TRI), *tri.ptrs(), train_src=src)
        m, out = ProjOut(n, kcap), Out(n, 1, kcap)
        _sync()
        c.match_proj_batch_device(tri.points.data_ptr(), tri.desc.data_ptr(), tri.npts.data_ptr(), n, kcap, views, PC.combo_params(binding, combo), *m.ptrs(),
                                  point_src=[1, 1, 1])
        c.local_ba_batch_device(tri.points.data_ptr(), tri.npts.data_ptr(), n, kcap, m.idx.data_ptr(), table, views, start, _params(binding, p), *out.ptrs())
        c.synchronize()
        th, got, idx = tri.host(), out.host(), m.host()[0]
        n_p = int(th[4][1])
        pr = dict(views=np.array([np.frombuffer(bytes(v), P.VIEW_DTYPE)[0] for v in views]), start=start, n_free=1, points=th[1][1][:n_p],
                  kp=np.stack([np.concatenate([kp, np.zeros(kcap - len(kp), binding.KP_DTYPE)]) for kp in kps]), idx=idx[:, :n_p],
                  n_kp=np.array([len(kp) for kp in kps], np.int32), skip=None, right=None)
        want = BC.solve(pr, p)
        _check("chain, batch form", got, 0, 0, want, kcap)
        assert n_p > 30 and want[4]["n_obs"] > 2 * n_p and want[4]["state"] == 0 and want[4]["accepted"].sum() > 0
        # the pairs form on the same arrays, the host-pointer form on host copies
        d_kp, d_nk = _to_dev(pr["kp"]), _to_dev(pr["n_kp"])
        out2 = Out(n, 1, kcap)
        c.local_ba_pairs_device(tri.points.data_ptr(), tri.npts.data_ptr(), n, kcap, d_kp.data_ptr(), d_nk.data_ptr(), n, kcap, m.idx.data_ptr(), table, views, start,
                                _params(binding, p), *out2.ptrs())
        c.synchronize()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out2.host(), got))
        one = c.local_ba(pr["views"], start, 1, pr["points"], pr["kp"], pr["idx"], _params(binding, p), pr["n_kp"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, want[:5]))
        # the adjusted points into their block, the adjusted poses into views, the narrower search
        c.local_ba_points_to_block(out.xyz.data_ptr(), out.pflag.data_ptr(), 1, kcap, tri.points.data_ptr(), n, block_of=[1])
        c.synchronize()
        block = tri.host()[1]
        moved = th[1][1][:n_p].copy()
        for e, name in enumerate("xyz"):
            moved[name] = np.where(want[2] != 2, want[1][:, e].astype(np.float32), moved[name])
        assert block[1][:n_p].tobytes() == moved.tobytes() and block[0].tobytes() == th[1][0].tobytes() and block[1][n_p:].tobytes() == th[1][1][n_p:].tobytes()
        v2 = [binding.proj_view(cam, got[0][b][:9], got[0][b][9:], PC.BF) for b in range(n)]
        narrow = dict(combo, th=1.5)
        m2 = ProjOut(n, kcap)
        _sync()
        c.match_proj_batch_device(tri.points.data_ptr(), tri.desc.data_ptr(), tri.npts.data_ptr(), n, kcap, v2, PC.combo_params(binding, narrow), *m2.ptrs(),
                                  point_src=[1, 1, 1])
        c.synchronize()
        for b in range(n):
            tk, td = G.features(CHAIN[b])
            wv = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, want[0][b][:9], want[0][b][9:], PC.BF)
            second = P.match(wv, moved, th[2][1][:n_p], tk, td, PC.scale(), th=1.5, ratio_num=8, ratio_den=10, one_to_one=True)
            _check_proj(f"chain, second search, frame {b}", m2.host(), b, second)
    with binding.OrbContext(0, n_features=G.NF) as c:  # no batch
        with pytest.raises(binding.OrbError) as e:
            c.local_ba_batch_device(1, 1, 1, kcap, 1, table, views, start, _params(binding, p), 1, 1, 1, 1, 1)
        assert e.value.code == binding.SS_ERR_STATE and "ss_local_ba_batch_device" in e.value.message
    # frame 1 flagged: the problem carries the status, state 1, no point and no observation
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1")
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _extract(c, CHAIN)
        d_pts, d_np, d_idx = _to_dev(th[1]), _to_dev(th[4]), _to_dev(idx)
        out = Out(n, 1, kcap)
        c.local_ba_batch_device(d_pts.data_ptr(), d_np.data_ptr(), n, kcap, d_idx.data_ptr(), table, views, start, _params(binding, p), *out.ptrs())
        c.synchronize()
        void = BC.solve(pr, p, status=binding.SS_ERR_OVERFLOW)
        _check("flagged frame", out.host(), 0, 0, void, kcap)
        assert void[4]["status"] == binding.SS_ERR_OVERFLOW and void[4]["state"] == 1 and (void[2] == 2).all() and (void[3] == 2).all()


def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    pr = BC.case_problem(0)
    dev = _upload([pr], 310, 310)
    out = Out(8, 1, 310)
    ptrs = out.ptrs()
    good = dict(d_points=dev["points"].data_ptr(), d_n_points=dev["np"].data_ptr(), n_blocks=1, point_rows=310, d_kp=dev["kp"].data_ptr(), d_n_kp=dev["nk"].data_ptr(),
                n_frames=8, rows_per_frame=310, d_idx=dev["idx"].data_ptr(), problems=dev["table"], views=dev["views"], start_poses=dev["start"],
                params=binding.ba_params(), d_poses=ptrs[0], d_xyz=ptrs[1], d_point_flags=ptrs[2], d_obs_flags=ptrs[3], d_result=ptrs[4])
    nan, inf = float("nan"), float("inf")
    bp = binding.ba_params
    tab = lambda *rows: np.array(list(rows), binding.BA_PROBLEM_DTYPE)  # noqa: E731
    bad = [(dict(rows_per_frame=MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"), (dict(point_rows=MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"),
           (dict(point_rows=0), "bad frame, problem, block or row count"), (dict(n_blocks=0), "point_block 0 names no block of points (0)"),
           (dict(problems=tab((0, 8, 8, 0))), "n_free 8 of n_kf 8 leaves no fixed keyframe to hold the gauge"),
           (dict(problems=tab((0, 8, 0, 0))), "n_free 0 outside 1 .. SS_BA_MAX_FREE (32)"), (dict(problems=tab((0, 8, 33, 0))), "n_free 33 outside 1 .. SS_BA_MAX_FREE (32)"),
           (dict(problems=tab((0, 65, 4, 0))), "n_kf 65 outside 1 .. SS_BA_MAX_KF (64)"), (dict(problems=tab((0, 0, 1, 0))), "n_kf 0 outside 1 .. SS_BA_MAX_KF (64)"),
           (dict(problems=tab((1, 8, 4, 0))), "frames 1 .. + 8 lie outside the call's 8"), (dict(problems=tab((-1, 8, 4, 0))), "lie outside the call's 8"),
           (dict(problems=tab((0, 4, 2, 0), (3, 4, 2, 0))), "problem 1: frame 3 belongs to problem 0 already"),
           (dict(problems=tab((0, 8, 4, 1))), "point_block 1 names no block of points (1)"),
           (dict(params=bp(chi2_mono=0.0)), "chi2_mono must be finite and > 0"), (dict(params=bp(chi2_stereo=inf)), "chi2_stereo must be finite and > 0"),
           (dict(params=bp(lambda_=-1e-6)), "lambda must be finite and >= 0"), (dict(params=bp(lambda_=nan)), "lambda must be finite and >= 0"),
           (dict(params=bp(lambda_factor=1.0)), "lambda_factor must be finite and > 1"), (dict(params=bp(lambda_factor=inf)), "lambda_factor must be finite and > 1"),
           (dict(params=bp(lambda_min=-1.0)), "lambda_min must be finite and >= 0"), (dict(params=bp(step_eps=inf)), "step_eps must be finite and >= 0"),
           (dict(params=bp(n_rounds=0)), "n_rounds must be 1 .. 4"), (dict(params=bp(n_rounds=5)), "n_rounds must be 1 .. 4"),
           (dict(params=bp(iterations=(5, 0, 0, 0))), "iterations must be 1 .. 32 in every round"), (dict(params=bp(iterations=(33, 1, 0, 0))), "iterations must be 1 .. 32"),
           (dict(params=bp(robust_rounds=-1)), "robust_rounds must be 0 .. 4"), (dict(params=bp(robust_rounds=5)), "robust_rounds must be 0 .. 4"),
           (dict(params=bp(min_point_obs=0)), "min_point_obs must be >= 1"), (dict(params=bp(reserved=(0, 0, 1, 0))), "reserved fields must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.local_ba_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    for kw, msg in ((dict(point_rows=0), "bad problem, block or row count"), (dict(block_of=[1]), "block_of[0] = 1 names no block of points (1)"),
                    (dict(d_xyz=0), "NULL buffer")):
        with pytest.raises(binding.OrbError) as e:
            ctx.local_ba_points_to_block(**dict(dict(d_xyz=ptrs[1], d_point_flags=ptrs[2], n_problems=1, point_rows=310, d_points=dev["points"].data_ptr(), n_blocks=1), **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
    ctx.local_ba_pairs_device(**dict(good, n_frames=0, problems=tab(), views=dev["views"][:0], start_poses=dev["start"][:0]))  # nothing to do, nothing written
    ctx.synchronize()
    assert out.host()[0].tobytes() == bytes([FILL]) * (8 * 96)
    ctx.local_ba_pairs_device(**good)  # the context is usable after the refusals
    ctx.synchronize()
    _check("after the refusals", out.host(), 0, 0, BC.solve(pr, {}), 310)
