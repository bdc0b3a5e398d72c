"""GPU parity of the pose-only optimisation (ss_pose_opt_pairs_device, ss_pose_opt_batch_device, ss_pose_opt) against
tests/pose_ref.py through the C ABI: bit for bit, no tolerance -- every byte of every ss_pose_result and every flag.  Every output
starts prefilled with a pattern no result has.  tests/test_pose_ref.py asserts on the reference that the shared cases are live."""
import numpy as np
import pytest

import camera_cases as CC
import guided_cases as G
import pose_cases as C
import pose_ref as PR
import proj_cases as PC
import proj_ref as P

pytestmark = pytest.mark.gpu

CHUNK = 1024          # SSK_POSE_CHUNK: the slots k_pose_gather numbers at a time
MAX_ROWS = 16384      # SS_GUIDED_MAX_ROWS


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
    """device flags [n, slots] and results [n], prefilled with a pattern no result has"""

    def __init__(self, n, slots):
        import torch
        self.n, self.slots = n, slots
        self.flags = torch.full((n, slots), 0x5A, dtype=torch.uint8, device=_dev())
        self.result = torch.full((n, 160), 0x5A, dtype=torch.uint8, device=_dev())
        _sync()

    def host(self):
        from send_slam_amd import binding
        return self.flags.cpu().numpy().copy(), self.result.cpu().numpy().copy().view(binding.POSE_RESULT_DTYPE).reshape(self.n)


def _told(fr):
    """the counts the device is told, where they are not the lengths of the arrays"""
    return fr.get("n_points", len(fr["points"])), fr.get("n_kp", len(fr["kp"]))


def _reference(fr, params, status=0, scale=None):
    """pose_ref on what the device may read of fr: the rows under the counts it is told; the flags of all its slots"""
    n_p, n_k = _told(fr)
    n_p, n_k = min(max(n_p, 0), len(fr["points"])), min(max(n_k, 0), len(fr["kp"]))
    by_row = bool(params.get("idx_by_row", False))
    cut = dict(fr, points=fr["points"][:n_p], kp=fr["kp"][:n_k], idx=fr["idx"][:n_k if by_row else n_p],
               skip=None if fr.get("skip") is None else fr["skip"][:n_p], right=None if fr.get("right") is None else fr["right"][:n_k])
    res, flags = C.solve_frame(cut, params, status, scale=scale)
    full = np.full(len(fr["idx"]), 2, np.uint8)
    full[:len(flags)] = flags
    return res, full


def _upload(frames, point_rows, rows, by_row):
    from send_slam_amd import binding
    n, slots = len(frames), rows if by_row else point_rows
    host = {"points": np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), "skip": np.zeros((n, point_rows), np.uint8), "kp": np.zeros((n, rows), binding.KP_DTYPE),
            "right": np.full((n, rows), 5.0, np.float32), "idx": np.full((n, slots), -1, np.int32), "np": np.zeros(n, np.int32), "nk": np.zeros(n, np.int32)}
    for b, fr in enumerate(frames):
        k_p, k_k, k_s = len(fr["points"]), len(fr["kp"]), len(fr["idx"])
        host["np"][b], host["nk"][b] = _told(fr)
        host["points"][b, :k_p], host["kp"][b, :k_k], host["idx"][b, :k_s] = fr["points"], fr["kp"], fr["idx"]
        if fr.get("skip") is not None:
            host["skip"][b, :k_p] = fr["skip"]
        if fr.get("right") is not None:
            host["right"][b, :k_k] = fr["right"]
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["views"] = np.concatenate([np.asarray(fr["view"]).reshape(1) for fr in frames])
    dev["start"] = np.stack([fr["start"] for fr in frames])
    _sync()
    return dev


def _params(binding, p):
    return binding.pose_opt_params(**{k: p[k] for k in PR.UPSTREAM if k in p})


def _run(ctx, dev, n, point_rows, rows, params, skip=False, right=True, point_src=None, n_blocks=None, views=None, start=None):
    from send_slam_amd import binding
    out = Out(n, rows if params.get("idx_by_row") else point_rows)
    ctx.pose_opt_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), n if n_blocks is None else n_blocks, point_rows, dev["kp"].data_ptr(),
                              dev["nk"].data_ptr(), n, rows, dev["idx"].data_ptr(), dev["views"] if views is None else views,
                              dev["start"] if start is None else start, _params(binding, params), out.flags.data_ptr(), out.result.data_ptr(),
                              point_src=point_src, d_point_skip=dev["skip"].data_ptr() if skip else 0, d_right=dev["right"].data_ptr() if right else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, b, want):
    flags, results = got
    wres, wflags = want
    for name in PR.RESULT_DTYPE.names:
        assert results[b][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[b][name]} != {wres[name]}"
    k = len(wflags)
    bad = np.flatnonzero(flags[b][:k] != wflags)
    assert len(bad) == 0, f"{tag}: flags differ at slots {bad[:8]}: {flags[b][:k][bad[:8]]} != {wflags[bad[:8]]}"
    assert (flags[b][k:] == 2).all(), f"{tag}: the slots past the frame's are not 2"
    assert np.isfinite(results[b]["rcw"]).all() and np.isfinite(results[b]["tcw"]).all() and np.isfinite(results[b]["cost"]), f"{tag}: not finite"


def _against_reference(ctx, frames, point_rows, rows, params, tag, **kw):
    by_row = bool(params.get("idx_by_row", False))
    dev = _upload(frames, point_rows, rows, by_row)
    got = _run(ctx, dev, len(frames), point_rows, rows, params, **kw)
    skip, right = kw.get("skip", False), kw.get("right", True)
    wants = [_reference(dict(fr, skip=fr.get("skip") if skip else None, right=fr.get("right") if right else None), params) for fr in frames]
    for b, w in enumerate(wants):
        _check(f"{tag}, frame {b}", got, b, w)
    return wants, got, dev


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


def _dims(frames):
    return max(len(f["points"]) for f in frames) + 3, max(len(f["kp"]) for f in frames) + 5


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=C.CASE_NAMES)
def test_cases_three_frames_per_call(ctx, k):
    """case k, the same frame started at the truth, and a frame without matches, in one call under case k's parameters"""
    fr, p = C.case_frame(k), C.CASES[k]["params"]
    frames = [fr, dict(fr, start=C.start_of(*fr["truth"])), dict(fr, idx=np.full(len(fr["idx"]), -1, np.int32))]
    wants, _, _ = _against_reference(ctx, frames, *_dims(frames), p, C.CASES[k]["name"])
    assert wants[0][0].tobytes() == C.reference(k)[0].tobytes() and np.array_equal(wants[0][1], C.reference(k)[1])
    assert [int(w[0]["state"]) for w in wants] == [0, 0, 1] and wants[2][0]["n_obs"] == 0
    assert wants[1][0]["rcw"].tobytes() != wants[0][0]["rcw"].tobytes()


N_OBS = [0, 2, 3, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("by_row", [False, True])
def test_observation_counts_around_the_wave_and_the_tree(ctx, by_row):
    """n_obs of 0, 2, 3, one wave, the 256 slots of a tree and their neighbours, and 513, as ten frames of one call"""
    frames = [C.make_frame(100 + n, max(n, 1), n_out=n // 8, n_border=n // 8, by_row=by_row, stereo_every=3, n_points=600, n_kp=560) for n in N_OBS]
    frames[0] = dict(frames[0], idx=np.full(len(frames[0]["idx"]), -1, np.int32))
    p = dict(PR.UPSTREAM, idx_by_row=by_row, check_right=True)
    wants, _, _ = _against_reference(ctx, frames, 600, 560, p, f"counts, idx_by_row {by_row}")
    assert [int(w[0]["n_obs"]) for w in wants] == N_OBS
    assert [int(w[0]["state"]) for w in wants] == [1, 1] + [0] * 8


@pytest.mark.parametrize("by_row", [False, True])
def test_compaction_across_the_chunk_with_bad_rows(ctx, by_row):
    """1025 slots: matches scattered so that observations straddle the wave and chunk boundaries; skip bytes; idx entries negative, at
    and past the count; octaves out of range; counts below the array lengths; without the skip array the skipped are observations"""
    slots = CHUNK + 1
    rng = np.random.Generator(np.random.PCG64(77 + by_row))
    frames = []
    for b in range(2):
        fr = dict(C.make_frame(40 + b, 900, n_out=90, n_border=90, by_row=by_row, stereo_every=4, n_points=slots if not by_row else 1000,
                               n_kp=slots if by_row else 1000))
        fr["idx"], fr["kp"] = fr["idx"].copy(), fr["kp"].copy()
        obs = fr["obs_slots"]
        fr["idx"][rng.choice(np.flatnonzero(fr["idx"] < 0), 6, replace=False)] = [-7, 1000, 1 << 30, 995, 2000, -(1 << 31)]
        bad_oct = rng.choice(obs, 7, replace=False)
        krow = bad_oct if by_row else fr["idx"][bad_oct]
        fr["kp"]["octave"][krow] = [-1, 8, 16, 255, -(1 << 31), (1 << 31) - 1, 9]
        fr["skip"] = np.zeros(len(fr["points"]), np.uint8)
        sk = rng.choice(obs, 9, replace=False)
        fr["skip"][fr["idx"][sk] if by_row else sk] = rng.integers(1, 256, 9)
        fr["n_points"], fr["n_kp"] = len(fr["points"]) - 5 - b, len(fr["kp"]) - 5
        frames.append(fr)
    p = dict(PR.UPSTREAM, idx_by_row=by_row, check_right=True)
    pr, kr = (1000, slots) if by_row else (slots, 1000)
    wants, _, dev = _against_reference(ctx, frames, pr, kr, p, f"compaction, idx_by_row {by_row}", skip=True)
    for fr, (res, flags) in zip(frames, wants):
        assert res["state"] == 0 and 800 < res["n_obs"] < 900 and 0 < res["n_stereo"] < res["n_obs"]
        assert {63, 64, 65, CHUNK - 1, CHUNK} & set(np.flatnonzero(flags != 2).tolist()) and (flags != 2).sum() == res["n_obs"]
        assert np.flatnonzero(flags != 2).max() > res["n_obs"]  # a flag sits on a slot, not on an observation number
    got = _run(ctx, dev, 2, pr, kr, p, skip=False)
    for b, fr in enumerate(frames):
        w = _reference(dict(fr, skip=None), p)
        _check(f"compaction without skip bytes, frame {b}", got, b, w)
        assert w[0]["n_obs"] > wants[b][0]["n_obs"]


def test_compaction_with_a_wave_that_keeps_nothing(ctx):
    """CHUNK + 65 slots, every one an observation but for the 64 of one wave (skip bytes): a wave without a kept slot ahead of waves with
    some, and the chunk boundary inside a run of kept slots"""
    slots = CHUNK + 65
    fr = dict(C.make_frame(48, slots, n_out=100, n_border=100, stereo_every=4))
    fr["skip"] = np.zeros(slots, np.uint8)
    fr["skip"][192:256] = 1
    wants, _, _ = _against_reference(ctx, [fr], slots, slots, dict(PR.UPSTREAM, check_right=True), "a wave that keeps nothing", skip=True)
    res, flags = wants[0]
    assert res["n_obs"] == slots - 64 and res["state"] == 0
    assert (flags[192:256] == 2).all() and (flags[[191, 256, CHUNK - 1, CHUNK, slots - 1]] != 2).all()


def test_two_frames_at_the_row_limit(ctx):
    """SS_GUIDED_MAX_ROWS slots: every slot an observation (64 per thread, the whole mask) and a frame of 9000"""
    frames = [C.make_frame(60, MAX_ROWS, n_out=2000, n_border=2000, stereo_every=2), C.make_frame(61, 9000, n_out=1000, n_border=1000, n_points=MAX_ROWS, n_kp=MAX_ROWS)]
    p = dict(PR.UPSTREAM, check_right=True)
    wants, _, _ = _against_reference(ctx, frames, MAX_ROWS, MAX_ROWS, p, "row limit")
    assert [int(w[0]["n_obs"]) for w in wants] == [MAX_ROWS, 9000] and all(w[0]["state"] == 0 for w in wants)
    p = dict(p, idx_by_row=True)
    frames = [C.make_frame(62, MAX_ROWS, n_out=2000, n_border=2000, stereo_every=2, by_row=True)]
    wants, _, _ = _against_reference(ctx, frames, MAX_ROWS, MAX_ROWS, p, "row limit by row")
    assert wants[0][0]["n_obs"] == MAX_ROWS and wants[0][0]["state"] == 0


def test_stereo_rows(ctx):
    """mixed monocular and stereo observations; right coordinates of 0, -1, NaN and -0.0 are monocular; check_right = 0 and a NULL
    right array make every observation monocular"""
    fr = dict(C.make_frame(70, 200, n_out=25, n_border=30, stereo_every=2))
    fr["right"] = fr["right"].copy()
    st = np.flatnonzero(fr["right"] > 0)
    fr["right"][st[:4]] = [0.0, -1.0, np.nan, -0.0]
    p = dict(PR.UPSTREAM, check_right=True)
    wants, got, dev = _against_reference(ctx, [fr], 200, 200, p, "stereo")
    assert 0 < wants[0][0]["n_stereo"] == len(st) - 4 < wants[0][0]["n_obs"] and wants[0][0]["state"] == 0
    mono = _reference(dict(fr, right=None), PR.UPSTREAM)
    assert mono[0]["n_stereo"] == 0 and mono[0]["rcw"].tobytes() != wants[0][0]["rcw"].tobytes()
    _check("check_right = 0", _run(ctx, dev, 1, 200, 200, PR.UPSTREAM), 0, mono)
    _check("no right array", _run(ctx, dev, 1, 200, 200, p, right=False), 0, mono)


def test_geometry_and_failure_states(ctx):
    """points on and behind the camera plane take no part, nor does a point with a NaN coordinate; every point behind: state 3; a NaN keypoint coordinate: state 2,
    the start pose and no NaN bytes; a start sheared by 1e-3 is orthonormalised; a start so far off that a step exceeds pi: state 4; a start that is not
    finite: state 2 with the identity"""
    cases = C.failure_frames()
    frames = [f for f, _ in cases.values()]
    wants, got, _ = _against_reference(ctx, frames, 128, 128, PR.UPSTREAM, "failures")
    for (name, (fr, state)), (res, flags) in zip(cases.items(), wants):
        assert res["state"] == state, f"{name}: state {res['state']}"
    assert (wants[0][1][frames[0]["obs_slots"][10:31]] == 1).all() and wants[0][0]["n_inliers"] > 60  # on or behind the plane: outliers
    assert wants[1][0]["n_inliers"] == 0 and wants[1][0]["steps"][0] == 1
    r = wants[2][0]
    assert r["rcw"].tobytes() == PR.optimise(frames[2]["view"], frames[2]["start"], PC.scale(), frames[2]["points"][:0], frames[2]["kp"][:0], [], {})[0]["rcw"].tobytes()
    assert r["n_obs"] == 120 and r["n_inliers"] == 0 and r["cost"] == 0 and (wants[2][1][frames[2]["obs_slots"]] == 1).all()  # the NaN pose saw no inlier
    R3 = wants[3][0]["rcw"].reshape(3, 3)
    assert np.abs(R3 @ R3.T - np.eye(3)).max() < 1e-12 and np.abs(R3 - C.R_TRUE).max() < 0.02
    assert wants[4][0]["steps"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert wants[8][1][frames[8]["obs_slots"][50]] == 1 and wants[8][0]["n_obs"] == 120
    for b in (5, 6, 7):
        assert wants[b][0]["rcw"].tolist() == np.eye(3).reshape(9).tolist() and wants[b][0]["tcw"].tolist() == [0, 0, 0]
    assert not np.isnan(got[1].view(np.uint8).reshape(len(frames), 160)[:, :104].copy().view(np.float64)).any()


def test_shared_block_twice_and_permuted(ctx):
    """three frames read one block of points (point_src 0 0 0) from their own starts; the same call twice gives the same bytes; the
    frames of a call permuted leave each frame's bytes unchanged"""
    fr = C.make_frame(90, 300, n_out=40, n_border=40)
    other = dict(fr, start=C.start_of(*fr["truth"]))
    third = dict(fr, start=C.start_of(PC.rot(-0.03, 0.02, 0.0) @ C.R_TRUE, C.T_TRUE - 0.05))
    frames = [fr, other, third]
    dev = _upload(frames, 300, 300, False)
    one_block = dict(dev, points=dev["points"][:1].contiguous(), np=dev["np"][:1].contiguous())
    _sync()
    got = _run(ctx, one_block, 3, 300, 300, PR.UPSTREAM, point_src=[0, 0, 0], n_blocks=1)
    wants = [_reference(f, PR.UPSTREAM) for f in frames]
    for b, w in enumerate(wants):
        _check(f"shared block, frame {b}", got, b, w)
    assert len({w[0]["rcw"].tobytes() for w in wants}) == 3
    again = _run(ctx, one_block, 3, 300, 300, PR.UPSTREAM, point_src=[0, 0, 0], n_blocks=1)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    order = [2, 0, 1]
    perm = _upload([frames[i] for i in order], 300, 300, False)
    pg = _run(ctx, perm, 3, 300, 300, PR.UPSTREAM)
    for j, i in enumerate(order):
        assert pg[0][j].tobytes() == got[0][i].tobytes() and pg[1][j].tobytes() == got[1][i].tobytes()
    with pytest.raises(Exception) as e:
        _run(ctx, one_block, 3, 300, 300, PR.UPSTREAM, point_src=[0, 1, 0], n_blocks=1)
    assert "point_src[1]" in str(e.value)


# ---- odd cameras, per frame ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(C.CAMERA_KINDS))
def test_three_cameras_per_call(ctx, kind):
    """one call whose frames are seen by camera A, camera B and the square camera (fx != fy, principal points off the centre, three
    values of bf), monocular, with every third row stereo, and by keypoint row; the stereo call has a fourth frame whose view has
    bf = 0.  The pairs form and the host form.  tests/test_pose_ref.py shows that a kernel which exchanged fx and fy or cx and cy,
    or read another frame's view or bf, would give other bytes"""
    from send_slam_amd import binding
    frames, p = list(C.camera_frames(kind)), C.camera_params(kind)
    if kind == "every_third_row_stereo":
        frames.append(C.no_baseline_frame())
    assert len({fr["view"].tobytes() for fr in frames}) == len(frames)
    wants, got, _ = _against_reference(ctx, frames, *_dims(frames), p, kind)
    for b, (res, flags, _) in enumerate(C.camera_reference(kind)):
        assert wants[b][0].tobytes() == res.tobytes() and np.array_equal(wants[b][1][:len(flags)], flags) and res["state"] == 0
    for b, fr in enumerate(frames):
        flags, res = ctx.pose_opt(fr["view"], fr["start"], fr["points"], fr["kp"], fr["idx"], _params(binding, p), right=fr["right"])
        _check(f"{kind}, host form, frame {b}", (flags[None], np.array([res])), 0, (wants[b][0], wants[b][1][:len(flags)]))
    if len(frames) == 4:
        assert frames[3]["view"]["bf"] == 0 and wants[3][0]["n_stereo"] > 40 and wants[3][0]["state"] == 0


@pytest.mark.parametrize("name", ["one_level", "sixteen_levels"])
def test_other_pyramid_tables(name):
    """the octave test and the weights read the context's table: one level (every octave but 0 is outside) and SS_MAX_LEVELS"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    fr = C.pyramid_frame(n_levels)
    octave = fr["kp"]["octave"][fr["idx"][fr["obs_slots"]]]
    outside = int(((octave < 0) | (octave >= n_levels)).sum())
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        dev = _upload([fr], *_dims([fr]), False)
        got = _run(c, dev, 1, *_dims([fr]), PR.UPSTREAM)
        flags, res = c.pose_opt(fr["view"], fr["start"], fr["points"], fr["kp"], fr["idx"], _params(binding, PR.UPSTREAM))
    want = _reference(fr, PR.UPSTREAM, scale=sc)
    _check(name, got, 0, want)
    _check(name + ", host form", (flags[None], np.array([res])), 0, want)
    assert outside > 20 and want[0]["n_obs"] == 120 - outside and want[0]["state"] == 0


@pytest.mark.parametrize("name", list(C.LIMITS))
def test_parameter_limits(ctx, name):
    """n_rounds, iterations and robust_rounds at 8, 32 and 0 / 8, step_eps and lambda at 0, min_obs at and above n_obs, on a frame
    of 65 observations and the same frame started at the truth"""
    kw, states = C.LIMITS[name]
    fr = C.make_frame(**C.LIMIT_FRAME)
    frames = [fr, dict(fr, start=C.start_of(*fr["truth"]))]
    wants, _, _ = _against_reference(ctx, frames, *_dims(frames), dict(PR.UPSTREAM, **kw), name)
    assert wants[0][0]["n_obs"] == 65 and wants[0][0]["state"] in states and wants[1][0]["state"] in states
    if name == "eight rounds of 32 steps":
        assert wants[0][0]["steps"].tolist() == [32] * 8 and wants[1][0]["steps"].tolist() == [32] * 8
    if name == "min_obs above n_obs":
        assert wants[0][0]["steps"].tolist() == [0] * 8


def test_singular_system_with_finite_sums(ctx):
    """every observation is one map point on the optical axis, lambda = 0: a pivot is not > 0 (tests/test_pose_ref.py), the frame ends
    in state 2 and carries its start pose; the frame next to it in the call is solved"""
    fr, p = C.singular_frame(), C.SINGULAR_PARAMS
    other = C.camera_frames("by_keypoint_row")[0]
    frames = [fr, dict(other, right=None)]
    wants, got, _ = _against_reference(ctx, frames, *_dims(frames), p, "singular", right=False)
    R, t, ok = PR.start_pose(fr["start"])
    assert ok and got[1][0]["state"] == 2 and got[1][0]["steps"].tolist() == [0] * 8
    assert got[1][0]["rcw"].tobytes() == np.array(R, np.float64).tobytes() and got[1][0]["tcw"].tobytes() == np.array(t, np.float64).tobytes()
    assert got[1][0]["rcw"].tolist() != np.eye(3).reshape(9).tolist() and wants[1][0]["state"] == 0


def test_point_src_neither_identity_nor_constant(ctx):
    """point_src [1, 0, 1] over two blocks with different counts (both under their arrays' lengths) and different skip bytes:
    frames 0 and 2 read block 1's points, count and skip bytes, frame 1 block 0's"""
    a = C.make_frame(91, 130, n_out=15, n_border=20, n_points=150, n_kp=140, cam=CC.A)
    b = C.make_frame(92, 120, n_out=12, n_border=20, n_points=128, n_kp=140, cam=CC.B)
    rng = np.random.Generator(np.random.PCG64(0x5C1))
    for fr, cut in ((a, 7), (b, 3)):
        fr["skip"] = np.zeros(len(fr["points"]), np.uint8)
        fr["skip"][rng.choice(fr["obs_slots"], 9, replace=False)] = rng.integers(1, 256, 9)
        fr["n_points"] = len(fr["points"]) - cut
    frames, blocks, src = [a, b, dict(a, start=C.start_of(*a["truth"]))], [b, a], [1, 0, 1]
    point_rows, rows = _dims(frames)
    dev, blk = _upload(frames, point_rows, rows, False), _upload(blocks, point_rows, rows, False)
    dev = dict(dev, points=blk["points"], np=blk["np"], skip=blk["skip"])
    _sync()
    got = _run(ctx, dev, 3, point_rows, rows, PR.UPSTREAM, skip=True, point_src=src, n_blocks=2)
    wants = [_reference(fr, PR.UPSTREAM) for fr in frames]
    for k, w in enumerate(wants):
        _check(f"point_src {src}, frame {k}", got, k, w)
    assert [int(w[0]["state"]) for w in wants] == [0, 0, 0] and wants[0][0]["rcw"].tobytes() != wants[2][0]["rcw"].tobytes()
    for fr, w in zip(frames, wants):  # the count and the skip bytes of the frame's block both removed observations
        seen = fr["obs_slots"] < fr["n_points"]
        assert 0 < w[0]["n_obs"] == int((seen & (fr["skip"][fr["obs_slots"]] == 0)).sum()) < seen.sum() < len(seen)
    assert wants[0][0]["n_obs"] != wants[1][0]["n_obs"] and a["n_points"] != b["n_points"]


BATCH = ["synth_t0", "synth_t1", "flat"]


def _batch_scene():
    """the map points of proj_cases' first scene (back-projected from synth_t0's keypoints under the identity), the views of its
    first two scenes, a third frame without keypoints"""
    s0, s1 = PC.scenes()[0], PC.scenes()[1]
    views = np.concatenate([np.asarray(v).reshape(1) for v in (s0["view"], s1["view"], s1["view"])])
    start = np.stack([np.concatenate([v["rcw"].astype(np.float64), v["tcw"].astype(np.float64)]) for v in views])
    return s0, s1, views, start


def test_batch_form_pairs_form_and_host_form_and_the_chain(monkeypatch):
    """ss_match_proj_batch_device -> ss_pose_opt_batch_device on the device's own idx -> ss_proj_view_init -> a second, narrower
    search: every stage equals the same chain on the references.  The pairs form and the host form give the batch form's bytes; a
    frame without keypoints has state 1; a flagged frame carries its status"""
    import torch
    from send_slam_amd import binding
    from test_guided import _extract
    from test_proj import Outputs as ProjOut
    from test_proj import _check as _check_proj
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    s0, s1, views, start = _batch_scene()
    n, point_rows = len(BATCH), 500
    combo = dict(ratio=(8, 10), one_to_one=True, th=3.0, check_right=False, taken=False)
    p = dict(PR.UPSTREAM)
    kps = [G.features(name)[0] for name in BATCH]
    k = len(s0["points"])
    pts = np.zeros((1, point_rows), binding.MAP_POINT_DTYPE)
    pd = np.zeros((1, point_rows, 32), np.uint8)
    pts[0, :k], pd[0, :k] = s0["points"], s0["p_desc"]
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        d_pts, d_pd, d_n = _to_dev(pts), _to_dev(pd), _to_dev(np.array([k], np.int32))
        m, out = ProjOut(n, point_rows), Out(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, views, PC.combo_params(binding, combo), *m.ptrs(),
                                  point_src=[0, 0, 0])
        c.pose_opt_batch_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, m.idx.data_ptr(), views, start, _params(binding, p), out.flags.data_ptr(),
                                out.result.data_ptr(), point_src=[0, 0, 0])  # the search's idx, never on the host
        c.synchronize()
        mg, got = m.host(), out.host()
        _check_proj("chain, first search, frame 0", mg, 0, PC.scene_reference(0, combo))
        wants = []
        for b in range(n):
            fr = dict(view=views[b], start=start[b], points=pts[0], kp=kps[b], idx=mg[0][b], n_points=k)
            wants.append(_reference(fr, p))
            _check(f"batch form, frame {b}", got, b, wants[-1])
        assert wants[0][0]["state"] == 0 and wants[0][0]["n_inliers"] > 100 and wants[2][0]["state"] == 1 and wants[2][0]["n_obs"] == 0
        # the map points were back-projected under the identity: the optimum of frame 0
        assert np.abs(wants[0][0]["rcw"].reshape(3, 3) - np.eye(3)).max() < 2e-3 and np.abs(wants[0][0]["tcw"]).max() < 2e-2
        # the pairs form on the same arrays, the host form on frame 0
        d_kp = _to_dev(np.stack([np.concatenate([kp, np.zeros(kcap - len(kp), binding.KP_DTYPE)]) for kp in kps]))
        d_nk = _to_dev(np.array([len(kp) for kp in kps], np.int32))
        out2 = Out(n, point_rows)
        c.pose_opt_pairs_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, d_kp.data_ptr(), d_nk.data_ptr(), n, kcap, m.idx.data_ptr(), views, start,
                                _params(binding, p), out2.flags.data_ptr(), out2.result.data_ptr(), point_src=[0, 0, 0])
        c.synchronize()
        g2 = out2.host()
        assert g2[0].tobytes() == got[0].tobytes() and g2[1].tobytes() == got[1].tobytes()
        flags, one = c.pose_opt(views[0], start[0], pts[0, :k], kps[0], mg[0][0][:k], _params(binding, p))
        assert one.tobytes() == got[1][0].tobytes() and np.array_equal(flags, got[0][0][:k])
        # the next view from the result unchanged, then the narrower search
        cam = binding.Camera(fx=PC.FX, fy=PC.FY, cx=PC.CX, cy=PC.CY, width=G.W, height=G.H)
        v2 = binding.proj_view(cam, got[1][0]["rcw"], got[1][0]["tcw"], PC.BF)
        want_v2 = P.view_init(PC.FX, PC.FY, PC.CX, PC.CY, G.W, G.H, wants[0][0]["rcw"], wants[0][0]["tcw"], PC.BF)
        assert bytes(v2) == want_v2.tobytes()
        narrow = dict(combo, th=1.0)
        m2 = ProjOut(n, point_rows)
        _sync()
        c.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), 1, point_rows, [v2, v2, v2], PC.combo_params(binding, narrow), *m2.ptrs(),
                                  point_src=[0, 0, 0])
        c.synchronize()
        tk, td = G.features(BATCH[0])
        second = P.match(want_v2, s0["points"], s0["p_desc"], tk, td, PC.scale(), th=1.0, ratio_num=8, ratio_den=10, one_to_one=True)
        _check_proj("chain, second search", m2.host(), 0, second)
        assert second[4]["n_accepted"] >= PC.scene_reference(0, narrow)[4]["n_accepted"] > 50
    with binding.OrbContext(0, n_features=G.NF) as c:  # no batch
        with pytest.raises(binding.OrbError) as e:
            c.pose_opt_batch_device(1, 1, 1, point_rows, 1, views[:1], start[:1], _params(binding, p), 1, 1)
        assert e.value.code == binding.SS_ERR_STATE and "ss_pose_opt_batch_device" in e.value.message
    # frame 0 flagged: it carries the status and has no observation
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "0")
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        d_idx = _to_dev(mg[0])
        out = Out(n, point_rows)
        c.pose_opt_batch_device(d_pts.data_ptr(), d_n.data_ptr(), 1, point_rows, d_idx.data_ptr(), views, start, _params(binding, p), out.flags.data_ptr(),
                                out.result.data_ptr(), point_src=[0, 0, 0])
        c.synchronize()
        got = out.host()
        void = _reference(dict(view=views[0], start=start[0], points=pts[0], kp=kps[0], idx=mg[0][0], n_points=k), p, status=binding.SS_ERR_OVERFLOW)
        _check("flagged frame", got, 0, void)
        assert void[0]["status"] == binding.SS_ERR_OVERFLOW and void[0]["state"] == 1 and (void[1] == 2).all()
        _check("the frame next to the flagged one", got, 1, wants[1])
    del torch


def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    fr = C.case_frame(0)
    dev = _upload([fr], 300, 300, False)
    out = Out(1, 300)
    good = dict(d_points=dev["points"].data_ptr(), d_n_points=dev["np"].data_ptr(), n_blocks=1, point_rows=300, d_kp=dev["kp"].data_ptr(),
                d_n_kp=dev["nk"].data_ptr(), n_frames=1, rows_per_frame=300, d_idx=dev["idx"].data_ptr(), views=dev["views"], start_poses=dev["start"],
                params=binding.pose_opt_params(), d_flags=out.flags.data_ptr(), d_result=out.result.data_ptr())
    nan, inf = float("nan"), float("inf")
    pp = binding.pose_opt_params
    bad = [(dict(rows_per_frame=MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"), (dict(point_rows=MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"),
           (dict(point_rows=0), "bad frame, block or row count"), (dict(n_blocks=0), "names no block of points"),
           (dict(params=pp(chi2_mono=0.0)), "chi2_mono must be finite and > 0"), (dict(params=pp(chi2_mono=nan)), "chi2_mono must be finite and > 0"),
           (dict(params=pp(chi2_stereo=inf)), "chi2_stereo must be finite and > 0"), (dict(params=pp(chi2_stereo=-1.0)), "chi2_stereo must be finite and > 0"),
           (dict(params=pp(lambda_=-1e-6)), "lambda must be finite and >= 0"), (dict(params=pp(lambda_=nan)), "lambda must be finite and >= 0"),
           (dict(params=pp(step_eps=-1.0)), "step_eps must be finite and >= 0"), (dict(params=pp(step_eps=inf)), "step_eps must be finite and >= 0"),
           (dict(params=pp(n_rounds=0)), "n_rounds must be 1 .. 8"), (dict(params=pp(n_rounds=9)), "n_rounds must be 1 .. 8"),
           (dict(params=pp(iterations=0)), "iterations must be 1 .. 32"), (dict(params=pp(iterations=33)), "iterations must be 1 .. 32"),
           (dict(params=pp(robust_rounds=-1)), "robust_rounds must be 0 .. 8"), (dict(params=pp(robust_rounds=9)), "robust_rounds must be 0 .. 8"),
           (dict(params=pp(min_obs=2)), "min_obs must be >= 3"), (dict(params=pp(reserved=(0, 1))), "reserved fields must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.pose_opt_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message and e.value.message.startswith(("pose optimisation: ", "frame [")), (kw, e.value.message)
    ctx.pose_opt_pairs_device(**dict(good, n_frames=0, views=dev["views"][:0], start_poses=dev["start"][:0]))  # no frames: nothing is written
    ctx.synchronize()
    assert (out.result.cpu().numpy() == 0x5A).all()
    with pytest.raises(binding.OrbError) as e:
        ctx.pose_opt(fr["view"], fr["start"], fr["points"], fr["kp"], fr["idx"], pp(iterations=0))
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    # the context is usable after every refusal; the host form with skip bytes, by keypoint row, and without rows
    _check("after the refusals", _run(ctx, dev, 1, 300, 300, PR.UPSTREAM), 0, (C.reference(0)[0], C.reference(0)[1]))
    skip = np.zeros(len(fr["points"]), np.uint8)
    skip[fr["obs_slots"][50:60]] = 1
    flags, res = ctx.pose_opt(fr["view"], fr["start"], fr["points"], fr["kp"], fr["idx"], pp(), skip=skip)
    _check("host form with skip bytes", (flags[None], np.array([res])), 0, _reference(dict(fr, skip=skip), PR.UPSTREAM))
    fr2, p2 = C.case_frame(3), C.CASES[3]["params"]
    flags, res = ctx.pose_opt(fr2["view"], fr2["start"], fr2["points"], fr2["kp"], fr2["idx"], _params(binding, p2), right=fr2["right"])
    _check("host form by keypoint row", (flags[None], np.array([res])), 0, (C.reference(3)[0], C.reference(3)[1]))
    flags, res = ctx.pose_opt(fr["view"], fr["start"], fr["points"][:0], fr["kp"][:0], fr["idx"][:0], pp())
    assert len(flags) == 0 and (res["state"], res["n_obs"], res["n_inliers"]) == (1, 0, 0)


def test_stages_and_their_byte_figures(ctx):
    frames = [C.case_frame(0), C.case_frame(0)]
    dev = _upload(frames, 300, 300, False)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        _run(ctx, dev, 2, 300, 300, PR.UPSTREAM, skip=True)
        stats = {s["name"]: s for s in ctx.stats() if s["name"].startswith("pose_")}
    finally:
        ctx.profile(False)
    ns = 2 * 300
    want = {"pose_gather": ns * (4 + 4 + 32 + 24 + 1 + 4 + 28) + 2 * 4, "pose_solve": ns * (28 * 4 * 11 + 4 + 1) + 2 * (96 + 96 + 160)}
    assert list(stats) == list(want)
    for name, b in want.items():
        assert stats[name]["launches"] == 1 and stats[name]["algorithmic_bytes"] == b and stats[name]["total_ms"] > 0, (name, stats[name])
