"""GPU parity of the Sim3 refinement (ss_sim3_opt_pairs_device, ss_sim3_opt_batch_device, ss_sim3_opt, ss_sim3_marks_*, ss_sim3_mutual_*)
against tests/sim3opt_ref.py through the C ABI: bit for bit, no tolerance -- every byte of every ss_sim3_opt_result, every flag and
every index.  Every output starts prefilled with a pattern no result has.  tests/test_sim3opt_ref.py asserts on the reference that the
shared cases and the chain are live, and that the scenes under odd cameras, other pyramid tables, the parameters' limits, a singular
system and skip bytes per frame change their bytes under every confusion a kernel could make."""
import numpy as np
import pytest

import guided_cases as G
import proj_cases as PC
import proj_ref as P
import sim3_cases as SC
import sim3_ref as S
import sim3opt_cases as OC
import sim3opt_ref as O
from test_sim3 import _dev, _sync, _to_dev, _told, _upload

pytestmark = pytest.mark.gpu

ROWS = 320  # rows of the pairs form the shared cases run through
FILL = 0x5A


class Out:
    """device flags [n, rows] and results [n], prefilled"""

    def __init__(self, n, rows):
        import torch
        self.n, self.rows = n, rows
        self.flags = torch.full((n, rows), FILL, dtype=torch.uint8, device=_dev())
        self.result = torch.full((n, 272), FILL, dtype=torch.uint8, device=_dev())
        _sync()

    def host(self):
        return self.flags.cpu().numpy().copy(), self.result.cpu().numpy().copy().view(O.RESULT_DTYPE).reshape(self.n)


def _starts(pairs):
    return _to_dev(np.array([np.asarray(pr["start"], S.RESULT_DTYPE).reshape(()) for pr in pairs], S.RESULT_DTYPE))


def _reference(pr, params, status=0, scale=None):
    """sim3opt_ref on what the device may read of pr: the rows under the counts it is told"""
    nq, nt = _told(pr)
    cut = dict(pr, q_xyz=pr["q_xyz"][:nq], q_kp=pr["q_kp"][:nq], idx=pr["idx"][:nq], t_xyz=pr["t_xyz"][:nt], t_kp=pr["t_kp"][:nt],
               q_skip=None if pr["q_skip"] is None else pr["q_skip"][:nq], t_skip=None if pr["t_skip"] is None else pr["t_skip"][:nt])
    return OC.solve_pair(cut, params, status=status, scale=scale)


def _run(ctx, dev, d_start, n, rows, params, skip=True):
    from send_slam_amd import binding
    out = Out(n, rows)
    ctx.sim3_opt_pairs_device(dev["q_xyz"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_xyz"].data_ptr(), dev["t_kp"].data_ptr(),
                              dev["nt"].data_ptr(), dev["idx"].data_ptr(), n, rows, dev["views1"], dev["views2"], d_start.data_ptr(),
                              binding.sim3_opt_params(**params), out.flags.data_ptr(), out.result.data_ptr(),
                              d_query_skip=dev["q_skip"].data_ptr() if skip else 0, d_train_skip=dev["t_skip"].data_ptr() if skip else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, b, want, rows=None):
    flags, results = got
    wres, wflags = want
    for name in O.RESULT_DTYPE.names:
        assert np.asarray(results[b][name]).tobytes() == np.asarray(wres[name]).tobytes(), f"{tag}: result.{name} {results[b][name]} != {wres[name]}"
    nq = len(wflags)
    bad = np.flatnonzero(flags[b][:nq] != wflags)
    assert len(bad) == 0, f"{tag}: flags differ at query rows {bad[:8]}: {flags[b][:nq][bad[:8]]} != {wflags[bad[:8]]}"
    assert (flags[b][nq:rows] == 2).all(), f"{tag}: a row past the query rows is not flagged 2"
    raw = np.frombuffer(results[b].tobytes(), np.uint8)
    assert not np.isnan(raw[:112].view(np.float64)).any() and not np.isnan(raw[144:244].view(np.float32)).any(), f"{tag}: NaN bits in a result"


def _pairs_against_reference(ctx, pairs, rows, params, tag, skip=True, scale=None):
    dev = _upload(pairs, rows)
    got = _run(ctx, dev, _starts(pairs), len(pairs), rows, params, skip)
    wants = [_reference(pr, params, scale=scale) for pr in pairs]
    for b, w in enumerate(wants):
        _check(f"{tag}, pair {b}", got, b, w)
    return wants, got


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=2) as c:
        yield c


@pytest.mark.parametrize("k", range(len(OC.CASES)), ids=OC.CASE_NAMES)
def test_cases_three_pairs_per_call(ctx, k):
    """case k with two other cases behind it in one call under case k's parameters"""
    n = len(OC.CASES)
    pairs = [OC.case_pair(j) for j in (k, (k + 1) % n, (k + 3) % n)]
    wants, _ = _pairs_against_reference(ctx, pairs, ROWS, OC.CASES[k]["params"], OC.CASES[k]["name"], skip=False)
    assert wants[0][0].tobytes() == OC.reference(k)[0].tobytes()


@pytest.mark.parametrize("fix", [False, True], ids=["scale", "fix_scale"])
def test_counts_twelve_pairs_of_one_call(ctx, fix):
    counts = [0, 2, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513]
    pairs = [OC.count_pair(n, fix) for n in counts]
    wants, _ = _pairs_against_reference(ctx, pairs, 520, dict(O.UPSTREAM, fix_scale=fix), f"counts, fix_scale {fix}", skip=False)
    assert [int(w[0]["n_corr"]) for w in wants] == counts
    assert [int(w[0]["state"]) for w in wants[:5]] == [1, 1, 1, 3, 0] and all(w[0]["state"] == 0 for w in wants[5:])  # ten with one mismatch: nine left


def _scattered():
    """1025 rows: scattered matches, skip bytes on both sides, negative and out-of-range idx, octaves out of range, counts below the
    array lengths"""
    pr = OC.with_skips(OC.make_pair(60, 400, 40, 1025, 1025), 2, every=9)
    rows = pr["rows"]
    idx, q_kp, t_kp = pr["idx"].copy(), pr["q_kp"].copy(), pr["t_kp"].copy()
    free = np.setdiff1d(np.arange(1025), rows)
    idx[free[:20]] = [-3, 1025, 5000, -1, 2 ** 30] * 4
    idx[free[20:30]] = 1000  # past the train count the device is told
    q_kp["octave"][rows[::17]] = 8
    q_kp["octave"][rows[5::31]] = -1
    t_kp["octave"][idx[rows[3::23]]] = 9
    return dict(pr, idx=idx, q_kp=q_kp, t_kp=t_kp, n_query=1011, n_train=990)


def test_compaction_over_chunks(ctx):
    pr = _scattered()
    wants, got = _pairs_against_reference(ctx, [pr, OC.case_pair(0)], 1025, O.UPSTREAM, "1025 scattered rows")
    assert 150 < wants[0][0]["n_corr"] < 400 and wants[0][0]["state"] == 0


def test_compaction_with_a_wave_that_keeps_nothing(ctx):
    """1024 + 65 rows, every one a correspondence but for the 64 of one wave (skip bytes): a wave without a kept row ahead of waves with
    some, and the chunk boundary inside a run of kept rows"""
    rows = 1024 + 65
    pr = dict(OC.make_pair(62, rows, rows // 8, rows, rows))
    pr["q_skip"] = np.zeros(rows, np.uint8)
    pr["q_skip"][192:256] = 1
    wants, _ = _pairs_against_reference(ctx, [pr], rows, O.UPSTREAM, "a wave that keeps nothing")
    res, flags = wants[0]
    assert res["n_corr"] == rows - 64 and res["state"] == 0
    assert (flags[192:256] == 2).all() and (flags[[191, 256, 1023, 1024, rows - 1]] != 2).all()


def test_two_full_pairs(ctx):
    from send_slam_amd import binding
    rows = binding.SS_GUIDED_MAX_ROWS
    pairs = [OC.make_pair(90, rows, rows // 8, rows, rows), OC.with_skips(OC.make_pair(91, 9000, 900, rows, rows), 3)]
    wants, _ = _pairs_against_reference(ctx, pairs, rows, O.UPSTREAM, "two pairs of SS_GUIDED_MAX_ROWS rows")
    assert wants[0][0]["n_corr"] == rows and wants[0][0]["state"] == 0 and wants[1][0]["state"] == 0


def _moved(pr, side, sel, fn):
    """the map points of the correspondences `sel` (indices into pr["rows"]) of keyframe `side` moved to fn(camera coordinates)"""
    pose, key = (SC.POSE1, "q_xyz") if side == 1 else (SC.POSE2, "t_xyz")
    r = pr["rows"][sel] if side == 1 else pr["idx"][pr["rows"][sel]]
    xyz = pr[key].copy()
    w = np.stack([xyz[n][r] for n in "xyz"], 1).astype(np.float64)
    cam = fn(w @ np.asarray(pose[0]).T + np.asarray(pose[1]))
    back = (cam - np.asarray(pose[1])) @ np.asarray(pose[0])
    xyz["x"][r], xyz["y"][r], xyz["z"][r] = back[:, 0], back[:, 1], back[:, 2]
    return dict(pr, **{key: xyz})


def test_points_on_and_behind_either_camera(ctx):
    base = OC.make_pair(61, 120, 10, 128, 128)
    flip, plane = lambda c: c * [1, 1, -1], lambda c: c * [1, 1, 0]  # noqa: E731
    some = _moved(_moved(base, 2, np.arange(0, 120, 9), flip), 1, np.arange(4, 120, 9), flip)
    flips = some
    some = _moved(_moved(flips, 2, np.array([2]), plane), 1, np.array([6]), plane)
    more = _moved(_moved(flips, 2, np.array([2, 62]), plane), 1, np.array([6, 66]), plane)  # four points at almost no depth: a step too large
    every = _moved(_moved(base, 2, np.arange(120), flip), 1, np.arange(120), flip)
    wants, _ = _pairs_against_reference(ctx, [some, every, base, more], 128, O.UPSTREAM, "behind the cameras", skip=False)
    assert wants[0][0]["state"] == 0 and wants[0][0]["n_removed"] >= 27 + 10 - 2 and wants[2][0]["state"] == 0 and wants[2][0]["n_removed"] == 10
    assert wants[1][0]["state"] == 3 and wants[1][0]["n_inliers"] == 0 and wants[3][0]["state"] == 4


def test_non_finite_and_degenerate_inputs(ctx):
    base = OC.make_pair(62, 80, 8, 96, 96)
    nan_kp, nan_pt = dict(base, q_kp=base["q_kp"].copy(), t_kp=base["t_kp"].copy()), dict(base, q_xyz=base["q_xyz"].copy(), t_xyz=base["t_xyz"].copy())
    nan_kp["q_kp"]["x"][base["rows"][3]] = np.nan
    nan_kp["t_kp"]["y"][base["idx"][base["rows"][7]]] = np.inf
    nan_pt["q_xyz"]["z"][base["rows"][5]] = np.nan
    nan_pt["t_xyz"]["x"][base["idx"][base["rows"][9]]] = np.nan
    shear = base["start"].copy()
    shear["sr12"][1] += np.float32(1e-3)
    no_model = base["start"].copy()
    no_model["state"] = 1
    nan_start = base["start"].copy()
    nan_start["t12"][1] = np.nan
    pairs = [nan_kp, nan_pt, dict(base, start=shear), dict(base, start=np.zeros((), S.RESULT_DTYPE)), dict(base, start=no_model), dict(base, start=nan_start)]
    wants, got = _pairs_against_reference(ctx, pairs, 96, O.UPSTREAM, "non-finite and degenerate", skip=False)
    assert [int(w[0]["state"]) for w in wants[2:]] == [0, 2, 1, 2]
    assert not np.isnan(got[1].view(np.uint8).reshape(len(pairs), 272)[:, :112].copy().view(np.float64)).any()


def test_same_call_twice_and_pairs_permuted(ctx):
    pairs = [OC.case_pair(0), OC.case_pair(5), OC.case_pair(2), OC.case_pair(4)]
    p = O.UPSTREAM
    dev, st = _upload(pairs, ROWS), _starts(pairs)
    a, b = _run(ctx, dev, st, 4, ROWS, p), _run(ctx, dev, st, 4, ROWS, p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    order = [2, 0, 3, 1]
    perm = [pairs[j] for j in order]
    c = _run(ctx, _upload(perm, ROWS), _starts(perm), 4, ROWS, p)
    for at, j in enumerate(order):
        assert c[0][at].tobytes() == a[0][j].tobytes() and c[1][at].tobytes() == a[1][j].tobytes()
        _check(f"permuted, pair {at}", c, at, _reference(pairs[j], p))


def _host_form(ctx, pr, params, tag, scale=None):
    from send_slam_amd import binding
    flags, one = ctx.sim3_opt(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], pr["start"],
                              binding.sim3_opt_params(**params), pr["q_skip"], pr["t_skip"])
    _check(tag, (flags[None], np.array([one])), 0, _reference(pr, params, scale=scale))


# ---- odd cameras, per pair and per side ---------------------------------------------------------------------------------------------------
def test_three_camera_pairs_per_call(ctx):
    """one call whose pairs are seen by the cameras (P, Q), (Q, P) and (square, P): fx != fy, principal points off the centre, the two
    sides of a pair different.  Both residuals read all four intrinsics of their side (tests/test_sim3opt_ref.py shows that exchanging
    fx and fy, cx and cy, the sides, or the pairs' views changes the result and the flags of every pair it touches).  The pairs form
    and the host form"""
    pairs = OC.camera_pairs()
    wants, _ = _pairs_against_reference(ctx, pairs, 64, O.UPSTREAM, "cameras", skip=False)
    for b, w in enumerate(OC.camera_reference()):
        assert wants[b][0].tobytes() == w[0].tobytes() and wants[b][1].tobytes() == w[1].tobytes()
        assert w[0]["state"] == 0 and 0 < w[0]["n_removed"] < w[0]["n_corr"] == 60
    for b, pr in enumerate(pairs):
        _host_form(ctx, pr, O.UPSTREAM, f"cameras, host form of pair {b}")


def test_batch_form_under_a_camera_per_frame_with_skip_bytes():
    """ss_sim3_opt_batch_device and ss_sim3_marks_batch_device with views[b] and views[train_src[b]] different for every frame (frames
    1 and 2 train on frame 0; the frames are seen by P, Q and the square camera), the starts written by ss_sim3_batch_device on the
    device; without skip bytes and with one array of them, which the query side reads at frame b and the train side at frame
    train_src[b]"""
    import torch
    from send_slam_amd import binding
    from test_guided import _extract
    from test_sim3 import Out as RansacOut
    kps, xyz, idx, views = SC.camera_batch()
    n, src = len(SC.CAMERA_BATCH), SC.CAMERA_BATCH_SRC
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, SC.CAMERA_BATCH)
        assert kcap >= xyz.shape[1]
        pad = lambda a, fill: np.concatenate([a, np.full((n, kcap - a.shape[1]), fill, a.dtype)], axis=1)  # noqa: E731
        d_xyz, d_idx, skip = _to_dev(pad(xyz, 0)), _to_dev(pad(idx, -1)), pad(OC.camera_batch_skip(), 0)
        d_skip = _to_dev(skip)
        ransac = RansacOut(n, kcap)
        _sync()
        c.sim3_batch_device(d_xyz.data_ptr(), d_idx.data_ptr(), views, binding.sim3_params(**SC.camera_params(20)), ransac.inlier.data_ptr(),
                            ransac.result.data_ptr(), train_src=src)
        c.synchronize()
        starts = ransac.host()[1]
        for b, w in enumerate(OC.camera_batch_starts()):  # the starts the references below are computed from
            assert starts[b].tobytes() == w.tobytes(), b
        for with_skip in (False, True):
            out = Out(n, kcap)
            s1, s2 = (torch.full((n, kcap), FILL, dtype=torch.uint8, device=_dev()) for _ in range(2))
            _sync()
            c.sim3_opt_batch_device(d_xyz.data_ptr(), d_idx.data_ptr(), views, ransac.result.data_ptr(), binding.sim3_opt_params(**OC.BATCH_PARAMS),
                                    out.flags.data_ptr(), out.result.data_ptr(), train_src=src, d_skip=d_skip.data_ptr() if with_skip else 0)
            c.sim3_marks_batch_device(d_idx.data_ptr(), s1.data_ptr(), s2.data_ptr(), train_src=src, d_skip=d_skip.data_ptr() if with_skip else 0)
            c.synchronize()
            got, g1, g2 = out.host(), s1.cpu().numpy(), s2.cpu().numpy()
            for b, t in enumerate(src):
                tag = f"cameras, batch form, skip bytes {with_skip}, frame {b} against {t}"
                w = _reference(OC.camera_batch_pair(b, skip=skip if with_skip else None), OC.BATCH_PARAMS)
                _check(tag, got, b, w, kcap)
                nq, nt = len(kps[b]), len(kps[t]) if t >= 0 else 0
                full = pad(idx, -1)[b]
                w1, w2 = O.marks(full, skip[b] if with_skip else None, skip[t] if with_skip and t >= 0 else None, nq, nt)
                assert g1[b].tobytes() == w1.tobytes() and g2[b].tobytes() == w2.tobytes(), tag
                if t < 0:
                    assert w[0]["state"] == 1 and (w[1] == 2).all() and not w2.any()
                else:
                    assert w[0]["state"] == 0 and min(w[0]["steps"]) >= 1 and (w[0]["n_corr"] == 60) != with_skip and w[0]["n_corr"] > 20


# ---- other pyramid tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.PYRAMID_OCTAVES))
def test_other_pyramid_tables(name):
    """the octave test of the gather and both weights read the context's table: one level (every octave but 0 is outside) and
    SS_MAX_LEVELS, under cameras P and Q; the pairs form and the host form"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    pr, sc = OC.pyramid_pair(name)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        wants, _ = _pairs_against_reference(c, [pr, OC.camera_pairs()[0]], 128, O.UPSTREAM, name, skip=False, scale=sc)
        _host_form(c, pr, O.UPSTREAM, f"{name}, host form", scale=sc)
    assert wants[0][0]["state"] == 0 and 30 <= wants[0][0]["n_corr"] < 80 and wants[0][0]["n_removed"] > 0


# ---- the parameters at their limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.LIMITS))
def test_parameter_limits(ctx, name):
    """the 65-correspondence pair from a start a few pixels off and from the scene's own Sim3, in one call"""
    wants, _ = _pairs_against_reference(ctx, OC.limit_pairs(), 72, OC.limit_params(name), name, skip=False)
    for w, (state, steps, n_removed) in zip(wants, OC.LIMITS_RECORDED[name]):
        assert (int(w[0]["state"]), w[0]["steps"].tolist(), int(w[0]["n_removed"])) == (state, steps, n_removed) and state in OC.LIMITS[name][1]


@pytest.mark.parametrize("fix", [False, True], ids=["scale", "fix_scale"])
def test_singular_system_with_finite_sums(ctx, fix):
    """sim3opt_cases.singular_pair: finite sums, the third pivot 0 by structure, so the solve fails and the model stays the start (a
    quarter turn, not the identity); the pair behind it in the call is solved"""
    pairs = [OC.singular_pair(fix), OC.camera_pairs()[0]]
    p = dict(OC.SINGULAR_PARAMS, fix_scale=fix)
    wants, got = _pairs_against_reference(ctx, pairs, 64, p, f"singular, fix_scale {fix}", skip=False)
    R, t, s, _ = O.start(pairs[0]["start"], fix)
    one = got[1][0]
    assert one["state"] == 2 and one["steps"].tolist() == [0, 0] and one["n_corr"] == 30 and np.isfinite(one["cost"])
    assert one["r12"].tolist() == [float(v) for v in R] and one["t12"].tolist() == [float(v) for v in t] and one["s12"] == s and R[0] == 0.0
    assert got[1][1]["state"] == 0 and wants[1][0]["state"] == 0 and min(wants[1][0]["steps"]) >= 1
    _host_form(ctx, pairs[0], p, f"singular, fix_scale {fix}, host form")


def test_thresholds_from_both_sides(ctx):
    """sim3opt_cases.frozen_pair: no step moves the model, one correspondence has a keypoint two pixels off in one keyframe.  chi2 at
    its chi-square and one unit in the last place below, for either edge; min_corr at the count and one above; min_inliers at the
    count of inliers and one above.  The parameters are a call's: every call holds both pairs (each the other's bystander)"""
    (pr0, row0, both0, n0), (pr1, row1, both1, n1) = OC.frozen_pair(0), OC.frozen_pair(1)
    pairs, rows_off = [pr0, pr1], [row0, row1]
    th = [float(both0[0][n0]), float(both1[1][n1])]
    assert th[0] > 10 * float(both0[1][n0]) and th[1] > 10 * float(both1[0][n1]) and th[0] != th[1]

    def call(tag, **kw):
        wants, _ = _pairs_against_reference(ctx, pairs, 16, dict(OC.FROZEN, **kw), f"thresholds, {tag}", skip=False)
        return [w[0] for w in wants], [w[1] for w in wants]

    for e in (0, 1):
        res, flags = call(f"chi2 at edge {e}'s value", chi2=th[e])
        assert flags[e][rows_off[e]] == 0 and res[e]["n_removed"] == 0 and res[e]["steps"].tolist() == [5, 5]
        res, flags = call(f"chi2 below edge {e}'s value", chi2=float(np.nextafter(th[e], 0.0)))
        assert flags[e][rows_off[e]] == 1 and res[e]["n_removed"] == 1 and res[e]["n_inliers"] == 11 and res[e]["steps"].tolist() == [5, 10]
    below = float(np.nextafter(min(th), 0.0))  # one removal in either pair: 11 left
    res, flags = call("min_corr 12", chi2=below, min_corr=12)
    assert [int(r["state"]) for r in res] == [0, 0] and [int(r["n_removed"]) for r in res] == [1, 1]
    res, flags = call("min_corr 13", chi2=below, min_corr=13)
    assert [int(r["state"]) for r in res] == [1, 1] and [int(r["n_corr"]) for r in res] == [12, 12] and all((f[pr["rows"]] == 0).all() for f, pr in zip(flags, pairs))
    res, flags = call("min_inliers 11", chi2=below, min_inliers=11)
    assert [int(r["state"]) for r in res] == [0, 0] and [int(r["n_inliers"]) for r in res] == [11, 11]
    res, flags = call("min_inliers 12", chi2=below, min_inliers=12)
    assert [int(r["state"]) for r in res] == [3, 3] and [int(r["n_inliers"]) for r in res] == [11, 11] and [r["steps"].tolist() for r in res] == [[5, 0], [5, 0]]
    assert flags[0][row0] == 1 and flags[1][row1] == 1


# ---- marks and mutual -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1025, 16384])
def test_marks_and_mutual(ctx, rows):
    import torch
    tabs = [OC.marks_tables(rows, seed) for seed in range(3)]
    n = len(tabs)
    d = {k: _to_dev(np.stack([t[k] for t in tabs])) for k in ("idx", "idx12", "idx21", "q_skip", "t_skip")}
    d_nq, d_nt = _to_dev(np.array([t["nq"] for t in tabs], np.int32)), _to_dev(np.array([t["nt"] for t in tabs], np.int32))
    for skips in (True, False):
        s1, s2 = (torch.full((n, rows), FILL, dtype=torch.uint8, device=_dev()) for _ in range(2))
        out = torch.full((n, rows), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        summ = torch.full((n, 8), FILL, dtype=torch.uint8, device=_dev())
        _sync()
        ctx.sim3_marks_pairs_device(d["idx"].data_ptr(), d_nq.data_ptr(), d_nt.data_ptr(), n, rows, s1.data_ptr(), s2.data_ptr(),
                                    d_query_skip=d["q_skip"].data_ptr() if skips else 0, d_train_skip=d["t_skip"].data_ptr() if skips else 0)
        ctx.sim3_mutual_pairs_device(d["idx"].data_ptr(), d["idx12"].data_ptr(), d["idx21"].data_ptr(), d_nq.data_ptr(), d_nt.data_ptr(), n, rows,
                                     out.data_ptr(), summ.data_ptr())
        ctx.synchronize()
        g1, g2, gout = s1.cpu().numpy(), s2.cpu().numpy(), out.cpu().numpy()
        gs = summ.cpu().numpy().copy().view(O.MUTUAL_DTYPE).reshape(n)
        for b, t in enumerate(tabs):
            w1, w2 = O.marks(t["idx"], t["q_skip"] if skips else None, t["t_skip"] if skips else None, t["nq"], t["nt"])
            wout, ws = O.mutual(t["idx"], t["idx12"], t["idx21"], t["nq"], t["nt"])
            assert g1[b].tobytes() == w1.tobytes() and g2[b].tobytes() == w2.tobytes(), (rows, b, skips)
            assert gout[b].tobytes() == wout.tobytes() and gs[b].tobytes() == ws.tobytes(), (rows, b)


# ---- the batch form and the one-pair host form ----------------------------------------------------------------------------------------------
def test_batch_form_pairs_form_and_host_form_agree(monkeypatch):
    """test_sim3's batch scene: the matches of ss_match_bow_batch_device and the RANSAC's device results feed the refinement and the
    bookkeeping without leaving the device; the batch form, the pairs form on the same arrays and the host form give the reference's
    answer; a flagged frame voids its pairs"""
    import torch
    import bow_cases as BC
    from send_slam_amd import binding
    from test_bow import Transformed, _set
    from test_guided import Outputs, _extract
    from test_sim3 import BATCH, BATCH_SRC, _lifted_points
    from test_sim3 import Out as RansacOut
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    n = len(BATCH)
    p = dict(chi2=9.210, min_inliers=20, max_iterations=64, fix_scale=False, seed=9)
    # the extracted keypoints of frame 1 are not the projections of the lifted points: a wide threshold and heavy damping keep the steps
    # small and both rounds live
    po = dict(O.UPSTREAM, chi2=1e7, lambda_=1e3)
    kps = [G.features(name)[0] for name in BATCH]

    def pair_of(b, t, xyz, views, idx, start):
        nq, nt = len(kps[b]), len(kps[t]) if t >= 0 else 0
        return dict(view1=views[b], view2=views[max(t, 0)], q_xyz=xyz[b, :nq], q_kp=kps[b], t_xyz=xyz[max(t, 0), :nt], t_kp=kps[max(t, 0)][:nt],
                    idx=idx[b, :nq], q_skip=None, t_skip=None, start=start)

    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        _set(c, BC.vocab("cluster"))
        tr, m = Transformed(n, kcap), Outputs(n, kcap)
        _sync()
        c.bow_transform_batch_device(1, *tr.ptrs())
        c.match_bow_batch_device(binding.guided_params(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=1), *m.ptrs(), train_src=BATCH_SRC)
        c.synchronize()
        idx = m.host()[0]
        xyz, views, good = _lifted_points(kcap, idx[1])
        d_xyz = _to_dev(xyz)
        ransac, out = RansacOut(n, kcap), Out(n, kcap)
        s1, s2 = (torch.full((n, kcap), FILL, dtype=torch.uint8, device=_dev()) for _ in range(2))
        mo = torch.full((n, kcap), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        summ = torch.full((n, 8), FILL, dtype=torch.uint8, device=_dev())
        _sync()
        c.sim3_batch_device(d_xyz.data_ptr(), m.idx.data_ptr(), views, binding.sim3_params(**p), ransac.inlier.data_ptr(), ransac.result.data_ptr(),
                            train_src=BATCH_SRC)
        c.sim3_opt_batch_device(d_xyz.data_ptr(), m.idx.data_ptr(), views, ransac.result.data_ptr(), binding.sim3_opt_params(**po), out.flags.data_ptr(),
                                out.result.data_ptr(), train_src=BATCH_SRC)  # the RANSAC's d_result is d_start
        c.sim3_marks_batch_device(m.idx.data_ptr(), s1.data_ptr(), s2.data_ptr(), train_src=BATCH_SRC)
        c.sim3_mutual_batch_device(m.idx.data_ptr(), m.idx.data_ptr(), m.idx.data_ptr(), mo.data_ptr(), summ.data_ptr(), train_src=BATCH_SRC)
        c.synchronize()
        starts = ransac.host()[1]
        got = out.host()
        wants = []
        for b, t in enumerate(BATCH_SRC):
            pr = pair_of(b, t, xyz, views, idx, starts[b])
            wants.append(_reference(pr, po))
            _check(f"batch form, frame {b} against {t}", got, b, wants[-1], kcap)
            nq, nt = len(pr["q_xyz"]), len(pr["t_xyz"])
            full = np.full(kcap, -1, np.int32)
            full[:nq] = pr["idx"]
            w1, w2 = O.marks(full, None, None, nq, nt)
            assert s1[b].cpu().numpy().tobytes() == w1.tobytes() and s2[b].cpu().numpy().tobytes() == w2.tobytes(), b
            wout, ws = O.mutual(full, full, full, nq, nt)
            assert mo[b].cpu().numpy().tobytes() == wout.tobytes() and summ[b].cpu().numpy().tobytes() == ws.tobytes(), b
        assert starts[1]["state"] == 0 and wants[1][0]["n_corr"] > 20 and wants[1][0]["steps"][0] >= 1 and wants[1][0]["state"] != 1 and wants[0][0]["state"] == 1
        # the pairs form on the same data, and the host form
        pr1 = pair_of(1, 0, xyz, views, idx, starts[1])
        dev = _upload([pr1, pr1], kcap)
        _check("pairs form on the batch's data", _run(c, dev, _starts([pr1, pr1]), 2, kcap, po, skip=False), 1, wants[1], kcap)
        flags, one = c.sim3_opt(pr1["view1"], pr1["q_xyz"], pr1["q_kp"], pr1["view2"], pr1["t_xyz"], pr1["t_kp"], pr1["idx"], pr1["start"],
                                binding.sim3_opt_params(**po))
        _check("host form", (flags[None], np.array([one])), 0, wants[1])
        with pytest.raises(binding.OrbError) as e:
            c.sim3_opt_batch_device(d_xyz.data_ptr(), m.idx.data_ptr(), views, ransac.result.data_ptr(), binding.sim3_opt_params(**po), out.flags.data_ptr(),
                                    out.result.data_ptr(), train_src=[-1, 0, n])
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "train_src[2]" in e.value.message
    # frame 0 flagged: the pairs that touch it carry the status and have no correspondence, whatever their start says
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "0")
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        d_idx, d_start = _to_dev(idx), _to_dev(starts)
        out = Out(n, kcap)
        _sync()
        c.sim3_opt_batch_device(d_xyz.data_ptr(), d_idx.data_ptr(), views, d_start.data_ptr(), binding.sim3_opt_params(**po), out.flags.data_ptr(),
                                out.result.data_ptr(), train_src=BATCH_SRC)
        c.synchronize()
        got = out.host()
        for b in (0, 1):
            void = _reference(pair_of(b, BATCH_SRC[b], xyz, views, idx, starts[b]), po, status=binding.SS_ERR_OVERFLOW)
            assert void[0]["state"] == 1 and void[0]["status"] == binding.SS_ERR_OVERFLOW and (void[1] == 2).all()
            _check(f"flagged, pair {b}", got, b, void, kcap)
        _check("flagged, the pair that does not touch frame 0", got, 2, wants[2], kcap)


def test_without_a_batch_the_batch_forms_return_state():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as c:
        for name, call in (("ss_sim3_opt_batch_device", lambda: c.sim3_opt_batch_device(1, 1, [SC.views()[0]], 1, binding.sim3_opt_params(), 1, 1)),
                           ("ss_sim3_marks_batch_device", lambda: c.sim3_marks_batch_device(1, 1, 1)),
                           ("ss_sim3_mutual_batch_device", lambda: c.sim3_mutual_batch_device(1, 1, 1, 1, 1))):
            with pytest.raises(binding.OrbError) as e:
                call()
            assert e.value.code == binding.SS_ERR_STATE and name in e.value.message


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_from_the_bow_match_to_the_candidate_check(ctx):
    """ss_match_bow_pairs_device -> ss_sim3_pairs_device -> marks -> two ss_match_fuse_pairs_device -> mutual -> ss_sim3_opt_pairs_device ->
    ss_sim3_to_view -> candidate check, every stage on the device arrays the stage before wrote and against the same chain on the
    references; only the 128-byte models a view is built from come to the host"""
    import torch
    import fuse_ref
    from send_slam_amd import binding
    from test_fuse import Outputs as FuseOut
    from test_fuse import _check as _check_fuse
    from test_guided import Outputs as MatchOut
    from test_guided import _check as _check_match
    from test_sim3 import Out as RansacOut
    from test_sim3 import _check as _check_ransac
    pr, rows, ref = OC.chain_scene(), OC.CHAIN_ROWS, OC.chain_reference()
    dev = _upload([pr], rows)
    d = {k: _to_dev(np.ascontiguousarray(pr[k])[None]) for k in ("q_desc", "t_desc", "q_node", "t_node")}
    m, ransac, out = MatchOut(1, rows), RansacOut(1, rows), Out(1, rows)
    s1, s2 = (torch.full((1, rows), FILL, dtype=torch.uint8, device=_dev()) for _ in range(2))
    mo = torch.full((1, rows), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
    summ = torch.full((1, 8), FILL, dtype=torch.uint8, device=_dev())
    f21, f12, fc = FuseOut(1, rows), FuseOut(1, rows), FuseOut(1, rows)
    d_np = _to_dev(np.array([rows], np.int32))
    _sync()
    ctx.match_bow_pairs_device(d["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), d["q_node"].data_ptr(), dev["nq"].data_ptr(), d["t_desc"].data_ptr(),
                               dev["t_kp"].data_ptr(), d["t_node"].data_ptr(), dev["nt"].data_ptr(), 1, rows, binding.guided_params(**SC.CHAIN_BOW), *m.ptrs())
    ctx.sim3_pairs_device(dev["q_xyz"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_xyz"].data_ptr(), dev["t_kp"].data_ptr(),
                          dev["nt"].data_ptr(), m.idx.data_ptr(), 1, rows, dev["views1"], dev["views2"], binding.sim3_params(**SC.CHAIN_SIM3),
                          ransac.inlier.data_ptr(), ransac.result.data_ptr())
    ctx.sim3_marks_pairs_device(m.idx.data_ptr(), dev["nq"].data_ptr(), dev["nt"].data_ptr(), 1, rows, s1.data_ptr(), s2.data_ptr())
    ctx.synchronize()
    _check_match("chain, BoW match", m.host(), 0, ref["bow"])
    rg = ransac.host()
    _check_ransac("chain, RANSAC", rg, 0, ref["sim3"])
    assert s1.cpu().numpy()[0].tobytes() == ref["skip1"].tobytes() and s2.cpu().numpy()[0].tobytes() == ref["skip2"].tobytes()
    cam = binding.Camera(fx=SC.F, fy=SC.F, cx=SC.CX, cy=SC.CY, width=SC.W, height=SC.H)
    v12 = binding.sim3_to_view(cam, rg[1][0], SC.POSE2[0], SC.POSE2[1])[0]
    v21 = binding.sim3_to_view21(cam, rg[1][0], SC.POSE1[0], SC.POSE1[1])[0]
    assert bytes(v12) == ref["v12"].tobytes() and bytes(v21) == ref["v21"].tobytes()
    search = binding.fuse_params(extent_w=SC.W, extent_h=SC.H, **OC.CHAIN_SEARCH)
    # keyframe 2's points in keyframe 1, keyframe 1's points in keyframe 2: each skips what the BoW match holds
    ctx.match_fuse_pairs_device(dev["t_xyz"].data_ptr(), d["t_desc"].data_ptr(), d_np.data_ptr(), 1, rows, d["q_desc"].data_ptr(), dev["q_kp"].data_ptr(),
                                dev["nq"].data_ptr(), 1, rows, [v12], search, *f21.ptrs(), d_point_skip=s2.data_ptr(), d_train_taken=s1.data_ptr())
    ctx.match_fuse_pairs_device(dev["q_xyz"].data_ptr(), d["q_desc"].data_ptr(), d_np.data_ptr(), 1, rows, d["t_desc"].data_ptr(), dev["t_kp"].data_ptr(),
                                dev["nt"].data_ptr(), 1, rows, [v21], search, *f12.ptrs(), d_point_skip=s1.data_ptr(), d_train_taken=s2.data_ptr())
    ctx.sim3_mutual_pairs_device(m.idx.data_ptr(), f12.idx.data_ptr(), f21.idx.data_ptr(), dev["nq"].data_ptr(), dev["nt"].data_ptr(), 1, rows,
                                 mo.data_ptr(), summ.data_ptr())
    ctx.sim3_opt_pairs_device(dev["q_xyz"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_xyz"].data_ptr(), dev["t_kp"].data_ptr(),
                              dev["nt"].data_ptr(), mo.data_ptr(), 1, rows, dev["views1"], dev["views2"], ransac.result.data_ptr(),
                              binding.sim3_opt_params(**OC.CHAIN_OPT), out.flags.data_ptr(), out.result.data_ptr())
    ctx.synchronize()
    _check_fuse("chain, search of keyframe 2's points", f21.host(), 0, ref["search21"])
    _check_fuse("chain, search of keyframe 1's points", f12.host(), 0, ref["search12"])
    assert mo.cpu().numpy()[0].tobytes() == ref["idx"].tobytes() and summ.cpu().numpy().tobytes() == ref["mutual"].tobytes()
    got = out.host()
    _check("chain, refinement", got, 0, ref["opt"], rows)
    assert got[1][0]["state"] == 0 and ref["mutual"]["n_new"] == OC.CHAIN_HIDDEN
    view = binding.sim3_to_view(cam, got[1][0]["model"], SC.POSE2[0], SC.POSE2[1])[0]
    assert bytes(view) == ref["view"].tobytes()
    ctx.match_fuse_pairs_device(dev["t_xyz"].data_ptr(), d["t_desc"].data_ptr(), d_np.data_ptr(), 1, rows, d["q_desc"].data_ptr(), dev["q_kp"].data_ptr(),
                                dev["nq"].data_ptr(), 1, rows, [view], binding.fuse_params(extent_w=SC.W, extent_h=SC.H, **fuse_ref.CANDIDATE_CHECK), *fc.ptrs())
    ctx.synchronize()
    fg = fc.host()
    _check_fuse("chain, candidate check", fg, 0, ref["check"])
    assert int((fg[0][0] >= 0).sum()) >= int((ref["check_ransac"][0] >= 0).sum()) > 0  # the refined model finds at least the RANSAC model's matches


# ---- contract ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    pairs = [OC.case_pair(0)]
    dev, st = _upload(pairs, ROWS), _starts(pairs)
    out = Out(1, ROWS)
    good = dict(d_query_xyz=dev["q_xyz"].data_ptr(), d_query_kp=dev["q_kp"].data_ptr(), d_n_query=dev["nq"].data_ptr(), d_train_xyz=dev["t_xyz"].data_ptr(),
                d_train_kp=dev["t_kp"].data_ptr(), d_n_train=dev["nt"].data_ptr(), d_idx=dev["idx"].data_ptr(), n_pairs=1, rows=ROWS, views1=dev["views1"],
                views2=dev["views2"], d_start=st.data_ptr(), params=binding.sim3_opt_params(), d_flags=out.flags.data_ptr(), d_result=out.result.data_ptr())
    nan, inf, P_ = float("nan"), float("inf"), binding.sim3_opt_params
    bad = [(dict(rows=binding.SS_GUIDED_MAX_ROWS + 1), "exceeds SS_GUIDED_MAX_ROWS (16384)"), (dict(rows=0), "bad pair or row count"),
           (dict(params=P_(chi2=0.0)), "chi2 must be finite and > 0"), (dict(params=P_(chi2=nan)), "chi2 must be finite and > 0"),
           (dict(params=P_(chi2=inf)), "chi2 must be finite and > 0"), (dict(params=P_(lambda_=-1.0)), "lambda must be finite and >= 0"),
           (dict(params=P_(lambda_=inf)), "lambda must be finite and >= 0"), (dict(params=P_(step_eps=nan)), "step_eps must be finite and >= 0"),
           (dict(params=P_(iterations0=0)), "iterations0 must be 1 .. 32"), (dict(params=P_(iterations0=33)), "iterations0 must be 1 .. 32"),
           (dict(params=P_(iterations_more=0)), "iterations_more must be 1 .. 32"), (dict(params=P_(iterations_same=33)), "iterations_same must be 1 .. 32"),
           (dict(params=P_(min_corr=2)), "min_corr must be >= 3"), (dict(params=P_(min_inliers=-1)), "min_inliers must be >= 0"),
           (dict(params=P_(reserved=(0, 0, 1, 0))), "reserved fields must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.sim3_opt_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message and e.value.message.startswith("sim3 refinement: "), (kw, e.value.message)
    ctx.sim3_opt_pairs_device(**dict(good, n_pairs=0, views1=dev["views1"][:0], views2=dev["views2"][:0]))  # nothing is launched or written
    ctx.synchronize()
    assert (out.result.cpu().numpy() == FILL).all() and (out.flags.cpu().numpy() == FILL).all()
    a = dict(d_idx=dev["idx"].data_ptr(), d_n_query=dev["nq"].data_ptr(), d_n_train=dev["nt"].data_ptr(), n_pairs=1, rows=ROWS)
    marks = dict(a, d_skip1_out=out.flags.data_ptr(), d_skip2_out=out.flags.data_ptr())
    mutual = dict(a, d_idx12=dev["idx"].data_ptr(), d_idx21=dev["idx"].data_ptr(), d_idx_out=dev["idx"].data_ptr(), d_summary=out.result.data_ptr())
    for call, args, word in ((ctx.sim3_marks_pairs_device, marks, "sim3 marks: "), (ctx.sim3_mutual_pairs_device, mutual, "sim3 mutual: ")):
        refusals = [(dict(rows=binding.SS_GUIDED_MAX_ROWS + 1), "exceeds SS_GUIDED_MAX_ROWS"), (dict(rows=0), "bad pair or row count")]
        refusals += [({k: 0}, "NULL buffer") for k in args if k.startswith("d_")]
        for kw, msg in refusals:
            with pytest.raises(binding.OrbError) as e:
                call(**dict(args, **kw))
            assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message and e.value.message.startswith(word), (kw, e.value.message)
    pr = pairs[0]
    with pytest.raises(binding.OrbError) as e:
        ctx.sim3_opt(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], pr["start"], P_(chi2=nan))
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "chi2 must be finite and > 0" in e.value.message
    # the context is usable after every refusal; the host form with skip bytes and without rows
    _check("after the refusals", _run(ctx, dev, st, 1, ROWS, OC.CASES[0]["params"]), 0, OC.reference(0)[:2])
    sk = OC.with_skips(pr, 4)
    flags, res = ctx.sim3_opt(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], pr["start"], P_(), sk["q_skip"], sk["t_skip"])
    _check("host form with skip bytes", (flags[None], np.array([res])), 0, _reference(sk, O.UPSTREAM))
    flags, res = ctx.sim3_opt(pr["view1"], pr["q_xyz"][:0], pr["q_kp"][:0], pr["view2"], pr["t_xyz"][:0], pr["t_kp"][:0], pr["idx"][:0], pr["start"], P_())
    assert len(flags) == 0 and (res["state"], res["n_corr"]) == (1, 0)


def test_stages_and_their_byte_figures(ctx):
    pairs = [OC.case_pair(0), OC.case_pair(1)]
    dev, st = _upload(pairs, ROWS), _starts(pairs)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        _run(ctx, dev, st, 2, ROWS, O.UPSTREAM, skip=True)
        ctx.sim3_marks_pairs_device(dev["idx"].data_ptr(), dev["nq"].data_ptr(), dev["nt"].data_ptr(), 2, ROWS, dev["q_skip"].data_ptr(), dev["t_skip"].data_ptr())
        ctx.synchronize()
        stats = {s["name"]: s for s in ctx.stats() if s["name"].startswith("sim3opt_")}
    finally:
        ctx.profile(False)
    n, nr, passes = 2, 2 * ROWS, 5 + 10 + 2
    want = {"sim3opt_gather": nr * (4 + 4 + 2 * 32 + 2 * 24 + 1 + 1 + 48) + n * (128 + 4), "sim3opt_solve": nr * (48 * passes + 4 + 1) + n * (2 * P.VIEW_DTYPE.itemsize + 128 + 272),
            "sim3opt_marks": nr * (4 + 2 + 4 + 1) + n * 8}
    assert list(stats) == list(want)
    for name, b in want.items():
        assert stats[name]["launches"] == 1 and stats[name]["algorithmic_bytes"] == b and stats[name]["total_ms"] > 0, (name, stats[name])
