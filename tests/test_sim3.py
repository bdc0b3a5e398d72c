"""GPU parity of the Sim3 RANSAC (ss_sim3_pairs_device, ss_sim3_batch_device, ss_sim3) against tests/sim3_ref.py through the C ABI:
bit for bit, no tolerance -- every byte of every ss_sim3_result and every inlier flag.  Every output starts prefilled with a pattern
no result has; flags past the query rows must be 0.  tests/test_sim3_ref.py asserts on the reference that the shared cases are live."""
import numpy as np
import pytest

import guided_cases as G
import proj_cases as PC
import proj_ref as P
import sim3_cases as SC
import sim3_ref as S

pytestmark = pytest.mark.gpu

HYP_BLOCK = 32    # SSK_SIM3_HYP_BLOCK: the hypotheses one workgroup of k_sim3_count takes
COUNT_ROWS = 256  # SSK_SIM3_COUNT_ROWS: its correspondences
CHUNK = 1024      # SSK_SIM3_CHUNK: the rows k_sim3_gather numbers at a time


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
    """device flags [n, rows] and results [n], prefilled with a pattern no result has"""

    def __init__(self, n, rows):
        import torch
        self.n, self.rows = n, rows
        self.inlier = torch.full((n, rows), 0x5A, dtype=torch.uint8, device=_dev())
        self.result = torch.full((n, 128), 0x5A, dtype=torch.uint8, device=_dev())
        _sync()

    def host(self):
        from send_slam_amd import binding
        return self.inlier.cpu().numpy().copy(), self.result.cpu().numpy().copy().view(binding.SIM3_RESULT_DTYPE).reshape(self.n)


def _told(pr):
    """the counts the device is told, where they are not the lengths of the arrays"""
    return pr.get("n_query", len(pr["q_xyz"])), pr.get("n_train", len(pr["t_xyz"]))


def _reference(pr, params, pair, scale=None, status=0):
    """sim3_ref on what the device may read of pr: the rows under the counts it is told"""
    nq, nt = _told(pr)
    cut = dict(pr, q_xyz=pr["q_xyz"][:nq], q_kp=pr["q_kp"][:nq], idx=pr["idx"][:nq], t_xyz=pr["t_xyz"][:nt], t_kp=pr["t_kp"][:nt],
               q_skip=None if pr["q_skip"] is None else pr["q_skip"][:nq], t_skip=None if pr["t_skip"] is None else pr["t_skip"][:nt])
    return SC.solve_pair(cut, params, pair, scale, status)


def _upload(pairs, rows):
    from send_slam_amd import binding
    n = len(pairs)
    host = {"q_xyz": np.zeros((n, rows), binding.MAP_POINT_DTYPE), "t_xyz": np.zeros((n, rows), binding.MAP_POINT_DTYPE),
            "q_kp": np.zeros((n, rows), binding.KP_DTYPE), "t_kp": np.zeros((n, rows), binding.KP_DTYPE), "q_skip": np.zeros((n, rows), np.uint8),
            "t_skip": np.zeros((n, rows), np.uint8), "idx": np.full((n, rows), -1, np.int32), "nq": np.zeros(n, np.int32), "nt": np.zeros(n, np.int32)}
    for b, pr in enumerate(pairs):
        kq, kt = len(pr["q_xyz"]), len(pr["t_xyz"])
        host["nq"][b], host["nt"][b] = _told(pr)
        host["q_xyz"][b, :kq], host["q_kp"][b, :kq], host["idx"][b, :kq] = pr["q_xyz"], pr["q_kp"], pr["idx"]
        host["t_xyz"][b, :kt], host["t_kp"][b, :kt] = pr["t_xyz"], pr["t_kp"]
        if pr["q_skip"] is not None:
            host["q_skip"][b, :kq] = pr["q_skip"]
        if pr["t_skip"] is not None:
            host["t_skip"][b, :kt] = pr["t_skip"]
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["views1"] = np.concatenate([np.asarray(pr["view1"]).reshape(1) for pr in pairs]) if n else np.zeros(0, P.VIEW_DTYPE)
    dev["views2"] = np.concatenate([np.asarray(pr["view2"]).reshape(1) for pr in pairs]) if n else np.zeros(0, P.VIEW_DTYPE)
    _sync()
    return dev


def _params(binding, p):
    return binding.sim3_params(**p)


def _run(ctx, dev, n, rows, params, skip=True):
    from send_slam_amd import binding
    out = Out(n, rows)
    ctx.sim3_pairs_device(dev["q_xyz"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_xyz"].data_ptr(), dev["t_kp"].data_ptr(),
                          dev["nt"].data_ptr(), dev["idx"].data_ptr(), n, rows, dev["views1"], dev["views2"], _params(binding, params),
                          out.inlier.data_ptr(), out.result.data_ptr(), d_query_skip=dev["q_skip"].data_ptr() if skip else 0,
                          d_train_skip=dev["t_skip"].data_ptr() if skip else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, b, want):
    flags, results = got
    wres, wflags = want[0], want[1]
    for name in S.RESULT_DTYPE.names:
        assert results[b][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[b][name]} != {wres[name]}"
    nq = len(wflags)
    bad = np.flatnonzero(flags[b][:nq] != wflags)
    assert len(bad) == 0, f"{tag}: flags differ at query rows {bad[:8]}: {flags[b][:nq][bad[:8]]} != {wflags[bad[:8]]}"
    assert not flags[b][nq:].any(), f"{tag}: flags past the query rows are not 0"


def _pairs_against_reference(ctx, pairs, rows, params, tag, skip=True):
    dev = _upload(pairs, rows)
    got = _run(ctx, dev, len(pairs), rows, params, skip)
    wants = [_reference(pr, params, b) for b, pr in enumerate(pairs)]
    for b, w in enumerate(wants):
        _check(f"{tag}, pair {b}", got, b, w)
    return wants


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=2) as c:
        yield c


@pytest.mark.parametrize("k", range(len(SC.CASES)), ids=SC.CASE_NAMES)
def test_cases_three_pairs_per_call(ctx, k):
    """case k with two other cases behind it in one call under case k's parameters: three pairs of different N and states, the pair
    number in the draw stream"""
    n = len(SC.CASES)
    members = [k, (k + 3) % n, (k + 5) % n]
    pairs = [SC.case_pair(j) for j in members]
    wants = _pairs_against_reference(ctx, pairs, SC.ROWS, SC.CASES[k]["params"], SC.CASES[k]["name"], skip=False)
    assert wants[0][0].tobytes() == SC.reference(k, 0)[0].tobytes() and wants[0][0]["state"] == SC.CASES[k]["expect_state"]
    assert len({int(w[0]["n_corr"]) for w in wants}) == 3


def test_every_state_and_the_pair_number_in_one_call(ctx):
    """the same pair three times in one call: the pair number alone changes the draws, so the winners differ"""
    pairs = [SC.case_pair(0)] * 3
    p = dict(SC.CASES[0]["params"], seed=1)
    wants = _pairs_against_reference(ctx, pairs, SC.ROWS, p, "one pair three times")
    assert len({int(w[0]["iteration"]) for w in wants}) > 1 and all(w[0]["state"] == 0 for w in wants)


def test_compaction_with_a_wave_that_keeps_nothing(ctx):
    """CHUNK + 65 rows, every one a correspondence but for the 64 of one wave (skip bytes): a wave without a kept row ahead of waves with
    some, and the chunk boundary inside a run of kept rows"""
    rows = CHUNK + 65
    pr = dict(SC.make_pair(45, rows, rows // 3, rows, rows))
    pr["q_skip"] = np.zeros(rows, np.uint8)
    pr["q_skip"][192:256] = 1
    p = dict(chi2=9.210, min_inliers=20, max_iterations=48, fix_scale=False, seed=7)
    res, flags, _ = _pairs_against_reference(ctx, [pr], rows, p, "a wave that keeps nothing")[0]
    assert res["n_corr"] == rows - 64 and res["state"] == 0
    assert not flags[192:256].any() and flags[:192].any() and flags[256:CHUNK].any() and flags[CHUNK:].any()


@pytest.mark.parametrize("rows", [128, CHUNK + 76])
def test_compaction(ctx, rows):
    """matches and skip bytes scattered so that the kept rows straddle the wave (and, in the larger shape, the chunk) boundaries;
    n_query and n_train under the rows; idx entries at and past n_train and below -1; the flags land on the query rows"""
    rng = np.random.Generator(np.random.PCG64(rows))
    edges = [e + d for e in ((64, CHUNK) if rows > CHUNK else (64,)) for d in (-1, 0, 1)]
    pairs = []
    for b in range(2):
        pr = dict(SC.make_pair(40 + b + rows, rows, rows // 3, rows, rows))  # every row a correspondence, then a quarter of them unmatched
        pr["idx"] = pr["idx"].copy()
        inner = np.setdiff1d(np.arange(rows), edges)
        drop = rng.choice(inner, rows // 4, replace=False)
        pr["idx"][drop] = -1
        kept = np.setdiff1d(inner, drop)
        pr["rows"], pr["inlier_rows"] = np.setdiff1d(pr["rows"], drop), np.setdiff1d(pr["inlier_rows"], drop)
        pr["q_skip"], pr["t_skip"] = np.zeros(rows, np.uint8), np.zeros(rows, np.uint8)
        pr["q_skip"][rng.choice(kept, 5, replace=False)] = rng.integers(1, 256, 5)
        pr["q_skip"][drop[:3]] = 1
        pr["t_skip"][pr["idx"][rng.choice(kept, 5, replace=False)]] = 255
        nq, nt = rows - 9, rows - 14
        pr["n_query"], pr["n_train"] = nq, nt
        pr["idx"][drop[3:7]] = [nt, nt + 5, 1 << 30, -7]
        pairs.append(pr)
    p = dict(chi2=9.210, min_inliers=20, max_iterations=48, fix_scale=False, seed=7)
    wants = _pairs_against_reference(ctx, pairs, rows, p, f"compaction at {rows} rows")
    for pr, (res, flags, _) in zip(pairs, wants):
        nq, nt = _told(pr)
        assert res["state"] == 0 and 20 < res["n_corr"] < len(pr["rows"])  # the counts, flags and bad entries dropped some
        assert (pr["idx"][:nq] >= nt).sum() >= 2 and {63, 64, 65} <= set(np.flatnonzero(pr["idx"][:nq] >= 0).tolist())
        hit = np.flatnonzero(flags)
        assert set(hit.tolist()) <= set(pr["inlier_rows"].tolist()) and len(hit) == res["n_inliers"]
        assert hit.max() > res["n_corr"]  # a flag sits on a query row, not on a correspondence number
    # without the skip arrays the flagged rows are correspondences again
    dev = _upload(pairs, rows)
    got = _run(ctx, dev, 2, rows, p, skip=False)
    for b, pr in enumerate(pairs):
        w = _reference(dict(pr, q_skip=None, t_skip=None), p, b)
        _check(f"compaction at {rows} rows without skip bytes, pair {b}", got, b, w)
        assert w[0]["n_corr"] > wants[b][0]["n_corr"]


BLOCK_PAIR = dict(rng_seed=31, n=60, n_out=54, nq=64, nt=64)  # 6 inliers of 60: a winner needs all three draws among them
BLOCK_SEEDS = {"t = 0": (2348, 33, 0), "the last hypothesis of the first block": (42, 33, 31), "the only hypothesis of the last block": (1001, 33, 32),
               "the last block of SS_SIM3_MAX_ITERATIONS": (241, 1024, 993)}


@pytest.mark.parametrize("max_iterations", [1, HYP_BLOCK - 1, HYP_BLOCK, HYP_BLOCK + 1, 1024])
def test_hypothesis_blocking_counts(ctx, max_iterations):
    """max_iterations at 1, one below, at and one above the block of hypotheses of k_sim3_count, and at SS_SIM3_MAX_ITERATIONS: every
    count enters the result through best_inliers or the winner"""
    pairs = [SC.make_pair(**BLOCK_PAIR), SC.case_pair(0)]
    for seed in (42, 1001):
        p = dict(chi2=9.210, min_inliers=5, max_iterations=max_iterations, fix_scale=False, seed=seed)
        _pairs_against_reference(ctx, pairs, SC.ROWS, p, f"{max_iterations} iterations, seed {seed}")
        if max_iterations == 1024:
            break


@pytest.mark.parametrize("where", list(BLOCK_SEEDS))
def test_hypothesis_blocking_winner(ctx, where):
    seed, max_iterations, t = BLOCK_SEEDS[where]
    pairs = [SC.make_pair(**BLOCK_PAIR)]
    p = dict(chi2=9.210, min_inliers=5, max_iterations=max_iterations, fix_scale=False, seed=seed)
    (res, flags, counts), = _pairs_against_reference(ctx, pairs, SC.ROWS, p, where)
    assert res["state"] == 0 and res["iteration"] == t and t // HYP_BLOCK == (0 if t < HYP_BLOCK else (max_iterations - 1) // HYP_BLOCK)
    assert (counts[:t] <= 5).all() and res["n_inliers"] == 6


def test_correspondence_blocking(ctx):
    """N one below, at and one above the correspondences of one workgroup of k_sim3_count, and a pair without any"""
    rows = COUNT_ROWS + 44
    pairs = [SC.make_pair(50 + n, n, n // 4, rows, rows) for n in (COUNT_ROWS - 1, COUNT_ROWS, COUNT_ROWS + 1)]
    empty = dict(SC.make_pair(54, 30, 0, rows, rows))
    empty["idx"] = np.full(rows, -1, np.int32)
    pairs.append(empty)
    p = dict(chi2=9.210, min_inliers=100, max_iterations=40, fix_scale=False, seed=3)
    wants = _pairs_against_reference(ctx, pairs, rows, p, "correspondence blocking")
    assert [int(w[0]["n_corr"]) for w in wants] == [COUNT_ROWS - 1, COUNT_ROWS, COUNT_ROWS + 1, 0]
    assert [int(w[0]["state"]) for w in wants] == [0, 0, 0, 1]
    # the last correspondence of each is an inlier of the winner or an outlier the winner rejects: both kinds occur at the block edge
    p0 = dict(p, min_inliers=0)
    wants = _pairs_against_reference(ctx, pairs, rows, p0, "correspondence blocking, min_inliers 0")
    assert wants[3][0]["state"] == 1 and wants[3][0]["n_corr"] == 0  # N = 0 < 3


def test_limits(ctx):
    """two pairs of SS_GUIDED_MAX_ROWS rows, every row a correspondence, 300 iterations"""
    from send_slam_amd import binding
    rows = binding.SS_GUIDED_MAX_ROWS
    pairs = [SC.make_pair(60 + b, rows, rows // 2, scatter=False) for b in range(2)]
    p = dict(chi2=9.210, min_inliers=rows // 2 - 200, max_iterations=300, fix_scale=False, seed=11)
    wants = _pairs_against_reference(ctx, pairs, rows, p, "full capacity")
    for res, flags, counts in wants:
        assert res["n_corr"] == rows and res["state"] == 0 and res["n_inliers"] > rows // 2 - 200


def test_degenerate_and_fix_scale(ctx):
    """all correspondences one point: without fix_scale every model is the zero model, state 2, best_inliers 0; a pair of scale 1 next
    to it, solved with and without fix_scale"""
    k_deg, k_fix = SC.CASE_NAMES.index("degenerate: every correspondence is one point"), SC.CASE_NAMES.index("fix_scale on a scene of scale 1")
    pairs = [SC.case_pair(k_deg), SC.case_pair(k_fix)]
    p = dict(chi2=9.210, min_inliers=5, max_iterations=64, fix_scale=False, seed=2)
    wants = _pairs_against_reference(ctx, pairs, SC.ROWS, p, "degenerate, free scale")
    assert (wants[0][0]["state"], wants[0][0]["best_inliers"], wants[0][0]["n_corr"]) == (2, 0, 30)
    assert wants[1][0]["state"] == 0
    # with fix_scale the same triple gives a finite model, the translation between the two points, and every correspondence fits it
    wants = _pairs_against_reference(ctx, pairs, SC.ROWS, dict(p, fix_scale=True), "degenerate, fix_scale")
    assert (wants[0][0]["state"], wants[0][0]["n_inliers"], wants[0][0]["iteration"]) == (0, 30, 0)
    assert wants[1][0]["state"] == 0 and wants[1][0]["s12"] == 1.0


@pytest.mark.parametrize("name", ["one_level", "sixteen_levels"])
def test_other_pyramid_tables(name):
    """the octave test and the thresholds read the context's table: one level (every octave but 0 is outside) and SS_MAX_LEVELS"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    pr = SC.make_pair(70, 50, 10, 64, 64, octaves=(0, 1, n_levels - 1, n_levels))
    p = dict(chi2=9.210, min_inliers=3, max_iterations=32, fix_scale=False, seed=5)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        dev = _upload([pr], 64)
        got = _run(c, dev, 1, 64, p)
    want = _reference(pr, p, 0, scale=sc)
    _check(name, got, 0, want)
    assert 3 <= want[0]["n_corr"] < 50 and want[0]["state"] == 0


# ---- odd cameras, per pair and per side ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_inliers", SC.CAMERA_MIN_INLIERS)
def test_three_camera_pairs_per_call(ctx, min_inliers):
    """one call whose pairs are seen by the cameras (P, Q), (Q, P) and (square, P): fx != fy, principal points off the centre, the
    two sides of a pair different.  The query points carry noise, so the counts depend on the views (tests/test_sim3_ref.py shows
    that exchanging fx and fy, the sides, or the pairs' views changes the bytes compared here).  The pairs form and the host form"""
    from send_slam_amd import binding
    pairs, p = SC.camera_pairs(), SC.camera_params(min_inliers)
    wants = _pairs_against_reference(ctx, pairs, SC.ROWS, p, f"cameras, min_inliers {min_inliers}", skip=False)
    for b, w in enumerate(SC.camera_reference(min_inliers)):
        assert wants[b][0].tobytes() == w[0].tobytes() and w[0]["state"] == 0 and min_inliers < w[0]["n_inliers"] < w[0]["n_corr"] == 60
    for b, pr in enumerate(pairs):  # the host form is pair 0 of its own call
        flags, one = ctx.sim3(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], _params(binding, p))
        _check(f"cameras, host form of pair {b}", (flags[None], np.array([one])), 0, _reference(pr, p, 0))


def test_batch_form_under_a_camera_per_frame():
    """ss_sim3_batch_device with views[b] and views[train_src[b]] different for every frame: frames 1 and 2 train on frame 0, the
    frames are seen by P, Q and the square camera"""
    from send_slam_amd import binding
    from test_guided import _extract
    kps, xyz, idx, views = SC.camera_batch()
    n = len(SC.CAMERA_BATCH)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, SC.CAMERA_BATCH)
        assert kcap >= xyz.shape[1]
        pad = lambda a, fill: np.concatenate([a, np.full((n, kcap - a.shape[1]), fill, a.dtype)], axis=1)  # noqa: E731
        d_xyz, d_idx = _to_dev(pad(xyz, 0)), _to_dev(pad(idx, -1))
        _sync()
        for m in SC.CAMERA_MIN_INLIERS:
            p = SC.camera_params(m)
            out = Out(n, kcap)
            c.sim3_batch_device(d_xyz.data_ptr(), d_idx.data_ptr(), views, _params(binding, p), out.inlier.data_ptr(), out.result.data_ptr(),
                                train_src=SC.CAMERA_BATCH_SRC)
            c.synchronize()
            got = out.host()
            for b in range(n):
                w = _reference(SC.batch_pair(b), p, b)
                _check(f"cameras, batch form, min_inliers {m}, frame {b} against {SC.CAMERA_BATCH_SRC[b]}", got, b, w)
                assert (w[0]["state"], w[0]["n_corr"]) == ((1, 0) if b == 0 else (0, 60))


# ---- the batch form and the one-pair host form -----------------------------------------------------------------------------------------
BATCH = ["synth_t0", "synth_t1", "flat"]
BATCH_SRC = [-1, 0, 1]


def _lifted_points(kcap, matches):
    """map points for the rows of frames 0 (keyframe 2 of pair 1) and 1 (keyframe 1): frame 0's keypoints lifted to a depth of 3 - 9
    in its camera, frame 1's matched rows the same points under the scene's Sim3; a fifth of the matches keep a wrong point"""
    rng = np.random.Generator(np.random.PCG64(0xBA7C))
    k0, k1 = G.features(BATCH[0])[0], G.features(BATCH[1])[0]
    v1, v2 = SC.views()
    z = rng.uniform(3.0, 9.0, len(k0))
    x2 = np.stack([(k0["x"] - SC.CX) / SC.F * z, (k0["y"] - SC.CY) / SC.F * z, z], axis=1)
    w2 = (x2 - np.asarray(SC.POSE2[1])) @ SC.POSE2[0]
    x1 = rng.uniform(-3, 3, (len(k1), 3)) + [0, 0, 6.0]
    good = []
    for i, j in enumerate(matches[:len(k1)]):
        if j >= 0 and rng.random() > 0.2:
            x1[i] = SC.S_TRUE * (SC.rodrigues(SC.AXIS, SC.ANGLE) @ x2[j]) + SC.T_TRUE
            good.append(i)
    w1 = (x1 - np.asarray(SC.POSE1[1])) @ SC.POSE1[0]
    xyz = np.zeros((len(BATCH), kcap), P.MAP_POINT_DTYPE)
    xyz[0, :len(k0)], xyz[1, :len(k1)] = SC._points(w2), SC._points(w1)
    return xyz, [v2, v1, v1], good


def test_batch_form_pairs_form_and_host_form_agree(monkeypatch):
    """two 320 x 240 frames of tests/golden and a frame without keypoints, the matches of ss_match_bow_batch_device, synthetic map
    points: the batch form, the pairs form on the same arrays and the host form give the reference's answer; a flagged frame voids
    its pairs"""
    import bow_cases as BC
    from send_slam_amd import binding
    from test_bow import Transformed, _set
    from test_guided import Outputs, _extract
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    n = len(BATCH)
    p = dict(chi2=9.210, min_inliers=20, max_iterations=64, fix_scale=False, seed=9)
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
        _sync()
        out = Out(n, kcap)
        c.sim3_batch_device(d_xyz.data_ptr(), m.idx.data_ptr(), views, _params(binding, p), out.inlier.data_ptr(), out.result.data_ptr(), train_src=BATCH_SRC)
        c.synchronize()
        got = out.host()
        kps = [G.features(name)[0] for name in BATCH]
        wants = []
        for b, t in enumerate(BATCH_SRC):
            nq, nt = len(kps[b]), len(kps[t]) if t >= 0 else 0
            pr = dict(view1=views[b], view2=views[max(t, 0)], q_xyz=xyz[b, :nq], q_kp=kps[b], t_xyz=xyz[max(t, 0), :nt], t_kp=kps[max(t, 0)][:nt],
                      idx=idx[b, :nq], q_skip=None, t_skip=None)
            wants.append(_reference(pr, p, b))
            _check(f"batch form, frame {b} against {t}", got, b, wants[-1])
        res = wants[1][0]
        assert res["state"] == 0 and res["n_inliers"] >= len(good) - 2 > 20 and wants[0][0]["state"] == 1 and wants[2][0]["n_corr"] == 0
        assert abs(float(res["s12"]) - SC.S_TRUE) < 1e-3
        # the pairs form on the same data, as pair 1 of a call of two so that the pair number is the batch form's
        pr1 = dict(view1=views[1], view2=views[0], q_xyz=xyz[1, :len(kps[1])], q_kp=kps[1], t_xyz=xyz[0, :len(kps[0])], t_kp=kps[0],
                   idx=idx[1, :len(kps[1])], q_skip=None, t_skip=None)
        dev = _upload([pr1, pr1], kcap)
        _check("pairs form on the batch's data", _run(c, dev, 2, kcap, p, skip=False), 1, wants[1])
        # the host form is pair 0 of its own call
        flags, one = c.sim3(views[1], xyz[1, :len(kps[1])], kps[1], views[0], xyz[0, :len(kps[0])], kps[0], idx[1, :len(kps[1])], _params(binding, p))
        w = _reference(dict(view1=views[1], view2=views[0], q_xyz=xyz[1, :len(kps[1])], q_kp=kps[1], t_xyz=xyz[0, :len(kps[0])], t_kp=kps[0],
                            idx=idx[1, :len(kps[1])], q_skip=None, t_skip=None), p, 0)
        _check("host form", (flags[None], np.array([one])), 0, w)
        assert w[0]["state"] == 0
        for bad in (-2, n):
            with pytest.raises(binding.OrbError) as e:
                c.sim3_batch_device(d_xyz.data_ptr(), m.idx.data_ptr(), views, _params(binding, p), out.inlier.data_ptr(), out.result.data_ptr(),
                                    train_src=[-1, 0, bad])
            assert e.value.code == binding.SS_ERR_INVALID_ARG and "train_src[2]" in e.value.message
    # frame 0 flagged: the pair that trains on it carries the status and has no correspondence
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "0")
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        d_idx = _to_dev(idx)
        _sync()
        out = Out(n, kcap)
        c.sim3_batch_device(d_xyz.data_ptr(), d_idx.data_ptr(), views, _params(binding, p), out.inlier.data_ptr(), out.result.data_ptr(), train_src=BATCH_SRC)
        c.synchronize()
        got = out.host()
        for b in (0, 1):
            void = S.solve(views[b], xyz[b, :len(kps[b])], kps[b], None, views[0], xyz[0, :0], kps[0][:0], None, idx[b, :len(kps[b])], PC.scale(),
                           status=binding.SS_ERR_OVERFLOW, pair=b, **p)
            _check(f"flagged, pair {b}", got, b, void)
        _check("flagged, the pair that does not touch frame 0", got, 2, wants[2])


def test_without_a_batch_the_batch_form_returns_state():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as c:
        with pytest.raises(binding.OrbError) as e:
            c.sim3_batch_device(1, 1, [SC.views()[0]], binding.sim3_params(), 1, 1)
        assert e.value.code == binding.SS_ERR_STATE and "ss_sim3_batch_device" in e.value.message


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_bow_match_sim3_view_projection_search(ctx):
    """ss_match_bow_pairs_device -> ss_sim3_pairs_device on the device's own idx -> ss_sim3_to_view / ss_fuse_view_sim3 ->
    ss_match_fuse_pairs_device with the candidate check's parameters: every stage equals the same chain on the references, and the
    projection search finds the map point of every RANSAC inlier (asserted on the reference in tests/test_sim3_ref.py)"""
    import fuse_ref
    from send_slam_amd import binding
    from test_fuse import Outputs as FuseOut
    from test_fuse import _check as _check_fuse
    from test_guided import Outputs as MatchOut
    from test_guided import _check as _check_match
    pr, rows = SC.chain_scene(), SC.CHAIN_ROWS
    bow, sim3, view, fuse = SC.chain_reference()
    dev = _upload([pr], rows)
    d = {k: _to_dev(np.ascontiguousarray(pr[k])[None]) for k in ("q_desc", "t_desc", "q_node", "t_node")}
    m, out = MatchOut(1, rows), Out(1, rows)
    _sync()
    ctx.match_bow_pairs_device(d["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), d["q_node"].data_ptr(), dev["nq"].data_ptr(), d["t_desc"].data_ptr(),
                               dev["t_kp"].data_ptr(), d["t_node"].data_ptr(), dev["nt"].data_ptr(), 1, rows, binding.guided_params(**SC.CHAIN_BOW), *m.ptrs())
    ctx.sim3_pairs_device(dev["q_xyz"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_xyz"].data_ptr(), dev["t_kp"].data_ptr(),
                          dev["nt"].data_ptr(), m.idx.data_ptr(), 1, rows, dev["views1"], dev["views2"], _params(binding, SC.CHAIN_SIM3),
                          out.inlier.data_ptr(), out.result.data_ptr())  # the match's idx, never on the host
    ctx.synchronize()
    _check_match("chain, BoW match", m.host(), 0, bow)
    got = out.host()
    _check("chain, Sim3", got, 0, sim3)
    cam = binding.Camera(fx=SC.F, fy=SC.F, cx=SC.CX, cy=SC.CY, width=SC.W, height=SC.H)
    v, srcw, t = binding.sim3_to_view(cam, got[1][0], SC.POSE2[0], SC.POSE2[1])
    assert bytes(v) == view.tobytes()
    fo = FuseOut(1, rows)
    d_np = _to_dev(np.array([rows], np.int32))
    _sync()
    # the candidate's map points (keyframe 2's) searched in the current keyframe (keyframe 1) under Scw
    ctx.match_fuse_pairs_device(dev["t_xyz"].data_ptr(), d["t_desc"].data_ptr(), d_np.data_ptr(), 1, rows, d["q_desc"].data_ptr(), dev["q_kp"].data_ptr(),
                                dev["nq"].data_ptr(), 1, rows, [v], binding.fuse_params(extent_w=SC.W, extent_h=SC.H, **fuse_ref.CANDIDATE_CHECK), *fo.ptrs())
    ctx.synchronize()
    fg = fo.host()
    _check_fuse("chain, projection search", fg, 0, fuse)
    for i in np.flatnonzero(got[0][0]):
        assert fg[0][0][pr["idx"][i]] == i


# ---- contract ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    pairs = [SC.case_pair(0)]
    dev = _upload(pairs, SC.ROWS)
    out = Out(1, SC.ROWS)
    good = dict(d_query_xyz=dev["q_xyz"].data_ptr(), d_query_kp=dev["q_kp"].data_ptr(), d_n_query=dev["nq"].data_ptr(), d_train_xyz=dev["t_xyz"].data_ptr(),
                d_train_kp=dev["t_kp"].data_ptr(), d_n_train=dev["nt"].data_ptr(), d_idx=dev["idx"].data_ptr(), n_pairs=1, rows=SC.ROWS, views1=dev["views1"],
                views2=dev["views2"], params=binding.sim3_params(), d_inlier=out.inlier.data_ptr(), d_result=out.result.data_ptr())
    nan, inf = float("nan"), float("inf")
    bad = [(dict(rows=binding.SS_GUIDED_MAX_ROWS + 1), "exceeds SS_GUIDED_MAX_ROWS (16384)"), (dict(rows=0), "bad pair or row count"),
           (dict(params=binding.sim3_params(max_iterations=0)), "max_iterations must be 1 .. SS_SIM3_MAX_ITERATIONS"),
           (dict(params=binding.sim3_params(max_iterations=binding.SS_SIM3_MAX_ITERATIONS + 1)), "max_iterations must be 1 .. SS_SIM3_MAX_ITERATIONS"),
           (dict(params=binding.sim3_params(min_inliers=-1)), "min_inliers must be >= 0"),
           (dict(params=binding.sim3_params(chi2=0.0)), "chi2 must be finite and > 0"), (dict(params=binding.sim3_params(chi2=-9.21)), "chi2 must be finite and > 0"),
           (dict(params=binding.sim3_params(chi2=nan)), "chi2 must be finite and > 0"), (dict(params=binding.sim3_params(chi2=inf)), "chi2 must be finite and > 0"),
           (dict(params=binding.sim3_params(reserved=(0, 1, 0))), "reserved fields must be 0")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.sim3_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message and e.value.message.startswith("sim3: "), (kw, e.value.message)
    # no pairs: nothing is launched, nothing is written
    ctx.sim3_pairs_device(**dict(good, n_pairs=0, views1=dev["views1"][:0], views2=dev["views2"][:0]))
    ctx.synchronize()
    assert (out.result.cpu().numpy() == 0x5A).all()
    pr = pairs[0]
    with pytest.raises(binding.OrbError) as e:
        ctx.sim3(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], binding.sim3_params(chi2=nan))
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    # the context is usable after every refusal; the host form with skip bytes and without rows
    p = SC.CASES[0]["params"]
    _check("after the refusals", _run(ctx, dev, 1, SC.ROWS, p), 0, SC.reference(0, 0))
    q_skip = np.zeros(len(pr["q_xyz"]), np.uint8)
    q_skip[pr["inlier_rows"][:3]] = 1
    flags, res = ctx.sim3(pr["view1"], pr["q_xyz"], pr["q_kp"], pr["view2"], pr["t_xyz"], pr["t_kp"], pr["idx"], _params(binding, p), q_skip=q_skip)
    _check("host form with skip bytes", (flags[None], np.array([res])), 0, _reference(dict(pr, q_skip=q_skip), p, 0))
    flags, res = ctx.sim3(pr["view1"], pr["q_xyz"][:0], pr["q_kp"][:0], pr["view2"], pr["t_xyz"][:0], pr["t_kp"][:0], pr["idx"][:0], _params(binding, p))
    assert len(flags) == 0 and (res["state"], res["n_corr"], res["iteration"]) == (1, 0, -1)


def test_stages_and_their_byte_figures(ctx):
    from send_slam_amd import binding
    pairs = [SC.case_pair(0), SC.case_pair(1)]
    dev = _upload(pairs, SC.ROWS)
    p = dict(SC.CASES[0]["params"], max_iterations=40)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        _run(ctx, dev, 2, SC.ROWS, p, skip=True)
        stats = {s["name"]: s for s in ctx.stats() if s["name"].startswith("sim3_")}
    finally:
        ctx.profile(False)
    n, nr, nh, hb = 2, 2 * SC.ROWS, 2 * 40, 2
    want = {"sim3_gather": nr * (4 + 4 + 2 * 32 + 2 * 4 + 1 + 1 + 48) + n * 4, "sim3_model": nh * (3 * 24 + 128 + 4),
            "sim3_count": nr * 48 * hb + nh * (128 + 4), "sim3_finish": nh * 4 + nr * (4 + 1 + 48) + n * (128 + 128)}
    assert list(stats) == list(want)
    for name, b in want.items():
        assert stats[name]["launches"] == 1 and stats[name]["algorithmic_bytes"] == b and stats[name]["total_ms"] > 0, (name, stats[name])
