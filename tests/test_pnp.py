"""GPU parity of the PnP RANSAC (ss_pnp_pairs_device, ss_pnp_batch_device, ss_pnp) through the C ABI: bit for bit, no tolerance --
every byte of every ss_pnp_result and every inlier flag.  Every output starts prefilled with a pattern no result has; flags past the
keypoint rows must be 0.  The reference is tests/pnp_ref.py where a test says "restatement" (the case table, the chain), and else
ss_pnp_host, the twin that tests/test_pnp_ref.py holds to the restatement bit for bit on every case: the restatement takes up to 20
ms per hypothesis, the twin microseconds, and a GPU test has seconds."""
import numpy as np
import pytest

import guided_cases as G
import pnp_cases as NC
import pnp_ref as N
import proj_cases as PC
import proj_ref as P

pytestmark = pytest.mark.gpu

HYP_BLOCK = 32    # SSK_PNP_HYP_BLOCK: the hypotheses one workgroup of k_pnp_count takes
MODEL_BLOCK = 64  # the hypotheses one workgroup of k_pnp_model takes
COUNT_ROWS = 256  # SSK_PNP_COUNT_ROWS: its correspondences
CHUNK = 1024      # SSK_PNP_CHUNK: the rows k_pnp_gather numbers at a time


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
        return self.inlier.cpu().numpy().copy(), self.result.cpu().numpy().copy().view(binding.PNP_RESULT_DTYPE).reshape(self.n)


def _told(sc):
    """the counts the device is told, where they are not the lengths of the arrays"""
    return sc.get("n_points", len(sc["points"])), sc.get("n_kp", len(sc["kp"]))


def _cut(sc):
    """what the device may read of sc: the rows under the counts it is told"""
    n_p, n_k = _told(sc)
    return dict(sc, points=sc["points"][:n_p], kp=sc["kp"][:n_k], idx=sc["idx"][:n_k], skip=None if sc["skip"] is None else sc["skip"][:n_p])


def _twin(sc, params, problem, scale=None):
    """(result, flags of every keypoint row) of ss_pnp_host"""
    res, flags = NC.host(_cut(sc), params, problem, scale)
    full = np.zeros(len(sc["kp"]), np.uint8)
    full[:len(flags)] = flags
    return res, full


def _restatement(sc, params, problem, scale=None, status=0):
    res, flags, _ = NC.solve_scene(_cut(sc), params, problem, scale, status)
    full = np.zeros(len(sc["kp"]), np.uint8)
    full[:len(flags)] = flags
    return res, full


def _upload(scenes, point_rows, rows):
    """block b and frame b are scene b's"""
    from send_slam_amd import binding
    n = len(scenes)
    host = {"points": np.zeros((n, point_rows), binding.MAP_POINT_DTYPE), "skip": np.zeros((n, point_rows), np.uint8),
            "kp": np.zeros((n, rows), binding.KP_DTYPE), "idx": np.full((n, rows), -1, np.int32), "np": np.zeros(n, np.int32), "nk": np.zeros(n, np.int32)}
    for b, sc in enumerate(scenes):
        k_p, k_k = len(sc["points"]), len(sc["kp"])
        host["np"][b], host["nk"][b] = _told(sc)
        host["points"][b, :k_p], host["kp"][b, :k_k], host["idx"][b, :k_k] = sc["points"], sc["kp"], sc["idx"]
        if sc["skip"] is not None:
            host["skip"][b, :k_p] = sc["skip"]
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["views"] = np.concatenate([np.asarray(sc["view"]).reshape(1) for sc in scenes]) if n else np.zeros(0, P.VIEW_DTYPE)
    _sync()
    return dev


def _params(binding, p):
    return binding.pnp_params(**p)


def _run(ctx, dev, n, point_rows, rows, params, skip=False, n_blocks=None, n_kp_frames=None, views=None, kp_src=None, point_src=None):
    from send_slam_amd import binding
    out = Out(n, rows)
    ctx.pnp_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), n if n_blocks is None else n_blocks, point_rows, dev["kp"].data_ptr(),
                         dev["nk"].data_ptr(), n if n_kp_frames is None else n_kp_frames, rows, dev["idx"].data_ptr(), n,
                         dev["views"] if views is None else views, _params(binding, params), out.inlier.data_ptr(), out.result.data_ptr(),
                         kp_src=kp_src, point_src=point_src, d_point_skip=dev["skip"].data_ptr() if skip else 0)
    ctx.synchronize()
    return out.host()


def _check(tag, got, b, want):
    flags, results = got
    wres, wflags = want[0], want[1]
    for name in N.RESULT_DTYPE.names:
        assert results[b][name].tobytes() == wres[name].tobytes(), f"{tag}: result.{name} {results[b][name]} != {wres[name]}"
    nk = len(wflags)
    bad = np.flatnonzero(flags[b][:nk] != wflags)
    assert len(bad) == 0, f"{tag}: flags differ at keypoint rows {bad[:8]}: {flags[b][:nk][bad[:8]]} != {wflags[bad[:8]]}"
    assert not flags[b][nk:].any(), f"{tag}: flags past the keypoint rows are not 0"


def _against_twin(ctx, scenes, point_rows, rows, params, tag, skip=False):
    dev = _upload(scenes, point_rows, rows)
    got = _run(ctx, dev, len(scenes), point_rows, rows, params, skip)
    wants = [_twin(sc if skip else dict(sc, skip=None), params, b) for b, sc in enumerate(scenes)]
    for b, w in enumerate(wants):
        _check(f"{tag}, problem {b}", got, b, w)
    return wants


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=2) as c:
        yield c


@pytest.mark.parametrize("k", range(len(NC.CASES)), ids=NC.CASE_NAMES)
def test_cases_three_problems_per_call(ctx, k):
    """case k with two other cases behind it in one call under case k's parameters: three problems of different N and states, the
    problem number in the draw stream.  Problem 0 against the restatement, the others against the twin"""
    n = len(NC.CASES)
    members = [k, (k + 4) % n, (k + 9) % n]
    scenes = [NC.case_scene(j) for j in members]
    p = NC.CASES[k]["params"]
    dev = _upload(scenes, NC.ROWS, NC.ROWS)
    got = _run(ctx, dev, 3, NC.ROWS, NC.ROWS, p)
    ref = NC.reference(k, 0)
    _check(NC.CASES[k]["name"] + " (restatement)", got, 0, ref)
    assert ref[0]["state"] == NC.CASES[k]["expect_state"]
    wants = [_twin(sc, p, b) for b, sc in enumerate(scenes)]
    for b, w in enumerate(wants):
        _check(f"{NC.CASES[k]['name']}, problem {b}", got, b, w)
    assert len({int(w[0]["n_corr"]) for w in wants}) >= 2


def test_one_problem_three_times(ctx):
    """the same problem three times in one call: the problem number alone changes the draws, so the winners differ"""
    scenes = [NC.case_scene(0)] * 3
    p = dict(NC.CASES[0]["params"], seed=1)
    wants = _against_twin(ctx, scenes, NC.ROWS, NC.ROWS, p, "one problem three times")
    assert len({int(w[0]["iteration"]) for w in wants}) > 1 and all(w[0]["state"] == 0 for w in wants)
    for b in range(3):
        assert wants[b][0].tobytes() == NC.reference(0, b)[0].tobytes()  # seed 1 is the case's own: the restatement's answer


def test_three_candidates_share_one_keypoint_frame(ctx):
    """three candidate keyframes of one lost frame: three problems that read keypoint frame 1 of two through kp_src and three blocks of
    points in another order through point_src, equal to three calls on copied keypoints"""
    lost = NC.make_scene(60, 50, 20, 64, 64, noise=0.5)
    other = NC.make_scene(61, 30, 0, 64, 64)
    # candidate 0 sees the scene; candidate 1 has half of the matches; candidate 2 has map points of another place
    c0 = dict(lost)
    c1 = dict(lost, idx=np.where(np.arange(64) % 2 == 0, lost["idx"], -1).astype(np.int32))
    c2 = dict(lost, points=other["points"])
    cands = [c0, c1, c2]
    p = dict(NC.CASES[0]["params"], max_iterations=48, seed=5)
    dev = _upload([other, lost, lost], 64, 64)  # frames: [other, lost]; blocks: [other, lost, lost] before the next line
    dev["points"] = _to_dev(np.stack([c2["points"], c0["points"], c1["points"]]))
    dev["np"] = _to_dev(np.array([64, 64, 64], np.int32))
    dev["idx"] = _to_dev(np.stack([c["idx"] for c in cands]))
    dev["views"] = np.concatenate([np.asarray(c["view"]).reshape(1) for c in cands])
    _sync()
    got = _run(ctx, dev, 3, 64, 64, p, n_blocks=3, n_kp_frames=2, kp_src=[1, 1, 1], point_src=[1, 2, 0])
    wants = [_twin(c, p, q) for q, c in enumerate(cands)]
    for q, w in enumerate(wants):
        _check(f"shared keypoint frame, candidate {q}", got, q, w)
    assert wants[0][0]["state"] == 0 and wants[0][0]["n_inliers"] >= 30 and wants[2][0]["state"] == 2
    assert wants[1][0]["n_corr"] < wants[0][0]["n_corr"]
    # three calls of one problem each on copied keypoints: the problem number is 0 in each, so the twin's too
    for q, c in enumerate(cands):
        one = _upload([c], 64, 64)
        _check(f"copied keypoints, candidate {q}", _run(ctx, one, 1, 64, 64, p), 0, _twin(c, p, 0))
    # and the same three problems with copies in one call give the shared call's bytes
    three = _upload(cands, 64, 64)
    again = _run(ctx, three, 3, 64, 64, p)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("rows", [128, CHUNK + 76])
def test_compaction(ctx, rows):
    """matches and skip bytes scattered so that the kept rows straddle the wave (and, in the larger shape, the chunk) boundaries: rows
    63 / 64 / 65 (and 1023 / 1024 / 1025) kept; n_kp and n_points under their rows; idx at and past n_points and below -1; the flags
    land on the keypoint rows"""
    rng = np.random.Generator(np.random.PCG64(rows))
    edges = [e + d for e in ((64, CHUNK) if rows > CHUNK else (64,)) for d in (-1, 0, 1)]
    scenes = []
    for b in range(2):
        sc = dict(NC.make_scene(40 + b + rows, rows, rows // 3, rows, rows, noise=0.5))  # every row a correspondence, then a quarter unmatched
        sc["idx"] = sc["idx"].copy()
        inner = np.setdiff1d(np.arange(rows), edges)
        drop = rng.choice(inner, rows // 4, replace=False)
        sc["idx"][drop] = -1
        kept = np.setdiff1d(inner, drop)
        sc["skip"] = np.zeros(rows, np.uint8)
        sc["skip"][sc["idx"][rng.choice(kept, 6, replace=False)]] = rng.integers(1, 256, 6)
        n_p, n_k = rows - 14, rows - 9
        sc["n_points"], sc["n_kp"] = n_p, n_k
        sc["points"] = sc["points"].copy()
        for e in edges:  # an edge row whose point lies past n_points trades point rows with a kept row whose point does not
            if sc["idx"][e] >= n_p:
                r = next(r for r in kept if sc["idx"][r] < n_p and sc["skip"][sc["idx"][r]] == 0)
                a, c = sc["idx"][e], sc["idx"][r]
                sc["points"][[a, c]] = sc["points"][[c, a]]
                sc["idx"][e], sc["idx"][r] = c, a
        sc["idx"][drop[3:7]] = [n_p, n_p + 5, 1 << 30, -7]
        scenes.append(sc)
    p = dict(NC.CASES[0]["params"], max_iterations=48, seed=5)
    wants = _against_twin(ctx, scenes, rows, rows, p, f"compaction at {rows} rows", skip=True)
    for sc, (res, flags) in zip(scenes, wants):
        n_p, n_k = _told(sc)
        assert res["state"] == 0 and 20 < res["n_corr"] < rows - rows // 4  # the counts, flags and bad entries dropped some
        assert (sc["idx"][:n_k] >= n_p).sum() >= 2 and set(edges) <= set(np.flatnonzero((sc["idx"][:n_k] >= 0) & (sc["idx"][:n_k] < n_p)).tolist())
        hit = np.flatnonzero(flags)
        assert len(hit) == res["n_inliers"] and hit.max() > res["n_corr"]  # a flag sits on a keypoint row, not on a correspondence number
    # without the skip array the flagged rows are correspondences again
    again = _against_twin(ctx, scenes, rows, rows, p, f"compaction at {rows} rows without skip bytes", skip=False)
    assert all(a[0]["n_corr"] > w[0]["n_corr"] for a, w in zip(again, wants))
    if rows == 128:  # the restatement once
        _check("compaction, restatement", (wants[0][1][None], np.array([wants[0][0]])), 0, _restatement(scenes[0], p, 0))


def test_compaction_with_a_wave_that_keeps_nothing(ctx):
    rows = CHUNK + 65
    sc = dict(NC.make_scene(45, rows, rows // 3, rows, rows, scatter=False))
    sc["skip"] = np.zeros(rows, np.uint8)
    sc["skip"][sc["idx"][192:256]] = 1
    p = dict(NC.CASES[0]["params"], max_iterations=48, seed=7)
    (res, flags), = _against_twin(ctx, [sc], rows, rows, p, "a wave that keeps nothing", skip=True)
    assert res["n_corr"] == rows - 64 and res["state"] == 0
    assert not flags[192:256].any() and flags[:192].any() and flags[256:CHUNK].any() and flags[CHUNK:].any()


def test_correspondence_counts(ctx):
    """N at 0, 5, 6, 7 and one below, at and one above the correspondences of one workgroup of k_pnp_count"""
    rows = COUNT_ROWS + 44
    counts = (0, 5, 6, 7, COUNT_ROWS - 1, COUNT_ROWS, COUNT_ROWS + 1)
    scenes = [NC.make_scene(50 + n, max(n, 1), n // 4, rows, rows) for n in counts]
    scenes[0] = dict(scenes[0], idx=np.full(rows, -1, np.int32))
    p = dict(NC.CASES[0]["params"], min_inliers=5, max_iterations=40, seed=3)
    wants = _against_twin(ctx, scenes, rows, rows, p, "correspondence counts")
    assert [int(w[0]["n_corr"]) for w in wants] == list(counts)
    assert [int(w[0]["state"]) for w in wants][:2] == [1, 1] and all(w[0]["state"] == 0 for w in wants[4:])
    small = [sc for sc, n in zip(scenes, counts) if n <= 7]
    for b, sc in enumerate(small):  # the restatement on the small ones, as the same problem numbers
        assert _restatement(sc, p, b)[0].tobytes() == wants[b][0].tobytes()


BLOCK_SEEDS = {"t = 0 of 1": (8337, 1, 0), "the last lane of the first model block": (2010, 64, 63), "one before it": (27, 63, 62),
               "the first lane of the second model block": (760, 65, 64), "the last hypothesis of the first count block": (3148, 32, 31),
               "the only hypothesis of the second count block": (6550, 33, 32), "the last of SS_PNP_MAX_ITERATIONS": (1829, 1024, 1023),
               "t = 0 of SS_PNP_MAX_ITERATIONS": (8337, 1024, 0)}


@pytest.mark.parametrize("max_iterations", [1, HYP_BLOCK - 1, HYP_BLOCK + 1, MODEL_BLOCK - 1, MODEL_BLOCK, MODEL_BLOCK + 1, 1024])
def test_hypothesis_blocking_counts(ctx, max_iterations):
    """max_iterations at 1, around the blocks of hypotheses of k_pnp_count and k_pnp_model, and at SS_PNP_MAX_ITERATIONS: every count
    enters the result through best_inliers or the winner"""
    scenes = [NC.make_scene(**NC.BLOCK_SCENE), NC.case_scene(0)]
    p = dict(NC.BLOCK_PARAMS, max_iterations=max_iterations, seed=42)
    _against_twin(ctx, scenes, NC.ROWS, NC.ROWS, p, f"{max_iterations} iterations")


@pytest.mark.parametrize("where", list(BLOCK_SEEDS))
def test_hypothesis_blocking_winner(ctx, where):
    """the only hypothesis that draws six of the twelve inliers planted at the first and the last t"""
    seed, max_iterations, t = BLOCK_SEEDS[where]
    p = dict(NC.BLOCK_PARAMS, max_iterations=max_iterations, seed=seed)
    (res, flags), = _against_twin(ctx, [NC.make_scene(**NC.BLOCK_SCENE)], NC.ROWS, NC.ROWS, p, where)
    assert res["state"] == 0 and res["iteration"] == t and res["n_inliers"] == 12
    if max_iterations <= 65:
        ref = _restatement(NC.make_scene(**NC.BLOCK_SCENE), p, 0)
        assert ref[0].tobytes() == res.tobytes() and np.array_equal(ref[1], flags)


@pytest.mark.parametrize("refine_steps", [0, 5, 16])
def test_refinement_counts(ctx, refine_steps):
    scenes = [NC.case_scene(0), NC.make_scene(70, 50, 10, 64, 64, noise=1.0)]
    p = dict(NC.CASES[0]["params"], refine_steps=refine_steps, max_iterations=48, min_ratio=0.2)  # unrefined models keep a third of the inliers
    wants = _against_twin(ctx, scenes, NC.ROWS, NC.ROWS, p, f"refine_steps {refine_steps}")
    assert all(w[0]["state"] == 0 for w in wants)
    _check(f"refine_steps {refine_steps}, restatement", (wants[0][1][None], np.array([wants[0][0]])), 0, _restatement(scenes[0], p, 0))


def test_limits(ctx):
    """two problems of SS_GUIDED_MAX_ROWS rows, every row a correspondence, 300 iterations"""
    from send_slam_amd import binding
    rows = binding.SS_GUIDED_MAX_ROWS
    scenes = [NC.make_scene(60 + b, rows, rows * 2 // 5, scatter=False, noise=0.5) for b in range(2)]
    p = dict(NC.RECOVERY, seed=11)
    wants = _against_twin(ctx, scenes, rows, rows, p, "full capacity")
    for res, flags in wants:
        assert res["n_corr"] == rows and res["state"] == 0 and res["n_inliers"] >= rows * 3 // 5 - 50


def test_degenerate_scenes(ctx):
    """coplanar, collinear and identical points in every hypothesis, and a good scene with 1e30, infinite and NaN numbers and a doubled
    point row among its correspondences: the device gives the twin's bytes, all finite"""
    named = NC.degenerate_scenes()
    scenes = [sc for _, sc in named]
    rows = max(len(sc["kp"]) for sc in scenes)
    p = dict(NC.CASES[0]["params"], max_iterations=64)
    dev = _upload(scenes, rows, rows)
    got = _run(ctx, dev, len(scenes), rows, rows, p)
    for b, (name, sc) in enumerate(named):
        _check(name, got, b, _twin(sc, p, b))
        assert np.isfinite(got[1][b]["rcw"]).all() and np.isfinite(got[1][b]["tcw"]).all()
    assert got[1][3]["n_corr"] == 40  # the broken rows are correspondences: their numbers are, not their count


@pytest.mark.parametrize("name", ["one_level", "sixteen_levels"])
def test_other_pyramid_tables(name):
    """the octave test and the thresholds read the context's table: one level (every octave but 0 is outside) and SS_MAX_LEVELS"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    table = PC.scale_table(factor, n_levels)
    sc = NC.make_scene(70, 50, 10, 64, 64, octaves=(0, 0, 1, n_levels - 1, n_levels), noise=0.5)
    p = dict(NC.CASES[0]["params"], min_inliers=6, min_ratio=0.3, max_iterations=48, seed=5)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        dev = _upload([sc], 64, 64)
        got = _run(c, dev, 1, 64, 64, p)
    want = _restatement(sc, p, 0, scale=table)
    _check(name, got, 0, want)
    _check(name + ", twin", got, 0, _twin(sc, p, 0, scale=table))
    assert 6 <= want[0]["n_corr"] < 50 and want[0]["state"] == 0


# ---- a camera per problem, strides that differ, counts told wrong, a small call after a large one ------------------------------------------
def _run_into(ctx, dev, out, n, point_rows, rows, params, skip=False, kp_src=None, point_src=None):
    """_run into outputs of the caller's, which may be longer than the call's"""
    from send_slam_amd import binding
    ctx.pnp_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), n, point_rows, dev["kp"].data_ptr(), dev["nk"].data_ptr(), n, rows,
                         dev["idx"].data_ptr(), n, dev["views"], _params(binding, params), out.inlier.data_ptr(), out.result.data_ptr(),
                         kp_src=kp_src, point_src=point_src, d_point_skip=dev["skip"].data_ptr() if skip else 0)
    ctx.synchronize()
    return out.host()


def _twin_of_told(sc, params, problem):
    """_twin under counts that may lie past the rows or below 0: the rule clamps them"""
    res, flags = NC.host(NC.cut(sc), params, problem)
    full = np.zeros(len(sc["kp"]), np.uint8)
    full[:len(flags)] = flags
    return res, full


def test_a_camera_per_problem(ctx):
    """three problems under the cameras P, Q and the square one, each with its own pose, against the restatement: views[0] for
    views[b] in any of the three kernels that read a view loses problems 1 and 2.  Then the same problems with their keypoint frames
    and point blocks uploaded in another order, views still by problem: views[kp_src[b]] or views[point_src[b]] for views[b] would
    change the bytes"""
    scenes = NC.camera_scenes()
    p = NC.CAMERA_PARAMS
    dev = _upload(scenes, 80, 64)
    got = _run(ctx, dev, 3, 80, 64, p)
    for b, sc in enumerate(scenes):
        want = _restatement(sc, p, b)
        _check(f"camera scene {b}", got, b, want)
        assert want[0]["state"] == 0 and want[0]["n_inliers"] == NC.CAMERA_INLIERS and want[0]["iteration"] == NC.CAMERA_WINNERS[b]
    kp_src, point_src = [2, 0, 1], [1, 2, 0]
    frames, blocks = [scenes[kp_src.index(f)] for f in range(3)], [scenes[point_src.index(f)] for f in range(3)]
    moved = _upload(frames, 80, 64)  # kp and nk by frame
    by_block = _upload(blocks, 80, 64)
    moved["points"], moved["np"] = by_block["points"], by_block["np"]
    moved["idx"], moved["views"] = dev["idx"], dev["views"]  # by problem
    again = _run(ctx, moved, 3, 80, 64, p, kp_src=kp_src, point_src=point_src)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("layout", list(NC.STRIDE_LAYOUTS))
def test_point_rows_and_keypoint_rows_differ(ctx, layout):
    """point_rows != rows_per_frame, with and without the skip array: a stride of points, p_skip, idx, kp, corr_of_row or inlier taken
    from the wrong one of the two reads another scene's rows or the rows past the counts, which look live.  The flags past n_kp are
    0, and the bytes of d_inlier behind the call's problems stay as they were"""
    scenes, point_rows, rows = NC.stride_scenes(layout)
    dev = _upload(scenes, point_rows, rows)
    for skip in (True, False):
        out = Out(len(scenes) + 1, rows)
        got = _run_into(ctx, dev, out, len(scenes), point_rows, rows, NC.STRIDE_PARAMS, skip)
        for b, sc in enumerate(scenes):
            want = _twin(sc if skip else dict(sc, skip=None), NC.STRIDE_PARAMS, b)
            _check(f"{layout}, skip {skip}, problem {b}", got, b, want)
            assert not got[0][b][sc["n_kp"]:].any() and want[0]["n_corr"] == (35 if skip else 40) and want[0]["state"] == 0
        assert (got[0][len(scenes)] == 0x5A).all() and (got[1].view(np.uint8).reshape(len(scenes) + 1, -1)[len(scenes)] == 0x5A).all()


def test_counts_told_wrong(ctx):
    """n_kp and n_points past their rows and below 0: the device clamps them as the rule does, and a count past the rows gives the
    bytes of the rows"""
    named = NC.count_scenes()
    scenes = [sc for _, sc in named]
    dev = _upload(scenes, NC.COUNT_POINT_ROWS, NC.COUNT_ROWS)
    assert dev["nk"].cpu().numpy().tolist() == [NC.COUNT_ROWS + 9, -3, NC.COUNT_ROWS, NC.COUNT_ROWS]
    assert dev["np"].cpu().numpy().tolist() == [NC.COUNT_POINT_ROWS, NC.COUNT_POINT_ROWS, NC.COUNT_POINT_ROWS + 5, -2]
    got = _run(ctx, dev, len(scenes), NC.COUNT_POINT_ROWS, NC.COUNT_ROWS, NC.COUNT_PARAMS)
    for b, (name, sc) in enumerate(named):
        want = _twin_of_told(sc, NC.COUNT_PARAMS, b)
        _check(name, got, b, want)
        assert (want[0]["state"], want[0]["n_corr"]) == ((0, 44) if "+" in name else (1, 0))
    plain = dict(scenes[0], n_kp=NC.COUNT_ROWS, n_points=NC.COUNT_POINT_ROWS)
    exact = _run(ctx, _upload([plain] * 4, NC.COUNT_POINT_ROWS, NC.COUNT_ROWS), 4, NC.COUNT_POINT_ROWS, NC.COUNT_ROWS, NC.COUNT_PARAMS)
    for b in (0, 2):
        assert got[0][b].tobytes() == exact[0][b].tobytes() and got[1][b].tobytes() == exact[1][b].tobytes()


def test_a_small_call_after_a_large_one():
    """3 problems of 300 rows and 1024 hypotheses, 1 problem of 64 rows and 8 hypotheses, the first again, on one context: each gives
    the bytes of a context that has run nothing else, so nothing of a call's workspace outlives it"""
    from send_slam_amd import binding
    large = [NC.make_scene(340 + b, 200, 80, 300, 300, noise=0.5) for b in range(3)]
    small = [NC.case_scene(0)]
    calls = [(large, 300, dict(NC.RECOVERY, max_iterations=1024, seed=6)), (small, 64, dict(NC.CASES[0]["params"], max_iterations=8)),
             (large, 300, dict(NC.RECOVERY, max_iterations=1024, seed=6))]
    devs = [_upload(scenes, rows, rows) for scenes, rows, _ in calls]
    fresh = []
    for (scenes, rows, p), dev in zip(calls[:2], devs):
        with binding.OrbContext(0, n_features=G.NF) as c:
            fresh.append(_run(c, dev, len(scenes), rows, rows, p))
    fresh.append(fresh[0])
    _check("fresh context, 64 rows", fresh[1], 0, _twin(small[0], calls[1][2], 0))
    assert all(r["state"] == 0 and r["n_inliers"] == 120 for r in fresh[0][1]) and fresh[1][1][0]["n_corr"] == 60  # the large call is live
    with binding.OrbContext(0, n_features=G.NF) as c:
        for k, ((scenes, rows, p), dev) in enumerate(zip(calls, devs)):
            got = _run(c, dev, len(scenes), rows, rows, p)
            assert got[0].tobytes() == fresh[k][0].tobytes() and got[1].tobytes() == fresh[k][1].tobytes(), f"call {k} on the used context"


# ---- the batch form and the one-problem host form ---------------------------------------------------------------------------------------
BATCH = ["synth_t0", "synth_t1"]


def _lifted_blocks(kcap):
    """a block of map points per frame: the frame's keypoints lifted to a depth of 3 - 9 in the camera of NC.POSE (point row = a
    permutation of the keypoint row; a fifth of the rows keep a wrong point), and idx by keypoint row"""
    rng = np.random.Generator(np.random.PCG64(0xBA7D))
    kps = [G.features(name)[0] for name in BATCH]
    pts, idx, good = np.zeros((len(BATCH), kcap), P.MAP_POINT_DTYPE), np.full((len(BATCH), kcap), -1, np.int32), []
    for b, kp in enumerate(kps):
        n = len(kp)
        z = rng.uniform(3.0, 9.0, n)
        xc = np.stack([(kp["x"] - NC.CX) / NC.FX * z, (kp["y"] - NC.CY) / NC.FY * z, z], axis=1)
        wrong = rng.random(n) < 0.2
        xc[wrong] = rng.uniform(-3, 3, (int(wrong.sum()), 3)) + [0, 0, 6.0]
        perm = rng.permutation(n)
        pts[b, perm] = NC.points_of(NC.to_world(xc))
        idx[b, :n] = perm
        idx[b, rng.choice(n, n // 10, replace=False)] = -1
        good.append(np.flatnonzero(~wrong & (idx[b, :n] >= 0)))
    return kps, pts, idx, good


def test_batch_form_pairs_form_and_host_form_agree(monkeypatch):
    """two 320 x 240 frames of tests/golden, synthetic map points: three problems (frame 0 with its block, frame 1 with its block,
    frame 0 with the other frame's block) through the batch form, the pairs form on copied keypoints and ss_pnp_host; a flagged frame
    voids its problems"""
    from send_slam_amd import binding
    from test_guided import _extract
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    n = len(BATCH)
    p = dict(NC.CASES[0]["params"], max_iterations=64, seed=9)
    kp_src, point_src = [0, 1, 0], [0, 1, 1]
    views = [NC.view()] * 3
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        kps, pts, idx, good = _lifted_blocks(kcap)
        idx3 = np.stack([idx[0], idx[1], idx[0]])
        d_pts, d_np, d_idx = _to_dev(pts), _to_dev(np.array([len(k) for k in kps], np.int32)), _to_dev(idx3)
        _sync()
        out = Out(3, kcap)
        c.pnp_batch_device(d_pts.data_ptr(), d_np.data_ptr(), n, kcap, d_idx.data_ptr(), 3, views, _params(binding, p), out.inlier.data_ptr(),
                           out.result.data_ptr(), kp_src=kp_src, point_src=point_src)
        c.synchronize()
        got = out.host()
        scenes = [dict(view=views[q], points=pts[point_src[q], :len(kps[point_src[q]])], kp=kps[kp_src[q]], idx=idx3[q, :len(kps[kp_src[q]])], skip=None)
                  for q in range(3)]
        wants = [_twin(sc, p, q) for q, sc in enumerate(scenes)]
        for q, w in enumerate(wants):
            _check(f"batch form, problem {q}", got, q, w)
        for q in (0, 1):
            assert wants[q][0]["state"] == 0 and wants[q][0]["n_inliers"] >= len(good[q]) - 2 > 100
            assert np.abs(wants[q][0]["rcw"].reshape(3, 3) - NC.POSE[0]).max() < 0.01
        assert wants[2][0]["state"] == 2
        _check("batch form, problem 1 on the restatement", got, 1, _restatement(scenes[1], p, 1))
        # the pairs form on copied keypoints
        d_kp = _to_dev(np.stack([np.concatenate([kp, np.zeros(kcap - len(kp), binding.KP_DTYPE)]) for kp in kps]))
        d_nk = _to_dev(np.array([len(kp) for kp in kps], np.int32))
        _sync()
        out2 = Out(3, kcap)
        c.pnp_pairs_device(d_pts.data_ptr(), d_np.data_ptr(), n, kcap, d_kp.data_ptr(), d_nk.data_ptr(), n, kcap, d_idx.data_ptr(), 3, views,
                           _params(binding, p), out2.inlier.data_ptr(), out2.result.data_ptr(), kp_src=kp_src, point_src=point_src)
        c.synchronize()
        g2 = out2.host()
        assert g2[0].tobytes() == got[0].tobytes() and g2[1].tobytes() == got[1].tobytes()
        # the host form is problem 0 of its own call
        flags, one = c.pnp(views[0], scenes[0]["points"], scenes[0]["kp"], scenes[0]["idx"], _params(binding, p))
        assert one.tobytes() == got[1][0].tobytes() and np.array_equal(flags, got[0][0][:len(flags)])
        for bad_src, word in ((dict(kp_src=[0, 1, 2]), "kp_src[2] = 2 names no frame of keypoints (2)"),
                              (dict(point_src=[0, -1, 1]), "point_src[1] = -1 names no block of points (2)")):
            with pytest.raises(binding.OrbError) as e:
                c.pnp_batch_device(d_pts.data_ptr(), d_np.data_ptr(), n, kcap, d_idx.data_ptr(), 3, views, _params(binding, p), out.inlier.data_ptr(),
                                   out.result.data_ptr(), **dict(dict(kp_src=kp_src, point_src=point_src), **bad_src))
            assert e.value.code == binding.SS_ERR_INVALID_ARG and word in e.value.message, e.value.message
    # frame 0 flagged: the problems on it carry the status and have no correspondence
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "0")
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, BATCH)
        out = Out(3, kcap)
        c.pnp_batch_device(d_pts.data_ptr(), d_np.data_ptr(), n, kcap, d_idx.data_ptr(), 3, views, _params(binding, p), out.inlier.data_ptr(),
                           out.result.data_ptr(), kp_src=kp_src, point_src=point_src)
        c.synchronize()
        got = out.host()
        for q in (0, 2):
            void = _restatement(scenes[q], p, q, status=binding.SS_ERR_OVERFLOW)
            _check(f"flagged, problem {q}", got, q, void)
            assert void[0]["state"] == 1 and void[0]["n_corr"] == 0 and void[0]["status"] == binding.SS_ERR_OVERFLOW
        _check("the problem next to the flagged ones", got, 1, wants[1])


def test_without_a_batch_the_batch_form_returns_state():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as c:
        with pytest.raises(binding.OrbError) as e:
            c.pnp_batch_device(1, 1, 1, 1, 1, 1, [NC.view()], binding.pnp_params(), 1, 1)
        assert e.value.code == binding.SS_ERR_STATE and "ss_pnp_batch_device" in e.value.message


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_bow_match_pnp_pose_optimisation_view_projection_search(ctx):
    """ss_match_bow_pairs_device -> ss_pnp_pairs_device on the device's own idx -> ss_pose_opt_pairs_device (start = the result's twelve
    doubles, idx_by_row = 1) -> ss_proj_view_init -> ss_match_proj_pairs_device: every stage equals the same chain on the references
    (the restatements), and the optimised pose lies within the pose test's own tolerance of the planted one"""
    from send_slam_amd import binding
    from test_guided import Outputs as MatchOut
    from test_guided import _check as _check_match
    from test_pose import Out as PoseOut
    from test_pose import _check as _check_pose
    from test_proj import Outputs as ProjOut
    from test_proj import _check as _check_proj
    sc, rows = NC.chain_scene(), NC.CHAIN_ROWS
    bow, pnp, pose, view, proj = NC.chain_reference()
    dev = _upload([sc], rows, rows)
    d = {k: _to_dev(np.ascontiguousarray(sc[k])[None]) for k in ("q_desc", "t_desc", "q_node", "t_node", "t_kp")}
    m, out, po = MatchOut(1, rows), Out(1, rows), PoseOut(1, rows)
    _sync()
    # the lost frame is the query, the candidate keyframe the train: idx[i] is the candidate's row, and its map point's
    ctx.match_bow_pairs_device(d["q_desc"].data_ptr(), dev["kp"].data_ptr(), d["q_node"].data_ptr(), dev["nk"].data_ptr(), d["t_desc"].data_ptr(),
                               d["t_kp"].data_ptr(), d["t_node"].data_ptr(), dev["np"].data_ptr(), 1, rows, binding.guided_params(**NC.CHAIN_BOW), *m.ptrs())
    ctx.pnp_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), 1, rows, dev["kp"].data_ptr(), dev["nk"].data_ptr(), 1, rows, m.idx.data_ptr(), 1,
                         dev["views"], _params(binding, NC.CHAIN_PNP), out.inlier.data_ptr(), out.result.data_ptr())  # the match's idx, never on the host
    ctx.synchronize()
    _check_match("chain, BoW match", m.host(), 0, bow)
    got = out.host()
    _check("chain, PnP", got, 0, pnp)
    assert pnp[0]["state"] == 0 and pnp[0]["n_inliers"] >= 38
    start = np.concatenate([got[1][0]["rcw"], got[1][0]["tcw"]])
    ctx.pose_opt_pairs_device(dev["points"].data_ptr(), dev["np"].data_ptr(), 1, rows, dev["kp"].data_ptr(), dev["nk"].data_ptr(), 1, rows, m.idx.data_ptr(),
                              dev["views"], start, binding.pose_opt_params(idx_by_row=True), po.flags.data_ptr(), po.result.data_ptr())
    ctx.synchronize()
    pg = po.host()
    _check_pose("chain, pose optimisation", pg, 0, pose)
    assert pose[0]["state"] == 0
    assert np.abs(pg[1][0]["rcw"].reshape(3, 3) - NC.POSE[0]).max() < 2e-3 and np.abs(pg[1][0]["tcw"] - NC.POSE[1]).max() < 2e-2
    cam = binding.Camera(fx=NC.FX, fy=NC.FY, cx=NC.CX, cy=NC.CY, width=NC.W, height=NC.H)
    v = binding.proj_view(cam, pg[1][0]["rcw"], pg[1][0]["tcw"], 0.0)
    assert bytes(v) == view.tobytes()
    fo = ProjOut(1, rows)
    _sync()
    # the candidate's map points searched in the lost frame under the found pose
    ctx.match_proj_pairs_device(dev["points"].data_ptr(), d["t_desc"].data_ptr(), dev["np"].data_ptr(), 1, rows, d["q_desc"].data_ptr(), dev["kp"].data_ptr(),
                                dev["nk"].data_ptr(), 1, rows, [v], binding.proj_params(extent_w=NC.W, extent_h=NC.H, **NC.CHAIN_PROJ), *fo.ptrs())
    ctx.synchronize()
    fg = fo.host()
    _check_proj("chain, projection search", fg, 0, proj)
    for i in np.flatnonzero(got[0][0]):
        assert fg[0][0][bow[0][i]] == i  # the search finds the keypoint of every RANSAC inlier again


# ---- contract ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_and_their_messages(ctx):
    from send_slam_amd import binding
    sc = NC.case_scene(0)
    dev = _upload([sc], NC.ROWS, NC.ROWS)
    out = Out(1, NC.ROWS)
    good = dict(d_points=dev["points"].data_ptr(), d_n_points=dev["np"].data_ptr(), n_blocks=1, point_rows=NC.ROWS, d_kp=dev["kp"].data_ptr(),
                d_n_kp=dev["nk"].data_ptr(), n_kp_frames=1, rows_per_frame=NC.ROWS, d_idx=dev["idx"].data_ptr(), n_problems=1, views=dev["views"],
                params=binding.pnp_params(), d_inlier=out.inlier.data_ptr(), d_result=out.result.data_ptr())
    nan, inf = float("nan"), float("inf")
    bad = [(dict(rows_per_frame=binding.SS_GUIDED_MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"),
           (dict(point_rows=binding.SS_GUIDED_MAX_ROWS + 1), "exceed SS_GUIDED_MAX_ROWS (16384)"), (dict(rows_per_frame=0), "bad problem, frame, block or row count"),
           (dict(point_rows=0), "bad problem, frame, block or row count"), (dict(n_blocks=-1), "bad problem, frame, block or row count"),
           (dict(params=binding.pnp_params(max_iterations=0)), "max_iterations must be 1 .. SS_PNP_MAX_ITERATIONS"),
           (dict(params=binding.pnp_params(max_iterations=binding.SS_PNP_MAX_ITERATIONS + 1)), "max_iterations must be 1 .. SS_PNP_MAX_ITERATIONS"),
           (dict(params=binding.pnp_params(refine_steps=-1)), "refine_steps must be 0 .. SS_PNP_MAX_REFINE"),
           (dict(params=binding.pnp_params(refine_steps=binding.SS_PNP_MAX_REFINE + 1)), "refine_steps must be 0 .. SS_PNP_MAX_REFINE"),
           (dict(params=binding.pnp_params(min_inliers=-1)), "min_inliers must be >= 0"),
           (dict(params=binding.pnp_params(min_ratio=-0.5)), "min_ratio must be finite and >= 0"), (dict(params=binding.pnp_params(min_ratio=nan)), "min_ratio must be finite and >= 0"),
           (dict(params=binding.pnp_params(lambda_=-1e-6)), "lambda must be finite and >= 0"), (dict(params=binding.pnp_params(lambda_=inf)), "lambda must be finite and >= 0"),
           (dict(params=binding.pnp_params(chi2=0.0)), "chi2 must be finite and > 0"), (dict(params=binding.pnp_params(chi2=nan)), "chi2 must be finite and > 0"),
           (dict(params=binding.pnp_params(chi2=inf)), "chi2 must be finite and > 0"),
           (dict(params=binding.pnp_params(reserved=(0, 1))), "reserved fields must be 0"), (dict(params=binding.pnp_params(reserved=(1, 0))), "reserved fields must be 0"),
           (dict(kp_src=[1]), "kp_src[0] = 1 names no frame of keypoints (1)"), (dict(kp_src=[-1]), "kp_src[0] = -1 names no frame of keypoints (1)"),
           (dict(point_src=[1]), "point_src[0] = 1 names no block of points (1)"), (dict(n_blocks=0), "problem [0] = 0 names no block of points (0)"),
           (dict(n_kp_frames=0), "problem [0] = 0 names no frame of keypoints (0)")]
    bad += [({k: 0}, "NULL buffer") for k in good if k.startswith("d_")]
    for kw, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.pnp_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (kw, e.value.message)
        assert e.value.message.startswith(("pnp: ", "kp_src[", "point_src[", "problem [")), e.value.message
    # no problems: nothing is launched, nothing is written
    ctx.pnp_pairs_device(**dict(good, n_problems=0, views=dev["views"][:0]))
    ctx.synchronize()
    assert (out.result.cpu().numpy() == 0x5A).all()
    with pytest.raises(binding.OrbError) as e:
        ctx.pnp(sc["view"], sc["points"], sc["kp"], sc["idx"], binding.pnp_params(chi2=nan))
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "chi2" in e.value.message
    # the context is usable after every refusal; the host form with skip bytes and without rows
    p = NC.CASES[0]["params"]
    _check("after the refusals", _run(ctx, dev, 1, NC.ROWS, NC.ROWS, p), 0, NC.reference(0, 0))
    skip = np.zeros(len(sc["points"]), np.uint8)
    skip[sc["idx"][sc["inlier_rows"][:3]]] = 1
    flags, res = ctx.pnp(sc["view"], sc["points"], sc["kp"], sc["idx"], _params(binding, p), skip=skip)
    _check("host form with skip bytes", (flags[None], np.array([res])), 0, _restatement(dict(sc, skip=skip), p, 0))
    flags, res = ctx.pnp(sc["view"], sc["points"][:0], sc["kp"][:0], sc["idx"][:0], _params(binding, p))
    assert len(flags) == 0 and (res["state"], res["n_corr"], res["iteration"]) == (1, 0, -1)


def test_stages_and_their_byte_figures(ctx):
    """the four stages of a call with their algorithmic bytes; stats() reads at most 32 stages per context, so the context is the
    module's own after a reset and only the pnp_ stages are looked at"""
    scenes = [NC.case_scene(0), NC.case_scene(1)]
    dev = _upload(scenes, NC.ROWS, NC.ROWS)
    p = dict(NC.CASES[0]["params"], max_iterations=40)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        _run(ctx, dev, 2, NC.ROWS, NC.ROWS, p, skip=True)
        stats = {s["name"]: s for s in ctx.stats() if s["name"].startswith("pnp_")}
    finally:
        ctx.profile(False)
    n, nr, nh, hb = 2, 2 * NC.ROWS, 2 * 40, 2
    want = {"pnp_gather": nr * (4 + 4 + 32 + 24 + 1 + 32) + n * 4, "pnp_model": nh * (6 * 28 + 64 + 96 + 4),
            "pnp_count": nr * 24 * hb + nh * (64 + 4), "pnp_finish": nh * 4 + nr * (4 + 1 + 24) + n * (64 + 96 + 128)}
    assert list(stats) == list(want)
    for name, b in want.items():
        assert stats[name]["launches"] == 1 and stats[name]["algorithmic_bytes"] == b and stats[name]["total_ms"] > 0, (name, stats[name])
