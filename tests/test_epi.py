"""GPU parity of the epipolar search (ss_match_epi_pairs_device, ss_match_epi_batch_device) and of the triangulation
(ss_triangulate_pairs_device, ss_triangulate_batch_device) against tests/epi_ref.py: bit for bit, no tolerance -- idx and d1 of every
row, every summary field, the info record of every row, the compact block of map points with its descriptors and rows, in order.
Every output starts prefilled with a pattern no result has; rows past the queries must be "none", rows past the points untouched.
tests/test_epi_ref.py asserts on the reference that the shared cases are live."""
import numpy as np
import pytest

import bow_cases as BC
import epi_cases as EC
import epi_ref as E
import guided_cases as G
import proj_cases as PC
import proj_ref as P
from test_guided import _extract

pytestmark = pytest.mark.gpu
FILL = 0x5A


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


def _filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=_dev())


class SearchOut:
    def __init__(self, n, rows):
        self.n, self.rows = n, rows
        self.idx, self.d1, self.summary = _filled(n, rows * 4), _filled(n, rows * 2), _filled(n, 40)
        _sync()

    def ptrs(self):
        return self.idx.data_ptr(), self.d1.data_ptr(), self.summary.data_ptr()

    def host(self):
        from send_slam_amd import binding
        summ = self.summary.cpu().numpy().copy().view(binding.EPI_SUMMARY_DTYPE).reshape(self.n)
        return (self.idx.cpu().numpy().copy().view(np.int32), self.d1.cpu().numpy().copy().view(np.uint16),
                [{f: int(s[f]) for f in E.EPI_SUMMARY_FIELDS} for s in summ])


class TriOut:
    def __init__(self, n, rows):
        self.n, self.rows = n, rows
        self.info, self.points, self.desc = _filled(n, rows * 16), _filled(n, rows * 32), _filled(n, rows * 32)
        self.prows, self.npts, self.summary = _filled(n, rows * 8), _filled(n * 4), _filled(n, 64)
        _sync()

    def ptrs(self):
        return tuple(t.data_ptr() for t in (self.info, self.points, self.desc, self.prows, self.npts, self.summary))

    def host(self):
        from send_slam_amd import binding
        n, rows = self.n, self.rows
        summ = self.summary.cpu().numpy().copy().view(binding.TRI_SUMMARY_DTYPE).reshape(n)
        return (self.info.cpu().numpy().copy().view(binding.TRI_INFO_DTYPE).reshape(n, rows),
                self.points.cpu().numpy().copy().view(binding.MAP_POINT_DTYPE).reshape(n, rows), self.desc.cpu().numpy().copy().reshape(n, rows, 32),
                self.prows.cpu().numpy().copy().view(np.int32).reshape(n, rows, 2), self.npts.cpu().numpy().copy().view(np.int32),
                [dict({f: int(s[f]) for f in E.TRI_SUMMARY_FIELDS[:-1]}, n_state=[int(v) for v in s["n_state"]]) for s in summ])


def _check_search(tag, got, b, want):
    idx, d1, summ = got
    widx, wd1, wsumm = want
    n = len(widx)
    assert summ[b] == wsumm, f"{tag}: summary {summ[b]} != {wsumm}"
    for name, g, w in (("idx", idx[b], widx), ("d1", d1[b], wd1)):
        bad = np.flatnonzero(g[:n] != w)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {g[:n][bad[:8]]} != {w[bad[:8]]}"
    assert (idx[b][n:] == -1).all() and (d1[b][n:] == E.NONE).all(), f"{tag}: rows past the queries are not 'none'"


def _check_tri(tag, got, b, want):
    info, points, desc, prows, npts, summ = got
    winfo, wpts, wdesc, wrows, wsumm = want
    n, m = len(winfo), len(wpts)
    assert summ[b] == wsumm, f"{tag}: summary {summ[b]} != {wsumm}"
    assert npts[b] == m == wsumm["n_points"], f"{tag}: n_points {npts[b]} != {m}"
    for name in E.TRI_INFO_DTYPE.names:
        bad = np.flatnonzero(info[b][name][:n].view(np.int32) != winfo[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: info.{name} differs at rows {bad[:8]}: {info[b][name][:n][bad[:8]]} != {winfo[name][bad[:8]]}"
    assert info[b][n:].tobytes() == E.none_info(len(info[b]) - n).tobytes(), f"{tag}: rows past the queries are not 'none'"
    assert np.array_equal(prows[b][:m], wrows), f"{tag}: point rows differ"
    for name in E.MAP_POINT_DTYPE.names:
        bad = np.flatnonzero(points[b][name][:m].view(np.int32) != wpts[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: point.{name} differs at points {bad[:8]}: {points[b][name][:m][bad[:8]]} != {wpts[name][bad[:8]]}"
    assert np.array_equal(desc[b][:m], wdesc), f"{tag}: point descriptors differ"
    for name, arr in (("points", points[b][m:]), ("descriptors", desc[b][m:]), ("rows", prows[b][m:])):
        assert (np.ascontiguousarray(arr).view(np.uint8) == FILL).all(), f"{tag}: {name} past n_points were written"


def _upload(frames, rows):
    """frames: dicts pair q_kp q_desc q_node [q_taken] t_kp t_desc t_node [t_taken] [nq] [nt] [idx] -> device arrays [n][rows] of the
    pairs form.  Rows past the data repeat row 0 of their side: they would match if they were read."""
    from send_slam_amd import binding
    n = len(frames)
    host = {"q_desc": np.zeros((n, rows, 32), np.uint8), "t_desc": np.zeros((n, rows, 32), np.uint8), "q_kp": np.zeros((n, rows), binding.KP_DTYPE),
            "t_kp": np.zeros((n, rows), binding.KP_DTYPE), "q_node": np.zeros((n, rows), np.int32), "t_node": np.zeros((n, rows), np.int32),
            "q_taken": np.zeros((n, rows), np.uint8), "t_taken": np.zeros((n, rows), np.uint8), "nq": np.zeros(n, np.int32), "nt": np.zeros(n, np.int32),
            "idx": np.full((n, rows), -1, np.int32)}
    for b, f in enumerate(frames):
        for side, cnt in (("q", "nq"), ("t", "nt")):
            k = len(f[side + "_kp"])
            host[cnt][b] = f.get(cnt, k)
            for name in ("desc", "kp", "node", "taken"):
                src = f.get(f"{side}_{name}")
                if src is None:
                    continue
                host[f"{side}_{name}"][b, :k] = src
                if k and name != "taken":
                    host[f"{side}_{name}"][b, k:] = src[0]
        if "idx" in f:
            host["idx"][b, :len(f["idx"])] = f["idx"]
    dev = {k: _to_dev(v) for k, v in host.items()}
    dev["pairs"] = np.concatenate([np.asarray(f["pair"]).reshape(1) for f in frames])
    _sync()
    return dev


def _search(ctx, dev, n, rows, params, taken=True):
    out = SearchOut(n, rows)
    ctx.match_epi_pairs_device(dev["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), dev["q_node"].data_ptr(), dev["nq"].data_ptr(), dev["t_desc"].data_ptr(),
                               dev["t_kp"].data_ptr(), dev["t_node"].data_ptr(), dev["nt"].data_ptr(), n, rows, dev["pairs"][:n], params, *out.ptrs(),
                               d_q_taken=dev["q_taken"].data_ptr() if taken else 0, d_t_taken=dev["t_taken"].data_ptr() if taken else 0)
    ctx.synchronize()
    return out


def _triangulate(ctx, dev, n, rows, tp, d_idx=None):
    out = TriOut(n, rows)
    ctx.triangulate_pairs_device(dev["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_kp"].data_ptr(), dev["nt"].data_ptr(),
                                 dev["idx"].data_ptr() if d_idx is None else d_idx, n, rows, dev["pairs"][:n], tp, *out.ptrs())
    ctx.synchronize()
    return out


@pytest.fixture(scope="module")
def ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=3) as c:
        yield c


# ---- the boundary tables ----------------------------------------------------------------------------------------------------------------
def _check_table_on(c, sc, tag):
    """tests 1 - 3 through the pairs form: couple k is query row k and train row k of a node of their own, so idx[k] is k iff the
    couple passes; and through the host twin"""
    from send_slam_amd import binding
    rng = np.random.Generator(np.random.PCG64(0xC4EC))
    table = EC.check_table(sc)
    passed = 0
    for coarse in (False, True):
        rows_ = [r for r in table if r[2] == coarse]
        frames, wants = [], []
        for name, pair, _, k1, k2, expect in rows_:
            n = len(k1)
            d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            node = np.arange(n, dtype=np.int32) + 5
            frames.append({"pair": pair, "q_kp": k1, "q_desc": d, "q_node": node, "t_kp": k2, "t_desc": d, "t_node": node})
            want = E.match(pair, k1, d, node, k2, d, node, sc, 256, coarse)
            codes = np.array([E.check(pair, coarse, sc, E.line_of(pair, k1["x"][i], k1["y"][i]), k2["x"][i], k2["y"][i], k2["octave"][i]) for i in range(n)])
            assert np.array_equal(want[0] >= 0, codes == 0) and (expect is None or list(codes) == expect), name
            assert list(binding.epi_check_host(pair, binding.epi_params(coarse=coarse), sc, k1, k2)) == list(codes), name
            wants.append(want)
        rows = max(len(f["q_kp"]) for f in frames) + 3
        got = _search(c, _upload(frames, rows), len(frames), rows, binding.epi_params(th=256, coarse=coarse, orientation=0), taken=False).host()
        for b, (name, *_) in enumerate(rows_):
            _check_search(f"{tag}: {name}", got, b, wants[b])
            passed += wants[b][2]["n_accepted"]
    return passed


def _tri_table_on(c, sc, tag):
    """steps 1 - 9 through the pairs form (couple k is query row k with idx[k] = k) and the host twin, one call per parameter set"""
    from send_slam_amd import binding
    table = EC.tri_table(sc)
    groups = {}
    for row in table:
        groups.setdefault(repr(sorted(row[2].items())), []).append(row)
    states = set()
    for rows_ in groups.values():
        tp = rows_[0][2]
        frames, wants = [], []
        for name, pair, _, k1, k2, expect in rows_:
            n = len(k1)
            d = np.full((n, 32), len(frames), np.uint8)
            frames.append({"pair": pair, "q_kp": k1, "q_desc": d, "t_kp": k2, "idx": np.arange(n)})
            want = E.triangulate_rows(pair, tp, sc, k1, d, k2, np.arange(n))
            assert expect is None or list(want[0]["state"]) == expect, name
            gp, gi = binding.triangulate_host(pair, binding.tri_params(**tp), sc, k1, k2)
            assert gi.tobytes() == want[0].tobytes() and gp[gi["state"] == 0].tobytes() == want[1].tobytes(), name
            wants.append(want)
            states |= set(int(v) for v in want[0]["state"])
        rows = max(len(f["q_kp"]) for f in frames) + 2
        got = _triangulate(c, _upload(frames, rows), len(frames), rows, binding.tri_params(**tp)).host()
        for b, (name, *_) in enumerate(rows_):
            _check_tri(f"{tag}: {name}", got, b, wants[b])
    return states


def test_boundary_tables(ctx):
    """every threshold of the search's tests 1 - 3 and of the triangulation's steps 1 - 9 with np.nextafter on both sides (all but d1 > 0 && d2 > 0), den == 0,
    NaN and infinite pairs and keypoints, every state 1 .. 10"""
    assert _check_table_on(ctx, EC.scale(), "check table") > 20
    assert _tri_table_on(ctx, EC.scale(), "triangulation table") == set(range(11))


@pytest.mark.parametrize("name", ["one_level", "sixteen_levels"])
def test_boundary_tables_under_other_pyramid_tables(name):
    """a pyramid of one level (sigma2 1 everywhere, min_dist == max_dist) and of SS_MAX_LEVELS levels of scale 1.1"""
    from send_slam_amd import binding
    factor, n_levels = PC.PYRAMIDS[name]
    sc = PC.scale_table(factor, n_levels)
    with binding.OrbContext(0, n_features=G.NF, scale_factor=factor, n_levels=n_levels) as c:
        assert _check_table_on(c, sc, name) > 5
        assert {0, 1, 5, 6, 8, 9, 10} <= _tri_table_on(c, sc, name)


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
SCENE_ROWS = 483  # no multiple of the 64 query rows of a workgroup


@pytest.fixture(scope="module")
def scene_arrays():
    frames = [dict(s, idx=EC.scene_matches(k)) for k, s in enumerate(EC.scenes())]
    assert all(len(f["q_kp"]) <= SCENE_ROWS for f in frames)
    return _upload(frames, SCENE_ROWS)


@pytest.mark.parametrize("combo", EC.COMBOS, ids=EC.combo_name)
def test_scenes(ctx, scene_arrays, combo):
    from send_slam_amd import binding
    n = len(EC.SCENES)
    got = _search(ctx, scene_arrays, n, SCENE_ROWS, EC.combo_params(binding, combo), taken=combo["taken"]).host()
    for k in range(n):
        _check_search(f"scene {k} {EC.combo_name(combo)}", got, k, EC.scene_reference(k, combo))
    assert sum(s["n_final"] for s in got[2]) > 300


def test_scene_triangulation(ctx, scene_arrays):
    """the matches of the coarse search plus caller-made ones: idx entries of -7 and n_train are no match"""
    from send_slam_amd import binding
    n = len(EC.SCENES)
    got = _triangulate(ctx, scene_arrays, n, SCENE_ROWS, binding.tri_params(**EC.TRI)).host()
    for k in range(n):
        want = EC.scene_triangulation(k)
        _check_tri(f"scene {k}", got, k, want)
        m = EC.scene_matches(k)
        for bad in (-7, len(EC.scenes()[k]["t_kp"])):
            assert (got[0][k]["state"][np.flatnonzero(m == bad)] == -1).all()
        assert want[4]["n_points"] > 150 and len(set(want[0]["state"])) >= 5


def test_search_then_triangulate_then_project(ctx, scene_arrays):
    """end to end on the device: the search's idx feeds the triangulation, whose block ss_match_proj_pairs_device reads as it was
    written (point_rows = rows); the result equals proj_ref.match on the reference's block"""
    from send_slam_amd import binding
    n, rows = len(EC.SCENES), SCENE_ROWS
    combo = dict(coarse=False, one_to_one=True, orientation=1, taken=True)
    found = _search(ctx, scene_arrays, n, rows, EC.combo_params(binding, combo))
    tri = _triangulate(ctx, scene_arrays, n, rows, binding.tri_params(**EC.TRI), d_idx=found.idx.data_ptr())
    views, thirds = [], []
    for k, s in enumerate(EC.scenes()):
        rng = np.random.Generator(np.random.PCG64(0xE91 + k))  # the scene's own seed: its first draws are the depths of the rows
        p3 = EC.pose((k + 2) % 3)
        views.append(P.view_init(*EC.CAM, G.W, G.H, p3[0], p3[1], PC.BF))
        k3, _ = EC.second_view(rng, s["q_kp"], s["poses"][0], p3)
        thirds.append({"pair": s["pair"], "q_kp": s["q_kp"][:0], "q_desc": s["q_desc"][:0], "t_kp": k3, "t_desc": PC.desc_near(rng, s["q_desc"])})
    third = _upload(thirds, rows)
    import torch
    idx, d1, d2 = (torch.full((n, rows), 0x5A5A, dtype=t, device=_dev()) for t in (torch.int32, torch.int16, torch.int16))
    proj, summ = _filled(n, rows * 32), _filled(n, 32)
    _sync()
    pp = binding.proj_params(th=3.0, one_to_one=True, extent_w=G.W, extent_h=G.H)
    ctx.match_proj_pairs_device(tri.points.data_ptr(), tri.desc.data_ptr(), tri.npts.data_ptr(), n, rows, third["t_desc"].data_ptr(),
                                third["t_kp"].data_ptr(), third["nt"].data_ptr(), n, rows, np.concatenate([v.reshape(1) for v in views]), pp,
                                idx.data_ptr(), d1.data_ptr(), d2.data_ptr(), proj.data_ptr(), summ.data_ptr())
    ctx.synchronize()
    got_tri = tri.host()
    hidx, hd1, hd2 = idx.cpu().numpy(), d1.cpu().numpy().view(np.uint16), d2.cpu().numpy().view(np.uint16)
    hproj = proj.cpu().numpy().copy().view(binding.PROJ_POINT_DTYPE).reshape(n, rows)
    hsumm = summ.cpu().numpy().copy().view(binding.PROJ_SUMMARY_DTYPE).reshape(n)
    for k, s in enumerate(EC.scenes()):
        ref_idx = EC.scene_reference(k, combo)[0]
        _check_search(f"scene {k}", found.host(), k, EC.scene_reference(k, combo))
        want_tri = E.triangulate_rows(s["pair"], EC.TRI, EC.scale(), s["q_kp"], s["q_desc"], s["t_kp"], ref_idx)
        _check_tri(f"scene {k}", got_tri, k, want_tri)
        w = P.match(views[k], want_tri[1], want_tri[2], thirds[k]["t_kp"], thirds[k]["t_desc"], EC.scale(), th=3.0, one_to_one=True)
        m = len(want_tri[1])
        assert {f: int(hsumm[k][f]) for f in P.SUMMARY_FIELDS} == w[4], (k, w[4])
        assert np.array_equal(hidx[k][:m], w[0]) and np.array_equal(hd1[k][:m], w[1]) and np.array_equal(hd2[k][:m], w[2])
        assert hproj[k][:m].tobytes() == w[3].tobytes()
        assert w[4]["n_in_view"] > 50 and w[4]["n_unique"] > 30, w[4]


# ---- odd cameras, per pair and per side ---------------------------------------------------------------------------------------------------
def test_three_camera_pairs_per_call(ctx):
    """one call whose pairs are (camera A, camera B), (B, A) and (square, A), their records made by ss_epi_pair_init: the search, the
    triangulation of the search's own idx on the device, and the triangulation of looser matches; every idx, d1, info record, point,
    descriptor and row couple.  tests/test_epi_ref.py shows that exchanging fx and fy, cx and cy, the sides or the pairs changes
    these bytes"""
    from send_slam_amd import binding
    scenes = EC.camera_scenes()
    frames = [dict(s, pair=np.frombuffer(bytes(EC.library_pair(binding, *s["poses"], *s["cams"])), E.PAIR_DTYPE)[0], idx=EC.camera_matches(k))
              for k, s in enumerate(scenes)]
    assert len({f["pair"].tobytes() for f in frames}) == 3 and all(f["pair"].tobytes() == s["pair"].tobytes() for f, s in zip(frames, scenes))
    n, rows = 3, SCENE_ROWS
    dev = _upload(frames, rows)
    found = _search(ctx, dev, n, rows, EC.combo_params(binding, EC.CAMERA_COMBO))
    tri = _triangulate(ctx, dev, n, rows, binding.tri_params(**EC.TRI), d_idx=found.idx.data_ptr()).host()
    loose = _triangulate(ctx, dev, n, rows, binding.tri_params(**EC.TRI)).host()
    got = found.host()
    for k in range(n):
        want, want_tri = EC.camera_reference(k)
        _check_search(f"cameras, pair {k}", got, k, want)
        _check_tri(f"cameras, pair {k}, the search's matches", tri, k, want_tri)
        _check_tri(f"cameras, pair {k}, looser matches", loose, k, EC.camera_triangulation(k))
        assert want[2]["n_final"] > 150 and want_tri[4]["n_points"] > 150


# ---- counts, capacity, compaction -----------------------------------------------------------------------------------------------------
def test_counts_on_both_sides(ctx):
    """0, 1, 63, 64, 65 rows, counts above the rows (clamped) and negative (0), at 65 rows per frame: every frame of the call holds all
    the rows, live, whatever its counts say"""
    from send_slam_amd import binding
    base, rows = EC.count_frame(), EC.COUNT_ROWS
    frames = [dict(base, nq=a, nt=b, idx=EC.count_reference(a, b)[0]) for a, b in EC.COUNTS]
    dev = _upload(frames, rows)
    got = _search(ctx, dev, len(frames), rows, EC.combo_params(binding, EC.COUNT_COMBO)).host()
    tri = _triangulate(ctx, dev, len(frames), rows, binding.tri_params(**EC.TRI)).host()
    for b, (nq, nt) in enumerate(EC.COUNTS):
        want = EC.count_reference(nq, nt)
        _check_search(f"counts {nq} / {nt}", got, b, want[:3])
        _check_tri(f"counts {nq} / {nt}", tri, b, want[3])
    assert EC.count_reference(65, 65)[2]["n_accepted"] > 20


def test_full_capacity_pairs(ctx):
    """two pairs of SS_GUIDED_MAX_ROWS rows on both sides under a small vocabulary: contested train rows on both sides of row 8192, so
    both passes of the conflict table run"""
    from send_slam_amd import binding
    frames = EC.capacity_pairs()
    dev = _upload(frames, EC.CAP_ROWS)
    got = _search(ctx, dev, 2, EC.CAP_ROWS, binding.epi_params(th=50, coarse=True, one_to_one=True, orientation=2)).host()
    for b in range(2):
        want = EC.capacity_reference(b, coarse=True)
        _check_search(f"capacity pair {b}", got, b, want)
        assert want[2]["n_unique"] < want[2]["n_accepted"] - 500
    got = _search(ctx, dev, 1, EC.CAP_ROWS, binding.epi_params(th=50, coarse=False, one_to_one=True, orientation=2)).host()
    _check_search("capacity pair 0, with the line test", got, 0, EC.capacity_reference(0, coarse=False))


def test_compaction_around_the_chunk(ctx):
    """0, 1, 1023, 1024 and 1025 points, once at the head of the rows (one chunk) and once spread over two chunks and more: the
    compact outputs equal the reference's, order included"""
    from send_slam_amd import binding
    b = EC.compact_base()
    cases = [(c, lay) for c in EC.COMPACT_COUNTS for lay in ("head", "spread")]
    wants = [EC.compact_case(c, lay) for c, lay in cases]
    frames = [{"pair": b["pair"], "q_kp": b["q_kp"], "q_desc": b["q_desc"], "t_kp": b["t_kp"], "idx": w[0]} for w in wants]
    rows = EC.COMPACT_ROWS + 1
    got = _triangulate(ctx, _upload(frames, rows), len(frames), rows, binding.tri_params(**EC.TRI)).host()
    for k, (c, lay) in enumerate(cases):
        _check_tri(f"{c} points, {lay}", got, k, wants[k][1:])
        assert got[4][k] == c


# ---- the batch forms ----------------------------------------------------------------------------------------------------------------------
BATCH = ["synth_t0", "synth_t1", "synth_t2", "flat", "synth_t3", "dots"]
BATCH_SRC = [-1, 0, 0, 0, 3, 5]  # frame 0 is searched by two; flat has no keypoints (a query side, then a train side); dots against itself
BATCH_COMBOS = [dict(coarse=False, one_to_one=False, orientation=1, taken=False), dict(coarse=True, one_to_one=True, orientation=2, taken=True)]


def _batch_pairs():
    return [EC.make_pair(EC.pose(b % 3), EC.pose((b + 1) % 3) if t != b else EC.pose("forward")) for b, t in enumerate(BATCH_SRC)]


def _batch_reference(names, src, pairs, combo, taken):
    wants = []
    for b, t in enumerate(src):
        qk, qd = G.features(names[b])
        qn = BC.frame_transform(EC.VOC, names[b], EC.LEVELSUP)[1]
        tk, td = G.features(names[t]) if t >= 0 else (None, None)
        tn = BC.frame_transform(EC.VOC, names[t], EC.LEVELSUP)[1] if t >= 0 else []
        found = E.match(pairs[b], qk, qd, qn, tk, td, tn, EC.scale(), 50, combo["coarse"], combo["one_to_one"], combo["orientation"],
                        taken[b][:len(qk)] if combo["taken"] else None, taken[t][:len(tk)] if (combo["taken"] and t >= 0) else None, exclude_self=t == b)
        tri = E.triangulate_rows(pairs[b], EC.TRI, EC.scale(), qk, qd, tk, found[0])
        wants.append((found, tri))
    return wants


def _batch_run(binding, names, src, pairs, combo, taken):
    from test_bow import _set, Transformed
    n = len(names)
    with binding.OrbContext(0, n_features=G.NF, max_batch=n) as c:
        _, kcap = _extract(c, names)
        _set(c, BC.vocab(EC.VOC))
        out = SearchOut(n, kcap)
        with pytest.raises(binding.OrbError) as e:  # no transform of this batch yet
            c.match_epi_batch_device(pairs, EC.combo_params(binding, combo), *out.ptrs(), train_src=src)
        assert e.value.code == binding.SS_ERR_STATE and "ss_bow_transform_batch_device" in e.value.message
        tr = Transformed(n, kcap)
        c.bow_transform_batch_device(EC.LEVELSUP, *tr.ptrs())
        d_taken = _to_dev(np.ascontiguousarray(taken[:, :kcap]))
        _sync()
        c.match_epi_batch_device(pairs, EC.combo_params(binding, combo), *out.ptrs(), train_src=src, d_taken=d_taken.data_ptr() if combo["taken"] else 0)
        tri = TriOut(n, kcap)
        c.triangulate_batch_device(out.idx.data_ptr(), pairs, binding.tri_params(**EC.TRI), *tri.ptrs(), train_src=src)
        c.synchronize()
        for bad in (-2, n):
            t2 = list(src)
            t2[2] = bad
            for call in (lambda: c.match_epi_batch_device(pairs, EC.combo_params(binding, combo), *out.ptrs(), train_src=t2),
                         lambda: c.triangulate_batch_device(out.idx.data_ptr(), pairs, binding.tri_params(**EC.TRI), *tri.ptrs(), train_src=t2)):
                with pytest.raises(binding.OrbError) as e:
                    call()
                assert e.value.code == binding.SS_ERR_INVALID_ARG and "train_src[2]" in e.value.message
        c.synchronize()
        return out.host(), tri.host(), kcap


def _taken(n):
    return (np.random.Generator(np.random.PCG64(0x7A4E)).random((n, 4096)) < 0.1).astype(np.uint8)


@pytest.mark.parametrize("combo", BATCH_COMBOS, ids=EC.combo_name)
def test_batch_forms(combo, monkeypatch):
    """after ss_bow_transform_batch_device (SS_ERR_STATE before it): a frame searched by two, a frame without keypoints on either side,
    no train, the self pair; the triangulation of the search's own idx on the same table"""
    from send_slam_amd import binding
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    pairs, taken = _batch_pairs(), _taken(len(BATCH))
    found, tri, kcap = _batch_run(binding, BATCH, BATCH_SRC, pairs, combo, taken)
    wants = _batch_reference(BATCH, BATCH_SRC, pairs, combo, taken)
    for b, (wf, wt) in enumerate(wants):
        _check_search(f"frame {b} against {BATCH_SRC[b]}", found, b, wf)
        _check_tri(f"frame {b} against {BATCH_SRC[b]}", tri, b, wt)
    assert wants[1][0][2]["n_accepted"] > 5 and wants[2][0][2]["n_accepted"] > 5 and wants[3][0][2]["n_query"] == 0 and wants[4][0][2]["n_train"] == 0
    nq = wants[5][0][2]["n_query"]
    assert not (found[0][5][:nq] == np.arange(nq)).any()


def test_flagged_frames_are_voided_in_the_batch_forms(monkeypatch):
    """SENDSLAM_TEST_FLAG_BATCH=1: frame 1 is flagged although it has keypoints.  The pair that queries from it and the pair that
    trains on it carry the status, zero counts, all rows "none" and no point; the other pairs are what the reference gives"""
    from send_slam_amd import binding
    names, src = ["synth_t0", "synth_t1", "synth_t2", "synth_t3"], [-1, 0, 1, 0]
    pairs = [EC.make_pair(EC.pose(b % 3), EC.pose((b + 1) % 3)) for b in range(4)]
    combo, taken = BATCH_COMBOS[1], _taken(4)
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1")
    found, tri, kcap = _batch_run(binding, names, src, pairs, combo, taken)
    wants = _batch_reference(names, src, pairs, combo, taken)
    for b in range(4):
        if b in (1, 2):
            _check_search(f"pair {b} voided", found, b, E.voided(0, binding.SS_ERR_OVERFLOW))
            none = E.triangulate_rows(pairs[b], EC.TRI, EC.scale(), G.features(names[b])[0][:0], np.zeros((0, 32), np.uint8), None, [])
            _check_tri(f"pair {b} voided", tri, b, none[:4] + (dict(none[4], status=binding.SS_ERR_OVERFLOW),))
        else:
            _check_search(f"pair {b}", found, b, wants[b][0])
            _check_tri(f"pair {b}", tri, b, wants[b][1])
    assert wants[3][0][2]["n_accepted"] > 5


# ---- refused arguments --------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_context_usable(ctx, scene_arrays):
    from send_slam_amd import binding
    dev, n, rows = scene_arrays, len(EC.SCENES), SCENE_ROWS
    out, tri = SearchOut(n, rows), TriOut(n, rows)
    good = dict(d_q=dev["q_desc"].data_ptr(), d_q_kp=dev["q_kp"].data_ptr(), d_q_node=dev["q_node"].data_ptr(), d_nq=dev["nq"].data_ptr(),
                d_t=dev["t_desc"].data_ptr(), d_t_kp=dev["t_kp"].data_ptr(), d_t_node=dev["t_node"].data_ptr(), d_nt=dev["nt"].data_ptr(), n_frames=n,
                rows_per_frame=rows, pairs=dev["pairs"], params=binding.epi_params(), d_idx=out.idx.data_ptr(), d_d1=out.d1.data_ptr(),
                d_summary=out.summary.data_ptr())
    bad = [dict(rows_per_frame=binding.SS_GUIDED_MAX_ROWS + 1), dict(rows_per_frame=0), dict(params=binding.epi_params(th=-1)),
           dict(params=binding.epi_params(th=257)), dict(params=binding.epi_params(orientation=3))]
    bad += [{k: 0} for k in good if k.startswith("d_")]
    for kw in bad:
        with pytest.raises(binding.OrbError) as e:
            ctx.match_epi_pairs_device(**dict(good, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    lib = binding.load()
    import ctypes as C
    assert lib.ss_match_epi_pairs_device(ctx._h, *[C.c_void_p(1)] * 10, n, rows, None, C.byref(binding.epi_params()), *[C.c_void_p(1)] * 3) == binding.SS_ERR_INVALID_ARG
    tgood = dict(d_q=dev["q_desc"].data_ptr(), d_q_kp=dev["q_kp"].data_ptr(), d_nq=dev["nq"].data_ptr(), d_t_kp=dev["t_kp"].data_ptr(),
                 d_nt=dev["nt"].data_ptr(), d_idx=dev["idx"].data_ptr(), n_frames=n, rows_per_frame=rows, pairs=dev["pairs"],
                 params=binding.tri_params(**EC.TRI))
    tgood.update(zip(("d_info", "d_points", "d_point_desc", "d_point_rows", "d_n_points", "d_summary"), tri.ptrs()))
    for kw in [dict(rows_per_frame=binding.SS_GUIDED_MAX_ROWS + 1), dict(rows_per_frame=0)] + [{k: 0} for k in tgood if k.startswith("d_")]:
        with pytest.raises(binding.OrbError) as e:
            ctx.triangulate_pairs_device(**dict(tgood, **kw))
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    # nothing was written, and the next good calls match the reference
    assert (out.idx.cpu().numpy() == FILL).all() and (tri.info.cpu().numpy() == FILL).all()
    combo = dict(coarse=False, one_to_one=False, orientation=1, taken=False)
    ctx.match_epi_pairs_device(**good)
    ctx.triangulate_pairs_device(**tgood)
    ctx.synchronize()
    for k in range(n):
        _check_search(f"scene {k} after the refusals", out.host(), k, EC.scene_reference(k, combo))
        _check_tri(f"scene {k} after the refusals", tri.host(), k, EC.scene_triangulation(k))
