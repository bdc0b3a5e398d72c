"""CPU tests of the epipolar search and the triangulation as tests/epi_ref.py states them, and of their C ABI surface:
ss_epi_pair_init and the host twins ss_epi_check_host / ss_triangulate_host (the text the kernels compile) against the reference
bit for bit, struct layouts, the DLT against LAPACK's SVD, upstream's loops against the key rule, the stand-alone sanitizer run of
the steps, and that the shared cases are what they claim to be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import epi_cases as EC
import epi_ref as E
import guided_cases as G
import proj_cases as PC
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")
f32 = np.float32
NAMES = ["ss_epi_pair_init", "ss_epi_check_host", "ss_triangulate_host", "ss_match_epi_pairs_device", "ss_match_epi_batch_device",
         "ss_triangulate_pairs_device", "ss_triangulate_batch_device"]


def _same(got, want, tag):
    """two structured arrays of one dtype, bit for bit (NaN bits included)"""
    assert got.dtype == want.dtype and len(got) == len(want), tag
    for name in got.dtype.names:
        a, b = np.ascontiguousarray(got[name]).view(np.int32), np.ascontiguousarray(want[name]).view(np.int32)
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {got[name][bad[:8]]} != {want[name][bad[:8]]}"


def test_symbols_structs_and_constants(tmp_path):
    text = open(HEADER).read()
    lib = binding.load()
    for n in NAMES:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("match_epi_pairs_device", "match_epi_batch_device", "triangulate_pairs_device", "triangulate_batch_device"):
        assert callable(getattr(binding.OrbContext, m))
    for f in ("epi_params", "tri_params", "epi_pair", "epi_check_host", "triangulate_host"):
        assert callable(getattr(binding, f))
    assert C.sizeof(binding.EpiPair) == 384 and C.sizeof(binding.EpiParams) == 16 and C.sizeof(binding.EpiSummary) == 40
    assert C.sizeof(binding.TriParams) == 32 and C.sizeof(binding.TriSummary) == 64
    assert binding.EPI_PAIR_DTYPE == E.PAIR_DTYPE and binding.EPI_PAIR_DTYPE.itemsize == 384
    assert binding.TRI_INFO_DTYPE == E.TRI_INFO_DTYPE and binding.TRI_INFO_DTYPE.itemsize == 16
    assert binding.EPI_SUMMARY_DTYPE.itemsize == 40 and binding.TRI_SUMMARY_DTYPE.itemsize == 64
    assert tuple(n for n, _ in binding.EpiSummary._fields_) == E.EPI_SUMMARY_FIELDS
    assert tuple(n for n, _ in binding.TriSummary._fields_) == E.TRI_SUMMARY_FIELDS
    assert tuple(n for n, _ in binding.EpiPair._fields_) == E.PAIR_DTYPE.names
    assert [E.PAIR_DTYPE.fields[n][1] for n in ("ex", "epipole_test", "rcw1", "ow1", "rcw2", "fx1", "fx2", "invfy2")] == [36, 44, 48, 144, 168, 288, 336, 376]
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_epi_pair) == 384, "pair");\n'
                   '_Static_assert(sizeof(ss_epi_params) == 16 && sizeof(ss_epi_summary) == 40, "search");\n'
                   '_Static_assert(sizeof(ss_tri_params) == 32 && sizeof(ss_tri_info) == 16 && sizeof(ss_tri_summary) == 64, "triangulation");\n'
                   '_Static_assert(offsetof(ss_epi_pair, ex) == 36 && offsetof(ss_epi_pair, epipole_test) == 44 && offsetof(ss_epi_pair, rcw1) == 48, "pair floats");\n'
                   '_Static_assert(offsetof(ss_epi_pair, ow1) == 144 && offsetof(ss_epi_pair, rcw2) == 168 && offsetof(ss_epi_pair, fx1) == 288, "pair doubles");\n'
                   '_Static_assert(offsetof(ss_epi_pair, fx2) == 336 && offsetof(ss_epi_pair, invfy2) == 376, "pair cameras");\n'
                   '_Static_assert(offsetof(ss_epi_summary, n_geometric) == 16 && offsetof(ss_epi_summary, rot_bins) == 36, "summary fields");\n'
                   '_Static_assert(offsetof(ss_tri_params, far_limit) == 24 && offsetof(ss_tri_info, err2_sq) == 12, "fields");\n'
                   '_Static_assert(offsetof(ss_tri_summary, n_points) == 16 && offsetof(ss_tri_summary, n_state) == 20, "summary fields");\n'
                   '_Static_assert(sizeof(ss_map_point) == 32 && SS_TRI_SWEEPS == 6, "the block the projection search reads");\n'
                   '_Static_assert(SS_GUIDED_MAX_ROWS == 16384 && SS_ABI_VERSION == 5 && SS_MAX_LEVELS == 16, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5 and E.SWEEPS == 6


def _library_pair(cam1, p1, cam2, p2):
    return np.frombuffer(bytes(EC.library_pair(binding, p1, p2, cam1, cam2)), E.PAIR_DTYPE)[0]


def test_pair_init_agrees_with_its_restatement():
    rng = np.random.Generator(np.random.PCG64(0xE91F))
    cams = [EC.CAM, (517.3, 516.5, 318.6, 255.3)]
    poses = [EC.pose(k) for k in (0, 1, 2, None, "forward")] + [(PC.rot(*rng.normal(0, 1, 3)), tuple(rng.normal(0, 3, 3))) for _ in range(40)]
    seen = 0
    for a in range(len(poses)):
        for b in (a - 1, (a + 7) % len(poses)):
            cam1, cam2 = cams[a % 2], cams[b % 2]
            got, want = _library_pair(cam1, poses[a], cam2, poses[b]), E.pair_init(cam1, *poses[a], cam2, *poses[b])
            assert got.tobytes() == want.tobytes(), (a, b, got, want)
            assert np.abs(want["f12"]).max() == 1 and np.isfinite(want["f12"]).all()
            seen += int(want["epipole_test"])
    assert seen > 40
    # identical poses: no baseline, F is zero and the epipole is 0 / 0 (exactly so where R.R^T is exact; under a general rotation
    # the rounding of R12 leaves a baseline of a few ulp, and the pair is compared bit for bit like any other)
    for p in ((np.eye(3), (0.3, -0.2, 0.1)), (np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 0.0))):
        same = E.pair_init(EC.CAM, *p, EC.CAM, *p)
        assert _library_pair(EC.CAM, p, EC.CAM, p).tobytes() == same.tobytes()
        assert (same["f12"] == 0).all() and same["epipole_test"] == 0 and same["ex"] == 0 and same["ey"] == 0
    for p in poses[:8]:
        assert _library_pair(EC.CAM, p, EC.CAM, p).tobytes() == E.pair_init(EC.CAM, *p, EC.CAM, *p).tobytes()
    # pure sideways motion: the epipole is at infinity
    side = (np.eye(3), (0.0, 0.0, 0.0)), (np.eye(3), (-0.4, 0.0, 0.0))
    want = E.pair_init(EC.CAM, *side[0], EC.CAM, *side[1])
    assert _library_pair(EC.CAM, side[0], EC.CAM, side[1]).tobytes() == want.tobytes()
    assert want["epipole_test"] == 0 and want["ex"] == 0 and np.abs(want["f12"]).max() == 1
    assert list(want["f12"]) == [0, 0, 0, 0, 0, 1, 0, -1, 0] or list(want["f12"]) == [0, 0, 0, 0, 0, -1, 0, 1, 0]
    # a pose or a camera that is not finite: nothing matches
    for bad in ((np.eye(3), (np.nan, 0.0, 0.0)), (np.full((3, 3), np.inf), (0.0, 0.0, 0.0))):
        want = E.pair_init(EC.CAM, *bad, EC.CAM, *poses[1])
        assert _library_pair(EC.CAM, bad, EC.CAM, poses[1]).tobytes() == want.tobytes()
        assert (want["f12"] == 0).all() and want["epipole_test"] == 0
    want = E.pair_init((0.0, 300.0, 1.0, 1.0), *poses[0], EC.CAM, *poses[1])
    assert _library_pair((0.0, 300.0, 1.0, 1.0), poses[0], EC.CAM, poses[1]).tobytes() == want.tobytes() and (want["f12"] == 0).all()
    lib = binding.load()
    assert lib.ss_epi_pair_init(None, None, None, None, None, None, None) == binding.SS_ERR_INVALID_ARG


def _ref_check(pair, coarse, sc, k1, k2):
    return np.array([E.check(pair, coarse, sc, E.line_of(pair, k1["x"][i], k1["y"][i]), k2["x"][i], k2["y"][i], k2["octave"][i]) for i in range(len(k1))], np.uint8)


TABLES = {"default": None, "one_level": PC.PYRAMIDS["one_level"], "sixteen_levels": PC.PYRAMIDS["sixteen_levels"]}


def _table(name):
    return EC.scale() if TABLES[name] is None else PC.scale_table(*TABLES[name])


@pytest.mark.parametrize("pyramid", list(TABLES))
def test_check_table_through_the_host_twin(pyramid):
    """every threshold of tests 1 - 3 from both sides, den == 0, odd inputs; the expectation of a row is written in the table"""
    sc = _table(pyramid)
    codes = set()
    for name, pair, coarse, k1, k2, expect in EC.check_table(sc):
        want = _ref_check(pair, coarse, sc, k1, k2)
        got = binding.epi_check_host(pair, binding.epi_params(coarse=coarse), sc, k1, k2)
        assert list(got) == list(want), (name, got, want)
        assert expect is None or list(want) == expect, (name, want, expect)
        codes |= set(int(v) for v in want)
    assert codes == {0, 1, 2, 3}
    names = [r[0] for r in EC.check_table(sc)]
    assert sum(n.startswith("epipole disc") for n in names) == len(sc) == sum(n.startswith("line,") for n in names)


@pytest.mark.parametrize("pyramid", list(TABLES))
def test_triangulation_table_through_the_host_twin(pyramid):
    """every threshold of steps 1 - 9 from both sides (all but d1 > 0 && d2 > 0: unreachable on finite input) and every state 1 .. 10 (state -1 belongs to the rows without a match)"""
    sc = _table(pyramid)
    states = set()
    for name, pair, tp, k1, k2, expect in EC.tri_table(sc):
        info, pts, _ = E.triangulate_couples(pair, tp, sc, k1, k2)
        gp, gi = binding.triangulate_host(pair, binding.tri_params(**tp), sc, k1, k2)
        _same(gi, info, name)
        _same(gp, pts, name)
        assert expect is None or list(info["state"]) == expect, (name, info, expect)
        states |= set(int(v) for v in info["state"])
    assert states == set(range(11))
    # the sign tests have their two-sided rows, with the states written in the table: fail, fail / pass, pass on adjacent float32 values
    for name, st in (("cos at 0", 1), ("depth 1 at 0", 3), ("depth 2 at 0", 4)):
        got = [r[5][0] for r in EC.tri_table(sc) if r[0] == name]
        assert len(got) == 4 and [g == st for g in got] == [False, False, True, True], (name, got)
    rows = E.triangulate_rows(EC.scenes()[0]["pair"], EC.TRI, sc, EC.scenes()[0]["q_kp"][:4], EC.scenes()[0]["q_desc"][:4], EC.scenes()[0]["t_kp"], [-1, -7, 461, 1 << 20])
    assert list(rows[0]["state"]) == [-1] * 4 and rows[4]["n_matches"] == 0


def _random_couples(rng, pair_poses, n):
    k1 = G.kp_rows(rng.uniform(-20, 340, n), rng.uniform(-20, 260, n), octave=rng.integers(0, 8, n))
    k2, _ = EC.second_view(rng, k1, *pair_poses, noise=0.5)
    what = rng.random(n)
    k2["x"] += np.where(what < 0.25, rng.normal(0, 30, n), 0).astype(np.float32)   # false couples
    k2["y"] += np.where((what > 0.2) & (what < 0.4), rng.normal(0, 3, n), 0).astype(np.float32)
    k2["octave"] = rng.integers(-1, 9, n)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, 1e-45, 3e38], np.float32)
    for k in rng.integers(0, n, n // 50):
        (k1 if rng.random() < 0.5 else k2)[("x", "y")[rng.integers(0, 2)]][k] = odd[rng.integers(0, len(odd))]
    return k1, k2


def test_host_twins_agree_with_the_reference_on_random_couples():
    """the compiler's steps against numpy's float32 and Python's doubles: 10 000 random couples under three pose pairs"""
    sc = EC.scale()
    rng = np.random.Generator(np.random.PCG64(0x10000))
    states, codes = np.zeros(11, int), np.zeros(4, int)
    pose_pairs = [(EC.pose(0), EC.pose(1)), (EC.pose(1), EC.pose(2)), (EC.pose(None), EC.pose("forward"))]
    tps = [EC.TRI, dict(EC.TRI, far_limit=6.0, chi2=2.0), dict(EC.TRI, ratio_factor=1.05, cos_parallax_max=0.99999)]
    for k, (p1, p2) in enumerate(pose_pairs):
        pair = EC.make_pair(p1, p2)
        k1, k2 = _random_couples(rng, (p1, p2), 3334 if k == 0 else 3333)
        for coarse in (False, True):
            want = _ref_check(pair, coarse, sc, k1, k2)
            assert list(binding.epi_check_host(pair, binding.epi_params(coarse=coarse), sc, k1, k2)) == list(want), (k, coarse)
            assert (E.check_many(pair, coarse, sc, E.line_of(pair, k1["x"][0], k1["y"][0]), k2["x"], k2["y"], k2["octave"]) ==
                    np.array([E.check(pair, coarse, sc, E.line_of(pair, k1["x"][0], k1["y"][0]), k2["x"][i], k2["y"][i], k2["octave"][i])
                              for i in range(len(k2))])).all()
            codes += np.bincount(want, minlength=4)
        info, pts, _ = E.triangulate_couples(pair, tps[k], sc, k1, k2)
        gp, gi = binding.triangulate_host(pair, binding.tri_params(**tps[k]), sc, k1, k2)
        _same(gi, info, f"random couples, pose pair {k}")
        _same(gp, pts, f"random couples, pose pair {k}")
        states += np.bincount(info["state"], minlength=11)
    print("states", states, "codes", codes)
    assert (codes > 100).all() and states[0] > 1000 and (states[[1, 3, 5, 6, 9, 10]] > 20).all()
    # other tables: one level, sixteen levels
    for factor, n in ((1.2, 1), (1.1, 16)):
        t = PC.scale_table(factor, n)
        k2["octave"] = rng.integers(-1, n + 1, len(k2))
        k1["octave"] = rng.integers(0, n, len(k1))
        info, pts, _ = E.triangulate_couples(pair, EC.TRI, t, k1[:500], k2[:500])
        gp, gi = binding.triangulate_host(pair, binding.tri_params(**EC.TRI), t, k1[:500], k2[:500])
        _same(gi, info, f"{n} levels")
        _same(gp, pts, f"{n} levels")
        assert list(binding.epi_check_host(pair, binding.epi_params(), t, k1[:500], k2[:500])) == list(_ref_check(pair, False, t, k1[:500], k2[:500]))
    assert len(binding.epi_check_host(pair, binding.epi_params(), sc, k1[:0], k2[:0])) == 0


def test_invalid_arguments_are_refused_without_a_device():
    sc = EC.scale()
    s = EC.scenes()[0]
    k1, k2 = s["q_kp"][:3], s["t_kp"][:3]
    for kw in (dict(th=-1), dict(th=257), dict(orientation=3), dict(orientation=-1)):
        with pytest.raises(binding.OrbError) as e:
            binding.epi_check_host(s["pair"], binding.epi_params(**kw), sc, k1, k2)
        assert e.value.code == binding.SS_ERR_INVALID_ARG, kw
    for good in (dict(th=0), dict(th=256), dict(orientation=2), dict(coarse=True)):
        assert len(binding.epi_check_host(s["pair"], binding.epi_params(**good), sc, k1, k2)) == 3
    for levels in (np.zeros(0, np.float32), np.ones(17, np.float32)):
        with pytest.raises(binding.OrbError):
            binding.epi_check_host(s["pair"], binding.epi_params(), levels, k1, k2)
        with pytest.raises(binding.OrbError):
            binding.triangulate_host(s["pair"], binding.tri_params(), levels, k1, k2)
    lib = binding.load()
    p, tp = binding.epi_params(), binding.tri_params()
    assert lib.ss_match_epi_pairs_device(None, *([None] * 10), 0, 1, None, C.byref(p), None, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_match_epi_batch_device(None, None, None, None, C.byref(p), None, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_triangulate_pairs_device(None, *([None] * 6), 0, 1, None, C.byref(tp), *([None] * 6)) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_triangulate_batch_device(None, None, None, None, C.byref(tp), *([None] * 6)) == binding.SS_ERR_INVALID_ARG


def test_dlt_against_the_float64_svd():
    """the fixed six sweeps of cyclic Jacobi against numpy.linalg.svd of the same 4 x 4 matrix, on EVERY state-0 point of the
    scenes (parallax of at least 1.146 degrees: cos < 0.9998).  Asserted per point: np.allclose(rtol=1e-6, atol=1e-9), the bound
    tests/test_track.py::test_triangulate_and_checks holds sst_triangulate to.  Seen, and printed by the test: 690 points, worst
    relative deviation 8.5e-14, every off-diagonal entry of M exactly 0.0 after the six sweeps."""
    sc = EC.scale()
    worst, worst_off, n = 0.0, 0.0, 0
    for k, s in enumerate(EC.scenes()):
        w = E.PairD(s["pair"])
        idx = EC.scene_matches(k)
        info = EC.scene_triangulation(k)[0]
        for i in np.flatnonzero(info["state"] == 0):
            j = int(idx[i])
            k1, k2 = s["q_kp"][i], s["t_kp"][j]
            a1, b1 = (float(k1["x"]) - w.cx1) * w.invfx1, (float(k1["y"]) - w.cy1) * w.invfy1
            a2, b2 = (float(k2["x"]) - w.cx2) * w.invfx2, (float(k2["y"]) - w.cy2) * w.invfy2
            A = E.dlt_rows(w, a1, b1, a2, b2)
            v, M = E.dlt(A)
            X = np.array(v[:3]) / v[3]
            vt = np.linalg.svd(np.array(A, np.float64))[2]
            want = vt[3, :3] / vt[3, 3]
            assert np.allclose(X, want, rtol=1e-6, atol=1e-9), (k, i, X, want)
            worst = max(worst, float(np.abs(X - want).max() / np.abs(want).max()))
            worst_off = max(worst_off, max(abs(M[p][q]) for p, q in E.PAIRS_ORDER))
            n += 1
    print(f"{n} state-0 points, worst relative deviation from the SVD {worst:.3g}, worst off-diagonal entry after {E.SWEEPS} sweeps {worst_off:.3g}")
    assert n > 500


def test_upstream_loops_against_the_key_rule():
    """ORBmatcher::SearchForTriangulation's loops as written (ascending scan, dist > bestDist -> continue, the geometric tests after
    the distance) give the key rule's winner on every row whose winning distance is unique; the rows that differ are exactly
    distance ties, where upstream keeps the last row and the rule the lowest."""
    sc = EC.scale()
    ties = rows = 0
    for k, s in enumerate(EC.scenes()):
        for coarse in (False, True):
            up = E.upstream_search(s["pair"], s["q_kp"], s["q_desc"], s["q_node"], s["t_kp"], s["t_desc"], s["t_node"], sc, 50, coarse, s["q_taken"], s["t_taken"])
            row1, d1, visited, _, _ = EC.scene_found(k, coarse, True)
            assert ((up >= 0) == (row1 >= 0)).all()
            for i in np.flatnonzero(up != row1):
                # both are candidates at the winning distance: a tie, and upstream's is the later row
                du = int(E.R._POPCOUNT[s["q_desc"][i] ^ s["t_desc"][up[i]]].sum())
                assert du == d1[i] and up[i] > row1[i], (k, i, up[i], row1[i])
                ties += 1
            rows += int((row1 >= 0).sum())
    print(f"{rows} rows with a winner, {ties} distance ties resolved differently")
    assert rows > 1500


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/epi_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with
    the environment as it is"""
    exe = str(tmp_path / "epi_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "epi_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split()[1]) > 1000000


def test_scenes_give_every_test_work():
    """no vacuous pass on the GPU, asserted on the reference: every scene has couples rejected by the epipole test, by the line, by
    th, by a taken flag on each side and by node -1; coarse changes a winner; one_to_one and both orientation forms each remove
    something; every scene yields points and at least three other states"""
    sc = EC.scale()
    for k, s in enumerate(EC.scenes()):
        base = dict(coarse=False, one_to_one=False, orientation=0, taken=True)
        row1, d1, visited, n_geo, n_near = EC.scene_found(k, False, True)
        causes = np.zeros(4, int)
        for i, js in enumerate(visited):
            if js:
                js = np.array(js)
                causes += np.bincount(E.check_many(s["pair"], False, sc, E.line_of(s["pair"], s["q_kp"]["x"][i], s["q_kp"]["y"][i]), s["t_kp"]["x"][js],
                                                   s["t_kp"]["y"][js], s["t_kp"]["octave"][js]), minlength=4)
        print(k, "causes", causes, "geometric", n_geo, "near", n_near)
        assert causes[0] == n_geo and causes[2] > 0 and causes[3] > 100 and 0 < n_near < n_geo
        idx, _, summ = EC.scene_reference(k, base)
        free = EC.scene_reference(k, dict(base, taken=False))
        assert free[2]["n_candidates"] > summ["n_candidates"] and not np.array_equal(free[0], idx)
        assert (s["q_taken"] != 0).sum() > 10 and (s["t_taken"] != 0).sum() > 10
        assert (idx[s["q_taken"] != 0] == -1).all() and not np.isin(np.flatnonzero(s["t_taken"]), idx).any()
        assert (free[0][s["q_taken"] != 0] >= 0).any() and np.isin(np.flatnonzero(s["t_taken"]), free[0]).any()
        assert (s["q_node"] < 0).sum() > 10 and (s["t_node"] < 0).sum() > 10 and (idx[s["q_node"] < 0] == -1).all()
        coarse = EC.scene_reference(k, dict(base, coarse=True))
        both = (coarse[0] >= 0) & (idx >= 0)
        assert (coarse[0][both] != idx[both]).any() and coarse[2]["n_geometric"] > summ["n_geometric"]
        uni = EC.scene_reference(k, dict(base, coarse=True, one_to_one=True))[2]
        assert uni["n_unique"] < uni["n_accepted"]
        for o in (1, 2):
            rot = EC.scene_reference(k, dict(base, orientation=o))[2]
            assert rot["n_final"] < rot["n_unique"] and rot["rot_bins"] != 0xFFFFFF
        assert (idx == s["truth"]).sum() > 150
        tri = EC.scene_triangulation(k)
        states = set(int(v) for v in tri[0]["state"])
        assert {0, -1} <= states and len(states - {0, -1}) >= 3, states
        assert tri[4]["n_points"] > 150 and len(tri[1]) == tri[4]["n_points"] and (np.diff(tri[3][:, 0]) > 0).all()
        m = EC.scene_matches(k)
        assert (m == -7).any() and (m == len(s["t_kp"])).any()


def test_count_capacity_and_compaction_cases():
    base = EC.count_frame()
    assert len(base["q_kp"]) == len(base["t_kp"]) == EC.COUNT_ROWS == 65
    assert {0, 1, 63, 64, 65} <= {a for a, _ in EC.COUNTS} and {0, 1, 63, 64, 65} <= {b for _, b in EC.COUNTS}
    assert any(a > 65 for a, _ in EC.COUNTS) and any(b > 65 for _, b in EC.COUNTS) and any(a < 0 for a, _ in EC.COUNTS) and any(b < 0 for _, b in EC.COUNTS)
    full = EC.count_reference(65, 65)
    assert full[2]["n_candidates"] > 100 and full[2]["n_accepted"] > 20 and full[3][4]["n_points"] > 10
    assert EC.count_reference(64, 65)[2] != full[2] != EC.count_reference(65, 64)[2]  # the 65th row of either side matters
    assert EC.count_reference(70, 1 << 30)[2] == full[2]
    assert EC.CHUNK == 1024 and set(EC.COMPACT_COUNTS) == {0, 1, 1023, 1024, 1025}
    b = EC.compact_base()
    good = np.flatnonzero(b["info"]["state"] == 0)
    assert len(good[::2]) >= 1025 and (b["info"]["state"] != 0).sum() > 5
    for count in EC.COMPACT_COUNTS:
        head, spread = EC.compact_case(count, "head"), EC.compact_case(count, "spread")
        assert head[5]["n_points"] == spread[5]["n_points"] == count == len(head[2])
        if 1 < count <= 1024:
            assert head[4][-1, 0] < 1024 + 64 < spread[4][-1, 0]  # in one chunk (nearly: a few couples are no point) / across two and more


def test_capacity_pairs_need_both_conflict_passes():
    for b in range(2):
        idx, d1, summ = EC.capacity_reference(b, coarse=True)
        loose = EC.capacity_reference(b, coarse=True, one_to_one=False, orientation=0)[0]
        wanted, times = np.unique(loose[loose >= 0], return_counts=True)
        contested = wanted[times >= 2]
        print(b, summ, "contested rows below / from 8192:", int((contested < 8192).sum()), int((contested >= 8192).sum()))
        assert summ["n_query"] == summ["n_train"] == EC.CAP_ROWS == binding.SS_GUIDED_MAX_ROWS
        assert (contested >= 8192).sum() > 300 and summ["n_unique"] < summ["n_accepted"] - 500
        if b == 0:
            assert (contested < 8192).sum() > 300
        fine = EC.capacity_reference(b, coarse=False)[2]
        assert 0 < fine["n_geometric"] < summ["n_geometric"] and fine["n_accepted"] > 1000


# ---- odd cameras: what makes the camera test of tests/test_epi.py able to fail ---------------------------------------------------------------
def test_camera_scenes_are_live_and_the_library_makes_their_pairs():
    """the three scenes under (A, B), (B, A) and (square, A): ss_epi_pair_init gives the reference's record; the search has matches
    that the line test shaped, the triangulation of its matches points and rejections, the triangulation of the looser matches most
    of its states.  The rule has no image bounds: the train keypoints of a scene whose cameras differ fall outside 320 x 240, and
    match all the same"""
    for k, s in enumerate(EC.camera_scenes()):
        c1, c2 = CC.PAIR_CAMERAS[k]
        assert s["cams"] == (CC.intrinsics(c1), CC.intrinsics(c2))
        assert bytes(EC.library_pair(binding, *s["poses"], *s["cams"])) == s["pair"].tobytes(), k
        assert [float(s["pair"][n]) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] == list(c1[:4] + c2[:4])
        (idx, d1, summ), tri = EC.camera_reference(k)
        assert summ["n_final"] > 150 and summ["n_geometric"] < summ["n_candidates"] // 5 and summ["n_near"] > summ["n_accepted"] > summ["n_unique"], (k, summ)
        assert (idx[idx >= 0] == s["truth"][idx >= 0]).mean() > 0.9  # the search finds the partners the scene planted
        assert tri[4]["n_points"] > 150 and tri[4]["n_matches"] == summ["n_final"], (k, tri[4])
        m = np.flatnonzero(idx >= 0)
        gp, gi = binding.triangulate_host(s["pair"], binding.tri_params(**EC.TRI), EC.scale(), s["q_kp"][m], s["t_kp"][idx[m]])  # the host twins
        assert gi.tobytes() == tri[0][m].tobytes() and gp[gi["state"] == 0].tobytes() == tri[1].tobytes(), k
        codes = binding.epi_check_host(s["pair"], binding.epi_params(), EC.scale(), s["q_kp"], s["t_kp"][s["truth"]])
        assert list(codes) == [E.check(s["pair"], False, EC.scale(), E.line_of(s["pair"], s["q_kp"]["x"][i], s["q_kp"]["y"][i]), *[s["t_kp"][n][s["truth"][i]]
                                       for n in ("x", "y", "octave")]) for i in range(len(codes))] and 0 < (codes == 0).sum() < len(codes)
        loose = EC.camera_triangulation(k)[4]
        assert loose["n_points"] > 100 and sum(n > 0 for n in loose["n_state"]) >= 4, (k, loose)
        outside = (s["t_kp"]["x"] < 0) | (s["t_kp"]["x"] >= G.W) | (s["t_kp"]["y"] < 0) | (s["t_kp"]["y"] >= G.H)
        assert k == 2 or (outside.sum() > 20 and (np.isin(idx[idx >= 0], np.flatnonzero(outside))).sum() > 5), (k, int(outside.sum()))
    assert EC.camera_reference(1)[1][4]["n_state"][1] > 0 and EC.camera_reference(2)[1][4]["n_state"][1] > 0


@pytest.mark.parametrize("mixup", list(CC.PAIR_MIXUPS))
def test_camera_mixups_change_the_reference(mixup):
    """under the pair record a confusion of the cameras would make, every pair it changes has other idx and d1, and on the SAME
    matches other triangulation info, other points and another compact block.  No mix-up is exempt"""
    cams = list(CC.PAIR_CAMERAS)
    mixed = CC.PAIR_MIXUPS[mixup](cams)
    hit = CC.changed(cams, mixed, fields=(0, 1, 2, 3))
    assert hit, mixup
    for k in hit:
        (ri, rd, rs), _ = EC.camera_reference(k)
        (wi, wd, ws), _ = EC.camera_reference(k, mixed[k])
        assert (ri != wi).sum() > 50 and (rd != wd).sum() > 50 and rs != ws, (mixup, k)
        right, wrong = EC.camera_triangulation(k), EC.camera_triangulation(k, mixed[k])
        assert right[0].tobytes() != wrong[0].tobytes() and right[4] != wrong[4], (mixup, k)
        both = np.intersect1d(right[3][:, 0], wrong[3][:, 0])
        assert len(both) == 0 or right[1][np.isin(right[3][:, 0], both)].tobytes() != wrong[1][np.isin(wrong[3][:, 0], both)].tobytes(), (mixup, k)
        rows = np.flatnonzero((right[0]["state"] >= 0) & (wrong[0]["state"] >= 0))
        assert (right[0]["cos_parallax"][rows] != wrong[0]["cos_parallax"][rows]).mean() > 0.9, (mixup, k)
