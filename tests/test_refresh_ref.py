"""The map-point refresh on the CPU: the ABI surface, the host twin (ss_refresh_host: the text the kernels compile) against the reference
(tests/refresh_ref.py) bit for bit on the shared cases, the ladder of list lengths and calls of two problems, the liveness of the cases
asserted on the reference, ss_global_ba_rows_from_idx_host against its restatement, the refusals with their messages and the steps under
the sanitizers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import refresh_cases as RC
import refresh_ref as RR
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED, LADDERS = RC.shared_cases(), RC.ladder_cases()
SCALE = RR.scale_table(1.2, RC.N_LEVELS)


def twin(call, geometry=1, descriptor=1, **over):
    k = dict(call, **over)
    return binding.refresh_host(k["table"], k["n_kf"], k["n_blocks"], k["point_rows"], k["obs"], k["obs_row"], SCALE, k["points"], k["point_desc"], k["n_points"],
                                k["desc"], k["views"], binding.refresh_params(geometry, descriptor), ref_kf=k["ref_kf"], select=k["select"], check_right=k["check_right"],
                                rows_per_frame=k["rows_per_frame"])


def ref(call, geometry=1, descriptor=1, **kw):
    return RR.refresh(call, geometry, descriptor, SCALE, **kw)


def same(tag, got, want):
    (pts, pd, info, summary), (wpts, wpd, winfo, wsummary) = got, want
    for name in RR.INFO_DTYPE.names:
        assert np.array_equal(info[name], winfo[name]), f"{tag}: info.{name} differs at {np.argwhere(info[name] != winfo[name])[:6].tolist()}: {info[name][info[name] != winfo[name]][:6]} != {winfo[name][info[name] != winfo[name]][:6]}"
    for name in RR.SUMMARY_DTYPE.names:
        assert np.array_equal(summary[name], wsummary[name]), f"{tag}: summary.{name} {summary[name][:8]} != {wsummary[name][:8]}"
    a, b = np.ascontiguousarray(pts).view(np.uint8).reshape(-1, 32), np.ascontiguousarray(wpts).view(np.uint8).reshape(-1, 32)
    assert np.array_equal(a, b), f"{tag}: points differ in rows {np.flatnonzero((a != b).any(axis=1))[:8]}"
    assert np.array_equal(pd, wpd), f"{tag}: descriptors differ in rows {np.argwhere((pd != wpd).any(axis=-1))[:8].tolist()}"


def differs(got, want):
    try:
        same("", got, want)
    except AssertionError:
        return True
    return False


def one_point(lst, seed=0, **kw):
    """a case of one point with the list lst over max(kf) + 1 keyframes"""
    return RC.case(max([k[0] for k in lst] + [0]) + 1, [lst], seed, **kw)


def test_abi_surface():
    assert C.sizeof(binding.RefreshParams) == 32 and binding.REFRESH_INFO_DTYPE.itemsize == 32 and binding.REFRESH_SUMMARY_DTYPE.itemsize == 32
    assert RR.INFO_DTYPE == binding.REFRESH_INFO_DTYPE and RR.SUMMARY_DTYPE == binding.REFRESH_SUMMARY_DTYPE and RR.MAP_POINT_DTYPE == binding.MAP_POINT_DTYPE
    assert RR.OBS_DTYPE == binding.GBA_OBS_DTYPE and RR.PROBLEM_DTYPE == binding.GBA_PROBLEM_DTYPE and RC.VIEW_DTYPE == binding.PROJ_VIEW_DTYPE
    assert [binding.REFRESH_INFO_DTYPE.fields[n][1] for n in RR.INFO_DTYPE.names] == list(range(0, 32, 4))
    assert [binding.REFRESH_SUMMARY_DTYPE.fields[n][1] for n in RR.SUMMARY_DTYPE.names] == list(range(0, 32, 4))
    assert (binding.RefreshParams.geometry.offset, binding.RefreshParams.descriptor.offset, binding.RefreshParams.reserved.offset) == (0, 4, 8)
    lib = binding.load()
    for sym in ("ss_covis_set_map_rows", "ss_global_ba_rows_from_idx_host", "ss_refresh_params_default", "ss_refresh_device", "ss_refresh", "ss_refresh_host"):
        assert hasattr(lib, sym), sym
    header = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    for text in ("} ss_refresh_params;", "} ss_refresh_info;", "} ss_refresh_summary;", "int32_t state;", "int32_t n_obs, count;", "int32_t ref_kf, level;", "int32_t best_kf, best_median;",
                 "int32_t n_rows, n_selected, n_refreshed, n_no_obs, n_degenerate, max_obs;", "int ss_refresh_device(ss_ctx *ctx, void *d_points, void *d_point_desc, const void *d_n_points, const void *d_ref_kf,"):
        assert text in header, text
    p = binding.RefreshParams()
    assert lib.ss_refresh_params_default(C.byref(p)) == binding.SS_OK and lib.ss_refresh_params_default(None) == binding.SS_ERR_INVALID_ARG
    assert bytes(p) == bytes(binding.refresh_params()) and (p.geometry, p.descriptor, tuple(p.reserved)) == (1, 1, (0,) * 6)
    assert lib.ss_abi_version() == 5
    assert np.array_equal(SCALE, np.array(__import__("proj_cases").scale_table(1.2, 8), np.float32))


@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_cases_host_twin_is_the_reference(name):
    call = RC.single(SHARED[name])
    for g, d in ((1, 1), (1, 0), (0, 1)):
        same(f"{name} geometry {g} descriptor {d}", twin(call, g, d), ref(call, g, d))


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder_host_twin_is_the_reference(name):
    call = RC.single(LADDERS[name])
    got = twin(call)
    same(name, got, ref(call))
    n = int(name.split("_")[1])
    assert got[2][0, 0]["n_obs"] == n and got[2][0, 0]["state"] == (0 if n else 1) and got[2][0, 1]["n_obs"] <= n and got[3][0]["max_obs"] == max(n, 1)


def _first(make, ok, tries=400):
    for seed in range(tries):
        c = make(seed)
        if ok(c):
            return c
    raise AssertionError("no seed gives the case")


def _pooled(n, seed):
    """one point seen by n keyframes whose descriptors differ in few bits, so that medians lie close together"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, 32).astype(np.uint8)
    desc = np.repeat(base[None, None, :], n, axis=0).copy()
    for k in range(n):
        for bit in rng.choice(256, int(rng.integers(0, 9)), replace=False):
            desc[k, 0, bit // 8] ^= 1 << (bit % 8)
    return RC.case(n, [[(k, 2) for k in range(n)]], seed, rows_per_frame=1, desc=desc)


def _winner(c, **kw):
    return int(ref(RC.single(c), **kw)[2][0, 0]["best_kf"])


def test_the_rank_is_live_for_an_even_and_an_odd_length():
    for n in (6, 7):
        c = _first(lambda s: _pooled(n, s), lambda c: len({_winner(c), _winner(c, rank_shift=-1), _winner(c, rank_shift=1)}) == 3)
        call = RC.single(c)
        same(f"rank, n {n}", twin(call), ref(call))
        assert differs(twin(call), ref(call, rank_shift=-1)) and differs(twin(call), ref(call, rank_shift=1))


def test_ties_go_to_the_lowest_observation_and_the_last_one_can_win():
    tied = _first(lambda s: _pooled(9, s), lambda c: _winner(c) != _winner(c, tie_last=True))
    call = RC.single(tied)
    same("a tie", twin(call), ref(call))
    assert _winner(tied) < _winner(tied, tie_last=True) and differs(twin(call), ref(call, tie_last=True))
    last = _first(lambda s: _pooled(9, s), lambda c: _winner(c) == 8)
    same("the last observation wins", twin(RC.single(last)), ref(RC.single(last)))
    decided = total = 0
    for name, c in SHARED.items():  # random descriptors alone tie often
        call = RC.single(c)
        a, b = ref(call)[2], ref(call, tie_last=True)[2]
        decided, total = decided + int((a["best_kf"] != b["best_kf"]).sum()), total + int((a["state"] == 0).sum())
    assert 0 < decided < total, (decided, total)


def test_distances_of_exactly_0_and_256():
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, 32).astype(np.uint8)
    desc = np.stack([a, ~a, ~a, a, ~a])[:, None, :]
    c = RC.case(5, [[(0, 1), (1, 1), (2, 1)], [(0, 1), (3, 1)], [(k, 1) for k in range(5)]], 1, rows_per_frame=1, desc=desc)
    D, med = RR.medians(desc[:3, 0])
    assert D.tolist() == [[0, 256, 256], [256, 0, 0], [256, 0, 0]] and med.tolist() == [256, 0, 0]
    call = RC.single(c)
    got = twin(call)
    same("0 and 256", got, ref(call))
    assert got[2][0]["best_kf"].tolist() == [1, 0, 1] and got[2][0]["best_median"].tolist() == [0, 0, 0] and np.array_equal(got[1][0, 0], ~a)


@pytest.mark.parametrize("bit", [32 * k + 5 for k in range(8)] + [255])
def test_a_planted_bit_in_every_word_changes_the_winner(bit):
    rng = np.random.default_rng(bit)
    flip = lambda d, bits: np.bitwise_xor.reduce([d] + [np.eye(1, 32, b // 8, dtype=np.uint8)[0] << (b % 8) for b in bits])  # noqa: E731
    cdesc = rng.integers(0, 256, 32).astype(np.uint8)
    adesc = flip(cdesc, [32 * j + 1 for j in range(8)] + [2, 34])
    bdesc = flip(cdesc, [32 * j + 9 for j in range(8)] + [10, bit])  # ten bits from c, the planted one among them: without it nine
    winners = []
    for planted in (False, True):
        desc = np.stack([adesc, flip(bdesc, [bit]) if planted else bdesc, cdesc])[:, None, :]
        call = RC.single(RC.case(3, [[(0, 0), (1, 0), (2, 0)]], 2, rows_per_frame=1, desc=desc))
        got = twin(call)
        same(f"bit {bit} planted {planted}", got, ref(call))
        winners.append((int(got[2][0, 0]["best_kf"]), int(got[2][0, 0]["best_median"])))
    assert winners == [(0, 10), (1, 9)]


@pytest.mark.parametrize("n", [65, 129])
def test_the_tree_is_not_the_sequential_sum(n):
    def apart(c):
        P, ow = c["points"][0], c["ow"]
        d = [[float(P[k]) - float(ow[j][i]) for i, k in enumerate("xyz")] for j in range(n)]
        t = [dj[0] / math.sqrt((dj[0] * dj[0] + dj[1] * dj[1]) + dj[2] * dj[2]) for dj in d]
        seq = 0.0
        for v in t:
            seq = seq + v
        return seq != RR.tree(t) and abs(seq - RR.tree(t)) <= 2 * math.ulp(seq)
    c = _first(lambda s: RC.case(n, [[(k, 1) for k in range(n)]], s, rows_per_frame=1), apart)
    same(f"tree of {n}", twin(RC.single(c)), ref(RC.single(c)))


def test_the_reference_keyframe():
    lst = [(1, 2), (4, 5), (6, -1), (7, 3)]
    out = {}
    for tag, entry in (("observing", 4), ("not observing", 3), ("octave invalid", 6), ("minus one", -1), ("no table", None)):
        call = RC.single(one_point(lst, 4, ref_kf=None if entry is None else [entry]))
        got = twin(call)
        same(tag, got, ref(call))
        out[tag] = (int(got[2][0, 0]["ref_kf"]), int(got[2][0, 0]["level"]), float(got[0][0, 0]["min_dist"]))
    assert out["observing"][:2] == (4, 5) and all(out[t][:2] == (1, 2) for t in ("not observing", "octave invalid", "minus one", "no table"))
    assert out["observing"][2] != out["no table"][2] and len({out[t] for t in out}) == 2
    moved = RC.single(one_point([(1, 2), (3, 2), (4, 5)], 4, ref_kf=[3]))  # the same level, another distance
    assert ref(moved)[2][0, 0]["level"] == 2 and ref(moved)[0][0, 0]["min_dist"] != ref(dict(moved, ref_kf=None))[0][0, 0]["min_dist"]
    same("moved", twin(moved), ref(moved))


def test_records_that_are_no_observation_stereo_counts_and_a_point_on_a_camera_centre():
    with_junk = one_point([(0, 3), (1, -1, 5.0), (2, 4, 5.0), (3, RC.N_LEVELS), (5, 0)], 9, check_right=True)
    without = one_point([(0, 3), (2, 4, 5.0), (5, 0)], 9, check_right=True)
    for key in ("ow", "desc", "points"):
        without[key] = with_junk[key]
    without["obs_row"] = with_junk["obs_row"][[0, 2, 4]]
    a, b = twin(RC.single(with_junk)), twin(RC.single(without))
    same("octaves -1 and n_levels are left out of n, of the normal and of the descriptors", a, b)
    same("against the reference", a, ref(RC.single(with_junk)))
    assert (a[2][0, 0]["n_obs"], a[2][0, 0]["count"]) == (3, 4) and twin(RC.single(dict(with_junk, check_right=False)))[2][0, 0]["count"] == 3
    centre = one_point([(0, 1), (1, 1), (2, 1)], 10)
    centre["points"]["x"], centre["points"]["y"], centre["points"]["z"] = centre["ow"][1]
    call = RC.single(centre)
    for g, d, state in ((1, 1, 2), (1, 0, 2), (0, 1, 0)):
        got = twin(call, g, d)
        same(f"centre {g} {d}", got, ref(call, g, d))
        assert got[2][0, 0]["state"] == state and got[2][0, 0]["n_obs"] == 3 and got[3][0]["n_degenerate"] == (state == 2)
        assert (got[0][0, 0]["nx"] == np.float32(-77)) and ((got[1][0, 0] == 0xC3).all() == (state == 2))


def test_select_bytes_non_finite_points_and_counts_outside_the_block():
    c = RC.random_case(11, n_points=24)
    c["select"] = np.arange(24, dtype=np.uint8) % 3
    c["points"]["x"][[3, 9]], c["points"]["z"][6] = (np.nan, np.inf), -np.inf
    call = RC.single(c)
    got = twin(call)
    same("select, NaN, Inf", got, ref(call))
    st = got[2][0]["state"]
    assert (st[c["select"] != 0] == -1).all() and (st[[3, 6, 9]] == -1).all() and (st[[0, 12, 15]] >= 0).all() and got[3][0]["n_selected"] == (st >= 0).sum() > 0
    for count, rows in ((-3, 0), (0, 0), (7, 7), (26, 24), (2 ** 31 - 1, 24)):
        call = RC.single(dict(c, count=count), 24)
        got = twin(call)
        same(f"n_points {count}", got, ref(call))
        assert got[3][0]["n_rows"] == rows and (got[2][0]["state"][rows:] == -1).all()


def test_calls_of_two_problems_with_gaps_in_either_order():
    cases = [LADDERS["len_65"], SHARED["random_12"], LADDERS["len_5"]]
    for order, lead, gap, seed in (([0, 1, 2], 0, 0, None), ([2, 0, 1], 2, 3, 5)):
        call = RC.stack(cases, 16, lead=lead, gap=gap, order=order, shuffle_seed=seed)
        for g, d in ((1, 1), (1, 0), (0, 1)):
            same(f"order {order} {g} {d}", twin(call, g, d), ref(call, g, d))
    call = RC.stack([SHARED["random_12"], SHARED["random_12"]], 16, lead=1, gap=2)
    k0, k1, n = call["table"]["first_kf"][0], call["table"]["first_kf"][1], call["table"]["n_kf"][0]
    swap = np.arange(call["n_kf"])
    swap[k0:k0 + n], swap[k1:k1 + n] = np.arange(k1, k1 + n), np.arange(k0, k0 + n)
    call["views"]["ow"][k1:k1 + n] += 1  # the two problems are the same case: make their keyframes differ
    call["desc"][k1:k1 + n] ^= 0x0F
    base = twin(call)
    same("twice the same case", base, ref(call))
    assert differs(twin(call, views=call["views"][swap]), base) and differs(twin(call, desc=call["desc"][swap]), base)
    assert differs(twin(call, 1, 0, views=call["views"][swap]), twin(call, 1, 0)) and differs(twin(call, 0, 1, desc=call["desc"][swap]), twin(call, 0, 1))


def test_geometry_alone_and_descriptor_alone_leave_the_other_half():
    call = RC.single(SHARED["random_70"])
    both, geo, des = twin(call), twin(call, 1, 0), twin(call, 0, 1)
    ok = both[2]["state"] == 0
    assert ok.sum() > 10 and np.array_equal(geo[1], call["point_desc"]) and des[0].tobytes() == call["points"].tobytes()
    assert geo[0].tobytes() == both[0].tobytes() and np.array_equal(des[1], both[1])
    assert (geo[2]["best_kf"] == -1).all() and (des[2]["ref_kf"] == -1).all() and (des[2]["level"] == -1).all() and np.array_equal(geo[2]["ref_kf"], both[2]["ref_kf"])
    twin(dict(call, desc=None, point_desc=None, obs_row=None), 1, 0)  # a geometry-only call needs neither rows nor descriptors


def test_rows_from_idx_against_its_restatement():
    rng = np.random.default_rng(12)
    n_kf, rows, P = 5, 40, 60
    kp = np.zeros((n_kf, rows), binding.KP_DTYPE)
    kp["x"], kp["octave"] = rng.random((n_kf, rows)), rng.integers(0, 8, (n_kf, rows))
    idx = rng.integers(-2, rows + 3, (n_kf, P)).astype(np.int32)
    n_kp = np.array([rows, 0, rows + 9, 17, -4], np.int32)
    want = [(i, k, int(idx[k, i])) for i in range(P) for k in range(n_kf) if 0 <= idx[k, i] < min(max(int(n_kp[k]), 0), rows)]
    obs, got = binding.global_ba_obs_from_idx(kp, idx, n_kp), binding.global_ba_rows_from_idx(idx, n_kp, rows)
    assert len(want) > 50 and got.tolist() == [w[2] for w in want] and obs["point"].tolist() == [w[0] for w in want] and obs["kf"].tolist() == [w[1] for w in want]
    assert np.array_equal(obs["u"], kp["x"][obs["kf"], got])
    fn = binding.load().ss_global_ba_rows_from_idx_host
    out = np.full(4, -9, np.int32)
    assert fn(n_kp.ctypes.data, n_kf, rows, idx.ctypes.data, P, out.ctypes.data, 3) == len(want) and out.tolist() == [w[2] for w in want[:3]] + [-9]
    assert fn(None, n_kf, rows, idx.ctypes.data, P, None, 0) == binding.SS_ERR_INVALID_ARG and fn(n_kp.ctypes.data, n_kf, 0, idx.ctypes.data, P, None, 0) == binding.SS_ERR_INVALID_ARG
    assert fn(None, 0, rows, None, 0, None, 0) == 0


def test_refused_arguments_with_their_messages():
    call = RC.single(SHARED["random_12"])
    rp = binding.refresh_params
    low, high = call["obs_row"].copy(), call["obs_row"].copy()
    low[7], high[9] = -1, 16384
    kf_out = call["obs"].copy()
    kf_out["kf"][5] = 12
    bad = [(dict(obs_row=low), 1, 1, "covis: problem 0: record 7: row -1 outside 0 .. SS_GUIDED_MAX_ROWS - 1 (16383)"),
           (dict(obs_row=high), 1, 1, "record 9: row 16384 outside 0 .. SS_GUIDED_MAX_ROWS - 1 (16383)"),
           (dict(obs=kf_out), 1, 1, "covis: problem 0: record 5: kf 12 outside 0 .. 11"),
           (dict(rows_per_frame=int(call["obs_row"].max())), 1, 1, f"rows_per_frame {call['obs_row'].max()} is not above the map's largest row {call['obs_row'].max()}"),
           (dict(rows_per_frame=16385), 1, 1, "rows_per_frame 16385 exceeds SS_GUIDED_MAX_ROWS (16384)"),
           (dict(desc=None), 1, 1, "ss_refresh_host: NULL buffer"), (dict(point_desc=None), 0, 1, "ss_refresh_host: NULL buffer")]
    for over, g, d, msg in bad:
        with pytest.raises(binding.OrbError) as e:
            twin(call, g, d, **over)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message, (over, e.value.message)
    for params, msg in ((rp(0, 0), "geometry or descriptor must be set"), (rp(2, 1), "geometry must be 0 or 1"), (rp(1, -1), "descriptor must be 0 or 1"),
                        (rp(reserved=(0, 0, 0, 0, 0, 1)), "the reserved fields must be 0")):
        with pytest.raises(binding.OrbError) as e:
            binding.refresh_host(call["table"], call["n_kf"], 1, call["point_rows"], call["obs"], call["obs_row"], SCALE, call["points"], call["point_desc"],
                                 call["n_points"], call["desc"], call["views"], params)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and msg in e.value.message
    for over, msg in ((dict(obs_row=None), "the map has no rows, which descriptor needs"), (dict(table=call["table"][:0]), "ss_refresh_host: no map")):
        with pytest.raises(binding.OrbError) as e:
            twin(call, **over)
        assert e.value.code == binding.SS_ERR_STATE and msg in e.value.message


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/refresh_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with the
    environment as it is"""
    exe = str(tmp_path / "refresh_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "refresh_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
