"""Covisibility on the CPU: the ABI surface, the host twins (ss_covis_kf_host, ss_covis_frames_host: the text the kernels compile) against
the reference (tests/covis_ref.py) exactly on the shared cases, the ladders and the calls, the liveness of the cases, the reference's own
properties, ss_covis_edges_host against its restatement, the refused arguments with their messages and the steps under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED, LADDERS = CC.shared_cases(), CC.ladder_cases()


def twin_kf(call, params, cap, rows=None):
    return binding.covis_kf_host(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], CC.N_LEVELS, binding.covis_params(**params), cap,
                                 rows=rows, cull_skip=call["skip"], check_right=call["check_right"])


def twin_frames(call, idx, n_points, point_src, params, cap):
    return binding.covis_frames_host(call["table"], call["n_kf"], call["n_blocks"], call["point_rows"], call["obs"], CC.N_LEVELS, idx, n_points, point_src,
                                     binding.covis_params(**params), cap, cull_skip=call["skip"], check_right=call["check_right"])


def same(tag, got, want):
    nb, row = got
    wnb, wrow = want
    assert nb.shape == wnb.shape and len(row) == len(wrow), tag
    for name in CR.ROW_DTYPE.names:
        assert np.array_equal(row[name], wrow[name]), f"{tag}: row.{name} {row[name][:8]} != {wrow[name][:8]} at rows {np.flatnonzero(row[name] != wrow[name])[:8]}"
    assert np.array_equal(nb, wnb), f"{tag}: neighbour lists differ in rows {np.flatnonzero((nb != wnb).any(axis=(1, 2)))[:8]}"


def ref_of(c, call=None):
    call = call or CC.single(c)
    return CR.kf_rows(CC.ref_map(call), c["rows"], c["params"], c["cap"])


def test_abi_surface():
    assert C.sizeof(binding.CovisParams) == 32 and binding.COVIS_ROW_DTYPE.itemsize == 32 and CR.ROW_DTYPE == binding.COVIS_ROW_DTYPE
    assert CR.OBS_DTYPE == binding.GBA_OBS_DTYPE and CR.PROBLEM_DTYPE == binding.GBA_PROBLEM_DTYPE
    p = binding.CovisParams()
    assert binding.load().ss_covis_params_default(C.byref(p)) == binding.SS_OK and binding.load().ss_covis_params_default(None) == binding.SS_ERR_INVALID_ARG
    d = binding.covis_params()
    assert bytes(p) == bytes(d) and (p.min_weight, p.fallback, p.cull_obs, p.cull_slack, tuple(p.reserved)) == (15, 1, 3, 1, (0, 0, 0))
    assert np.float32(p.redundant_th) == np.float32(0.9)
    assert (binding.SS_COVIS_MAX_ROW_ITEMS, binding.SS_COVIS_MAX_NEIGHBOURS) == (CR.MAX_ROW_ITEMS, CR.MAX_NEIGHBOURS) == (262143, 1024)
    assert (CR.MAX_ROW_ITEMS << 14 | 16383) == 2 ** 32 - 1
    assert binding.load().ss_abi_version() == 5


@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_cases_host_twin_is_the_reference(name):
    c = SHARED[name]
    same(name, twin_kf(CC.single(c), c["params"], c["cap"], c["rows"]), ref_of(c))


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladders_host_twin_is_the_reference(name):
    c = LADDERS[name]
    same(name, twin_kf(CC.single(c), c["params"], c["cap"], c["rows"]), ref_of(c))


def test_shared_cases_are_live():
    """every shared case exercises the branch it is named for, on the reference"""
    nb, row = ref_of(SHARED["planted"])
    assert row[0]["n_shared"] == 40 and row[0]["n_listed"] == 26 and nb[0][:26].tolist() == [[j, j] for j in range(40, 14, -1)] and nb[0][26].tolist() == [-1, 0]
    assert (row[0]["max_weight"], row[0]["max_kf"]) == (40, 40)
    assert row[14]["n_listed"] == 1 and nb[14][0].tolist() == [0, 14] and row[15]["n_listed"] == 1 and nb[15][0].tolist() == [0, 15]
    nb, row = ref_of(SHARED["planted_no_fallback"])
    assert row[14]["n_listed"] == 0 and nb[14][0].tolist() == [-1, 0] and (row[14]["max_weight"], row[14]["max_kf"]) == (14, 0) and row[15]["n_listed"] == 1
    nb, row = ref_of(SHARED["planted_min1"])
    assert row[0]["n_listed"] == 40 and row[1]["n_listed"] == 1 and nb[1][0].tolist() == [0, 1]
    nb, row = ref_of(SHARED["lonely"])
    assert row["max_kf"].tolist() == [-1, -1, -1] and row["n_listed"].tolist() == [0, 0, 0] and row["n_mps"].tolist() == [5, 0, 1] and (nb == (-1, 0)).all()
    nb, row = ref_of(SHARED["ties"])
    assert (row[0]["max_weight"], row[0]["max_kf"], row[0]["n_listed"]) == (20, 1, 32) and nb[0][:32].tolist() == [[1, 20], [2, 20]] + [[j, 16] for j in range(3, 33)]
    for name, written in (("cap_1", 1), ("cap_listed", 32), ("cap_listed_less_1", 31)):
        cnb, crow = ref_of(SHARED[name])
        assert (crow[0]["n_listed"], crow[0]["n_written"]) == (32, written) and np.array_equal(cnb[0], nb[0][:written])
    nb, row = ref_of(SHARED["cap_1024_of_1500"])
    assert (row[0]["n_listed"], row[0]["n_written"]) == (1500, 1024) and (nb[0][:, 0] >= 0).all()
    assert nb[0][0].tolist() == [2, 3] and nb[0][499].tolist() == [1499, 3] and nb[0][500].tolist() == [1, 2] and nb[0][1023].tolist() == [72, 1]  # 500 of weight 3, 500 of weight 2, then 3, 6, .. 72
    m = CC.ref_map(CC.single(SHARED["culling"]))
    mono = CC.ref_map(CC.single(SHARED["culling_mono"]))
    counts = [CR.point_count(m, 0, i) for i in range(10)]
    assert counts[:3] == [3, 4, 5] and counts[6] == 5 and CR.point_count(mono, 0, 6) == 3 and counts[8] == 4
    assert [CR.point_near(m, 0, i, 0, 1) for i in range(9)] == [2, 3, 4, 4, 0, 3, 2, 4, 3]
    for name in ("culling", "culling_mono"):
        nb, row = ref_of(SHARED[name])
        assert (row[0]["n_mps"], row[0]["n_redundant"], row[0]["redundant"]) == (8, 2, 0)
        assert dict(nb[0][:row[0]["n_listed"]].tolist()) == {1: 9, 2: 9, 3: 7, 4: 5}  # keyframe 5 never votes: its only record is no observation
    _, row = ref_of(SHARED["ten_9"])
    assert (row[0]["n_mps"], row[0]["n_redundant"], row[0]["redundant"]) == (10, 9, 0) and np.float32(0.9) * np.float32(10) == np.float32(9)
    _, row = ref_of(SHARED["ten_10"])
    assert (row[0]["n_mps"], row[0]["n_redundant"], row[0]["redundant"]) == (10, 10, 1)


def test_ladders_are_live():
    for n in CC.KF_LADDER:
        c = LADDERS[f"kf_{n}"]
        _, row = ref_of(c)
        assert c["n_kf"] == n and (n < 3 or row["n_listed"].max() > 0), n
    for n in CC.ITEM_LADDER:
        c = LADDERS[f"items_{n}"]
        assert int((c["obs"]["kf"] == 0).sum()) == n
    for n in CC.LIST_LADDER:
        c = LADDERS[f"list_{n}"]
        assert np.bincount(c["obs"]["point"])[:3].tolist() == [n] * 3
    nb, row = ref_of(LADDERS["key_ends"])
    assert nb[0][:2].tolist() == [[16383, 16383], [5, 3]] and nb[1][0].tolist() == [0, 16383] and (row[0]["max_weight"], row[0]["max_kf"]) == (16383, 16383)


def test_reference_weights_are_symmetric_and_listing_is_mutual():
    for name in ("kf_65", "kf_257", "planted", "culling"):
        c = dict(SHARED, **LADDERS)[name]
        m = CC.ref_map(CC.single(c))
        w = [CR.weights_kf(m, k)[1] for k in range(c["n_kf"])]
        for k in range(c["n_kf"]):
            for j, v in w[k].items():
                assert w[j][k] == v
        p = dict(CR.DEFAULTS, **c["params"])
        nb, row = CR.kf_rows(m, None, c["params"], c["n_kf"] if c["n_kf"] <= 1024 else 1024)
        fell = [row[k]["n_listed"] == 1 and nb[k][0][1] < p["min_weight"] for k in range(c["n_kf"])]
        lists = [set(nb[k][:row[k]["n_written"], 0].tolist()) for k in range(c["n_kf"])]
        for k in range(c["n_kf"]):
            for j in range(c["n_kf"]):
                if not fell[k] and not fell[j]:
                    assert (j in lists[k]) == (k in lists[j]), (name, k, j)


def test_calls_two_problems_in_either_order_with_gaps_junk_and_shuffled_records():
    cases = [LADDERS["kf_65"], dict(LADDERS["items_257"], check_right=True)]
    for order, lead, gap, seed in (([0, 1], 0, 0, None), ([1, 0], 2, 3, 5), ([0, 1], 1, 1, 9)):
        call = CC.stack(cases, 100, lead=lead, gap=gap, order=order, shuffle_seed=seed)
        nb, row = twin_kf(call, cases[0]["params"], 48)
        assert len(row) == call["n_kf"]
        owned = np.zeros(call["n_kf"], bool)
        for q, c in enumerate(cases):
            k0, nk = int(call["table"][q]["first_kf"]), c["n_kf"]
            owned[k0:k0 + nk] = True
            ref = CR.kf_rows(CC.ref_map(CC.single(c)), None, cases[0]["params"], 48)
            same(f"order {order} problem {q}", (nb[k0:k0 + nk], row[k0:k0 + nk]), ref)
            same(f"order {order} problem {q} in the stack", (nb[k0:k0 + nk], row[k0:k0 + nk]), CR.kf_rows(CC.ref_map(call), range(k0, k0 + nk), cases[0]["params"], 48))
        assert (row[~owned].view(np.int32).reshape(-1, 8) == [0, 0, -1, 0, 0, 0, 0, 0]).all() and (nb[~owned] == (-1, 0)).all()  # keyframes of no problem
        rows = np.array([call["n_kf"] - 1, 0, 3, 3, 1] + list(range(call["n_kf"] - 1, -1, -1)), np.int32)
        enb, erow = twin_kf(call, cases[0]["params"], 48, rows)
        same("explicit rows", (enb, erow), (nb[rows], row[rows]))


def test_frame_rows_host_twin_is_the_reference():
    call, idx, n_points, point_src = CC.frames_case()
    for params, cap in ((dict(min_weight=1), 64), (dict(min_weight=3, fallback=0), 5), ({}, 16)):
        got = twin_frames(call, idx, n_points, point_src, params, cap)
        same(f"frames {params}", got, CR.frame_rows(CC.ref_map(call), idx, n_points, point_src, params, cap))
    nb, row = twin_frames(call, idx, n_points, point_src, dict(min_weight=1), 64)
    assert row["n_shared"][:3].min() > 0 and row["n_shared"][3] == 0 and row["n_shared"][6] == 0 and row["n_shared"][7] == 0 and row["n_shared"][4] > 0
    assert not row["n_mps"].any() and not row["n_redundant"].any() and not row["redundant"].any()
    assert not np.array_equal(nb[1], nb[2])  # two frames on one block


def test_edges_host_against_its_restatement():
    c = LADDERS["kf_65"]
    call = CC.single(c)
    nb, row = twin_kf(call, dict(min_weight=1), 7)
    row_kf = np.arange(c["n_kf"], dtype=np.int32)
    for mw in (1, 2, 3, 100):
        got = binding.covis_edges(nb, row, row_kf, mw)
        assert np.array_equal(got, CR.edges(nb, row, row_kf, mw)) and (mw > 3 or len(got))
    lib = binding.load()
    some = np.zeros((2, 2), np.int32)
    n = lib.ss_covis_edges_host(nb.ctypes.data, row.ctypes.data, row_kf.ctypes.data, len(row), 7, 1, some.ctypes.data, 2)
    assert n == len(CR.edges(nb, row, row_kf, 1)) > 2 and np.array_equal(some, CR.edges(nb, row, row_kf, 1)[:2])
    assert lib.ss_covis_edges_host(None, None, None, 3, 7, 1, None, 0) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_covis_edges_host(None, None, None, 0, 7, 1, None, 0) == 0


def _refused(fn, *fragments):
    with pytest.raises(binding.OrbError) as e:
        fn()
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    for f in fragments:
        assert f in e.value.message, e.value.message


def test_refused_maps_and_queries_with_their_messages():
    c = SHARED["lonely"]
    call = CC.single(c)

    def with_obs(**field):
        bad = dict(call, obs=call["obs"].copy())
        for k, v in field.items():
            bad["obs"][k][2] = v
        return lambda: twin_kf(bad, {}, 4)

    def with_table(of_call=None, **field):
        bad = dict(call, table=call["table"].copy())
        for k, v in field.items():
            bad["table"][k][0] = v
        bad.update(of_call or {})
        return lambda: twin_kf(bad, {}, 4, rows=[0])

    _refused(with_obs(kf=3), "covis: problem 0: record 2: kf 3 outside 0 .. 2")
    _refused(with_obs(kf=-1), "kf -1 outside")
    _refused(with_obs(point=6), "record 2: point 6 outside 0 .. 5")
    _refused(with_obs(point=1), "the pair (kf 0, point 1) has a record already")
    _refused(with_table(first_kf=1), "keyframes 1 .. + 3 lie outside the call's 3")
    _refused(with_table(n_kf=0), "n_kf 0 outside 1 .. SS_GBA_MAX_KF (16384)")
    _refused(with_table(dict(n_kf=16385), n_kf=16385), "n_kf 16385 outside 1 .. SS_GBA_MAX_KF")
    _refused(with_table(first_block=1), "blocks 1 .. + 1 lie outside the call's 1")
    _refused(with_table(first_obs=1), "records 1 .. + 6 lie outside the call's 6")
    _refused(with_table(n_obs=-1), "n_obs -1 outside 0 .. SS_GBA_MAX_OBS")
    _refused(with_table(dict(point_rows=16384, n_blocks=65), n_blocks=65), "n_blocks 65 of 16384 rows outside 0 .. SS_GBA_MAX_POINTS (1048576) points")
    _refused(with_table(dict(point_rows=16385)), "point_rows 16385 exceeds SS_GUIDED_MAX_ROWS (16384)")
    _refused(with_table(dict(point_rows=0)), "bad keyframe, problem, block, row or record count")
    _refused(with_table(dict(n_kf=binding.SS_COVIS_MAX_MAP_KF + 1)), "n_kf 1048577 exceeds SS_COVIS_MAX_MAP_KF (1048576) keyframes in one call")
    res = dict(call, table=call["table"].copy())
    res["table"]["reserved"][0] = (0, 1)
    _refused(lambda: twin_kf(res, {}, 4), "the reserved fields must be 0")
    two = CC.stack([c, c], 6)
    two["table"]["first_kf"][1] = 2
    _refused(lambda: twin_kf(two, {}, 4), "problem 1: keyframe 2 belongs to problem 0 already")
    two = CC.stack([c, c], 6)
    two["table"]["first_block"][1] = 0
    _refused(lambda: twin_kf(two, {}, 4), "problem 1: block 0 belongs to problem 0 already")
    two = CC.stack([c, c], 6)
    two["table"]["first_obs"][1] = 5
    _refused(lambda: twin_kf(two, {}, 4), "problem 1: record 5 belongs to problem 0 already")
    # more records above SS_GBA_MAX_OBS: the table alone is refused, no record is read
    lib, err = binding.load(), C.create_string_buffer(256)
    big = np.array([(0, 1, 0, 1, 0, 4194305, (0, 0))], CR.PROBLEM_DTYPE)
    p = binding.covis_params()
    out = np.zeros(64, np.int32)
    assert lib.ss_covis_kf_host(big.ctypes.data, 1, 1, 1, 1, None, 4194305, None, 0, 8, None, 1, C.byref(p), 1, out.ctypes.data, out.ctypes.data, err,
                                256) == binding.SS_ERR_INVALID_ARG
    assert b"n_obs 4194305 outside 0 .. SS_GBA_MAX_OBS (4194304)" in err.value
    # a keyframe with one record more than SS_COVIS_MAX_ROW_ITEMS
    n = CR.MAX_ROW_ITEMS + 1
    heavy = CC.case(2, n, [CR.obs_records(np.zeros(n, np.int32), np.arange(n, dtype=np.int32))], rows=[1])
    _refused(lambda: twin_kf(CC.single(heavy, 16384), {}, 1, rows=[1]), "keyframe 0 has more than SS_COVIS_MAX_ROW_ITEMS (262143) records")
    heavy["obs"] = heavy["obs"][:-1]
    nb, row = twin_kf(CC.single(heavy, 16384), dict(min_weight=1), 1, rows=[0, 1])  # at the limit: accepted
    assert row["n_mps"].tolist() == [CR.MAX_ROW_ITEMS, 0] and row["n_shared"].tolist() == [0, 0]
    # the pyramid
    _refused(lambda: binding.covis_kf_host(call["table"], 3, 1, 6, call["obs"], 0, binding.covis_params(), 4), "no pyramid of 1 .. SS_MAX_LEVELS levels")
    # queries
    _refused(lambda: twin_kf(call, {}, 4, rows=[0, 3]), "ss_covis_kf_host: row 1: keyframe 3 lies outside the map's 3")
    _refused(lambda: twin_kf(call, {}, 4, rows=[-1]), "row 0: keyframe -1 lies outside")
    _refused(lambda: twin_kf(call, {}, 0), "cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)")
    _refused(lambda: twin_kf(call, {}, 1025), "cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)")
    for params, msg in ((dict(min_weight=0), "min_weight must be >= 1"), (dict(fallback=2), "fallback must be 0 or 1"), (dict(cull_obs=-1), "cull_obs must be >= 0"),
                        (dict(cull_slack=17), "cull_slack must be 0 .. SS_MAX_LEVELS"), (dict(cull_slack=-1), "cull_slack"),
                        (dict(redundant_th=float("nan")), "redundant_th must be finite and 0 .. 1"), (dict(redundant_th=1.5), "redundant_th"),
                        (dict(redundant_th=-0.5), "redundant_th"), (dict(reserved=(0, 0, 1)), "the reserved fields must be 0")):
        _refused(lambda: twin_kf(call, params, 4), "covis: " + msg)
    _refused(lambda: binding._covis_host(False, call["table"], 3, 1, 6, call["obs"], 8, None, None, None, 2, binding.covis_params(), 4, None, False),
             "rows is NULL, so n_rows must be the map's 3 keyframes, not 2")
    _refused(lambda: binding.covis_kf_host(np.zeros(0, CR.PROBLEM_DTYPE), 0, 0, 6, call["obs"][:0], 8, binding.covis_params(), 4, rows=[0]), "no map")
    _refused(lambda: twin_frames(call, np.zeros((1, 6), np.int32), np.zeros(1, np.int32), [1], {}, 4), "ss_covis_frames_host: row 0: block 1 lies outside the map's 1")
    assert lib.ss_covis_kf_host(None, 0, 0, 0, 1, None, 0, None, 0, 8, None, 0, None, 1, None, None, None, 0) == binding.SS_ERR_INVALID_ARG
    # no context
    assert lib.ss_covis_set_map(None, None, 0, 0, 0, 1, None, 0, None, 0) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_covis_kf_device(None, None, 0, C.byref(p), 1, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_covis_frames_device(None, None, None, None, 0, C.byref(p), 1, None, None) == binding.SS_ERR_INVALID_ARG
    assert lib.ss_covis(None, 1, 0, None, 0, None, 0, C.byref(p), 1, None, None) == binding.SS_ERR_INVALID_ARG


def test_empty_queries_write_nothing():
    call = CC.single(SHARED["lonely"])
    nb, row = twin_kf(call, {}, 4, rows=[])
    assert nb.shape == (0, 4, 2) and len(row) == 0


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/covis_steps_asan.cpp: its own main, the steps header, -fsanitize=address,undefined; run as a child process with the
    environment as it is"""
    exe = str(tmp_path / "covis_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "covis_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
