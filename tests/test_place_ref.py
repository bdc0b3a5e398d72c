"""The place recognition on the CPU: the ABI surface, the host twin (ss_place_query_host: the text the kernels compile) against the
reference (tests/place_ref.py) byte for byte on every output of the shared scenes and of random databases, the scenes' hand-derived
candidates on the reference, the reference against the literal restatement of upstream's loops, the float truncation of the word
threshold, the refusals with their messages, and the steps under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import place_cases as PC
import place_ref as PR
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = PC.shared_cases()


def twin(k, **over):
    k = dict(k, **over)
    return binding.place_query_host(k["db_word"], k["db_value"], k["db_count"], k["n_words"], k["problems"], k["q_word"], k["q_value"], k["q_count"], k["q_kf"],
                                    k["q_problem"], k["nb"], binding.place_params(**k["params"]), k["cand_cap"], db_skip=k["db_skip"], q_nb=k["q_nb"], q_row=k["q_row"])


def same(tag, got, want):
    """byte for byte on cand, summary, words and score"""
    (cand, summary, words, score), (wcand, wsummary, wwords, wscore) = got, want
    for name in PR.SUMMARY_DTYPE.names:
        a, b = np.ascontiguousarray(summary[name]), np.ascontiguousarray(wsummary[name])
        assert a.tobytes() == b.tobytes(), f"{tag}: summary.{name} {a.tolist()[:8]} != {b.tolist()[:8]}"
    for name in PR.CAND_DTYPE.names:
        a, b = np.ascontiguousarray(cand[name]), np.ascontiguousarray(wcand[name])
        assert a.tobytes() == b.tobytes(), f"{tag}: cand.{name} {a.tolist()[:4]} != {b.tolist()[:4]}"
    assert cand.tobytes() == wcand.tobytes() and summary.tobytes() == wsummary.tobytes(), tag
    assert np.array_equal(words, wwords), f"{tag}: words differ at {np.argwhere(words != wwords)[:6].tolist()}"
    assert score.tobytes() == np.ascontiguousarray(wscore).tobytes(), f"{tag}: score differs at {np.argwhere(score.view(np.uint32) != wscore.view(np.uint32))[:6].tolist()}"


def test_abi_surface():
    assert C.sizeof(binding.PlaceParams) == 32 and binding.PLACE_CAND_DTYPE.itemsize == 24 and binding.PLACE_SUMMARY_DTYPE.itemsize == 48
    assert PR.CAND_DTYPE == binding.PLACE_CAND_DTYPE and PR.SUMMARY_DTYPE == binding.PLACE_SUMMARY_DTYPE
    assert PR.PROBLEM_DTYPE == binding.GBA_PROBLEM_DTYPE and PR.ROW_DTYPE == binding.COVIS_ROW_DTYPE
    assert (PR.MAX_DB, PR.MAX_QUERIES, PR.MAX_CANDIDATES, PR.MAX_NEIGHBOURS) == (binding.SS_PLACE_MAX_DB, binding.SS_PLACE_MAX_QUERIES, binding.SS_PLACE_MAX_CANDIDATES,
                                                                                 binding.SS_PLACE_MAX_NEIGHBOURS)
    assert binding.SS_PLACE_MAX_DB <= binding.SS_COVIS_MAX_MAP_KF and binding.SS_PLACE_MAX_NEIGHBOURS <= binding.SS_COVIS_MAX_NEIGHBOURS
    lib = binding.load()
    for sym in ("ss_place_params_default", "ss_place_set_database", "ss_place_query_device", "ss_place", "ss_place_query_host"):
        assert hasattr(lib, sym) and sym in binding.EXPORTS, sym
    header = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    for text in ("} ss_place_params;", "} ss_place_cand;", "} ss_place_summary;", "#define SS_PLACE_MAX_DB 262144", "#define SS_PLACE_MAX_QUERIES 256",
                 "#define SS_PLACE_MAX_CANDIDATES 256", "#define SS_PLACE_MAX_NEIGHBOURS 1024", "#define SS_ABI_VERSION 5"):
        assert text in header, text
    p = binding.PlaceParams()
    assert lib.ss_place_params_default(C.byref(p)) == binding.SS_OK
    d = binding.place_params()
    assert bytes(p) == bytes(d) and (p.min_score_mode, p.n_best, p.scope) == (1, 0, 1)
    assert np.float32(p.common_ratio) == np.float32(0.8) and np.float32(p.retain_ratio) == np.float32(0.75) and list(p.reserved) == [0, 0]


@pytest.mark.parametrize("name", sorted(SHARED))
def test_scene_reference_gives_the_hand_derived_candidates(name):
    k = SHARED[name]
    cand, summary, _, _ = PR.run(k)
    for q, rows in enumerate(k["expect"]):
        shown = rows[:k["cand_cap"]]
        assert cand[q]["kf"][:len(shown)].tolist() == shown and (cand[q]["kf"][len(shown):] == -1).all(), (name, cand[q]["kf"])
        assert summary[q]["n_candidates"] == len(rows) and summary[q]["n_written"] == len(shown)


def test_scenes_are_live():
    """each scene reaches the path it is named for, shown on the reference"""
    run = {n: PR.run(k) for n, k in SHARED.items()}
    s = {n: r[1][0] for n, r in run.items()}
    assert s["empty_query"]["n_sharing"] == 0 and s["shares_nothing"]["n_sharing"] == 0 and s["own_only_sharer"]["n_sharing"] == 0
    for n in ("connected_would_win", "skipped", "no_problem"):
        assert run[n][2][0][0] == 0 and s[n]["max_common"] == 3, n  # row 0, with four common words, does not vote
    assert run["connected_would_win"][3][0][0] == -1.0
    assert run["out_of_range"][2][0].tolist() == [1, 1, 0] and run["out_of_range"][3][0][0] == np.float32(0.1875)
    assert (s["max_common_5"]["max_common"], s["max_common_5"]["min_common"], s["max_common_5"]["n_survivors"]) == (5, 4, 1)
    assert (s["max_common_4"]["max_common"], s["max_common_4"]["min_common"], s["max_common_4"]["n_survivors"]) == (4, 3, 2)
    assert [s[n]["n_seeds"] for n in ("floor_equal", "floor_one_ulp_above", "floor_one_ulp_below")] == [1, 0, 1]
    assert s["mode1_no_connected"]["min_score"] == 1.0 and s["mode1_all_skipped"]["min_score"] == 1.0 and s["mode1_all_skipped"]["n_survivors"] == 2
    assert s["mode1_minimum_twice"]["min_score"] == np.float32(0.0625) and s["mode1_minimum_twice"]["n_seeds"] == 2
    assert s["non_seed_adds"]["n_seeds"] == 1 and s["non_seed_adds"]["n_survivors"] == 2 and s["non_seed_adds"]["best_acc"] == np.float32(0.234375)
    assert s["marked_not_survivor"]["n_sharing"] == 2 and s["marked_not_survivor"]["n_survivors"] == 1 and s["marked_not_survivor"]["best_acc"] == np.float32(0.3125)
    assert s["two_seeds_one_best"]["n_seeds"] == 3 and run["two_seeds_one_best"][0][0][0]["acc"] == np.float32(0.5625)
    assert s["cut_exact"]["n_seeds"] == 2 and s["cut_one_ulp_above"]["n_candidates"] == 2
    assert run["equal_acc"][0][0]["acc"][:2].tolist() == [0.25, 0.25] and s["cand_cap_small"]["n_candidates"] == 2
    assert run["n_best_3"][0][0]["class"][:6].tolist() == [1, 1, 1, 0, 0, 0] and run["n_best_3"][0][0]["problem"][:6].tolist() == [2, 2, 2, 1, 1, 1]
    assert s["scope_0_after_merge"]["max_common"] == 5 and s["scope_0_after_merge"]["n_seeds"] == 1 and s["scope_0_after_merge"]["n_candidates"] == 0
    assert PR.run(SHARED["scope_0_after_merge"], params=dict(SHARED["scope_0_after_merge"]["params"], scope=1))[0][0][0]["kf"] == 2
    assert s["nb_end_marker_first"]["best_acc"] == np.float32(0.125) and s["nb_cap_1"]["best_acc"] == np.float32(0.1875)
    z = run["zero_score"]
    assert z[3][0][0] == 0.0 and np.signbit(z[3][0][0]) and z[1][0]["n_seeds"] == 1 and np.signbit(z[1][0]["best_acc"]) and z[1][0]["n_candidates"] == 0
    assert np.signbit(run["zero_score_n_best"][0][0][0]["acc"])


@pytest.mark.parametrize("name", sorted(SHARED))
def test_host_twin_matches_reference_on_the_scenes(name):
    same(name, twin(SHARED[name]), PR.run(SHARED[name]))


@pytest.mark.parametrize("seed,n_db,kw", [(1, 9, {}), (2, 40, dict(mode=0)), (3, 70, dict(n_best=2, n_problems=3)), (4, 33, dict(scope=0, n_problems=3)),
                                          (5, 25, dict(conn=False, mode=0)), (6, 50, dict(empty=(1, 4), cand_cap=2)), (7, 1, dict(n_problems=1))])
def test_host_twin_matches_reference_on_random_databases(seed, n_db, kw):
    k = PC.random_case(seed, n_db, 8, **kw)
    want = PR.run(k)
    assert n_db == 1 or (want[1]["n_candidates"].max() > 0 and want[1]["n_survivors"].max() > 1)  # the scene n_db_1 is the live one-row case
    same(f"seed {seed}", twin(k), want)


def distinct(k, q):
    """no two acc* equal and no marked neighbour unscored: where the two restatements are defined to agree"""
    cand, summary, words, score = PR.run(k, cand_cap=PR.MAX_CANDIDATES, params=dict(k["params"], n_best=PR.MAX_CANDIDATES, scope=1))
    acc = cand[q]["acc"][:summary[q]["n_written"]]
    if len(set(acc.tolist())) != len(acc):
        return False
    db = PR.Database(k["db_word"], k["db_value"], k["db_count"], k["n_words"], k["problems"], k["db_skip"])
    for i in np.flatnonzero(score[q] >= summary[q]["min_score"]):
        for kf, _ in k["nb"][i]:
            j = None if kf < 0 else db.row_of(db.problem[i], int(kf))
            if kf < 0:
                break
            if j is not None and words[q][j] > 0 and words[q][j] <= summary[q]["min_common"]:
                return False
    return True


def test_reference_and_upstream_restatement_give_the_same_set():
    """The rule against the literal loops (marks, list pushes, GetBestCovisibilityKeyFrames, a set): the same candidate SET.  Only queries
    without equal acc* and without a marked neighbour that was never scored are compared (`distinct`): there upstream's order-dependent
    ties and the stale score of DetectNBestCandidates are the documented deviations."""
    compared = nonempty = 0
    cases = [k for n, k in sorted(SHARED.items()) if n not in ("equal_acc", "cand_cap_small", "marked_not_survivor")]
    cases += [PC.random_case(seed, 30, 8, mode=seed % 2, n_best=(0, 2)[seed % 3 == 0], scope=seed % 2, n_problems=1 + seed % 3) for seed in range(10, 34)]
    for k in cases:
        cand, summary, _, _ = PR.run(k, cand_cap=PR.MAX_CANDIDATES)
        for q in range(len(k["q_kf"])):
            if not distinct(k, q):
                continue
            assert PR.upstream(k, q) == set(cand[q]["kf"][:summary[q]["n_written"]].tolist()), q
            compared, nonempty = compared + 1, nonempty + (summary[q]["n_written"] > 0)
    assert compared >= 60 and nonempty >= 20, (compared, nonempty)


def test_word_threshold_truncation():
    """(int)((float)m * 0.8f) against the exact floor(4 m / 5): equal for every m below 5 242 881, where the float product 4 194 304.8 has
    half-unit spacing and rounds up to 4 194 305.  A query has at most 16 384 words, so no reachable max_common truncates differently;
    the step is restated here and the reachable range is what the scenes pin (5 -> 4, 4 -> 3)."""
    m = np.arange(1, 1 << 24, dtype=np.int64)
    got = (m.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    bad = np.flatnonzero(got != (4 * m) // 5)
    assert m[bad[0]] == 5242881 and got[bad[0]] == 4194305
    assert PR.min_common_of(5) == 4 and PR.min_common_of(4) == 3 and PR.min_common_of(5242881) == 4194305 and PR.min_common_of(16384) == 13107


BASE = PC.random_case(1, 9, 2)


def refusal(msg, code=binding.SS_ERR_INVALID_ARG, **over):
    with pytest.raises(binding.OrbError) as e:
        twin(BASE, **over)
    assert e.value.code == code and msg in e.value.message, e.value.message


def test_refusals_name_the_argument():
    pr = BASE["params"]
    refusal("n_words", n_words=0)
    refusal("n_words", n_words=(1 << 24) + 1)
    refusal("cand_cap", cand_cap=0)
    refusal("cand_cap", cand_cap=PR.MAX_CANDIDATES + 1)
    refusal("nb_cap", nb=np.zeros((9, PR.MAX_NEIGHBOURS + 1, 2), np.int32))
    refusal("q_cap", q_nb=np.zeros((2, PR.MAX_NEIGHBOURS + 1, 2), np.int32))
    refusal("q_kf", q_kf=np.array([9, -1], np.int32))
    refusal("q_kf", q_kf=np.array([-2, -1], np.int32))
    refusal("q_problem", q_kf=np.array([-1, -1], np.int32), q_problem=np.array([2, 0], np.int32))
    refusal("q_problem", q_kf=np.array([-1, -1], np.int32), q_problem=np.array([-1, 0], np.int32))
    kf0 = np.array([0, -1], np.int32)
    refusal("contradicts q_kf", q_kf=kf0, q_problem=np.array([1, 0], np.int32))
    refusal("problems[1]", problems=PR.problems_table([(0, 5), (4, 4)]))
    refusal("problems[0]", problems=PR.problems_table([(0, 10)]))
    refusal("problems[0]", problems=PR.problems_table([(0, 0)]))
    refusal("min_score_mode", params=dict(pr, min_score_mode=2))
    refusal("min_score", params=dict(pr, min_score=float("nan")))
    refusal("n_best", params=dict(pr, n_best=-1))
    refusal("n_best", params=dict(pr, n_best=PR.MAX_CANDIDATES + 1))
    refusal("scope", params=dict(pr, scope=2))
    refusal("common_ratio", params=dict(pr, common_ratio=1.5))
    refusal("retain_ratio", params=dict(pr, retain_ratio=float("nan")))
    refusal("reserved", params=dict(pr, reserved=(0, 1)))
    lib, p, err = binding.load(), binding.place_params(), C.create_string_buffer(256)
    a = np.zeros(64, np.float64)
    args = lambda **o: [o.get(n, d) for n, d in (("dw", a.ctypes.data), ("dv", a.ctypes.data), ("dc", a.ctypes.data), ("sk", None), ("n_db", 2), ("stride", 2), ("n_words", 8),  # noqa: E731
                                                 ("pr", PR.problems_table([(0, 2)]).ctypes.data), ("npr", 1), ("qw", a.ctypes.data), ("qv", a.ctypes.data), ("qc", a.ctypes.data),
                                                 ("q_stride", 2), ("n_q", 1), ("qk", a.ctypes.data), ("qp", a.ctypes.data), ("qn", None), ("qr", None), ("q_cap", 0),
                                                 ("nb", a.ctypes.data), ("nb_cap", 1), ("p", C.byref(p)), ("cand_cap", 1), ("cand", a.ctypes.data), ("sum", a.ctypes.data),
                                                 ("words", None), ("score", None))] + [err, len(err)]
    table = PR.problems_table([(0, 2)])
    for over, msg in ((dict(dw=None), "db_word"), (dict(qv=None), "q_value"), (dict(qk=None), "q_kf"), (dict(qp=None), "q_problem"), (dict(nb=None), "nb is NULL"),
                      (dict(cand=None), "cand"), (dict(pr=None), "problems is NULL"), (dict(qn=a.ctypes.data), "q_nb and q_row"), (dict(n_db=PR.MAX_DB + 1), "SS_PLACE_MAX_DB"),
                      (dict(n_q=PR.MAX_QUERIES + 1), "SS_PLACE_MAX_QUERIES"), (dict(stride=0), "stride"), (dict(q_stride=0), "q_stride"),
                      (dict(n_db=1 << 18, stride=1 << 13, pr=table.ctypes.data), "2^31"), (dict(p=None), "params is NULL"), (dict(n_db=0), "n_db")):
        assert lib.ss_place_query_host(*args(**over)) == binding.SS_ERR_INVALID_ARG and msg in err.value.decode(), (over, err.value)
    assert lib.ss_place_query_host(*args()) == binding.SS_OK


def test_steps_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/place_steps_asan.cpp: its own main, the steps headers, -fsanitize=address,undefined; run as a child process with the
    environment as it is"""
    exe = str(tmp_path / "place_steps_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "place_steps_asan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
