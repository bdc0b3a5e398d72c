"""CPU tests of the guided-matching rule as tests/guided_ref.py states it, and of its C ABI surface: the reference against
the all-pairs oracle, its two forms of the candidate set against each other, the float32 corner cases of the rotation
histogram, the committed goldens, the declared / exported / bound symbols."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import guided_cases as G
import guided_ref as R
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sendslam_orb.h")
PAIRS = [("synth_t1", "synth_t0"), ("dots_shift", "dots"), ("noise_shift", "noise")]


@pytest.mark.parametrize("query,train", PAIRS)
def test_whole_image_window_equals_the_all_pairs_oracle(oracle, query, train):
    """a window that holds every train row reproduces ss_match's rule: idx, d1, d2 equal to oracle.match"""
    qk, qd = G.features(query)
    tk, td = G.features(train)
    assert len(qk) > 100 and len(tk) > 100
    idx, d1, d2, summ, _ = R.match(qk, qd, tk, td, R.whole_windows(len(qk)), th=50, ratio_num=9, ratio_den=10)
    oidx, od1, od2 = oracle.match(qd, td, 50, 9, 10)
    assert np.array_equal(idx, oidx) and np.array_equal(d1, od1) and np.array_equal(d2, od2)
    assert summ["n_candidates"] == len(qk) * len(tk) and summ["n_accepted"] == int((oidx >= 0).sum())
    # and with the self pair excluded, on one frame
    idx, d1, d2, _, _ = R.match(qk, qd, qk, qd, R.whole_windows(len(qk)), exclude_self=True)
    oidx, od1, od2 = oracle.match(qd, qd, 50, 9, 10, exclude_self=True)
    assert np.array_equal(idx, oidx) and np.array_equal(d1, od1) and np.array_equal(d2, od2)


@pytest.mark.parametrize("query,train", PAIRS)
def test_grid_walk_and_box_test_give_the_same_candidates(query, train):
    """Frame::GetFeaturesInArea on upstream's 64 x 48 grid, as written, against the closed-form box: the grid only finds the
    candidates faster.  Also the serial box against the element-wise one the reference's search runs on."""
    qk, _ = G.features(query)
    tk, _ = G.features(train)
    win = G.own_windows(qk)
    grid, dropped = R.grid_candidates(win, tk, G.W, G.H)
    assert dropped == 0  # extractor keypoints keep 19 px from the border: every one is in the grid
    mask = R._box_mask(win, tk)
    total = 0
    for i in range(len(qk)):
        box = R.box_candidates(win[i], tk)
        assert grid[i] == box, (i, grid[i], box)
        assert box == list(np.flatnonzero(mask[i]))
        total += len(box)
    assert total > 1000


def test_three_maxima_in_float32():
    def hist(**bins):
        h = [0] * R.HISTO_LENGTH
        for k, v in bins.items():
            h[int(k[1:])] = v
        return h

    assert R.three_maxima(hist()) == (-1, -1, -1)
    assert R.three_maxima(hist(b4=7)) == (4, -1, -1)
    # ties keep the lower bin: the scan compares with a strict >
    assert R.three_maxima(hist(b3=5, b9=5, b20=5, b25=5)) == (3, 9, 20)
    assert R.three_maxima(hist(b2=4, b7=9, b11=9)) == (7, 11, 2)
    # 0.1f * 10.0f rounds to 1.0f, and 1 < 1 is false: kept.  0.1f * 11.0f = 1.1f: dropped
    assert np.float32(0.1) * np.float32(10) == np.float32(1)
    assert R.three_maxima(hist(b5=10, b6=1)) == (5, 6, -1)
    assert R.three_maxima(hist(b5=10, b6=1, b8=1)) == (5, 6, 8)
    assert R.three_maxima(hist(b5=11, b6=1)) == (5, -1, -1)
    assert R.three_maxima(hist(b5=11, b6=2, b8=1)) == (5, 6, -1)
    assert R.pack_bins((5, 6, -1)) == 0xFF0605 and R.pack_bins((-1, -1, -1)) == 0xFFFFFF


def test_rotation_bins_in_float32():
    # factor 2 = 30 / 360.0f: 12 degrees per bin, bin 30 wraps to 0
    assert R.rot_bin(359.0, 0.0, 2) == 0 and R.rot_bin(354.1, 0.0, 2) == 0 and R.rot_bin(353.9, 0.0, 2) == 29
    assert R.rot_bin(0.0, 1.0, 2) == 0  # -1 -> 359
    assert R.rot_bin(6.1, 0.0, 2) == 1 and R.rot_bin(5.9, 0.0, 2) == 0
    assert R.rot_bin(10.0, 350.0, 2) == 2  # -340 -> 20
    # factor 1 = 1.0f / 30: bins 0 .. 12 only, 359 degrees lands in bin 12, not 0
    assert R.rot_bin(359.0, 0.0, 1) == 12 and R.rot_bin(0.0, 1.0, 1) == 12
    assert {R.rot_bin(a, 0.0, 1) for a in np.arange(0, 360, 0.25)} == set(range(13))
    assert {R.rot_bin(a, 0.0, 2) for a in np.arange(0, 360, 0.25)} == set(range(30))
    # half away from zero: 45 / 30 = 1.5 -> 2
    assert R.rot_bin(45.0, 0.0, 1) == 2 and R.rot_bin(15.0, 0.0, 1) == 1
    # outside [0, 360) or NaN: no bin
    assert R.rot_bin(1000.0, 0.0, 2) == -1 and R.rot_bin(float("nan"), 0.0, 1) == -1


def test_windows_keep_matches_the_all_pairs_ratio_test_throws_away(oracle):
    """the motivating fact, on the reference: on repetitive content the ratio test against the whole image rejects matches
    that the same test inside a 15 px window accepts"""
    qk, qd = G.features("dots_shift")
    tk, td = G.features("dots")
    windowed = G.reference_pair("dots_shift", "dots", G.COMBOS[0])[3]
    all_pairs = int((oracle.match(qd, td, 50, 9, 10)[0] >= 0).sum())
    no_ratio = G.reference_pair("dots_shift", "dots", dict(th=100, ratio_num=0, ratio_den=0))[3]
    print(windowed, all_pairs, no_ratio)
    assert windowed["n_accepted"] > all_pairs > 0
    assert no_ratio["n_accepted"] == len(qk) >= windowed["n_accepted"]
    assert windowed["n_candidates"] < len(qk) * len(tk) // 20


def test_every_filter_has_work_on_the_batch():
    """no vacuous pass on the GPU: on the shared batch the acceptance test, one_to_one and both orientation forms each reject
    something, and the checker pair keeps three bins"""
    for c in G.COMBOS:
        s = G.reference_pair("synth_t1", "synth_t0", c)[3]
        assert 0 < s["n_accepted"] < s["n_query"] and s["n_candidates"] > 10 * s["n_query"]
        if c["one_to_one"]:
            assert s["n_unique"] < s["n_accepted"]
        if c["orientation"]:
            assert s["n_final"] < s["n_unique"]
    s = G.reference_pair("checker_shift", "checker", dict(G.RULES[0], one_to_one=False, orientation=1))[3]
    assert all(((s["rot_bins"] >> k) & 0xFF) != 0xFF for k in (0, 8, 16))


def _accepted(b, combo):
    """the rows the accepted queries of capacity frame b point at, before one_to_one and orientation"""
    idx = G.capacity_reference(b, dict(combo, one_to_one=False, orientation=0))[0]
    return idx[idx >= 0]


@pytest.mark.parametrize("combo", G.CAP_COMBOS, ids=G.combo_name)
def test_capacity_frames_need_both_conflict_passes(combo):
    """no vacuous pass on the GPU, asserted on the reference: at SS_GUIDED_MAX_ROWS train rows the accepted queries point at
    both halves of the train set, rows that several accepted queries want exist in both halves (the planted ones at 8191,
    8192 and 16383 among them), both filters drop something, and matches beyond 2^24 px survive"""
    f0, f1 = G.capacity_frames()
    assert len(f0["t_kp"]) == len(f1["q_kp"]) == G.CAP_ROWS == binding.SS_GUIDED_MAX_ROWS == 2 * G.CAP_KEY_ROWS
    assert len(f0["q_kp"]) == len(f1["t_kp"]) == 3006
    rows = _accepted(0, combo)
    wanted, times = np.unique(rows, return_counts=True)
    contested = wanted[times >= 2]
    lo, hi = int((rows < G.CAP_KEY_ROWS).sum()), int((rows >= G.CAP_KEY_ROWS).sum())
    clo, chi = int((contested < G.CAP_KEY_ROWS).sum()), int((contested >= G.CAP_KEY_ROWS).sum())
    idx, _, _, s, cands = G.capacity_reference(0, combo)
    print(G.combo_name(combo), s, "accepted", lo, hi, "contested rows", clo, chi)
    assert lo > 500 and hi > 500 and clo > 50 and chi > 50
    assert set(G.CAP_PLANTED) <= set(contested.tolist())
    assert s["n_candidates"] > 1000000 and s["n_unique"] < s["n_accepted"] == lo + hi
    if combo["orientation"] == 2:
        assert 0 < s["n_final"] < s["n_unique"]
    else:
        # of each planted pair the first query keeps the row; the far queries keep their rows beyond 2^24 px
        assert list(idx[-6:]) == [8191, -1, 8192, -1, 16383, -1]
        far = idx[[30, 31, 32, 1500, 1501, 1502]]
        assert list(far) == [101, 9001, 102, 9002, 103, 9003] and (f0["t_kp"]["x"][far] > G.CAP_FAR).all()
        assert f0["t_kp"]["y"][9003] > G.CAP_FAR and f0["windows"]["y"][1502] == G.CAP_FAR
    # frame 1: more queries than any other frame of the suite, most of them contesting a row
    s1 = G.capacity_reference(1, combo)[3]
    print(s1)
    assert s1["n_query"] == G.CAP_ROWS and s1["n_unique"] < s1["n_accepted"] // 2 and s1["n_unique"] > 1000
    assert np.unique(_accepted(1, combo) // 1024).size == 3  # every part of the 3006 train rows is wanted


def test_capacity_extents_form_the_grids_they_are_there_for():
    assert G.grid_shift(G.W, G.H) == G.grid_shift(1280, 720) == G.grid_shift(5000, 37) == 5  # all the suite had
    assert G.grid_shift(G.CAP_W, G.CAP_H) == 6
    assert [G.grid_shift(*e) for e in G.CAP_EXTENTS] == [8, 12, 5]
    assert G.CAP_EXTENTS[1][0] > G.CAP_FAR and ((G.CAP_EXTENTS[2][0] - 1) >> 5) + 1 == 2


def test_degenerate_windows():
    qk, qd = G.features("synth_t1")
    tk, td = G.features("synth_t0")
    win = G.own_windows(qk)
    base = R.match(qk, qd, tk, td, win)
    w = win.copy()
    w["radius"][0::4] = 0
    w["radius"][1::4] = -3
    w["radius"][2::4] = np.nan
    w["oct_lo"][3::4], w["oct_hi"][3::4] = 3, 2
    idx, d1, d2, summ, cands = R.match(qk, qd, tk, td, w)
    assert summ["n_candidates"] == 0 and (idx == -1).all() and (d1 == R.NONE).all() and (d2 == R.NONE).all()
    assert base[3]["n_candidates"] > 0
    # no train frame at all
    idx, d1, d2, summ, _ = R.match(qk, qd, None, None, win)
    assert summ["n_train"] == 0 and (idx == -1).all() and (d1 == R.NONE).all()


def test_goldens_reproduce(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "guided", "*.npz")))
    assert len(files) >= 3
    assert sum(os.path.getsize(f) for f in files) < 1 << 20
    for path in files:
        g = np.load(path)
        query, train = os.path.basename(path)[:-4].split("_vs_")
        qk, qd = G.features(query)
        tk, td = G.features(train)
        # the inputs are what the oracle extracts today, the windows what the batch form derives
        assert g["q_kp"].tobytes() == qk.tobytes() and np.array_equal(g["q_desc"], qd)
        assert g["t_kp"].tobytes() == tk.tobytes() and np.array_equal(g["t_desc"], td)
        assert g["windows"].tobytes() == G.own_windows(qk).tobytes()
        for c in G.COMBOS:
            n = G.combo_name(c)
            idx, d1, d2, summ, _ = R.match(g["q_kp"], g["q_desc"], g["t_kp"], g["t_desc"], g["windows"], **c)
            assert np.array_equal(idx, g[n + "_idx"]) and np.array_equal(d1, g[n + "_d1"]) and np.array_equal(d2, g[n + "_d2"]), (path, n)
            assert [summ[f] for f in R.SUMMARY_FIELDS] == list(g[n + "_summary"]), (path, n)


def test_symbols_are_declared_exported_and_bound(tmp_path):
    names = ["ss_match_guided_pairs_device", "ss_match_guided_batch_device", "ss_match_guided"]
    text = open(HEADER).read()
    lib = binding.load()
    for n in names:
        assert n + "(" in text and n in binding.EXPORTS and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    for m in ("match_guided_pairs_device", "match_guided_batch_device", "match_guided"):
        assert callable(getattr(binding.OrbContext, m))
    assert C.sizeof(binding.GuidedParams) == 40 and C.sizeof(binding.GuidedSummary) == 32
    assert binding.GUIDED_WINDOW_DTYPE.itemsize == 16 and binding.GUIDED_SUMMARY_DTYPE.itemsize == 32
    assert binding.GUIDED_WINDOW_DTYPE == R.WINDOW_DTYPE
    assert tuple(n for n, _ in binding.GuidedSummary._fields_) == R.SUMMARY_FIELDS
    assert binding.SS_GUIDED_MAX_ROWS == 16384
    src = tmp_path / "sizes.c"
    src.write_text('#include "sendslam_orb.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ss_guided_window) == 16, "window");\n'
                   '_Static_assert(sizeof(ss_guided_params) == 40, "params");\n'
                   '_Static_assert(sizeof(ss_guided_summary) == 32, "summary");\n'
                   '_Static_assert(offsetof(ss_guided_window, oct_lo) == 12 && offsetof(ss_guided_params, radius) == 20, "fields");\n'
                   '_Static_assert(offsetof(ss_guided_params, extent_w) == 32 && offsetof(ss_guided_summary, rot_bins) == 28, "fields");\n'
                   '_Static_assert(SS_GUIDED_MAX_ROWS == 16384 && SS_ABI_VERSION == 5, "constants");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    assert lib.ss_abi_version() == 5 and binding.ABI_VERSION == 5
