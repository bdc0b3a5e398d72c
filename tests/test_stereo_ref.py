"""CPU tests of the stereo depth path: the numpy restatement (tests/stereo_ref.py) against its committed goldens, its
geometric behaviour on pairs with known disparities, and the presence of the new C ABI symbols and their binding."""
import ctypes as C
import glob
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import stereo_ref as R
from send_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stereo", "*.npz")))


def test_stereo_golden_set_is_present_and_small():
    assert len(GOLDEN) == 6
    assert sum(os.path.getsize(p) for p in GOLDEN) < 1 << 20


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_reference_reproduces_golden(path, oracle):
    z = np.load(path)
    p = oracle.default_params(n_features=int(z["n_features"]), lapping_x0=0, lapping_x1=0, scale_factor=float(z["scale_factor"]),
                              n_levels=int(z["n_levels"]))
    kL, dL, kR, dR, pts, summ = R.stereo_pair(z["left"], z["right"], p, z["fx"], z["baseline"], z["th_depth"])
    assert pts.dtype == z["points"].dtype and pts.tobytes() == z["points"].tobytes()
    assert [summ[k] for k in R.SUMMARY_FIELDS] == list(z["summary"])


@pytest.mark.parametrize("w,h,nf,t,seed", [(640, 480, 1000, 4, 7), (1280, 720, 2000, 6, 3), (320, 240, 500, 3, 11)])
def test_disparities_of_a_parallax_pair(oracle, w, h, nf, t, seed):
    """left = frame t, right = frame 0 of one parallax scene: band b has disparity disparities[b] * t.  At least 95 % of the
    points with depth lie within one pixel of their own octave (scale^octave level-0 px) of their band's value, keypoints
    on a band boundary included in the count."""
    p = oracle.default_params(n_features=nf, lapping_x0=0, lapping_x1=0)
    sc = synth.scene(seed, w, h)
    left, right = synth.parallax_frame(seed, w, h, t, sc=sc), synth.parallax_frame(seed, w, h, 0, sc=sc)
    kL, dL, kR, dR, pts, summ = R.stereo_pair(left, right, p, 500.0, 0.1, 35.0)
    scale = R.level_scales(p, w, h)
    disp = synth.PARALLAX_DISPARITIES
    nb = len(disp)
    ok = pts["depth"] > 0
    assert ok.sum() >= 0.4 * len(kL)
    good = 0
    for i in np.flatnonzero(ok):
        y = int(kL["y"][i])
        b = next(b for b in range(nb) if h * b // nb <= y < h * (b + 1) // nb)
        good += abs(float(kL["x"][i]) - float(pts["u_right"][i]) - disp[b] * t) <= float(scale[int(kL["octave"][i])])
    print(f"{w}x{h} t={t}: {good} of {int(ok.sum())} within one octave pixel ({100.0 * good / ok.sum():.1f} %)")
    assert good >= 0.95 * ok.sum()
    # depth = bf / disparity and the close / far split
    bf = np.float32(np.float32(0.1) * np.float32(500.0))
    d = kL["x"][ok] - pts["u_right"][ok]
    assert np.array_equal(pts["depth"][ok], (bf / d).astype(np.float32))
    assert summ["n_close"] == int((pts["depth"][ok] < np.float32(np.float32(bf * np.float32(35.0)) / np.float32(500.0))).sum())


def _stereo_params(oracle, nf, scale=1.2, levels=8):
    return oracle.default_params(n_features=nf, lapping_x0=0, lapping_x1=0, scale_factor=scale, n_levels=levels)


def test_tiny_pairs_have_one_two_and_three_refined_points(oracle):
    """no vacuous pass on the GPU: the pairs of test_stereo.test_tiny_counts_through_the_median_select put 1, 2 and 3 SADs
    through the median; with two, the median is the LARGER one (element [n / 2]) and the cut, 2.1 times it, drops neither --
    the smaller one as the median would drop the larger"""
    import test_stereo as T
    want = {"patch22": (1, 389), "patch26": (2, 4656), "flat": (0, -1), "patch28": (3, 379)}
    pairs = T.tiny_pairs()
    assert [n for n, _ in pairs] == list(want)
    for name, (l, r) in pairs:
        st = Counter()
        kL, dL, kR, dR, pts, summ = R.stereo_pair(l, r, _stereo_params(oracle, 500), 500.0, T.BASELINE, T.TH_DEPTH, st)
        print(name, summ, dict(st))
        assert st["guard"] == 0 and (summ["n_refined"], summ["sad_median"]) == want[name]
        assert summ["n_depth"] == summ["n_refined"] and st["median_cut"] == 0
        if name == "flat":
            assert summ["n_left"] == summ["n_right"] == 0
        if name == "patch26":
            lo, hi = sorted(int(s) for s in pts["sad"][pts["depth"] > 0])
            assert hi == summ["sad_median"] and hi >= np.float32(np.float32(1.5) * np.float32(1.4)) * np.float32(lo) > lo


def test_odd_width_pairs_and_pyramid_shapes_have_depth(oracle):
    """the pairs of test_stereo.test_level_0_* and test_pyramid_shapes: no guard, a median cut that bites, enough depth; the
    narrow disparity range of fx = 20 rejects matches; every level of each pyramid holds keypoints"""
    import test_stereo as T
    for (w, h, t, seed), (n_depth, n_refined) in zip(T.ODD_PAIRS, ((201, 279), (290, 368))):
        assert w % 16 != 0 and 336 % 16 == 0 and 336 >= w
        left, right = T._parallax_pair(w, h, t, seed)
        summ = {}
        for fx in (500.0, 20.0):
            st = Counter()
            summ[fx] = R.stereo_pair(left, right, _stereo_params(oracle, 500), fx, T.BASELINE, T.TH_DEPTH, st)[5]
            assert st["guard"] == 0 and st["median_cut"] >= 1
        assert (summ[500.0]["n_depth"], summ[500.0]["n_refined"]) == (n_depth, n_refined)
        assert 0 < summ[20.0]["n_matched"] < summ[500.0]["n_matched"]
    for w, h, nf, t, seed, scale, levels in T.PYRAMIDS:
        left, right = T._parallax_pair(w, h, t, seed)
        st = Counter()
        kL, dL, kR, dR, pts, summ = R.stereo_pair(left, right, _stereo_params(oracle, nf, scale, levels), 500.0, T.BASELINE, T.TH_DEPTH, st)
        print(w, h, scale, levels, summ, dict(st))
        assert st["guard"] == 0 and st["median_cut"] >= 1 and summ["n_depth"] > 300
        assert set(kL["octave"].tolist()) == set(range(levels)) and len(R.level_scales(_stereo_params(oracle, nf, scale, levels), w, h)) == levels


def test_parabola_offset_is_bounded():
    """With d2 the first minimum of the 11 sums and an interior one, d1 > d2 <= d3: delta = (a - b) / (2 (a + b)) with
    a = d1 - d2 > 0, b = d3 - d2 >= 0 lies in [-0.5, 0.5] -- the |delta| > 1, inf and NaN branches of the routine are
    unreachable for integer sums, which is why no test input reaches them.  Exhaustive over small sums in float32."""
    f = np.float32
    for d2 in (0, 1, 7, 30855 - 40):
        for a in range(1, 40):
            for b in range(0, 40):
                d1, d3 = f(d2 + a), f(d2 + b)
                delta = f(d1 - d3) / f(f(2.0) * f(f(d1 + d3) - f(f(2.0) * f(d2))))
                assert -0.5 <= delta <= 0.5


def test_round_is_half_away_from_zero():
    assert [R.c_round(np.float32(v)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 2.4999, 7.0)] == [1, 2, 3, -1, -2, 2, 7]


def test_stereo_symbols_are_declared_exported_and_bound():
    from send_slam_amd import binding
    header = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "send-slam_amd"), "-s"])
    lib = binding.load()
    for name in ("ss_stereo_batch_device", "ss_extract_stereo"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert name in binding.EXPORTS and hasattr(lib, name), f"{name} is not exported / bound"
    assert lib.ss_abi_version() == 5
    assert C.sizeof(binding.StereoParams) == 12 and C.sizeof(binding.StereoSummary) == 32
    assert binding.STEREO_POINT_DTYPE.itemsize == 16 and binding.STEREO_SUMMARY_DTYPE.itemsize == 32
    assert binding.STEREO_POINT_DTYPE == R.POINT_DTYPE
    assert [n for n, _ in binding.StereoSummary._fields_] == list(R.SUMMARY_FIELDS)
    assert callable(binding.OrbContext.stereo_batch_device) and callable(binding.OrbContext.extract_stereo)
    # the header's own layout, as a C compiler sees it
    src = ('#include "sendslam_orb.h"\n#include <stddef.h>\n'
           '_Static_assert(sizeof(ss_stereo_params) == 12, "params");\n_Static_assert(sizeof(ss_stereo_point) == 16, "point");\n'
           '_Static_assert(offsetof(ss_stereo_point, right_idx) == 8 && offsetof(ss_stereo_point, sad) == 14, "point fields");\n'
           '_Static_assert(sizeof(ss_stereo_summary) == 32 && offsetof(ss_stereo_summary, sad_median) == 28, "summary");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(), check=True)
