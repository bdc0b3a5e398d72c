"""CPU tests of the stereo form of the triangulation: the host twin ss_triangulate_stereo_host (the text the kernel compiles) against
tests/tri_stereo_ref.py byte for byte; the modes and the fall-through from both sides of their inequalities; the else-if quirk; the
stereo error at its bound; all planes -1 against ss_triangulate_host; the closed form of the stereo parallax against libm."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import epi_ref as E
import tri_stereo_cases as K
import tri_stereo_ref as T
from send_slam_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["ss_triangulate_stereo_host", "ss_triangulate_stereo_pairs_device", "ss_triangulate_stereo_batch_device"]
f32 = np.float32


def test_header_structs_and_exports():
    lib = binding.load()
    text = open(os.path.join(ROOT, "include", "sendslam_orb.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\(", code), name
        assert name in binding.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(binding.TriStereoRig) == 32 == binding.TRI_STEREO_RIG_DTYPE.itemsize and C.sizeof(binding.TriStereoParams) == 40
    assert binding.TRI_STEREO_INFO_DTYPE.itemsize == 32 == T.INFO_DTYPE.itemsize and binding.TRI_STEREO_SUMMARY_DTYPE.itemsize == 80
    assert C.sizeof(binding.TriParams) == 32 and binding.TRI_INFO_DTYPE.itemsize == 16  # the mono form's structs stay as they are


def same_rows(tag, got, want):
    (gi, gp), (wi, wp) = got, want
    for f in T.INFO_DTYPE.names:
        bad = np.flatnonzero(np.ascontiguousarray(gi[f]).view(np.uint32) != np.ascontiguousarray(wi[f]).view(np.uint32))
        assert len(bad) == 0, f"{tag}: {f} differs at rows {bad[:6]}: {gi[f][bad[:6]]} != {wi[f][bad[:6]]}"
    assert np.ascontiguousarray(gp).tobytes() == np.ascontiguousarray(wp).tobytes(), f"{tag}: points differ"


@pytest.mark.parametrize("k", range(K.F))
def test_twin_equals_the_reference_on_mixed_rows(k):
    want = K.reference_rows(k)
    same_rows(f"pair {k}", K.twin_rows(k), want)
    s = K.summary_of(want[0])
    print(k, s)
    assert s["n_points"] > 10
    if k == 0:
        assert s["n_mode"][0] > 10  # the wide baseline triangulates
    else:
        assert s["n_mode"][1] > 3 and s["n_mode"][2] > 3 and s["n_state"][1] > 3  # the short one unprojects, or gives up on mono rows
    # row 20: its right coordinate is 9 px off; the mono form accepts the row
    c = K.pair_case(k)
    if c["right1"][20] >= 0 and 0 <= c["idx"][20] < K.ROWS:
        assert want[0]["state"][20] == 5 and K.reference_rows(k, mono=True)[0]["state"][20] != 5


def test_all_three_modes_are_present_over_the_pairs():
    modes = np.sum([K.summary_of(K.reference_rows(k)[0])["n_mode"] for k in range(K.F)], axis=0)
    assert (modes > 5).all(), modes


@pytest.mark.parametrize("k", range(K.F))
def test_all_planes_minus_one_is_the_mono_form(k):
    """states, points and the shared numbers of the info, byte for byte"""
    c = K.pair_case(k)
    ok = np.flatnonzero((c["idx"] >= 0) & (c["idx"] < K.ROWS))
    kp1, kp2 = c["q_kp"][ok], c["t_kp"][c["idx"][ok]]
    tp = binding.tri_params(**{n: K.TP[n] for n in ("cos_parallax_max", "chi2", "ratio_factor", "far_limit")})
    pts, info = binding.triangulate_host(K.twin_pair(k), tp, K.scale(), kp1, kp2)
    minus = np.full(len(ok), -1.0, np.float32)
    for planes in ((None,) * 4, (minus,) * 4):
        spts, sinfo = binding.triangulate_stereo_host(K.twin_pair(k), K.twin_rig(c["rig"]), K.twin_params(), K.scale(), kp1, kp2, *planes)
        assert spts.tobytes() == pts.tobytes()
        for a, b in (("state", "state"), ("cos_rays", "cos_parallax"), ("err1_sq", "err1_sq"), ("err2_sq", "err2_sq")):
            assert sinfo[a].tobytes() == info[b].tobytes(), a
        assert set(sinfo["mode"][sinfo["state"] == 0]) <= {0} and (sinfo["mode"][sinfo["state"] == 1] == -1).all()
    if k == 0:  # the short baselines fail the mono form's parallax test: state 1 on both sides
        assert (info["state"] == 0).sum() > 20


def _one(k, i, tp=None, **over):
    """couple i of pair k with some of its numbers replaced -> (reference info, twin info, trace)"""
    c = K.pair_case(k)
    j = int(c["idx"][i])
    v = dict(depth1=c["depth1"][i], right1=c["right1"][i], depth2=c["depth2"][j], right2=c["right2"][j])
    v.update(over)
    tp = K.TP if tp is None else tp
    trace = {}
    q, t = c["q_kp"][i:i + 1], c["t_kp"][j:j + 1]
    want = T.triangulate(E.PairD(K.ref_pair(k)), c["rig"], tp, K.scale(), q["x"][0], q["y"][0], q["octave"][0], v["depth1"], v["right1"], t["x"][0], t["y"][0],
                         t["octave"][0], v["depth2"], v["right2"], trace)
    pts, info = binding.triangulate_stereo_host(K.twin_pair(k), K.twin_rig(c["rig"]), K.twin_params(tp), K.scale(), q, t, *[np.array([v[n]], np.float32)
                                                for n in ("depth1", "right1", "depth2", "right2")])
    same_rows(f"pair {k} row {i} {over}", (info, pts), (np.array([want[0]]), np.array([want[1]])))
    return want[0], trace


def _good_row(k):
    """a matched row of pair k with octaves inside the table, away from the rows the case doctors"""
    c = K.pair_case(k)
    return next(i for i in range(25, K.ROWS) if 0 <= c["idx"][i] < K.ROWS and 0 <= c["t_kp"]["octave"][c["idx"][i]] < 8)


def _depth_at_the_parallax(b, cosr):
    """adjacent float32 depths lo < hi with stereo_cos(lo) <= cosr < stereo_cos(hi): the inequality cos_rays < cs flips between them"""
    lo, hi = f32(1e-3), f32(1e6)
    assert T.stereo_cos(b, lo) <= cosr < T.stereo_cos(b, hi)
    while np.nextafter(lo, f32(np.inf)) < hi:
        mid = f32((float(lo) + float(hi)) / 2)
        mid = mid if lo < mid < hi else np.nextafter(lo, f32(np.inf))
        lo, hi = (mid, hi) if T.stereo_cos(b, mid) <= cosr else (lo, mid)
    return lo, hi


def test_mode_0_against_mode_1_and_mode_2_from_both_sides_of_the_inequality():
    k = 0
    i = _good_row(k)
    _, trace = _one(k, i, right1=-1.0, right2=-1.0)
    cosr = trace["cos_rays"]
    assert 0 < cosr < 1
    lo, hi = _depth_at_the_parallax(K.B, cosr)
    # side 1 stereo: just above the depth the rays win (mode 0), at it the rig's parallax does (mode 1: cs1 < cs2 = cos_rays + 1)
    a, _ = _one(k, i, depth1=hi, right1=10.0, right2=-1.0)
    b, _ = _one(k, i, depth1=lo, right1=10.0, right2=-1.0)
    assert (int(a["mode"]), int(b["mode"])) == (0, 1), (a, b)
    # side 2 alone stereo: the else-if forms cs2, and mode 2 follows
    a, _ = _one(k, i, right1=-1.0, depth2=hi, right2=10.0)
    b, _ = _one(k, i, right1=-1.0, depth2=lo, right2=10.0)
    assert (int(a["mode"]), int(b["mode"])) == (0, 2), (a, b)
    assert b["cs1"] == f32(cosr + 1.0) and b["cs2"] == f32(T.stereo_cos(K.B, lo))


def test_the_else_if_quirk_with_both_sides_stereo():
    """cs2 is never formed when side 1 is stereo: it stays cos_rays + 1, so a far side 2 cannot win"""
    k = 0
    i = _good_row(k)
    _, trace = _one(k, i, right1=-1.0, right2=-1.0)
    lo, hi = _depth_at_the_parallax(K.B, trace["cos_rays"])
    both, _ = _one(k, i, depth1=hi, right1=10.0, depth2=lo, right2=10.0)
    assert both["cs2"] == f32(trace["cos_rays"] + 1.0) and int(both["mode"]) == 0  # side 2 alone at `lo` gave mode 2 above
    both, _ = _one(k, i, depth1=lo, right1=10.0, depth2=hi, right2=10.0)
    assert int(both["mode"]) == 1


def test_the_fall_through_to_state_1_from_both_sides():
    """mono rows: mode 0 iff cos_rays < cos_parallax_max"""
    k = 0
    i = _good_row(k)
    _, trace = _one(k, i, right1=-1.0, right2=-1.0)
    cosr = trace["cos_rays"]
    at, _ = _one(k, i, tp=dict(K.TP, cos_parallax_max=cosr), right1=-1.0, right2=-1.0)
    above, _ = _one(k, i, tp=dict(K.TP, cos_parallax_max=math.nextafter(cosr, 2.0)), right1=-1.0, right2=-1.0)
    assert (int(at["state"]), int(at["mode"])) == (1, -1) and int(above["mode"]) == 0 and int(above["state"]) != 1
    # a NaN right coordinate is mono
    nan, _ = _one(k, i, tp=dict(K.TP, cos_parallax_max=cosr), right1=np.nan, right2=-1.0)
    assert int(nan["state"]) == 1
    # ... and a stereo side takes the row although the parallax test of the mono form fails
    st, _ = _one(k, i, tp=dict(K.TP, cos_parallax_max=cosr), right1=-1.0, depth2=f32(50.0), right2=10.0)
    assert int(st["mode"]) == 0


def test_the_stereo_error_just_inside_and_outside_its_bound():
    k = 0
    c = K.pair_case(k)
    i = next(i for i in range(25, K.ROWS) if c["right1"][i] >= 0 and K.reference_rows(k)[0]["state"][i] == 0 and K.reference_rows(k)[0]["mode"][i] == 0)
    wide = dict(K.TP, chi2_stereo=1e9)
    info, trace = _one(k, i, tp=wide)
    s = float(K.scale()[c["q_kp"]["octave"][i]])
    sigma2, err1 = s * s, trace["err1"]
    cands = sorted({math.nextafter(err1 / sigma2, 0.0), err1 / sigma2, math.nextafter(err1 / sigma2, math.inf), math.nextafter(math.nextafter(err1 / sigma2, math.inf), math.inf)})
    inside = next(v for v in cands if err1 <= v * sigma2)
    outside = math.nextafter(inside, 0.0)
    assert not err1 <= outside * sigma2
    a, _ = _one(k, i, tp=dict(K.TP, chi2_stereo=inside))
    b, _ = _one(k, i, tp=dict(K.TP, chi2_stereo=outside))
    assert int(a["state"]) != 5 and int(b["state"]) == 5
    # the bound of a stereo side is chi2_stereo, not chi2: the mono bound at 0 changes nothing for it
    z, _ = _one(k, i, tp=dict(K.TP, chi2=0.0, chi2_stereo=inside), right2=-1.0)
    assert int(z["state"]) in (0, 6)


def test_the_closed_form_of_the_stereo_parallax_against_libm():
    """2 M (b, depth) pairs, b 0.01 .. 1 m, depth 1e-3 .. 200: (d*d - h*h)/(d*d + h*h) against cos(2 atan2(b/2, d)) in double.
    Recorded maximum: 3.4e-16"""
    rng = np.random.Generator(np.random.PCG64(0xC05))
    b = rng.uniform(0.01, 1.0, 2_000_000)
    d = np.exp(rng.uniform(np.log(1e-3), np.log(200.0), 2_000_000)).astype(np.float32).astype(np.float64)
    h = b / 2.0
    closed = (d * d - h * h) / (d * d + h * h)
    worst = float(np.abs(closed - np.cos(2.0 * np.arctan2(h, d))).max())
    print("largest difference", worst)
    assert worst <= 4 * 2.0 ** -52  # both sides are within a few roundings of the exact value, which lies in [-1, 1]
    for bb, dd in ((0.1, 2.5), (0.5, 0.001), (0.01, 200.0)):
        assert T.stereo_cos(bb, dd) == float(((f32(dd).astype(np.float64)) ** 2 - (bb / 2) ** 2) / ((f32(dd).astype(np.float64)) ** 2 + (bb / 2) ** 2))


def test_refusals():
    c = K.pair_case(0)
    pair, rig, tp, sc = K.twin_pair(0), K.twin_rig(c["rig"]), K.twin_params(), K.scale()
    kp = c["q_kp"][:2]
    one = np.ones(2, np.float32)
    with pytest.raises(binding.OrbError) as e:  # three planes of four
        binding.triangulate_stereo_host(pair, rig, tp, sc, kp, kp, one, one, one, None)
    assert e.value.code == binding.SS_ERR_INVALID_ARG
    with pytest.raises(binding.OrbError):
        binding.triangulate_stereo_host(pair, rig, tp, np.ones(17, np.float32), kp, kp)
    lib = binding.load()
    w = binding._pairs_array(pair)
    pts, info = np.zeros(2, binding.MAP_POINT_DTYPE), np.zeros(2, binding.TRI_STEREO_INFO_DTYPE)
    assert lib.ss_triangulate_stereo_host(w.ctypes.data, None, C.byref(tp), sc.ctypes.data, 8, kp.ctypes.data, kp.ctypes.data, None, None, None, None, 2,
                                          pts.ctypes.data, info.ctypes.data) == binding.SS_ERR_INVALID_ARG
    assert len(binding.triangulate_stereo_host(pair, rig, tp, sc, kp[:0], kp[:0])[0]) == 0
