"""The scenes, crafted tables and cached references the epipolar-search and triangulation tests share (test infrastructure, plain
module).

    scenes()           keyframe 1 = a frame's oracle keypoints back-projected at depths 2 - 8, keyframe 2 = their projection under a
                       second pose (sub-pixel noise, shuffled rows, descriptors with a few bits flipped); nodes from the k10
                       vocabulary; taken rows and node -1 on both sides; planted false couples (off the epipolar line, inside the
                       epipole's disc)
    check_table()      tests 1 - 3 of the search with np.nextafter on both sides of every threshold, den == 0
    tri_table()        steps 1 - 9 of the triangulation: every threshold from both sides (all but d1 > 0 && d2 > 0, which finite input
                       cannot fail), every state 1 .. 10
    count_frames()     counts at 0, 1, 63, 64, 65 and above the rows, negative, live rows behind them
    capacity_pairs()   two pairs of SS_GUIDED_MAX_ROWS rows under a small vocabulary
    compact_case()     matches whose number of state-0 rows is chosen around the compaction's chunk
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import bow_cases as BC
import bow_ref as B
import camera_cases as CC
import epi_ref as E
import guided_cases as G
import proj_cases as PC

f32 = np.float32
CAM = (PC.FX, PC.FY, PC.CX, PC.CY)
VOC, LEVELSUP = "k10", 2
BASELINE = 10.0  # proj_cases.POSES move a few centimetres: times 10, most true couples clear 1.15 degrees of parallax at depths 2 - 8
# (source frame, pose 1, pose 2): the last pair moves forward (FORWARD), its epipole lies inside the image
SCENES = [("synth_t0", 0, 1), ("checker", 1, 2), ("synth_t1", None, "forward")]
COMBOS = [dict(coarse=bool(c), one_to_one=bool(o), orientation=k, taken=bool(t))
          for c, o, k, t in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1))]
TRI = dict(E.UPSTREAM_TRI)


def combo_name(c) -> str:
    return f"coarse{int(c['coarse'])}_u{int(c['one_to_one'])}_o{c['orientation']}_taken{int(c['taken'])}"


def scale():
    return PC.scale()


def pose(k):
    """proj_cases.POSES[k] with its translation scaled; None: the identity; "forward": the rotation of POSES[2], half a metre ahead"""
    if k is None:
        return np.eye(3), (0.0, 0.0, 0.0)
    if k == "forward":
        return PC.POSES[2][0], (0.05, -0.08, 0.5)
    r, t = PC.POSES[k]
    return r, tuple(BASELINE * v for v in t)


def make_pair(p1, p2, cam1=CAM, cam2=CAM):
    return E.pair_init(cam1, p1[0], p1[1], cam2, p2[0], p2[1])


def library_pair(binding, p1, p2, cam1=CAM, cam2=CAM):
    c1 = binding.Camera(fx=cam1[0], fy=cam1[1], cx=cam1[2], cy=cam1[3], width=G.W, height=G.H)
    c2 = binding.Camera(fx=cam2[0], fy=cam2[1], cx=cam2[2], cy=cam2[3], width=G.W, height=G.H)
    return binding.epi_pair(c1, p1[0], p1[1], c2, p2[0], p2[1])


def second_view(rng, kp, p1, p2, noise=0.3, cam1=CAM, cam2=CAM):
    """the keypoints seen from pose 2: back-projected at depths 2 - 8 in camera 1 (cam1), projected by camera 2 (cam2), sub-pixel
    noise; octave and angle kept for most rows"""
    n = len(kp)
    z = 2.0 + 6.0 * rng.random(n)
    xc = np.stack([(kp["x"].astype(np.float64) - cam1[2]) / cam1[0] * z, (kp["y"].astype(np.float64) - cam1[3]) / cam1[1] * z, z], 1)
    xw = (xc - np.asarray(p1[1])) @ np.asarray(p1[0])          # R1^T (xc - t1)
    pc = xw @ np.asarray(p2[0]).T + np.asarray(p2[1])
    k2 = kp.copy()
    k2["x"] = cam2[0] * pc[:, 0] / pc[:, 2] + cam2[2] + rng.normal(0, noise, n)
    k2["y"] = cam2[1] * pc[:, 1] / pc[:, 2] + cam2[3] + rng.normal(0, noise, n)
    what = rng.random(n)
    k2["octave"] = np.clip(kp["octave"] + np.where(what < 0.1, 1, np.where(what < 0.2, -1, 0)), 0, 7)
    k2["angle"] = np.where(rng.random(n) < 0.15, rng.integers(0, 360, n), np.mod(kp["angle"] + rng.normal(0, 2.0, n) + 360.0, 360.0)).astype(np.float32)
    return k2, xw


@functools.lru_cache(maxsize=None)
def scenes(cams=None):
    """-> list of dicts pair poses cams q_kp q_desc q_node q_taken t_kp t_desc t_node t_taken truth (the train row of query row i).
    cams: the (camera 1, camera 2) of every scene, each (fx, fy, cx, cy) (a tuple of tuples; None: CAM on both sides of all)"""
    out = []
    voc = BC.vocab(VOC)
    for k, (src, a, b) in enumerate(SCENES):
        rng = np.random.Generator(np.random.PCG64(0xE91 + k))
        qk, qd = G.features(src)
        qn = np.array(BC.frame_transform(VOC, src, LEVELSUP)[1], np.int32)
        p1, p2 = pose(a), pose(b)
        c1, c2 = (CAM, CAM) if cams is None else cams[k]
        pair = make_pair(p1, p2, c1, c2)
        k2, _ = second_view(rng, qk, p1, p2, cam1=c1, cam2=c2)
        d2 = PC.desc_near(rng, qd)
        n = len(qk)
        perm = rng.permutation(n)             # train row j holds query row perm[j]
        truth = np.argsort(perm).astype(np.int32)
        tk, td = k2[perm].copy(), d2[perm].copy()
        tn = np.array(B.transform(voc, td, LEVELSUP)[1], np.int32)
        # planted false couples: a train row that copies the descriptor (and node) of a query row it does not belong to, where it
        # is (off that row's epipolar line); the true partner keeps at least two flipped bits, so the false one wins without geometry
        live = np.flatnonzero(qn >= 0)
        for i in live[rng.choice(len(live), 12, replace=False)]:
            j = int(rng.integers(0, n))
            if j == truth[i]:
                continue
            td[j], tn[j] = qd[i], qn[i]
            td[truth[i]] = qd[i]
            td[truth[i], 0] ^= 3
            tn[truth[i]] = qn[i]
        # ... and rows inside the epipole's disc: on every epipolar line, but no candidate
        if int(pair["epipole_test"]):
            for m, i in enumerate(live[rng.choice(len(live), 6, replace=False)]):
                j = int(rng.integers(0, n))
                if j == truth[i]:
                    continue
                tk["x"][j], tk["y"][j] = float(pair["ex"]) + 1.5 * m - 3.0, float(pair["ey"]) + 2.0 - m
                tk["octave"][j] = m % 3
                td[j], tn[j] = qd[i], qn[i]
                td[j, 1] ^= 1
        qn, tn = qn.copy(), tn.copy()
        qn[rng.random(n) < 0.05] = -1
        tn[rng.random(n) < 0.05] = -1
        out.append({"pair": pair, "poses": (p1, p2), "cams": (c1, c2), "q_kp": qk, "q_desc": qd, "q_node": qn, "q_taken": (rng.random(n) < 0.1).astype(np.uint8),
                    "t_kp": tk, "t_desc": td, "t_node": tn, "t_taken": (rng.random(n) < 0.1).astype(np.uint8), "truth": truth})
    return out


@functools.lru_cache(maxsize=None)
def scene_found(k: int, coarse: bool, taken: bool, th: int = 50):
    s = scenes()[k]
    return E.search(s["pair"], s["q_kp"], s["q_desc"], s["q_node"], s["t_kp"], s["t_desc"], s["t_node"], scale(), th, coarse,
                    s["q_taken"] if taken else None, s["t_taken"] if taken else None)


def scene_reference(k: int, combo, th: int = 50):
    """-> (idx, d1, summary) of scene k under a COMBOS entry; the search is computed once per (coarse, taken)"""
    s = scenes()[k]
    return E.finish(scene_found(k, combo["coarse"], combo["taken"], th), s["q_kp"], s["t_kp"], th, combo["one_to_one"], combo["orientation"])


def combo_params(binding, combo, th: int = 50):
    return binding.epi_params(th=th, coarse=combo["coarse"], one_to_one=combo["one_to_one"], orientation=combo["orientation"])


@functools.lru_cache(maxsize=None)
def scene_matches(k: int) -> np.ndarray:
    """the matches the triangulation tests run on: the coarse search (false couples included), every 7th unmatched row given a
    random train row, two entries outside the train rows"""
    s = scenes()[k]
    idx = scene_reference(k, dict(coarse=True, one_to_one=False, orientation=0, taken=True))[0].copy()
    rng = np.random.Generator(np.random.PCG64(0x7A1 + k))
    free = np.flatnonzero(idx < 0)
    idx[free[::7]] = rng.integers(0, len(s["t_kp"]), len(free[::7]))
    idx[free[1]], idx[free[2]] = -7, len(s["t_kp"])
    return idx


@functools.lru_cache(maxsize=None)
def scene_triangulation(k: int):
    """-> (info, points, point_desc, point_rows, summary) of scene k's matches"""
    s = scenes()[k]
    return E.triangulate_rows(s["pair"], TRI, scale(), s["q_kp"], s["q_desc"], s["t_kp"], scene_matches(k))


# ---- odd cameras: the three scenes, one pair of cameras each (CC.PAIR_CAMERAS) -----------------------------------------------------------
CAMERA_COMBO = dict(coarse=False, one_to_one=True, orientation=1, taken=True)


def camera_scenes():
    return scenes(tuple((CC.intrinsics(a), CC.intrinsics(b)) for a, b in CC.PAIR_CAMERAS))


@functools.lru_cache(maxsize=None)
def camera_reference(k: int, cams=None):
    """scene k of the camera scenes: the search, then the triangulation of its matches -> ((idx, d1, summary), (info, points,
    point_desc, point_rows, summary)); cams: the (camera 1, camera 2) a confused pair record would hold (None: the scene's own)"""
    s = camera_scenes()[k]
    pair = s["pair"] if cams is None else make_pair(*s["poses"], CC.intrinsics(cams[0]), CC.intrinsics(cams[1]))
    found = reference(dict(s, pair=pair), CAMERA_COMBO)
    return found, E.triangulate_rows(pair, TRI, scale(), s["q_kp"], s["q_desc"], s["t_kp"], found[0])


@functools.lru_cache(maxsize=None)
def camera_matches(k: int) -> np.ndarray:
    """matches for the triangulation alone, as scene_matches() makes them: the coarse search (false couples included) and every 7th
    unmatched row given a random train row"""
    s = camera_scenes()[k]
    idx = reference(s, dict(coarse=True, one_to_one=False, orientation=0, taken=True))[0].copy()
    rng = np.random.Generator(np.random.PCG64(0x7A1C + k))
    free = np.flatnonzero(idx < 0)
    idx[free[::7]] = rng.integers(0, len(s["t_kp"]), len(free[::7]))
    return idx


@functools.lru_cache(maxsize=None)
def camera_triangulation(k: int, cams=None):
    """-> (info, points, point_desc, point_rows, summary) of camera_matches(k), under the scene's pair or a confused one"""
    s = camera_scenes()[k]
    pair = s["pair"] if cams is None else make_pair(*s["poses"], CC.intrinsics(cams[0]), CC.intrinsics(cams[1]))
    return E.triangulate_rows(pair, TRI, scale(), s["q_kp"], s["q_desc"], s["t_kp"], camera_matches(k))


# ---- bisection on float32 / float64 bit patterns --------------------------------------------------------------------------------------
def _steps(dtype):
    return (np.float32, np.int32) if dtype == np.float32 else (np.float64, np.int64)


def flip_point(pred, good, bad, dtype=np.float32):
    """two adjacent floats (a, b) between `good` (pred true) and `bad` (pred false), both finite and of one sign, with pred(a) true
    and pred(b) false: the threshold from both sides"""
    ft, it = _steps(dtype)
    a, b = int(np.array(good, ft).view(it)), int(np.array(bad, ft).view(it))
    assert pred(ft(good)) and not pred(ft(bad))
    while abs(a - b) > 1:
        m = (a + b) // 2
        if pred(np.array(m, it).view(ft)[()]):
            a = m
        else:
            b = m
    return np.array(a, it).view(ft)[()], np.array(b, it).view(ft)[()]


# ---- tests 1 - 3 of the search -------------------------------------------------------------------------------------------------------
def crafted_pair(f12, ex=0.0, ey=0.0, epipole_test=0):
    w = make_pair(pose(0), pose(1))
    w["f12"], w["ex"], w["ey"], w["epipole_test"] = f12, ex, ey, epipole_test
    return w


@functools.lru_cache(maxsize=None)
def check_table(sc=None):
    """-> list of (name, pair, coarse, kp1, kp2, expected codes or None).  The crafted pair has a = 0, b = 1, c = -y_i: the distance
    to the line is y_j - y_i exactly."""
    sc = scale() if sc is None else sc
    n = len(sc)
    line = crafted_pair([0, 0, 0, 0, 0, -1, 0, 1, 0], 100.0, 50.0, 1)
    rows = []

    def add(name, pair, coarse, q, t, expect=None):
        qk = G.kp_rows([v[0] for v in q], [v[1] for v in q])
        tk = G.kp_rows([v[0] for v in t], [v[1] for v in t], octave=[v[2] for v in t])
        rows.append((name, pair, coarse, qk, tk, expect))

    octs = [-5, -1, 0, n - 1, n, 1000]
    add("octave", line, False, [(0, 0)] * len(octs), [(0, 0, o) for o in octs], [1, 1, 0, 0, 1, 1])
    for o in range(n):
        s = f32(sc[o])
        # the epipole's disc: dx * dx >= 100 * s with dy = 0
        ok = lambda d: E.check(line, True, sc, None, f32(100.0) - f32(d), 50.0, o) == 0
        a, b = flip_point(ok, 40.0, 1.0)
        add(f"epipole disc, octave {o}", line, True, [(0, 0)] * 3, [(f32(100.0) - v, 50.0, o) for v in (a, b, np.nextafter(b, f32(0)))], [0, 2, 2])
        # the line: (y_j - 0)^2 < 3.84f * s * s, far from the epipole
        ok = lambda y: E.check(line, False, sc, E.line_of(line, 0, 0), 300.0, f32(y), o) == 0
        a, b = flip_point(ok, 0.5, 40.0)
        add(f"line, octave {o}", line, False, [(0, 0)] * 3, [(300.0, v, o) for v in (np.nextafter(a, f32(0)), a, b)], [0, 0, 3])
    add("exact disc", line, True, [(0, 0)] * 2, [(90.0, 50.0, 0), (np.nextafter(f32(90.0), f32(100)), 50.0, 0)], [0, 2])
    add("den == 0, zero F", crafted_pair([0] * 9), False, [(3, 4)] * 2, [(3, 4, 0), (50, 60, n - 1)], [3, 3])
    add("den == 0, c alone", crafted_pair([0, 0, 0, 0, 0, 0, 0, 0, 1]), False, [(3, 4)], [(3, 4, 0)], [3])
    add("den == 0, coarse", crafted_pair([0] * 9), True, [(3, 4)], [(3, 4, 0)], [0])
    odd = [np.nan, np.inf, -np.inf, 3e38, 1e-45]
    add("odd coordinates", line, False, [(v, 0) for v in odd] + [(0, v) for v in odd] + [(0, 0)] * 10,
        [(0, 0, 0)] * 10 + [(v, 0, 1) for v in odd] + [(300, v, 1) for v in odd])
    add("odd pair", crafted_pair([np.nan, 1, 0, np.inf, 0, 0, 1, 1, 1], np.nan, 5.0, 1), False, [(1, 2)] * 2, [(3, 4, 0), (0, 0, 0)])
    return rows


# ---- steps 1 - 9 of the triangulation ---------------------------------------------------------------------------------------------------
def _one(kp):
    return kp[0:1]


@functools.lru_cache(maxsize=None)
def tri_table(sc=None):
    """-> list of (name, pair, tp, kp1, kp2, expected states or None).  Built on one true couple of scene 0 (state 0 under the
    upstream parameters): every parameter threshold is the computed quantity itself, taken with np.nextafter on both sides; the tests
    on computed depths are bisected on a keypoint coordinate."""
    sc = scale() if sc is None else sc
    n = len(sc)
    s = scenes()[0]
    pair = s["pair"]
    w = E.PairD(pair)
    rows = []
    tri = lambda tp, k1, k2, pr=w: E.triangulate(pr, tp, sc, k1["x"][0], k1["y"][0], k1["octave"][0], k2["x"][0], k2["y"][0], k2["octave"][0])
    # a clean couple: a true match that the upstream parameters accept
    for i in range(len(s["q_kp"])):
        k1, k2 = s["q_kp"][i:i + 1].copy(), s["t_kp"][s["truth"][i]:s["truth"][i] + 1].copy()
        k1["octave"], k2["octave"] = min(int(k1["octave"][0]), n - 1), min(int(k2["octave"][0]), n - 1)
        info, p, X = tri(TRI, k1, k2)
        if info["state"] == 0 and info["err1_sq"] > 0 and info["err2_sq"] > 0:
            break
    up, dn = lambda v: float(np.nextafter(v, np.inf)), lambda v: float(np.nextafter(v, -np.inf))

    def add(name, tp, a, b, expect=None, pr=pair):
        rows.append((name, pr, dict(tp), a.copy(), b.copy(), expect))

    # the exact double quantities of the clean couple, recomputed as the rule states them
    a1, b1 = (float(k1["x"][0]) - w.cx1) * w.invfx1, (float(k1["y"][0]) - w.cy1) * w.invfy1
    a2, b2 = (float(k2["x"][0]) - w.cx2) * w.invfx2, (float(k2["y"][0]) - w.cy2) * w.invfy2
    r1 = [(w.rcw1[k] * a1 + w.rcw1[3 + k] * b1) + w.rcw1[6 + k] for k in range(3)]
    r2 = [(w.rcw2[k] * a2 + w.rcw2[3 + k] * b2) + w.rcw2[6 + k] for k in range(3)]
    import math
    cosp = ((r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2]) / (math.sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]) *
                                                                math.sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]))
    for v, st in ((dn(cosp), 1), (cosp, 1), (up(cosp), 0)):
        add("cos on cos_parallax_max", dict(TRI, cos_parallax_max=v), k1, k2, [st])
    # chi2 * sigma2 against the errors: bisected on chi2 (a double).  The second error is the larger one on these couples, so side 1
    # is taken on the pair with its sides swapped
    swapped = make_pair(s["poses"][1], s["poses"][0])
    for side, st, pr in (("err1_sq", 5, swapped), ("err2_sq", 6, pair)):
        big, small = ("err1_sq", "err2_sq") if st == 5 else ("err2_sq", "err1_sq")
        for i in range(len(s["q_kp"])):
            c1, c2 = s["q_kp"][i:i + 1].copy(), s["t_kp"][s["truth"][i]:s["truth"][i] + 1].copy()
            c1["octave"] = c2["octave"] = 0
            if st == 5:
                c1, c2 = c2, c1
            got = tri(TRI, c1, c2, E.PairD(pr))[0]
            if got["state"] == 0 and got[small] > 0 and got[big] > got[small]:
                break
        ok = lambda c: tri(dict(TRI, chi2=float(c)), c1, c2, E.PairD(pr))[0]["state"] != st
        # octave 0: sigma2 is 1, so chi2 is compared with the errors themselves
        good, bad = flip_point(ok, 1e3, (float(got[big]) + float(got[small])) / 2.0, np.float64)
        for v, e in ((up(float(good)), 0), (float(good), 0), (float(bad), st), (dn(float(bad)), st)):
            add(f"{side} on chi2 * sigma2", dict(TRI, chi2=v), c1, c2, [e], pr)
    # the far limit and the scale ratio, on both distances
    n1 = [X[k] - w.ow1[k] for k in range(3)]
    n2 = [X[k] - w.ow2[k] for k in range(3)]
    d1, d2 = math.sqrt((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2]), math.sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2])
    big = max(d1, d2)
    for v, st in ((dn(big), 8), (big, 8), (up(big), 0), (0.0, 0), (-1.0, 0), (float("nan"), 0)):
        add("distance on far_limit", dict(TRI, far_limit=v), k1, k2, [st])
    for o1, o2 in ((0, 0), (0, n - 1), (n - 1, 0)):
        q1, q2 = k1.copy(), k2.copy()
        q1["octave"], q2["octave"] = o1, o2
        loose = dict(TRI, chi2=1e9)
        ok = lambda r: tri(dict(loose, ratio_factor=float(r)), q1, q2)[0]["state"] == 0
        good, bad = flip_point(ok, 1e6, 1e-6, np.float64)
        for v, st in ((up(float(good)), 0), (float(good), 0), (float(bad), 9), (dn(float(bad)), 9)):
            add(f"ratio_factor, octaves {o1} / {o2}", dict(loose, ratio_factor=v), q1, q2, [st])
    # the tests on a computed sign (cos > 0, z1 > 0, z2 > 0): bisected on one keypoint coordinate between a row the test fails and
    # a row it passes, so the two middle rows are adjacent float32 values on either side of the threshold.  Camera 2 stands one unit
    # ahead of camera 1 (identity rotations), so each epipole is the principal point:
    # - a train keypoint through the epipole of image 2 is a ray through camera 1's centre: z1 goes through 0 there;
    # - a query keypoint through the epipole of image 1 is a ray through camera 2's centre: z2 goes through 0 there
    #   (elsewhere a depth changes sign through infinity, with v[3], which is no boundary of these tests);
    # - camera 2 turned by 90 degrees about y: the rays are orthogonal where the train keypoint's a2 equals the query's a1.
    loose = dict(TRI, cos_parallax_max=2.0, chi2=1e300, ratio_factor=1e300)
    ahead = E.pair_init(CAM, np.eye(3), (0.0, 0.0, 0.0), CAM, np.eye(3), (0.0, 0.0, -1.0))
    turned = E.pair_init(CAM, np.eye(3), (0.0, 0.0, 0.0), CAM, PC.rot(0.0, np.pi / 2), (1.0, 0.0, 0.0))
    off = G.kp_rows([CAM[2] + 30.0], [CAM[3]])

    def two_sided(name, pr, st, side, lo, hi, depth=None, at=CAM[2]):
        wd = E.PairD(pr)

        def couple(x):
            q = G.kp_rows([x], [CAM[3]])
            return (q, off) if side == 1 else (off, q)

        def state(x):
            return tri(loose, *couple(x), wd)
        ok = lambda x: state(x)[0]["state"] != st
        good, bad = (lo, hi) if ok(f32(lo)) else (hi, lo)
        ga, gb = flip_point(ok, good, bad)
        out, inn = (f32(-np.inf), f32(np.inf)) if ga < gb else (f32(np.inf), f32(-np.inf))
        for v, fails in ((np.nextafter(ga, out), False), (ga, False), (gb, True), (np.nextafter(gb, inn), True)):
            got = state(v)
            assert (got[0]["state"] == st) == fails, (name, v, got[0])
            add(name, loose, *couple(v), [int(got[0]["state"])], pr)
        assert abs(float(ga) - at) < 1e-3, (name, ga)  # the threshold is where the geometry puts it
        if depth is not None:  # ... and the depth is next to 0 on its passing side, not beyond infinity
            q1, q2 = couple(ga)
            v, _ = E.dlt(E.dlt_rows(wd, (float(q1["x"][0]) - wd.cx1) * wd.invfx1, (float(q1["y"][0]) - wd.cy1) * wd.invfy1,
                                    (float(q2["x"][0]) - wd.cx2) * wd.invfx2, (float(q2["y"][0]) - wd.cy2) * wd.invfy2))
            X = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
            z = ((wd.rcw1[6] * X[0] + wd.rcw1[7] * X[1]) + wd.rcw1[8] * X[2]) + wd.tcw1[2] if depth == 1 else \
                ((wd.rcw2[6] * X[0] + wd.rcw2[7] * X[1]) + wd.rcw2[8] * X[2]) + wd.tcw2[2]
            assert 0.0 < z < 1e-3, (name, z)

    two_sided("depth 1 at 0", ahead, 3, 2, CAM[2] - 10.0, CAM[2] + 10.0, depth=1)
    two_sided("depth 2 at 0", ahead, 4, 1, CAM[2] - 10.0, CAM[2] + 10.0, depth=2)
    two_sided("cos at 0", turned, 1, 2, CAM[2] - 100.0, CAM[2] + 100.0, at=CAM[2] + 30.0)  # r1 = (0.1, 0, 1) meets r2 = (1, 0, -a2) at a right angle
    # a point behind camera 1 alone (camera 2 stands behind it), and one between the cameras (camera 2 stands ahead)
    for tz, st in ((1.0, 3), (-1.0, 4)):
        fwd = E.pair_init(CAM, np.eye(3), (0.0, 0.0, 0.0), CAM, np.eye(3), (0.0, 0.0, tz))
        zz = -0.5 if st == 3 else 0.5
        add(f"depth {st - 2} negative", TRI, G.kp_rows([CAM[0] * 0.1 / zz + CAM[2]], [CAM[1] * 0.05 / zz + CAM[3]]),
            G.kp_rows([CAM[0] * 0.1 / (zz + tz) + CAM[2]], [CAM[1] * 0.05 / (zz + tz) + CAM[3]]), [st], fwd)
    # octaves
    for o1, o2, st in ((-5, 0, 10), (-1, 0, 10), (0, -1, 10), (n, 0, 10), (0, n, 10), (1000, 1000, 10), (n - 1, n - 1, None), (0, 0, None)):
        q1, q2 = k1.copy(), k2.copy()
        q1["octave"], q2["octave"] = o1, o2
        add("octave", TRI, q1, q2, None if st is None else [st])
    # state 2: parallel rays under identity rotations, admitted by cos_parallax_max = 2: M has an exactly zero row, v = (0, 0, 1, 0)
    par = E.pair_init((256.0, 256.0, 0.0, 0.0), np.eye(3), (0.0, 0.0, 0.0), (256.0, 256.0, 0.0, 0.0), np.eye(3), (1.0, 0.0, 0.0))
    z = G.kp_rows([0.0], [0.0])
    add("point at infinity", dict(TRI, cos_parallax_max=2.0), z, z, [2], par)
    add("parallel rays", TRI, z, z, [1], par)
    # cos <= 0: the second camera looks backwards
    back = E.pair_init(CAM, np.eye(3), (0.0, 0.0, 0.0), CAM, PC.rot(0.0, 2.5), (0.3, 0.0, 0.0))
    add("cos below 0", TRI, k1, k2, [1], back)
    # state 7: a pair whose camera centre is not a number (the caller's own pair)
    odd = pair.copy()
    odd["ow1"] = [np.nan, 0, 0]
    add("ow1 is NaN", dict(TRI, far_limit=100.0), k1, k2, [7], odd)
    # non-finite everything
    for name in ("rcw1", "tcw2", "invfx1", "cx2"):
        bad = pair.copy()
        if bad[name].shape:
            bad[name][0] = np.nan
        else:
            bad[name] = np.inf
        add(f"{name} is not finite", TRI, k1, k2, None, bad)
    for v in (np.nan, np.inf, -np.inf, 3e38):
        q2 = k2.copy()
        q2["y"] = v
        add("odd keypoint", TRI, k1, q2)
        add("odd keypoint, loose", dict(TRI, cos_parallax_max=2.0, chi2=float("inf")), q2, k1)
    return rows


# ---- counts ---------------------------------------------------------------------------------------------------------------------------
COUNT_ROWS = 65
COUNTS = [(0, 65), (1, 65), (63, 65), (64, 65), (65, 65), (65, 0), (65, 1), (65, 63), (65, 64), (0, 0), (1, 1), (70, 65), (65, 1000), (-3, 65), (65, -1),
          (1 << 30, 1 << 30)]
COUNT_COMBO = dict(coarse=False, one_to_one=True, orientation=1, taken=True)


@functools.lru_cache(maxsize=None)
def count_frame():
    """scene 0 cut to COUNT_ROWS rows on both sides, the train rows being the partners of the query rows: every row of the call is
    live, whatever its counts say"""
    s = scenes()[0]
    n = COUNT_ROWS
    j = s["truth"][:n]
    return {"pair": s["pair"], "q_kp": s["q_kp"][:n], "q_desc": s["q_desc"][:n], "q_node": s["q_node"][:n], "q_taken": s["q_taken"][:n],
            "t_kp": s["t_kp"][j], "t_desc": s["t_desc"][j], "t_node": s["t_node"][j], "t_taken": s["t_taken"][j]}


def cut(f, nq: int, nt: int):
    """the first rows of a frame dict on both sides"""
    out = dict(f)
    for k in ("q_kp", "q_desc", "q_node", "q_taken"):
        out[k] = f[k][:nq]
    for k in ("t_kp", "t_desc", "t_node", "t_taken"):
        out[k] = f[k][:nt]
    return out


def reference(f, combo, th: int = 50):
    """E.match of a frame dict under a COMBOS-style entry"""
    return E.match(f["pair"], f["q_kp"], f["q_desc"], f["q_node"], f["t_kp"], f["t_desc"], f["t_node"], scale(), th, combo["coarse"],
                   combo["one_to_one"], combo["orientation"], f["q_taken"] if combo["taken"] else None, f["t_taken"] if combo["taken"] else None)


@functools.lru_cache(maxsize=None)
def count_reference(nq: int, nt: int):
    k, m = min(max(nq, 0), COUNT_ROWS), min(max(nt, 0), COUNT_ROWS)
    f = cut(count_frame(), k, m)
    idx, d1, summ = reference(f, COUNT_COMBO)
    tri = E.triangulate_rows(f["pair"], TRI, scale(), f["q_kp"], f["q_desc"], f["t_kp"], idx)
    return idx, d1, summ, tri


# ---- full capacity --------------------------------------------------------------------------------------------------------------------
CAP_ROWS = 16384
CAP_NODES = 1500
CAP_COMBO = dict(coarse=True, one_to_one=True, orientation=2, taken=True)


@functools.lru_cache(maxsize=None)
def capacity_pairs():
    """Two pairs of CAP_ROWS rows on both sides.  Every query row is the partner of a train row drawn WITH replacement (pair 1: from
    the upper half only), seen from pose 1, its descriptor that row's with a few bits flipped and its node that row's: many train rows
    are wanted by several queries, on both sides of row 8192."""
    out = []
    for b in range(2):
        rng = np.random.Generator(np.random.PCG64(0xCA9E + b))
        proto = rng.integers(0, 256, size=(48, 32), dtype=np.uint8)
        tk = G.kp_rows(rng.integers(0, PC.CAP_W * 4, CAP_ROWS).astype(np.float32) / f32(4), rng.integers(0, PC.CAP_H * 4, CAP_ROWS).astype(np.float32) / f32(4),
                       octave=rng.integers(0, 8, CAP_ROWS), angle=rng.integers(0, 1440, CAP_ROWS).astype(np.float32) / f32(4))
        td = G.near(rng, proto, CAP_ROWS)
        tn = rng.integers(0, CAP_NODES, CAP_ROWS).astype(np.int32)
        tn[rng.random(CAP_ROWS) < 0.03] = -1
        want = rng.integers(8192 if b else 0, CAP_ROWS, CAP_ROWS)
        cam = (PC.CAP_F, PC.CAP_F, PC.CAP_CX, PC.CAP_CY)
        p1, p2 = pose(b), pose(b + 1)
        pair = make_pair(p2, p1, cam, cam)  # the train rows are the given view: the queries are their second view
        z = 2.0 + 6.0 * rng.random(CAP_ROWS)
        t = tk[want]
        xc = np.stack([(t["x"].astype(np.float64) - cam[2]) / cam[0] * z, (t["y"].astype(np.float64) - cam[3]) / cam[1] * z, z], 1)
        xw = (xc - np.asarray(p1[1])) @ np.asarray(p1[0])
        pc = xw @ np.asarray(p2[0]).T + np.asarray(p2[1])
        qk = t.copy()
        qk["x"] = cam[0] * pc[:, 0] / pc[:, 2] + cam[2] + rng.normal(0, 0.3, CAP_ROWS)
        qk["y"] = cam[1] * pc[:, 1] / pc[:, 2] + cam[3] + rng.normal(0, 0.3, CAP_ROWS)
        out.append({"pair": pair, "q_kp": qk, "q_desc": PC.desc_near(rng, td[want], 3), "q_node": tn[want].copy(),
                    "q_taken": (rng.random(CAP_ROWS) < 0.05).astype(np.uint8), "t_kp": tk, "t_desc": td, "t_node": tn,
                    "t_taken": (rng.random(CAP_ROWS) < 0.05).astype(np.uint8)})
    return out


@functools.lru_cache(maxsize=None)
def capacity_found(b: int, coarse: bool):
    f = capacity_pairs()[b]
    return E.search(f["pair"], f["q_kp"], f["q_desc"], f["q_node"], f["t_kp"], f["t_desc"], f["t_node"], scale(), 50, coarse, f["q_taken"], f["t_taken"])


def capacity_reference(b: int, coarse: bool = False, one_to_one: bool = True, orientation: int = 2):
    f = capacity_pairs()[b]
    return E.finish(capacity_found(b, coarse), f["q_kp"], f["t_kp"], 50, one_to_one, orientation)


# ---- the compaction -------------------------------------------------------------------------------------------------------------------
CHUNK = 1024  # SSK_TRI_CHUNK: the rows one pass of k_tri_compact places
COMPACT_ROWS = 2200
COMPACT_COUNTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1)


@functools.lru_cache(maxsize=None)
def compact_base():
    """COMPACT_ROWS couples (query row i with train row i) and their per-row triangulation, computed once: clean second views of
    random keypoints under scene 0's pair, so nearly every couple is a point"""
    s = scenes()[0]
    rng = np.random.Generator(np.random.PCG64(0xC0A7))
    n = COMPACT_ROWS
    qk = G.kp_rows(rng.uniform(20, 300, n), rng.uniform(20, 220, n), octave=rng.integers(0, 8, n), angle=rng.uniform(0, 360, n))
    tk, _ = second_view(rng, qk, *s["poses"], noise=0.1)
    tk["y"][::40] += f32(25)  # ... but these
    qd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    info, pts, _ = E.triangulate_couples(s["pair"], TRI, scale(), qk, tk)
    return {"pair": s["pair"], "q_kp": qk, "q_desc": qd, "t_kp": tk, "info": info, "pts": pts}


def compact_case(count: int, layout: str):
    """-> (idx, info, points, point_desc, point_rows, summary): `count` of the state-0 couples keep their match, the others get -1.
    layout "head": the first ones (one chunk where they fit); "spread": every second one (they span two chunks and more)"""
    b = compact_base()
    good = np.flatnonzero(b["info"]["state"] == 0)
    keep = good[:count] if layout == "head" else good[::2][:count]
    assert len(keep) == count
    n = COMPACT_ROWS
    idx = np.full(n, -1, np.int32)
    idx[keep] = keep
    bad = np.flatnonzero(b["info"]["state"] != 0)
    idx[bad] = bad  # the couples that are no point stay matched: they count in their states
    info, pts = E.none_info(n), np.zeros(n, E.MAP_POINT_DTYPE)
    on = idx >= 0
    info[on], pts[on] = b["info"][on], b["pts"][on]
    return (idx, info) + E.compact(info, pts, idx, b["q_desc"], n)
