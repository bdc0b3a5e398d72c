"""numpy restatement of map-point fusion (test infrastructure, plain module): the NORMATIVE statement of the rule in
include/sendslam_orb.h ("map-point fusion"): ORBmatcher::Fuse, its Sim3 form and the Sim3
SearchByProjection, as this library restates them.  Parity with the real binary is not pinned.

Written from the rule, not from the kernel: one map point and one couple at a time, float32 at every step (every operation
rounded once, left to right as written), every test in its accepting form so that a NaN fails it.  The device code and the host
twins ss_fuse_points_host / ss_fuse_check_host must reproduce every number bit for bit.

    view_sim3    ss_fuse_view_sim3: Scw = [s.R | t] decomposed in double, then proj_ref.view_init
    eval_point   step 1: the state, the predicted level, the window
    check        step 2 of one couple: 0, or the number 1 .. 4 of the first failing test
    search       steps 2 and 3 of every point: the candidates, the best key
    finish       step 4: one action per point, the summary
    match        one frame
"""
from __future__ import annotations

import math

import numpy as np

import guided_ref as R
import proj_ref as P

f32 = np.float32
NONE = R.NONE
ACT_NONE, ACT_ADD, ACT_REPLACE, ACT_DUPLICATE = 0, 1, 2, 3

POINT_DTYPE = np.dtype([(n, "<f4") for n in ("u", "v", "u_right", "dot", "dist", "radius")] + [("level", "<i4"), ("state", "<i4")])
ACTION_DTYPE = np.dtype([("action", "<i4"), ("other", "<i4")])
SUMMARY_FIELDS = ("status", "n_points", "n_train", "n_in_view", "n_candidates", "n_add", "n_replace", "n_duplicate")
# upstream's calls: Fuse in LocalMapping::SearchInNeighbors; Fuse(pKF, Scw) in SearchAndFuse; the Sim3 SearchByProjection
LOCAL_MAPPING = dict(view_cos_limit=0.5, th=3.0, chi2_mono=5.99, chi2_stereo=7.8, th_low=50, check_right=False)
SEARCH_AND_FUSE = dict(view_cos_limit=0.5, th=4.0, chi2_mono=0.0, chi2_stereo=0.0, th_low=50, check_right=False)
CANDIDATE_CHECK = dict(view_cos_limit=0.5, th=8.0, chi2_mono=0.0, chi2_stereo=0.0, th_low=50, check_right=False)


def view_sim3(fx, fy, cx, cy, width, height, srcw, t, bf):
    """-> one proj_ref.VIEW_DTYPE record, or None where the call is refused (the scale is not finite or not > 0)"""
    m = [float(v) for v in np.asarray(srcw, np.float64).reshape(9)]
    tt = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        s = float(np.sqrt(np.float64((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])))
    if not (s > 0 and math.isfinite(s)):
        return None
    with np.errstate(all="ignore"):
        r = [float(np.float64(v) / np.float64(s)) for v in m]
        tc = [float(np.float64(v) / np.float64(s)) for v in tt]
        return P.view_init(fx, fy, cx, cy, width, height, r, tc, bf)


def _rejected(state: int) -> np.ndarray:
    o = np.zeros((), POINT_DTYPE)
    o["level"], o["state"] = -1, state
    return o


def eval_point(view, p, skip, view_cos_limit, th, scale) -> np.ndarray:
    """step 1 of one map point -> one POINT_DTYPE record; skip: the point's flag (0 / None: none)"""
    if skip is not None and int(skip) != 0:
        return _rejected(1)
    w = view
    r, t, ow = [f32(v) for v in w["rcw"]], [f32(v) for v in w["tcw"]], [f32(v) for v in w["ow"]]
    x, y, z = f32(p["x"]), f32(p["y"]), f32(p["z"])
    with np.errstate(all="ignore"):
        pc = [f32(f32(f32(f32(r[3 * k] * x) + f32(r[3 * k + 1] * y)) + f32(r[3 * k + 2] * z)) + t[k]) for k in range(3)]
        if not pc[2] > 0:
            return _rejected(2)
        invz = f32(f32(1.0) / pc[2])
        u = f32(f32(f32(f32(w["fx"]) * pc[0]) * invz) + f32(w["cx"]))
        v = f32(f32(f32(f32(w["fy"]) * pc[1]) * invz) + f32(w["cy"]))
        if not (u >= f32(w["min_x"]) and u < f32(w["max_x"]) and v >= f32(w["min_y"]) and v < f32(w["max_y"])):
            return _rejected(3)
        po = [f32(x - ow[0]), f32(y - ow[1]), f32(z - ow[2])]
        dist = f32(np.sqrt(f32(f32(f32(po[0] * po[0]) + f32(po[1] * po[1])) + f32(po[2] * po[2]))))
        if not (dist >= f32(f32(0.8) * f32(p["min_dist"])) and dist <= f32(f32(1.2) * f32(p["max_dist"]))):
            return _rejected(4)
        dot = f32(f32(f32(po[0] * f32(p["nx"])) + f32(po[1] * f32(p["ny"]))) + f32(po[2] * f32(p["nz"])))
        if not dot >= f32(f32(view_cos_limit) * dist):
            return _rejected(5)
        ratio = f32(f32(p["max_dist"]) / dist)
        level = P.level_table(ratio, scale)
        o = np.zeros((), POINT_DTYPE)
        o["u"], o["v"], o["u_right"] = u, v, f32(u - f32(f32(w["bf"]) * invz))
        o["dot"], o["dist"], o["radius"] = dot, dist, f32(f32(th) * f32(scale[level]))
        o["level"], o["state"] = level, 0
    return o


def eval_points(view, points, skip, view_cos_limit, th, scale) -> np.ndarray:
    out = np.zeros(len(points), POINT_DTYPE)
    for i in range(len(points)):
        out[i] = eval_point(view, points[i], None if skip is None else skip[i], view_cos_limit, th, scale)
    return out


def check(o, x, y, octave, right, taken, scale, chi2_mono, chi2_stereo, check_right) -> int:
    """step 2 of the couple (point o, a train row at (x, y) on `octave` with right coordinate `right` and flag `taken`; either None:
    the caller has no such array) -> 0 for a candidate, else the number of the first failing test"""
    level, octave = int(o["level"]), int(octave)
    if not (max(level - 1, 0) <= octave <= level):
        return 1
    u, v, radius = f32(o["u"]), f32(o["v"]), f32(o["radius"])
    x, y = f32(x), f32(y)
    with np.errstate(all="ignore"):
        if not (np.abs(f32(x - u)) < radius and np.abs(f32(y - v)) < radius):
            return 2
        if taken is not None and int(taken) != 0:
            return 3
        if f32(chi2_mono) > 0:
            ex, ey = f32(u - x), f32(v - y)
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            limit = f32(chi2_mono)
            if check_right and right is not None and f32(right) >= 0:
                er = f32(f32(o["u_right"]) - f32(right))
                e2 = f32(e2 + f32(er * er))
                limit = f32(chi2_stereo)
            s = f32(scale[octave])
            if not e2 <= f32(limit * f32(s * s)):
                return 4
    return 0


def windows_of(pts) -> np.ndarray:
    """tests 2.1 and 2.2 as guided-matching windows: octaves max(level - 1, 0) .. level; a rejected point holds nothing"""
    return R.make_windows(pts["u"], pts["v"], np.where(pts["state"] == 0, pts["radius"], f32(0)), np.maximum(pts["level"] - 1, 0), pts["level"])


def _popcount(a) -> int:
    return int(R._POPCOUNT[a].sum())


def search(pts, p_desc, t_kp, t_desc, scale, chi2_mono=5.99, chi2_stereo=7.8, check_right=False, right=None, taken=None, chunk: int = 512):
    """-> (best row or -1, d1, candidate lists, visited lists, failing-test counts [5]) of every point.  t_kp None = no train
    frame.  The rows that pass tests 1 and 2 (`visited`) are found element-wise for `chunk` points at a time (guided_ref._box_mask:
    the same float32 operations); every one of them then goes through check() as a whole."""
    n = len(pts)
    row1, d1, _ = R.none_result(n)
    cands, visited = [[] for _ in range(n)], [[] for _ in range(n)]
    failed = [0] * 5
    nt = 0 if t_kp is None else len(t_kp)
    if not n or not nt:
        return row1, d1, cands, visited, failed
    win = windows_of(pts)
    p_desc = np.ascontiguousarray(p_desc, np.uint8).reshape(-1, 32)
    t_desc = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
    for a in range(0, n, chunk):
        mask = R._box_mask(win[a:a + chunk], t_kp)
        for i in range(a, min(a + chunk, n)):
            if pts["state"][i] != 0:
                continue
            best = None
            for j in np.flatnonzero(mask[i - a]):  # ascending j
                j = int(j)
                visited[i].append(j)
                c = check(pts[i], t_kp["x"][j], t_kp["y"][j], t_kp["octave"][j], None if right is None else right[j],
                          None if taken is None else taken[j], scale, chi2_mono, chi2_stereo, check_right)
                assert c not in (1, 2), "the window and check() disagree"
                failed[c] += 1
                if c:
                    continue
                cands[i].append(j)
                key = (_popcount(p_desc[i] ^ t_desc[j]) << 20) | j
                if best is None or key < best:
                    best = key
            if best is not None:
                row1[i], d1[i] = best & 0xFFFFF, best >> 20
    return row1, d1, cands, visited, failed


def finish(found, pts, n_train, th_low=50, train_point=None):
    """steps 3 (the threshold) and 4 -> (idx, d1, ACTION_DTYPE rows, summary dict)"""
    row1, d1 = found[0], found[1]
    n = len(row1)
    idx = np.where((row1 >= 0) & (d1.astype(np.int64) <= th_low), row1, -1).astype(np.int32)
    act = np.zeros(n, ACTION_DTYPE)
    act["other"] = -1
    owner = {}
    for i in range(n):
        j = int(idx[i])
        if j < 0:
            continue
        if train_point is not None and int(train_point[j]) >= 0:
            act[i] = (ACT_REPLACE, int(train_point[j]))
            continue
        key = (int(d1[i]) << 20) | i
        if j not in owner or key < owner[j]:
            owner[j] = key
    for i in range(n):
        j = int(idx[i])
        if j < 0 or act["action"][i] == ACT_REPLACE:
            continue
        won = owner[j]
        act[i] = (ACT_ADD, -1) if won == ((int(d1[i]) << 20) | i) else (ACT_DUPLICATE, won & 0xFFFFF)
    summary = {"status": 0, "n_points": n, "n_train": n_train, "n_in_view": int((pts["state"] == 0).sum()),
               "n_candidates": sum(len(c) for c in found[2]), "n_add": int((act["action"] == ACT_ADD).sum()),
               "n_replace": int((act["action"] == ACT_REPLACE).sum()), "n_duplicate": int((act["action"] == ACT_DUPLICATE).sum())}
    return idx, d1.copy(), act, summary


def match(view, points, p_desc, t_kp, t_desc, scale, view_cos_limit=0.5, th=3.0, chi2_mono=5.99, chi2_stereo=7.8, th_low=50, check_right=False,
          skip=None, right=None, taken=None, train_point=None):
    """One frame.  t_kp None = no train frame.  -> (idx, d1, actions, points, summary dict, found)"""
    pts = eval_points(view, points, skip, view_cos_limit, th, scale)
    found = search(pts, p_desc, t_kp, t_desc, scale, chi2_mono, chi2_stereo, check_right, right, taken)
    idx, d1, act, summary = finish(found, pts, 0 if t_kp is None else len(t_kp), th_low, train_point)
    return idx, d1, act, pts, summary, found


def none_points(n: int) -> np.ndarray:
    """what rows past the points hold"""
    o = np.zeros(n, POINT_DTYPE)
    o["level"], o["state"] = -1, -1
    return o


def none_actions(n: int) -> np.ndarray:
    a = np.zeros(n, ACTION_DTYPE)
    a["other"] = -1
    return a
