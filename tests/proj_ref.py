"""numpy restatement of the map-point projection search (test infrastructure, plain module): the NORMATIVE statement of the rule
in include/sendslam_orb.h ("map-point projection search").

Written from the rule, not from the kernel: one map point at a time, float32 at every step (every operation rounded once, left
to right as written), every test in its accepting form so that a NaN fails it.  The device code and the host twin
ss_proj_points_host must reproduce every number bit for bit.

    view_init    ss_proj_view_init: the pose and intrinsics rounded to float32, ow = -R^T t formed in double
    eval_point   steps 1 - 3: frustum state, predicted level, window
    level_table  step 2 as the rule states it; level_log is upstream's ceil(logf(ratio) / logScaleFactor), clamped
    search       the candidates of every point (guided_ref's box test, the taken mask, the right-eye test), best and second key
    finish       the level-aware acceptance test and one_to_one
"""
from __future__ import annotations

import numpy as np

import guided_ref as R

f32 = np.float32
NONE = R.NONE

VIEW_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))] +
                      [(n, "<f4") for n in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y")])
MAP_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
POINT_DTYPE = np.dtype([(n, "<f4") for n in ("u", "v", "u_right", "view_cos", "dist", "radius")] + [("level", "<i4"), ("state", "<i4")])
SUMMARY_FIELDS = ("status", "n_points", "n_train", "n_in_view", "n_candidates", "n_accepted", "n_unique", "reserved")
UPSTREAM = dict(view_cos_limit=0.5, th=1.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10, one_to_one=False, check_right=False)


def view_init(fx, fy, cx, cy, width, height, rcw, tcw, bf) -> np.ndarray:
    """-> one VIEW_DTYPE record (shape ())"""
    r = [float(v) for v in np.asarray(rcw, np.float64).reshape(9)]
    t = [float(v) for v in np.asarray(tcw, np.float64).reshape(3)]
    v = np.zeros((), VIEW_DTYPE)
    v["rcw"], v["tcw"] = r, t
    v["ow"] = [-((r[k] * t[0] + r[3 + k] * t[1]) + r[6 + k] * t[2]) for k in range(3)]  # double, rounded by the store
    v["fx"], v["fy"], v["cx"], v["cy"], v["bf"] = fx, fy, cx, cy, bf
    v["min_x"], v["max_x"], v["min_y"], v["max_y"] = 0, width, 0, height
    return v


def level_table(ratio, scale) -> int:
    """the smallest n with ratio <= scale[n], else the last level (a NaN ratio too)"""
    for n in range(len(scale)):
        if f32(ratio) <= f32(scale[n]):
            return n
    return len(scale) - 1


def level_log(ratio, scale_factor, n_levels: int) -> int:
    """MapPoint::PredictScale: ceil(log(ratio) / mfLogScaleFactor), clamped, with numpy's float32 log"""
    with np.errstate(all="ignore"):
        n = np.ceil(f32(np.log(f32(ratio)) / np.log(f32(scale_factor))))
    return int(min(max(n, 0), n_levels - 1))


def _rejected(state: int) -> np.ndarray:
    o = np.zeros((), POINT_DTYPE)
    o["level"], o["state"] = -1, state
    return o


def eval_point(view, p, view_cos_limit, th, far_limit, scale) -> np.ndarray:
    """steps 1 - 3 of one map point -> one POINT_DTYPE record"""
    w = view
    r, t, ow = [f32(v) for v in w["rcw"]], [f32(v) for v in w["tcw"]], [f32(v) for v in w["ow"]]
    x, y, z = f32(p["x"]), f32(p["y"]), f32(p["z"])
    with np.errstate(all="ignore"):
        pc = [f32(f32(f32(f32(r[3 * k] * x) + f32(r[3 * k + 1] * y)) + f32(r[3 * k + 2] * z)) + t[k]) for k in range(3)]
        if not pc[2] > 0:
            return _rejected(1)
        invz = f32(f32(1.0) / pc[2])
        u = f32(f32(f32(f32(w["fx"]) * pc[0]) * invz) + f32(w["cx"]))
        v = f32(f32(f32(f32(w["fy"]) * pc[1]) * invz) + f32(w["cy"]))
        if not (u >= f32(w["min_x"]) and u <= f32(w["max_x"]) and v >= f32(w["min_y"]) and v <= f32(w["max_y"])):
            return _rejected(2)
        po = [f32(x - ow[0]), f32(y - ow[1]), f32(z - ow[2])]
        dist = f32(np.sqrt(f32(f32(f32(po[0] * po[0]) + f32(po[1] * po[1])) + f32(po[2] * po[2]))))
        if not (dist >= f32(f32(0.8) * f32(p["min_dist"])) and dist <= f32(f32(1.2) * f32(p["max_dist"]))):
            return _rejected(3)
        dot = f32(f32(f32(po[0] * f32(p["nx"])) + f32(po[1] * f32(p["ny"]))) + f32(po[2] * f32(p["nz"])))
        view_cos = f32(dot / dist)
        if not view_cos >= f32(view_cos_limit):
            return _rejected(4)
        if f32(far_limit) > 0 and not dist <= f32(far_limit):
            return _rejected(5)
        ratio = f32(f32(p["max_dist"]) / dist)
        level = level_table(ratio, scale)
        rr = f32((f32(2.5) if view_cos > f32(0.998) else f32(4.0)) * f32(th))
        o = np.zeros((), POINT_DTYPE)
        o["u"], o["v"], o["u_right"] = u, v, f32(u - f32(f32(w["bf"]) * invz))
        o["view_cos"], o["dist"], o["radius"] = view_cos, dist, f32(rr * f32(scale[level]))
        o["level"], o["state"] = level, 0
    return o


def eval_points(view, points, view_cos_limit, th, far_limit, scale) -> np.ndarray:
    out = np.zeros(len(points), POINT_DTYPE)
    for i in range(len(points)):
        out[i] = eval_point(view, points[i], view_cos_limit, th, far_limit, scale)
    return out


def windows_of(proj) -> np.ndarray:
    """the guided-matching window of every point: its projection, its radius, octaves level - 1 .. level; a point that is
    not in view gets a window without a radius, which holds nothing"""
    return R.make_windows(proj["u"], proj["v"], np.where(proj["state"] == 0, proj["radius"], f32(0)), proj["level"] - 1, proj["level"])


def _popcount(a) -> int:
    return int(R._POPCOUNT[a].sum())


def search(proj, p_desc, t_kp, t_desc, check_right=False, right=None, taken=None, chunk: int = 512):
    """-> (best row or -1, second row or -1, d1, d2, candidate lists) of every point, before the acceptance test.  t_kp None = no
    train frame.  The box test runs element-wise for `chunk` points at a time (guided_ref._box_mask: the float32 operations of
    box_candidates), the rest one point at a time."""
    n = len(proj)
    row1, d1, d2 = R.none_result(n)
    row2 = row1.copy()
    cands = [[] for _ in range(n)]
    nt = 0 if t_kp is None else len(t_kp)
    if not n or not nt:
        return row1, row2, d1, d2, cands
    win = windows_of(proj)
    p_desc = np.ascontiguousarray(p_desc, np.uint8).reshape(-1, 32)
    t_desc = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
    for a in range(0, n, chunk):
        mask = R._box_mask(win[a:a + chunk], t_kp)
        for i in range(a, min(a + chunk, n)):
            if proj["state"][i] != 0:
                continue
            keys = []
            for j in np.flatnonzero(mask[i - a]):  # ascending j
                if taken is not None and taken[j] != 0:
                    continue
                if check_right and f32(right[j]) > 0:
                    with np.errstate(all="ignore"):
                        if not np.abs(f32(f32(proj["u_right"][i]) - f32(right[j]))) <= f32(proj["radius"][i]):
                            continue
                cands[i].append(int(j))
                keys.append((_popcount(p_desc[i] ^ t_desc[j]) << 20) | int(j))
            keys.sort()
            if keys:
                row1[i], d1[i] = keys[0] & 0xFFFFF, keys[0] >> 20
            if len(keys) > 1:
                row2[i], d2[i] = keys[1] & 0xFFFFF, keys[1] >> 20
    return row1, row2, d1, d2, cands


def finish(found, proj, t_kp, th_high=100, ratio_num=8, ratio_den=10, one_to_one=False):
    """-> (idx, d1, d2, summary dict, candidate lists)"""
    row1, row2, d1, d2, cands = found
    n = len(row1)
    nt = 0 if t_kp is None else len(t_kp)
    idx = np.full(n, -1, np.int32)
    for i in range(n):
        if row1[i] < 0:
            continue
        lvl1 = int(t_kp["octave"][row1[i]])
        lvl2 = int(t_kp["octave"][row2[i]]) if row2[i] >= 0 else -1
        best, second = int(d1[i]), int(d2[i])
        if best <= th_high and not (ratio_den != 0 and lvl1 == lvl2 and best * ratio_den > second * ratio_num):
            idx[i] = row1[i]
    n_acc = int((idx >= 0).sum())
    if one_to_one:
        owner = {}
        for i in range(n):
            if idx[i] >= 0:
                key, j = (int(d1[i]) << 20) | i, int(idx[i])
                if j not in owner or key < owner[j]:
                    owner[j] = key
        for i in range(n):
            if idx[i] >= 0 and owner[int(idx[i])] != ((int(d1[i]) << 20) | i):
                idx[i] = -1
    summary = {"status": 0, "n_points": n, "n_train": nt, "n_in_view": int((proj["state"] == 0).sum()),
               "n_candidates": sum(len(c) for c in cands), "n_accepted": n_acc, "n_unique": int((idx >= 0).sum()), "reserved": 0}
    return idx, d1.copy(), d2.copy(), summary, cands


def match(view, points, p_desc, t_kp, t_desc, scale, view_cos_limit=0.5, th=1.0, far_limit=0.0, th_high=100, ratio_num=8, ratio_den=10,
          one_to_one=False, check_right=False, right=None, taken=None):
    """One frame.  t_kp None = no train frame.  -> (idx, d1, d2, proj, summary dict, candidate lists)"""
    proj = eval_points(view, points, view_cos_limit, th, far_limit, scale)
    found = search(proj, p_desc, t_kp, t_desc, check_right, right, taken)
    idx, d1, d2, summary, cands = finish(found, proj, t_kp, th_high, ratio_num, ratio_den, one_to_one)
    return idx, d1, d2, proj, summary, cands


def none_points(n: int) -> np.ndarray:
    """what rows past the points hold"""
    o = np.zeros(n, POINT_DTYPE)
    o["level"], o["state"] = -1, -1
    return o
