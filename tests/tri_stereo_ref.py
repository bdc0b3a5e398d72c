"""The normative statement of the stereo form of the triangulation (include/sendslam_orb.h, ss_triangulate_stereo_*; DESIGN.md
section 35) in Python floats (test infrastructure, plain module): tests/epi_ref.py's steps 1 - 9 with upstream's stereo parallax, the
unprojection modes (tests/unproject_ref.py's position) and the three-term errors.  Every step is one float64 operation, left to right."""
from __future__ import annotations

import math

import numpy as np

import epi_ref as E
from epi_ref import DBL_MAX, MAP_POINT_DTYPE, _div, _to_f32, f32

INFO_DTYPE = np.dtype([("state", "<i4"), ("mode", "<i4"), ("cos_rays", "<f4"), ("cs1", "<f4"), ("cs2", "<f4"), ("err1_sq", "<f4"), ("err2_sq", "<f4"),
                       ("reserved", "<i4")])
UPSTREAM = dict(E.UPSTREAM_TRI, chi2_stereo=7.8)


def stereo_cos(b: float, depth) -> float:
    """cos(2 atan2(b / 2, depth)) in its closed form"""
    d, h = float(f32(depth)), b / 2.0
    return _div(d * d - h * h, d * d + h * h)


def _rejected(state, mode=-1, cosr=0.0, cs1=0.0, cs2=0.0, e1=0.0, e2=0.0):
    info = np.zeros((), INFO_DTYPE)
    info["state"], info["mode"] = state, mode
    for name, v in (("cos_rays", cosr), ("cs1", cs1), ("cs2", cs2), ("err1_sq", e1), ("err2_sq", e2)):
        info[name] = _to_f32(v) if v == v else f32(0)  # a NaN is reported as 0
    return info, np.zeros((), MAP_POINT_DTYPE)


def unproject(R, ow, cx, cy, invfx, invfy, x, y, depth):
    """tests/unproject_ref.py::map_point's position, on Python floats"""
    z = float(f32(depth))
    xc, yc = ((x - cx) * z) * invfx, ((y - cy) * z) * invfy
    return [((R[k] * xc + R[3 + k] * yc) + R[6 + k] * z) + ow[k] for k in range(3)]


def triangulate(w: E.PairD, rig, tp, scale, x1, y1, o1, depth1, right1, x2, y2, o2, depth2, right2, trace=None):
    """one match -> (INFO_DTYPE record, MAP_POINT_DTYPE record).  rig: dict bf1 b1 bf2 b2; tp: UPSTREAM's keys; trace: a dict that
    receives cos_rays, err1 and err2 in double as far as they were formed"""
    trace = {} if trace is None else trace
    o1, o2 = int(o1), int(o2)
    n_levels = len(scale)
    if not (0 <= o1 < n_levels and 0 <= o2 < n_levels):
        return _rejected(10)
    x1, y1, x2, y2 = float(f32(x1)), float(f32(y1)), float(f32(x2)), float(f32(y2))
    s1, s2 = float(f32(scale[o1])), float(f32(scale[o2]))
    R1, t1, R2, t2 = w.rcw1, w.tcw1, w.rcw2, w.tcw2
    a1, b1 = (x1 - w.cx1) * w.invfx1, (y1 - w.cy1) * w.invfy1
    a2, b2 = (x2 - w.cx2) * w.invfx2, (y2 - w.cy2) * w.invfy2
    r1 = [(R1[k] * a1 + R1[3 + k] * b1) + R1[6 + k] for k in range(3)]
    r2 = [(R2[k] * a2 + R2[3 + k] * b2) + R2[6 + k] for k in range(3)]
    dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2]
    l1 = math.sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2])
    l2 = math.sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2])
    cosr = trace["cos_rays"] = _div(dot, l1 * l2)
    stereo1, stereo2 = bool(f32(right1) >= 0), bool(f32(right2) >= 0)
    cs1 = cs2 = cosr + 1.0
    if stereo1:
        cs1 = stereo_cos(rig["b1"], depth1)
    elif stereo2:  # upstream's else: with both sides stereo only cs1 is formed
        cs2 = stereo_cos(rig["b2"], depth2)
    cs = cs2 if cs2 < cs1 else cs1
    if cosr < cs and cosr > 0.0 and (stereo1 or stereo2 or cosr < tp["cos_parallax_max"]):
        mode = 0
        v, _ = E.dlt(E.dlt_rows(w, a1, b1, a2, b2))
        if not (abs(v[3]) <= DBL_MAX and v[3] != 0.0):
            return _rejected(2, mode, cosr, cs1, cs2)
        X = [_div(v[0], v[3]), _div(v[1], v[3]), _div(v[2], v[3])]
    elif stereo1 and cs1 < cs2:
        mode, X = 1, unproject(R1, w.ow1, w.cx1, w.cy1, w.invfx1, w.invfy1, x1, y1, depth1)
    elif stereo2 and cs2 < cs1:
        mode, X = 2, unproject(R2, w.ow2, w.cx2, w.cy2, w.invfx2, w.invfy2, x2, y2, depth2)
    else:
        return _rejected(1, -1, cosr, cs1, cs2)
    z1 = ((R1[6] * X[0] + R1[7] * X[1]) + R1[8] * X[2]) + t1[2]
    if not z1 > 0.0:
        return _rejected(3, mode, cosr, cs1, cs2)
    z2 = ((R2[6] * X[0] + R2[7] * X[1]) + R2[8] * X[2]) + t2[2]
    if not z2 > 0.0:
        return _rejected(4, mode, cosr, cs1, cs2)

    def side(R, t, fx, fy, cx, cy, z, x, y, stereo, bf, right):
        xc = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0]
        yc = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1]
        u = _div(fx * xc, z) + cx
        eu, ev = u - x, (_div(fy * yc, z) + cy) - y
        err, lim = eu * eu + ev * ev, tp["chi2"]
        if stereo:
            er = (u - bf * _div(1.0, z)) - float(f32(right))
            err, lim = err + er * er, tp["chi2_stereo"]
        return err, lim
    err1, lim1 = trace["err1"], _ = side(R1, t1, w.fx1, w.fy1, w.cx1, w.cy1, z1, x1, y1, stereo1, rig["bf1"], right1)
    if not err1 <= lim1 * (s1 * s1):
        return _rejected(5, mode, cosr, cs1, cs2, err1)
    err2, lim2 = trace["err2"], _ = side(R2, t2, w.fx2, w.fy2, w.cx2, w.cy2, z2, x2, y2, stereo2, rig["bf2"], right2)
    if not err2 <= lim2 * (s2 * s2):
        return _rejected(6, mode, cosr, cs1, cs2, err1, err2)
    n1 = [X[k] - w.ow1[k] for k in range(3)]
    n2 = [X[k] - w.ow2[k] for k in range(3)]
    d1 = math.sqrt((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2])
    d2 = math.sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2])
    if not (d1 > 0.0 and d2 > 0.0):
        return _rejected(7, mode, cosr, cs1, cs2, err1, err2)
    far = tp["far_limit"]
    if far > 0.0 and not (d1 < far and d2 < far):
        return _rejected(8, mode, cosr, cs1, cs2, err1, err2)
    rd, ro = _div(d2, d1), _div(s1, s2)
    if not (rd * tp["ratio_factor"] >= ro and rd <= ro * tp["ratio_factor"]):
        return _rejected(9, mode, cosr, cs1, cs2, err1, err2)
    info = _rejected(0, mode, cosr, cs1, cs2, err1, err2)[0]
    max_dist = d1 * s1
    p = np.zeros((), MAP_POINT_DTYPE)
    p["x"], p["y"], p["z"] = _to_f32(X[0]), _to_f32(X[1]), _to_f32(X[2])
    p["nx"], p["ny"], p["nz"] = [_to_f32((_div(n1[k], d1) + _div(n2[k], d2)) / 2.0) for k in range(3)]
    p["max_dist"] = _to_f32(max_dist)
    p["min_dist"] = _to_f32(_div(max_dist, float(f32(scale[n_levels - 1]))))
    return info, p


def couples(pair, rig, tp, scale, kp1, kp2, depth1, right1, depth2, right2):
    """the n couples (kp1[k], kp2[k]) -> (INFO_DTYPE [n], MAP_POINT_DTYPE [n])"""
    w, n = E.PairD(pair), len(kp1)
    info, pts = np.zeros(n, INFO_DTYPE), np.zeros(n, MAP_POINT_DTYPE)
    for k in range(n):
        info[k], pts[k] = triangulate(w, rig, tp, scale, kp1["x"][k], kp1["y"][k], kp1["octave"][k], depth1[k], right1[k], kp2["x"][k], kp2["y"][k],
                                      kp2["octave"][k], depth2[k], right2[k])
    return info, pts
