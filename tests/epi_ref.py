"""numpy / plain-Python restatement of the epipolar search and of the triangulation (test infrastructure, plain module): the
NORMATIVE statement of the rule in include/sendslam_orb.h ("epipolar search and triangulation").

Written from the rule, not from the kernels.  The float32 steps use numpy float32 scalars (every operation rounded once, left to
right as written), the double steps plain Python floats (IEEE double, one operation each); every test is in its accepting form,
so a NaN fails it.  The device code and the host twins must reproduce every number bit for bit.

    pair_init      ss_epi_pair_init: F12, the epipole, the double part
    line_of/check  tests 1 - 3 of one couple; check_many is the same float32 operations element-wise over the candidates of a row
    search         the candidates of every query row (same node, both untaken), the counters, the best key
    finish         guided_ref.finish (one_to_one, orientation) and the summary
    upstream_search a literal restatement of upstream's loops (scan order, dist > bestDist, the tests after the distance)
    triangulate    steps 1 - 9 of one match and its map point; triangulate_rows: a pair's info, compact block and summary
"""
from __future__ import annotations

import math

import numpy as np

import guided_ref as R
import proj_ref as P

f32 = np.float32
NONE = R.NONE
SWEEPS = 6
DBL_MAX = 1.7976931348623157e308

PAIR_DTYPE = np.dtype([("f12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"), ("epipole_test", "<i4")] +
                      [(n + s, "<f8", (k,)) for s in ("1", "2") for n, k in (("rcw", 9), ("tcw", 3), ("ow", 3))] +
                      [(n + s, "<f8") for s in ("1", "2") for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")])
MAP_POINT_DTYPE = P.MAP_POINT_DTYPE
TRI_INFO_DTYPE = np.dtype([("state", "<i4"), ("cos_parallax", "<f4"), ("err1_sq", "<f4"), ("err2_sq", "<f4")])
EPI_SUMMARY_FIELDS = ("status", "n_query", "n_train", "n_candidates", "n_geometric", "n_near", "n_accepted", "n_unique", "n_final", "rot_bins")
TRI_SUMMARY_FIELDS = ("status", "n_query", "n_train", "n_matches", "n_points", "n_state")
UPSTREAM_SEARCH = dict(th=50, coarse=False, one_to_one=False, orientation=1)
UPSTREAM_TRI = dict(cos_parallax_max=0.9998, chi2=5.991, ratio_factor=float(f32(1.5) * f32(1.2)), far_limit=0.0)


def _div(a: float, b: float) -> float:
    """IEEE double division (Python raises where IEEE gives an infinity or a NaN)"""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _to_f32(x: float):
    with np.errstate(all="ignore"):
        return f32(x)


# ---- the pair ---------------------------------------------------------------------------------------------------------------------
def pair_init(cam1, rcw1, tcw1, cam2, rcw2, tcw2) -> np.ndarray:
    """cam: (fx, fy, cx, cy).  -> one PAIR_DTYPE record (shape ())"""
    R1 = [float(v) for v in np.asarray(rcw1, np.float64).reshape(9)]
    R2 = [float(v) for v in np.asarray(rcw2, np.float64).reshape(9)]
    t1 = [float(v) for v in np.asarray(tcw1, np.float64).reshape(3)]
    t2 = [float(v) for v in np.asarray(tcw2, np.float64).reshape(3)]
    fx1, fy1, cx1, cy1 = [float(v) for v in cam1]
    fx2, fy2, cx2, cy2 = [float(v) for v in cam2]
    ifx1, ify1, ifx2, ify2 = _div(1.0, fx1), _div(1.0, fy1), _div(1.0, fx2), _div(1.0, fy2)
    ow1 = [-((R1[k] * t1[0] + R1[3 + k] * t1[1]) + R1[6 + k] * t1[2]) for k in range(3)]
    ow2 = [-((R2[k] * t2[0] + R2[3 + k] * t2[1]) + R2[6 + k] * t2[2]) for k in range(3)]
    R12 = [[(R1[3 * i] * R2[3 * j] + R1[3 * i + 1] * R2[3 * j + 1]) + R1[3 * i + 2] * R2[3 * j + 2] for j in range(3)] for i in range(3)]
    t12 = [t1[i] - ((R12[i][0] * t2[0] + R12[i][1] * t2[1]) + R12[i][2] * t2[2]) for i in range(3)]
    E = [[t12[1] * R12[2][j] - t12[2] * R12[1][j] for j in range(3)],
         [t12[2] * R12[0][j] - t12[0] * R12[2][j] for j in range(3)],
         [t12[0] * R12[1][j] - t12[1] * R12[0][j] for j in range(3)]]
    G = [[ifx1 * E[0][j] for j in range(3)], [ify1 * E[1][j] for j in range(3)], None]
    G[2] = [E[2][j] - (cx1 * G[0][j] + cy1 * G[1][j]) for j in range(3)]
    F = []
    for i in range(3):
        f0, f1 = G[i][0] * ifx2, G[i][1] * ify2
        F.append([f0, f1, G[i][2] - (f0 * cx2 + f1 * cy2)])
    m, finite = 0.0, True
    for row in F:
        for v in row:
            a = abs(v)
            if not a <= DBL_MAX:
                finite = False
            elif a > m:
                m = a
    w = np.zeros((), PAIR_DTYPE)
    if finite and m > 0.0:
        w["f12"] = [_to_f32(F[i][j] / m) for i in range(3) for j in range(3)]
    C2 = [((R2[3 * i] * ow1[0] + R2[3 * i + 1] * ow1[1]) + R2[3 * i + 2] * ow1[2]) + t2[i] for i in range(3)]
    ex = _to_f32(_div(fx2 * C2[0], C2[2]) + cx2)
    ey = _to_f32(_div(fy2 * C2[1], C2[2]) + cy2)
    if np.isfinite(ex) and np.isfinite(ey):
        w["ex"], w["ey"], w["epipole_test"] = ex, ey, 1
    w["rcw1"], w["tcw1"], w["ow1"], w["rcw2"], w["tcw2"], w["ow2"] = R1, t1, ow1, R2, t2, ow2
    w["fx1"], w["fy1"], w["cx1"], w["cy1"], w["invfx1"], w["invfy1"] = fx1, fy1, cx1, cy1, ifx1, ify1
    w["fx2"], w["fy2"], w["cx2"], w["cy2"], w["invfx2"], w["invfy2"] = fx2, fy2, cx2, cy2, ifx2, ify2
    return w


def sigma2_table(scale):
    return [f32(f32(s) * f32(s)) for s in scale]


# ---- tests 1 - 3 of a couple ------------------------------------------------------------------------------------------------------
def line_of(pair, x, y):
    """a, b, c of query keypoint (x, y): once per query row"""
    f = [f32(v) for v in pair["f12"]]
    x, y = f32(x), f32(y)
    with np.errstate(all="ignore"):
        return (f32(f32(f32(x * f[0]) + f32(y * f[3])) + f[6]), f32(f32(f32(x * f[1]) + f32(y * f[4])) + f[7]),
                f32(f32(f32(x * f[2]) + f32(y * f[5])) + f[8]))


def check(pair, coarse, scale, line, xj, yj, octave_j) -> int:
    """0 pass, 1 octave, 2 epipole, 3 line"""
    o = int(octave_j)
    if not 0 <= o < len(scale):
        return 1
    s = f32(scale[o])
    xj, yj = f32(xj), f32(yj)
    with np.errstate(all="ignore"):
        if int(pair["epipole_test"]):
            dx, dy = f32(f32(pair["ex"]) - xj), f32(f32(pair["ey"]) - yj)
            if not f32(f32(dx * dx) + f32(dy * dy)) >= f32(f32(100.0) * s):
                return 2
        if not coarse:
            a, b, c = line
            num = f32(f32(f32(a * xj) + f32(b * yj)) + c)
            den = f32(f32(a * a) + f32(b * b))
            if not (den > f32(0) and f32(f32(num * num) / den) < f32(f32(3.84) * f32(s * s))):
                return 3
    return 0


def check_many(pair, coarse, scale, line, xj, yj, octave_j) -> np.ndarray:
    """check() for the candidates of one row at once: the same float32 operations, element-wise"""
    xj, yj = np.asarray(xj, np.float32), np.asarray(yj, np.float32)
    o = np.asarray(octave_j, np.int64)
    out = np.zeros(len(xj), np.uint8)
    inside = (o >= 0) & (o < len(scale))
    s = np.asarray(scale, np.float32)[np.where(inside, o, 0)]
    with np.errstate(all="ignore"):
        ok = np.ones(len(xj), bool)
        if int(pair["epipole_test"]):
            dx, dy = f32(pair["ex"]) - xj, f32(pair["ey"]) - yj
            ok = (dx * dx + dy * dy) >= f32(100.0) * s
        out[~ok] = 2
        if not coarse:
            a, b, c = line
            num = (a * xj + b * yj) + c
            den = f32(f32(a * a) + f32(b * b))
            good = (den > f32(0)) & ((num * num) / den < f32(3.84) * (s * s))
            out[ok & ~good] = 3
    out[~inside] = 1
    return out


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def search(pair, q_kp, q_desc, q_node, t_kp, t_desc, t_node, scale, th=50, coarse=False, q_taken=None, t_taken=None, exclude_self=False):
    """-> (best row or -1, d1, visited lists, n_geometric, n_near) of every query row.  t_kp None = no train frame."""
    nq = len(q_kp)
    row1, d1, _ = R.none_result(nq)
    visited = [[] for _ in range(nq)]
    n_geo = n_near = 0
    nt = 0 if t_kp is None else len(t_kp)
    if not nq or not nt:
        return row1, d1, visited, 0, 0
    q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    t_desc = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
    rows_of = {}
    for j in range(nt):
        if t_taken is not None and t_taken[j] != 0:
            continue
        rows_of.setdefault(int(t_node[j]), []).append(j)
    for i in range(nq):
        node = int(q_node[i])
        if node < 0 or (q_taken is not None and q_taken[i] != 0):
            continue
        js = np.array([j for j in rows_of.get(node, []) if not (exclude_self and j == i)], np.int64)
        if not len(js):
            continue
        visited[i] = [int(j) for j in js]
        res = check_many(pair, coarse, scale, line_of(pair, q_kp["x"][i], q_kp["y"][i]), t_kp["x"][js], t_kp["y"][js], t_kp["octave"][js])
        geo = js[res == 0]
        n_geo += len(geo)
        if not len(geo):
            continue
        dist = R._POPCOUNT[q_desc[i][None, :] ^ t_desc[geo]].sum(axis=1).astype(np.int64)
        near = dist <= th
        n_near += int(near.sum())
        if near.any():
            key = int(((dist[near] << 20) | geo[near]).min())
            row1[i], d1[i] = key & 0xFFFFF, key >> 20
    return row1, d1, visited, n_geo, n_near


def finish(found, q_kp, t_kp, th=50, one_to_one=False, orientation=0):
    """-> (idx, d1, summary dict): guided_ref.finish as it is, without a ratio test, then the summary"""
    row1, d1, visited, n_geo, n_near = found
    idx, d1, _, g, _ = R.finish((row1, d1, np.full(len(row1), NONE, np.uint16), visited), q_kp, t_kp, th, 0, 0, one_to_one, orientation)
    summary = {"status": 0, "n_query": g["n_query"], "n_train": g["n_train"], "n_candidates": g["n_candidates"], "n_geometric": n_geo,
               "n_near": n_near, "n_accepted": g["n_accepted"], "n_unique": g["n_unique"], "n_final": g["n_final"], "rot_bins": g["rot_bins"]}
    return idx, d1, summary


def match(pair, q_kp, q_desc, q_node, t_kp, t_desc, t_node, scale, th=50, coarse=False, one_to_one=False, orientation=0, q_taken=None,
          t_taken=None, exclude_self=False):
    """one pair; t_kp None = no train frame -> (idx, d1, summary dict)"""
    found = search(pair, q_kp, q_desc, q_node, t_kp, t_desc, t_node, scale, th, coarse, q_taken, t_taken, exclude_self)
    return finish(found, q_kp, t_kp, th, one_to_one, orientation)


def voided(n_rows: int, status: int):
    """what a pair with a flagged frame gets"""
    idx, d1, _ = R.none_result(n_rows)
    return idx, d1, dict({k: 0 for k in EPI_SUMMARY_FIELDS}, status=status, rot_bins=0xFFFFFF)


def upstream_search(pair, q_kp, q_desc, q_node, t_kp, t_desc, t_node, scale, th=50, coarse=False, q_taken=None, t_taken=None):
    """ORBmatcher::SearchForTriangulation's loops as written: the rows of a node in ascending order, `dist > TH_LOW || dist >
    bestDist -> continue` (so the LAST of several equal distances wins), the epipole test and the epipolar line AFTER the
    distance.  The float steps are this library's.  -> best row or -1 per query row, before the rotation histogram"""
    nq, nt = len(q_kp), len(t_kp)
    q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    t_desc = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
    best = np.full(nq, -1, np.int32)
    for i in range(nq):
        if int(q_node[i]) < 0 or (q_taken is not None and q_taken[i] != 0):
            continue
        line = line_of(pair, q_kp["x"][i], q_kp["y"][i])
        best_dist, best_j = th, -1
        for j in range(nt):
            if int(t_node[j]) != int(q_node[i]) or (t_taken is not None and t_taken[j] != 0):
                continue
            dist = int(R._POPCOUNT[q_desc[i] ^ t_desc[j]].sum())
            if dist > th or dist > best_dist:
                continue
            if check(pair, coarse, scale, line, t_kp["x"][j], t_kp["y"][j], t_kp["octave"][j]) != 0:
                continue
            best_j, best_dist = j, dist
        best[i] = best_j
    return best


# ---- the triangulation ----------------------------------------------------------------------------------------------------------------
PAIRS_ORDER = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


class PairD:
    """the double part of a pair as Python floats"""

    def __init__(self, pair):
        for s in ("1", "2"):
            for n in ("rcw", "tcw", "ow"):
                setattr(self, n + s, [float(v) for v in pair[n + s]])
            for n in ("fx", "fy", "cx", "cy", "invfx", "invfy"):
                setattr(self, n + s, float(pair[n + s]))


def _rotate(M, V, p, q):
    apq = M[p][q]
    if apq != 0.0:
        theta = _div(M[q][q] - M[p][p], 2.0 * apq)
        t = _div(1.0 if theta >= 0.0 else -1.0, abs(theta) + math.sqrt(theta * theta + 1.0))
        c = _div(1.0, math.sqrt(t * t + 1.0))
        s = t * c
        for k in range(4):
            if k == p or k == q:
                continue
            akp, akq = M[k][p], M[k][q]
            M[k][p] = M[p][k] = c * akp - s * akq
            M[k][q] = M[q][k] = s * akp + c * akq
        M[p][p] = M[p][p] - t * apq
        M[q][q] = M[q][q] + t * apq
        M[p][q] = M[q][p] = 0.0
        for k in range(4):
            vkp, vkq = V[k][p], V[k][q]
            V[k][p] = c * vkp - s * vkq
            V[k][q] = s * vkp + c * vkq


def dlt_rows(w: PairD, a1, b1, a2, b2):
    """the 4 x 4 matrix A of step 2 from the normalised coordinates of both sides"""
    P1 = [w.rcw1[0:3] + [w.tcw1[0]], w.rcw1[3:6] + [w.tcw1[1]], w.rcw1[6:9] + [w.tcw1[2]]]
    P2 = [w.rcw2[0:3] + [w.tcw2[0]], w.rcw2[3:6] + [w.tcw2[1]], w.rcw2[6:9] + [w.tcw2[2]]]
    return [[a1 * P1[2][c] - P1[0][c] for c in range(4)], [b1 * P1[2][c] - P1[1][c] for c in range(4)],
            [a2 * P2[2][c] - P2[0][c] for c in range(4)], [b2 * P2[2][c] - P2[1][c] for c in range(4)]]


def dlt(A, sweeps: int = SWEEPS):
    """step 2 -> (v of the smallest diagonal entry, the swept M)"""
    M = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(i, 4):
            M[i][j] = M[j][i] = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS_ORDER:
            _rotate(M, V, p, q)
    best = 0
    for k in range(1, 4):
        if M[k][k] < M[best][best]:
            best = k
    return [V[k][best] for k in range(4)], M


def _rejected(state, cosp=0.0, e1=0.0, e2=0.0):
    info = np.zeros((), TRI_INFO_DTYPE)
    info["state"] = state
    info["cos_parallax"], info["err1_sq"], info["err2_sq"] = [_to_f32(v) if v == v else f32(0) for v in (cosp, e1, e2)]  # a NaN is reported as 0
    return info, np.zeros((), MAP_POINT_DTYPE), None


def triangulate(w: PairD, tp, scale, x1, y1, o1, x2, y2, o2, sweeps: int = SWEEPS):
    """steps 1 - 9 of one match -> (TRI_INFO_DTYPE record, MAP_POINT_DTYPE record, X in double or None).  tp: dict
    cos_parallax_max chi2 ratio_factor far_limit"""
    o1, o2 = int(o1), int(o2)
    n_levels = len(scale)
    if not (0 <= o1 < n_levels and 0 <= o2 < n_levels):
        return _rejected(10)
    x1, y1, x2, y2 = float(f32(x1)), float(f32(y1)), float(f32(x2)), float(f32(y2))
    s1, s2 = float(f32(scale[o1])), float(f32(scale[o2]))
    R1, t1, R2, t2 = w.rcw1, w.tcw1, w.rcw2, w.tcw2
    # 1
    a1, b1 = (x1 - w.cx1) * w.invfx1, (y1 - w.cy1) * w.invfy1
    a2, b2 = (x2 - w.cx2) * w.invfx2, (y2 - w.cy2) * w.invfy2
    r1 = [(R1[k] * a1 + R1[3 + k] * b1) + R1[6 + k] for k in range(3)]
    r2 = [(R2[k] * a2 + R2[3 + k] * b2) + R2[6 + k] for k in range(3)]
    dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2]
    l1 = math.sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2])
    l2 = math.sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2])
    cosp = _div(dot, l1 * l2)
    if not (cosp > 0.0 and cosp < tp["cos_parallax_max"]):
        return _rejected(1, cosp)
    # 2
    v, _ = dlt(dlt_rows(w, a1, b1, a2, b2), sweeps)
    if not (abs(v[3]) <= DBL_MAX and v[3] != 0.0):
        return _rejected(2, cosp)
    X = [_div(v[0], v[3]), _div(v[1], v[3]), _div(v[2], v[3])]
    # 3, 4
    z1 = ((R1[6] * X[0] + R1[7] * X[1]) + R1[8] * X[2]) + t1[2]
    if not z1 > 0.0:
        return _rejected(3, cosp)
    z2 = ((R2[6] * X[0] + R2[7] * X[1]) + R2[8] * X[2]) + t2[2]
    if not z2 > 0.0:
        return _rejected(4, cosp)
    # 5
    x1c = ((R1[0] * X[0] + R1[1] * X[1]) + R1[2] * X[2]) + t1[0]
    y1c = ((R1[3] * X[0] + R1[4] * X[1]) + R1[5] * X[2]) + t1[1]
    eu, ev = (_div(w.fx1 * x1c, z1) + w.cx1) - x1, (_div(w.fy1 * y1c, z1) + w.cy1) - y1
    err1 = eu * eu + ev * ev
    if not err1 <= tp["chi2"] * (s1 * s1):
        return _rejected(5, cosp, err1)
    # 6
    x2c = ((R2[0] * X[0] + R2[1] * X[1]) + R2[2] * X[2]) + t2[0]
    y2c = ((R2[3] * X[0] + R2[4] * X[1]) + R2[5] * X[2]) + t2[1]
    eu, ev = (_div(w.fx2 * x2c, z2) + w.cx2) - x2, (_div(w.fy2 * y2c, z2) + w.cy2) - y2
    err2 = eu * eu + ev * ev
    if not err2 <= tp["chi2"] * (s2 * s2):
        return _rejected(6, cosp, err1, err2)
    # 7
    n1 = [X[k] - w.ow1[k] for k in range(3)]
    n2 = [X[k] - w.ow2[k] for k in range(3)]
    d1 = math.sqrt((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2])
    d2 = math.sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2])
    if not (d1 > 0.0 and d2 > 0.0):
        return _rejected(7, cosp, err1, err2)
    # 8
    far = tp["far_limit"]
    if far > 0.0 and not (d1 < far and d2 < far):
        return _rejected(8, cosp, err1, err2)
    # 9
    rd, ro = _div(d2, d1), _div(s1, s2)
    if not (rd * tp["ratio_factor"] >= ro and rd <= ro * tp["ratio_factor"]):
        return _rejected(9, cosp, err1, err2)
    info = _rejected(0, cosp, err1, err2)[0]
    max_dist = d1 * s1
    p = np.zeros((), MAP_POINT_DTYPE)
    p["x"], p["y"], p["z"] = _to_f32(X[0]), _to_f32(X[1]), _to_f32(X[2])
    p["nx"], p["ny"], p["nz"] = [_to_f32((_div(n1[k], d1) + _div(n2[k], d2)) / 2.0) for k in range(3)]
    p["max_dist"] = _to_f32(max_dist)
    p["min_dist"] = _to_f32(_div(max_dist, float(f32(scale[n_levels - 1]))))
    return info, p, X


def triangulate_couples(pair, tp, scale, kp1, kp2):
    """the n couples (kp1[k], kp2[k]) -> (TRI_INFO_DTYPE [n], MAP_POINT_DTYPE [n], list of X or None)"""
    w = PairD(pair)
    n = len(kp1)
    info, pts, xs = np.zeros(n, TRI_INFO_DTYPE), np.zeros(n, MAP_POINT_DTYPE), []
    for k in range(n):
        info[k], pts[k], X = triangulate(w, tp, scale, kp1["x"][k], kp1["y"][k], kp1["octave"][k], kp2["x"][k], kp2["y"][k], kp2["octave"][k])
        xs.append(X)
    return info, pts, xs


def none_info(n: int) -> np.ndarray:
    o = np.zeros(n, TRI_INFO_DTYPE)
    o["state"] = -1
    return o


def compact(info, pts, idx, q_desc, n_train, status: int = 0):
    """the per-row results of a pair (info / pts aligned to the query rows) -> (points, point_desc, point_rows, summary dict): the
    state-0 rows in ascending query row"""
    rows = np.flatnonzero(info["state"] == 0)
    q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    states = [int((info["state"] == k).sum()) for k in range(11)]
    summary = {"status": status, "n_query": len(info), "n_train": n_train, "n_matches": int((info["state"] != -1).sum()), "n_points": len(rows),
               "n_state": states}
    return pts[rows].copy(), q_desc[rows].copy(), np.stack([rows, np.asarray(idx)[rows]], 1).astype(np.int32).reshape(-1, 2), summary


def triangulate_rows(pair, tp, scale, q_kp, q_desc, t_kp, idx):
    """one pair from its matches -> (info [n_query], points, point_desc, point_rows, summary dict).  t_kp None = no train frame;
    an idx entry outside 0 .. n_train - 1 is no match"""
    nq, nt = len(q_kp), 0 if t_kp is None else len(t_kp)
    idx = np.asarray(idx, np.int64)[:nq]
    info, pts = none_info(nq), np.zeros(nq, MAP_POINT_DTYPE)
    w = PairD(pair)
    for i in range(nq):
        j = int(idx[i])
        if 0 <= j < nt:
            info[i], pts[i], _ = triangulate(w, tp, scale, q_kp["x"][i], q_kp["y"][i], q_kp["octave"][i], t_kp["x"][j], t_kp["y"][j], t_kp["octave"][j])
    return (info,) + compact(info, pts, idx, q_desc, nt)
