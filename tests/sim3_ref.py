"""The Sim3 RANSAC of include/sendslam_orb.h (Sim3Solver as LoopClosing::DetectCommonRegionsFromBoW uses it), restated in numpy:
the NORMATIVE statement of the rule (test infrastructure, plain module).  Upstream's source is not in the reference tree; parity with
the real binary stays unpinned and every deviation is listed in the header.

    correspondences()   step 1: the kept (query row, train row) couples in ascending query row and their twelve float32 numbers
    mix32(), draw()     step 3a: the draw stream and the three draws of a hypothesis (sparse swap-with-last)
    model()             step 3b: Horn's closed form in double (Python floats), rounded to float32 once
    errors(), count()   step 3c: both reprojection errors of every correspondence, vectorised over correspondences in float32
    solve()             steps 1 - 4 of one pair -> (SIM3_RESULT_DTYPE record, uint8 flag per query row, count[t] or None)

Every float32 step is one numpy float32 operation and every double step one Python float operation, left to right as the header
writes them.  The Jacobi rotation is the triangulation's (epi_ref._rotate), not a copy.
"""
from __future__ import annotations

import math

import numpy as np

import epi_ref as E

f32 = np.float32
MAX_ITERATIONS = 1024
RESULT_DTYPE = np.dtype([("sr12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("sr21", "<f4", (9,)), ("t21", "<f4", (3,))] +
                        [(n, "<i4") for n in ("state", "n_corr", "n_inliers", "best_inliers", "iteration", "status", "reserved")])
MODEL_FIELDS = ("sr12", "t12", "s12", "sr21", "t21")
UPSTREAM = dict(chi2=9.210, min_inliers=20, max_iterations=300, fix_scale=False)
M32 = 0xFFFFFFFF


# ---- step 3a ------------------------------------------------------------------------------------------------------------------------
def mix32(seed: int, pair: int, n: int) -> int:
    h = ((seed ^ ((pair * 0x9E3779B1) & M32)) + n * 0x85EBCA77) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def draw(seed: int, pair: int, t: int, n: int):
    """three draws without replacement over 0 .. n-1: at most two slots are ever displaced, so no array is kept"""
    moved = {}
    out = []
    for k in range(3):
        j = (mix32(seed, pair, 3 * t + k) * (n - k)) >> 32
        out.append(moved.get(j, j))
        moved[j] = moved.get(n - 1 - k, n - 1 - k)
    return out


def draw_literal(seed: int, pair: int, t: int, n: int):
    """the same on upstream's vAvailableIndices, an array of n entries: take entry j, move the last entry into its place, drop the last"""
    avail = list(range(n))
    out = []
    for k in range(3):
        j = (mix32(seed, pair, 3 * t + k) * len(avail)) >> 32
        out.append(avail[j])
        avail[j] = avail[-1]
        avail.pop()
    return out


# ---- step 3b ------------------------------------------------------------------------------------------------------------------------
def _dot(a, b) -> float:
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def model(x1, x2, fix_scale: bool = False, sweeps: int = E.SWEEPS) -> np.ndarray:
    """x1[k], x2[k]: float32 camera coordinates of draw k in keyframe 1 and 2 -> a RESULT_DTYPE record holding the model"""
    P1 = [[float(f32(v)) for v in row] for row in np.asarray(x1).reshape(3, 3)]
    P2 = [[float(f32(v)) for v in row] for row in np.asarray(x2).reshape(3, 3)]
    with np.errstate(all="ignore"):
        o1 = [((P1[0][i] + P1[1][i]) + P1[2][i]) / 3.0 for i in range(3)]
        o2 = [((P2[0][i] + P2[1][i]) + P2[2][i]) / 3.0 for i in range(3)]
        a = [[P1[k][i] - o1[i] for i in range(3)] for k in range(3)]
        b = [[P2[k][i] - o2[i] for i in range(3)] for k in range(3)]
        m = [[(b[0][i] * a[0][j] + b[1][i] * a[1][j]) + b[2][i] * a[2][j] for j in range(3)] for i in range(3)]
        N = [[0.0] * 4 for _ in range(4)]
        N[0][0] = (m[0][0] + m[1][1]) + m[2][2]
        N[0][1] = m[1][2] - m[2][1]
        N[0][2] = m[2][0] - m[0][2]
        N[0][3] = m[0][1] - m[1][0]
        N[1][1] = (m[0][0] - m[1][1]) - m[2][2]
        N[1][2] = m[0][1] + m[1][0]
        N[1][3] = m[2][0] + m[0][2]
        N[2][2] = (m[1][1] - m[0][0]) - m[2][2]
        N[2][3] = m[1][2] + m[2][1]
        N[3][3] = (m[2][2] - m[0][0]) - m[1][1]
        for i in range(4):
            for j in range(i):
                N[i][j] = N[j][i]
        V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
        for _ in range(sweeps):
            for p, q in E.PAIRS_ORDER:
                E._rotate(N, V, p, q)
        best = 0
        for k in range(1, 4):
            if N[k][k] > N[best][best]:
                best = k
        qv = [V[k][best] for k in range(4)]
        qn = math.sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3])
        w, x, y, z = (E._div(v, qn) for v in qv)
        r = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
             2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
             2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
        s = 1.0
        if not fix_scale:
            p3 = [[_dot(r[3 * i:3 * i + 3], b[k]) for i in range(3)] for k in range(3)]
            nom = (_dot(a[0], p3[0]) + _dot(a[1], p3[1])) + _dot(a[2], p3[2])
            den = (_dot(p3[0], p3[0]) + _dot(p3[1], p3[1])) + _dot(p3[2], p3[2])
            s = E._div(nom, den)
        t12 = [o1[i] - s * _dot(r[3 * i:3 * i + 3], o2) for i in range(3)]
        s21 = E._div(1.0, s)
        out = np.zeros((), RESULT_DTYPE)
        out["sr12"] = [E._to_f32(s * r[k]) for k in range(9)]
        out["sr21"] = [E._to_f32(s21 * r[3 * (k % 3) + k // 3]) for k in range(9)]
        out["t12"] = [E._to_f32(v) for v in t12]
        out["t21"] = [E._to_f32(-(s21 * _dot([r[i], r[3 + i], r[6 + i]], t12))) for i in range(3)]
        out["s12"] = E._to_f32(s)
    if not all(np.isfinite(out[n]).all() for n in MODEL_FIELDS):
        out = np.zeros((), RESULT_DTYPE)  # the zero model
    out["iteration"] = -1
    return out


# ---- steps 1 and 3c -----------------------------------------------------------------------------------------------------------------
def _transform(m, t, X):
    """m: 9 float32, t: 3 float32, X: [n, 3] float32 -> [n, 3]"""
    return np.stack([((m[3 * i] * X[:, 0] + m[3 * i + 1] * X[:, 1]) + m[3 * i + 2] * X[:, 2]) + t[i] for i in range(3)], axis=1)


def _project(X, view):
    invz = f32(1.0) / X[:, 2]
    return view["fx"] * X[:, 0] * invz + view["cx"], view["fy"] * X[:, 1] * invz + view["cy"]


def correspondences(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale, chi2):
    """-> dict rows (query rows, ascending), cols (train rows), x1, x2 [N, 3], u1 v1 u2 v2 max1 max2 [N], all float32"""
    sc = np.asarray(scale, f32)
    nq, nt, n_levels = len(q_xyz), len(t_xyz), len(sc)
    idx = np.asarray(idx, np.int64)[:nq]
    rows = np.arange(nq)
    ok = (idx >= 0) & (idx < nt)
    j = np.where(ok, idx, 0)
    if nt:
        o2 = t_kp["octave"][j]
        ok &= (o2 >= 0) & (o2 < n_levels)
        if t_skip is not None:
            ok &= np.asarray(t_skip)[j] == 0
    else:
        ok[:] = False
    ok &= (q_kp["octave"][:nq] >= 0) & (q_kp["octave"][:nq] < n_levels)
    if q_skip is not None:
        ok &= np.asarray(q_skip)[:nq] == 0
    rows, cols = rows[ok], j[ok]
    with np.errstate(all="ignore"):
        P1 = np.stack([q_xyz[n][rows] for n in "xyz"], axis=1).astype(f32)
        P2 = np.stack([t_xyz[n][cols] for n in "xyz"], axis=1).astype(f32) if len(cols) else np.zeros((0, 3), f32)
        x1 = _transform(view1["rcw"], view1["tcw"], P1)
        x2 = _transform(view2["rcw"], view2["tcw"], P2)
        u1, v1 = _project(x1, view1)
        u2, v2 = _project(x2, view2)
        s1, s2 = sc[q_kp["octave"][rows]], sc[t_kp["octave"][cols]] if len(cols) else np.zeros(0, f32)
        c2 = f32(chi2)
        return dict(rows=rows, cols=cols, x1=x1, x2=x2, u1=u1, v1=v1, u2=u2, v2=v2, max1=c2 * (s1 * s1), max2=c2 * (s2 * s2))


def errors(c, m, view1, view2):
    """(e1, e2) of every correspondence of c under the model m"""
    with np.errstate(all="ignore"):
        qu, qv = _project(_transform(m["sr12"], m["t12"], c["x2"]), view1)
        du, dv = c["u1"] - qu, c["v1"] - qv
        e1 = du * du + dv * dv
        qu, qv = _project(_transform(m["sr21"], m["t21"], c["x1"]), view2)
        du, dv = c["u2"] - qu, c["v2"] - qv
        e2 = du * du + dv * dv
    return e1, e2


def inliers(c, m, view1, view2) -> np.ndarray:
    e1, e2 = errors(c, m, view1, view2)
    with np.errstate(all="ignore"):
        return (e1 < c["max1"]) & (e2 < c["max2"])


def hypothesis(c, t: int, seed: int, pair: int, fix_scale: bool):
    pick = draw(seed, pair, t, len(c["rows"]))
    return model(c["x1"][pick], c["x2"][pick], fix_scale)


def too_few(n: int, min_inliers: int) -> bool:
    return n < 3 or n < min_inliers


def select(counts, min_inliers: int) -> int:
    """step 4: the smallest t with count[t] > min_inliers, or -1"""
    over = np.flatnonzero(np.asarray(counts) > min_inliers)
    return int(over[0]) if len(over) else -1


def solve(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale, chi2=9.210, min_inliers=20, max_iterations=300, fix_scale=False,
          seed=0, pair=0, status=0):
    """-> (RESULT_DTYPE record, uint8 [n_query], int count[max_iterations] or None in state 1)"""
    res = np.zeros((), RESULT_DTYPE)
    flags = np.zeros(len(q_xyz), np.uint8)
    res["iteration"], res["status"] = -1, status
    if status != 0:
        res["state"] = 1
        return res, flags, None
    c = correspondences(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale, chi2)
    n = len(c["rows"])
    res["n_corr"] = n
    if too_few(n, min_inliers):
        res["state"] = 1
        return res, flags, None
    models = [hypothesis(c, t, seed, pair, fix_scale) for t in range(max_iterations)]
    counts = np.array([int(inliers(c, m, view1, view2).sum()) for m in models], np.int64)
    res["best_inliers"] = counts.max()
    t = select(counts, min_inliers)
    if t < 0:
        res["state"] = 2
        return res, flags, counts
    for name in MODEL_FIELDS:
        res[name] = models[t][name]
    res["n_inliers"], res["iteration"] = counts[t], t
    flags[c["rows"][inliers(c, models[t], view1, view2)]] = 1
    return res, flags, counts


def upstream_iterate(view1, view2, c, min_inliers, max_iterations, fix_scale, seed, pair):
    """Sim3Solver::iterate, literally in its order and early return, on this rule's draw stream and model: hypotheses in sequence, the
    best so far kept under >=, the return at the first best with more than min_inliers -> (t or -1, model or None, best count)"""
    best_inliers, best_model, n_iter = 0, None, 0
    n = len(c["rows"])
    if n < min_inliers or n < 3:
        return -1, None, 0
    while n_iter < max_iterations:
        m = hypothesis(c, n_iter, seed, pair, fix_scale)
        n_iter += 1
        n_in = int(inliers(c, m, view1, view2).sum())
        if n_in >= best_inliers:
            best_inliers, best_model = n_in, m
            if n_in > min_inliers:
                return n_iter - 1, best_model, best_inliers
    return -1, None, best_inliers


def to_scw(res, rcw2, tcw2):
    """ss_sim3_to_view's Sim3 in double: (srcw 3 x 3, t)"""
    a = [float(v) for v in res["sr12"]]
    r = [float(v) for v in np.asarray(rcw2, np.float64).reshape(9)]
    tc = [float(v) for v in np.asarray(tcw2, np.float64).reshape(3)]
    m = [[(a[3 * i] * r[j] + a[3 * i + 1] * r[3 + j]) + a[3 * i + 2] * r[6 + j] for j in range(3)] for i in range(3)]
    t = [((a[3 * i] * tc[0] + a[3 * i + 1] * tc[1]) + a[3 * i + 2] * tc[2]) + float(res["t12"][i]) for i in range(3)]
    return np.array(m), np.array(t)
