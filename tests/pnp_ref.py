"""The PnP RANSAC of include/sendslam_orb.h (MLPnPsolver as Tracking::Relocalization runs it on the matches of SearchByBoW), restated
in numpy: the NORMATIVE statement of the rule (test infrastructure, plain module).  Upstream's source is not in the reference tree;
parity with the real binary stays unpinned and every deviation is listed in the header.

    correspondences()   step 1: the kept (keypoint row, point row) couples in ascending keypoint row and their six float32 numbers
    draw()              step 3a: the six draws of a hypothesis on the Sim3 rule's mix32 (sparse swap-with-last)
    normal_matrix()     step 3b: the 12 x 12 matrix H of a sextuple
    linear()            step 3b: shift, Cholesky, six inverse iterations, sign, scale, Horn's rotation, tcw
    refine()            step 3c: plain steps of the pose rule on the six (tests/pose_ref.py's own functions)
    model()             steps 3b - 3d of a sextuple -> (rcw, tcw in double, or the zero model)
    errors(), count()   step 3e: depth and reprojection error of every correspondence, vectorised in float32
    solve()             steps 1 - 4 of one problem -> (RESULT_DTYPE record, uint8 flag per keypoint row, count[t] or None)

Every float32 step is one numpy float32 operation and every double step one Python float (or numpy float64) operation, left to right
as the header writes them.  The Jacobi rotation is the triangulation's (epi_ref._rotate), the draw stream the Sim3 rule's
(sim3_ref.mix32), the step the pose rule's (pose_ref.terms / solve / exp / update): none is a copy.
"""
from __future__ import annotations

import math

import numpy as np

import epi_ref as E
import pose_ref as PR
import sim3_ref as S

f32 = np.float32
f64 = np.float64
MAX_ITERATIONS = 1024
MAX_REFINE = 16
DRAWS = 6
INVERSE_STEPS = 6
SHIFT = 1e-13
RESULT_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,))] +
                        [(n, "<i4") for n in ("state", "status", "n_corr", "n_inliers", "best_inliers", "iteration")] + [("reserved", "<i4", (2,))])
UPSTREAM = dict(chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=300, refine_steps=5)


def _sqrt(x: float) -> float:
    """IEEE double square root (math.sqrt raises where IEEE gives a NaN)"""
    with np.errstate(all="ignore"):
        return float(np.sqrt(f64(x)))


# ---- step 3a ------------------------------------------------------------------------------------------------------------------------
def draw(seed: int, problem: int, t: int, n: int, k_draws: int = DRAWS):
    """k draws without replacement over 0 .. n-1: at most k slots are ever displaced, so no array is kept"""
    moved = {}
    out = []
    for k in range(k_draws):
        j = (S.mix32(seed, problem, k_draws * t + k) * (n - k)) >> 32
        out.append(moved.get(j, j))
        moved[j] = moved.get(n - 1 - k, n - 1 - k)
    return out


def draw_literal(seed: int, problem: int, t: int, n: int, k_draws: int = DRAWS):
    """the same on an array of n entries: take entry j, move the last entry into its place, drop the last"""
    avail = list(range(n))
    out = []
    for k in range(k_draws):
        j = (S.mix32(seed, problem, k_draws * t + k) * len(avail)) >> 32
        out.append(avail[j])
        avail[j] = avail[-1]
        avail.pop()
    return out


# ---- step 3b ------------------------------------------------------------------------------------------------------------------------
def camera(view):
    return {k: float(f32(view[k])) for k in ("fx", "fy", "cx", "cy")}


def bearing(u, v, cam):
    xn = E._div(float(f32(u)) - cam["cx"], cam["fx"])
    yn = E._div(float(f32(v)) - cam["cy"], cam["fy"])
    n = _sqrt((xn * xn + yn * yn) + 1.0)
    return [E._div(xn, n), E._div(yn, n), E._div(1.0, n)]


def centre(X):
    return [E._div(((((X[0][c] + X[1][c]) + X[2][c]) + X[3][c]) + X[4][c]) + X[5][c], 6.0) for c in range(3)]


def _widen(xyz, uv):
    X = [[float(f32(v)) for v in row] for row in np.asarray(xyz).reshape(DRAWS, 3)]
    UV = [[f32(v) for v in row] for row in np.asarray(uv).reshape(DRAWS, 2)]
    return X, UV


def normal_matrix(xyz, uv, cam):
    """-> (H as 12 lists of 12 Python floats, symmetric, before the shift; O; d; b)"""
    X, UV = _widen(xyz, uv)
    O = centre(X)
    d = [[X[i][c] - O[c] for c in range(3)] + [1.0] for i in range(DRAWS)]
    b = [bearing(UV[i][0], UV[i][1], cam) for i in range(DRAWS)]
    H = [[0.0] * 12 for _ in range(12)]
    for a in range(4):
        for e in range(a + 1):
            for r in range(3):
                for c in range(3):
                    acc = None
                    for i in range(DRAWS):
                        term = (d[i][a] * d[i][e]) * ((1.0 if r == c else 0.0) - b[i][r] * b[i][c])
                        acc = term if acc is None else acc + term
                    H[3 * a + r][3 * e + c] = H[3 * e + c][3 * a + r] = acc
    return H, O, d, b


def horn(m):
    """Horn's rotation of M exactly as sim3_ref.model has it: N, the sweeps, the largest diagonal entry, the nine polynomial entries"""
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
    for _ in range(E.SWEEPS):
        for p, q in E.PAIRS_ORDER:
            E._rotate(N, V, p, q)
    best = 0
    for k in range(1, 4):
        if N[k][k] > N[best][best]:
            best = k
    qv = [V[k][best] for k in range(4)]
    qn = _sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3])
    w, x, y, z = (E._div(v, qn) for v in qv)
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def linear(xyz, uv, cam, trace_out=None):
    """-> (R as nine Python floats, t as three, the Cholesky met only pivots > 0).  trace_out: a dict that receives H (shifted), the
    unknowns after the sign, s and O"""
    H, O, d, b = normal_matrix(xyz, uv, cam)
    trace = H[0][0]
    for k in range(1, 12):
        trace = trace + H[k][k]
    shift = SHIFT * trace
    for k in range(12):
        H[k][k] = H[k][k] + shift
    Hs = [row[:] for row in H]
    ok = True
    L = H
    for j in range(12):
        s = L[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        ok = ok and s > 0.0
        L[j][j] = _sqrt(s)
        for i in range(j + 1, 12):
            v = L[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = E._div(v, L[j][j])
    x = [E._div(1.0, _sqrt(12.0))] * 12
    for _ in range(INVERSE_STEPS):
        x = x[:]
        for i in range(12):
            v = x[i]
            for k in range(i):
                v = v - L[i][k] * x[k]
            x[i] = E._div(v, L[i][i])
        for i in range(11, -1, -1):
            v = x[i]
            for k in range(i + 1, 12):
                v = v - L[k][i] * x[k]
            x[i] = E._div(v, L[i][i])
        s = x[0] * x[0]
        for k in range(1, 12):
            s = s + x[k] * x[k]
        n = _sqrt(s)
        x = [E._div(v, n) for v in x]
    front = None
    for i in range(DRAWS):
        y = [((x[r] * d[i][0] + x[3 + r] * d[i][1]) + x[6 + r] * d[i][2]) + x[9 + r] for r in range(3)]
        f = (b[i][0] * y[0] + b[i][1] * y[1]) + b[i][2] * y[2]
        front = f if front is None else front + f
    if front < 0.0:
        x = [-v for v in x]
    nrm = [_sqrt((x[3 * a] * x[3 * a] + x[3 * a + 1] * x[3 * a + 1]) + x[3 * a + 2] * x[3 * a + 2]) for a in range(3)]
    s = E._div(3.0, (nrm[0] + nrm[1]) + nrm[2])
    R = horn([[x[3 * i + j] for j in range(3)] for i in range(3)])
    t = [s * x[9 + r] - ((R[3 * r] * O[0] + R[3 * r + 1] * O[1]) + R[3 * r + 2] * O[2]) for r in range(3)]
    if trace_out is not None:
        trace_out.update(H=Hs, x=x, s=s, O=O)
    return R, t, ok


# ---- step 3c ------------------------------------------------------------------------------------------------------------------------
def refine(xyz, uv, scale6, cam, R, t, lam, steps):
    """-> (R, t) as lists of float64 after up to `steps` plain steps of the pose rule; a refused or non-finite step ends it"""
    X = np.asarray(xyz, f32).reshape(DRAWS, 3).astype(f64)
    UV = np.asarray(uv, f32).reshape(DRAWS, 2).astype(f64)
    s = np.asarray(scale6, f32).reshape(DRAWS).astype(f64)
    with np.errstate(all="ignore"):
        o = {"X": X[:, 0], "Y": X[:, 1], "Z": X[:, 2], "u": UV[:, 0], "v": UV[:, 1], "w": 1.0 / (s * s), "ur": np.zeros(DRAWS, f64),
             "stereo": np.zeros(DRAWS, bool)}
    c = {k: f64(cam[k]) for k in ("fx", "fy", "cx", "cy")}
    c.update(bf=f64(0.0), chi2_mono=f64(0.0), chi2_stereo=f64(0.0), delta_mono=f64(0.0), delta_stereo=f64(0.0))
    R, t = [f64(v) for v in R], [f64(v) for v in t]
    for _ in range(steps):
        front, T = PR.terms(o, c, R, t, False)
        total = []
        with np.errstate(all="ignore"):
            for k in range(PR.SUMS):
                acc = f64(0.0)
                for i in range(DRAWS):
                    if front[i]:
                        acc = acc + T[k][i]
                total.append(acc)
        d = PR.solve(total, lam)
        if d is None:
            break
        e = PR.exp(d)
        if e is None:
            break
        Rn, tn = PR.update(e[0], e[1], R, t)
        if not all(np.isfinite(v) for v in list(Rn) + list(tn)):
            break
        R, t = Rn, tn
    return R, t


# ---- step 3d ------------------------------------------------------------------------------------------------------------------------
def model(xyz, uv, scale6, point_rows6, view, lam=1e-6, refine_steps=5):
    """steps 3b - 3d of a sextuple in draw order -> (rcw float64 [9], tcw float64 [3]); the zero model is all 0"""
    cam = camera(view)
    with np.errstate(all="ignore"):
        R, t, ok = linear(xyz, uv, cam)
        rows = [int(v) for v in np.asarray(point_rows6).reshape(DRAWS)]
        ok = ok and len(set(rows)) == DRAWS and all(math.isfinite(v) for v in R + t)
        if ok:
            R, t = refine(xyz, uv, scale6, cam, R, t, lam, refine_steps)
        rcw, tcw = np.array(R, f64), np.array(t, f64)
        ok = ok and bool(np.isfinite(rcw.astype(f32)).all() and np.isfinite(tcw.astype(f32)).all())
    if not ok:
        return np.zeros(9, f64), np.zeros(3, f64)
    return rcw, tcw


# ---- steps 1 and 3e -----------------------------------------------------------------------------------------------------------------
def correspondences(points, kp, skip, idx, scale, chi2):
    """-> dict rows (keypoint rows, ascending), cols (point rows), X [N, 3], u v max s [N], all float32"""
    sc = np.asarray(scale, f32)
    n_p, n_k, n_levels = len(points), len(kp), len(sc)
    idx = np.asarray(idx, np.int64)[:n_k]
    rows = np.arange(n_k)
    ok = (idx >= 0) & (idx < n_p)
    j = np.where(ok, idx, 0)
    octave = np.asarray(kp["octave"], np.int64)[:n_k]
    ok &= (octave >= 0) & (octave < n_levels)
    if skip is not None and n_p:
        ok &= np.asarray(skip)[j] == 0
    rows, cols = rows[ok], j[ok]
    X = np.stack([points[n][cols] for n in "xyz"], axis=1).astype(f32) if len(cols) else np.zeros((0, 3), f32)
    s = sc[octave[rows]] if len(rows) else np.zeros(0, f32)
    with np.errstate(all="ignore"):
        return dict(rows=rows, cols=cols, X=X, u=kp["x"][rows].astype(f32), v=kp["y"][rows].astype(f32), max=f32(chi2) * (s * s), s=s)


def errors(c, rcw, tcw, view):
    """(depth > 0, squared error) of every correspondence of c under the pose rounded to float32"""
    r, t = np.asarray(rcw, f64).astype(f32), np.asarray(tcw, f64).astype(f32)
    with np.errstate(all="ignore"):
        Y = S._transform(r, t, c["X"])
        qu, qv = S._project(Y, view)
        du, dv = c["u"] - qu, c["v"] - qv
        return Y[:, 2] > f32(0.0), du * du + dv * dv


def inliers(c, rcw, tcw, view) -> np.ndarray:
    front, e = errors(c, rcw, tcw, view)
    with np.errstate(all="ignore"):
        return front & (e < c["max"])


def hypothesis(c, t: int, seed: int, problem: int, view, lam, refine_steps):
    pick = draw(seed, problem, t, len(c["rows"]))
    uv = np.stack([c["u"][pick], c["v"][pick]], axis=1)
    return model(c["X"][pick], uv, c["s"][pick], c["cols"][pick], view, lam, refine_steps)


def too_few(n: int, min_inliers: int) -> bool:
    return n < DRAWS or n < min_inliers


def select(counts, n: int, min_inliers: int, min_ratio: float) -> int:
    """step 4: the t of the largest count (the smallest among equals) if that count qualifies, or -1"""
    counts = np.asarray(counts)
    t = int(np.argmax(counts))  # the first of the largest
    cnt = int(counts[t])
    with np.errstate(all="ignore"):
        ok = cnt >= min_inliers and f32(cnt) >= f32(min_ratio) * f32(n)
    return t if ok else -1


def solve(view, points, kp, skip, idx, scale, chi2=5.991, min_ratio=0.5, lambda_=1e-6, min_inliers=10, max_iterations=300, refine_steps=5,
          seed=0, problem=0, status=0):
    """-> (RESULT_DTYPE record, uint8 [n_kp], int count[max_iterations] or None in state 1)"""
    res = np.zeros((), RESULT_DTYPE)
    flags = np.zeros(len(kp), np.uint8)
    res["iteration"], res["status"] = -1, status
    if status != 0:
        res["state"] = 1
        return res, flags, None
    c = correspondences(points, kp, skip, idx, scale, chi2)
    n = len(c["rows"])
    res["n_corr"] = n
    if too_few(n, min_inliers):
        res["state"] = 1
        return res, flags, None
    models = [hypothesis(c, t, seed, problem, view, lambda_, refine_steps) for t in range(max_iterations)]
    counts = np.array([int(inliers(c, m[0], m[1], view).sum()) for m in models], np.int64)
    res["best_inliers"] = counts.max()
    t = select(counts, n, min_inliers, min_ratio)
    if t < 0:
        res["state"] = 2
        return res, flags, counts
    res["rcw"], res["tcw"] = models[t]
    res["n_inliers"], res["iteration"] = counts[t], t
    flags[c["rows"][inliers(c, models[t][0], models[t][1], view)]] = 1
    return res, flags, counts
