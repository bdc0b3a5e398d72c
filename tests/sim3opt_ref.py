"""The Sim3 refinement of include/sendslam_orb.h (the rest of ORBmatcher::SearchBySim3 and Optimizer::OptimizeSim3 as loop closing
runs them after the RANSAC), restated in numpy and plain Python: the NORMATIVE statement of the rule (test infrastructure, plain module).
Every deviation from upstream is listed in the header.

    correspondences()  step 1: the RANSAC's keep rule and float32 camera coordinates (sim3_ref), the keypoints and the weights, widened
    start()            step 2: scale, Gram-Schmidt rotation (pose_ref) and translation of a start model
    edge12(), edge21() step 3: residuals and the two Jacobian rows of every correspondence, vectorised over correspondences
    terms()            step 3: the 35 terms of one edge
    sums()             step 3: the 35 sums in the pose rule's tree, e12 before e21 in every slot
    solve()            step 3: the damped n x n Cholesky solve, n = 6 or 7, scalar
    retract()          step 3: R <- dR.R, s <- ds.s, t <- ds.(dR.t) + upsilon
    chi2()             step 4: both chi-squares of every correspondence
    floats()           step 5: the 25 floats of the embedded model
    optimise()         steps 1 - 5 of one pair -> (RESULT_DTYPE record, uint8 flag per query row)
    marks(), mutual()  the bookkeeping of SearchBySim3, plain loops
    to_s21w()          ss_sim3_to_view21's Sim3 in double

Every step is one numpy float64 operation (elementwise operations and sqrt are IEEE and correctly rounded; nothing is summed by numpy),
left to right as the header writes them.
"""
from __future__ import annotations

import numpy as np

import pose_ref as PR
import sim3_ref as S

f64 = np.float64
f32 = np.float32
SUMS = 35
SERIES = 20
BEHIND = 1e30
RESULT_DTYPE = np.dtype([("r12", "<f8", (9,)), ("t12", "<f8", (3,)), ("s12", "<f8"), ("cost", "<f8")] +
                        [(n, "<i4") for n in ("state", "status", "n_corr", "n_removed", "n_inliers")] +
                        [("steps", "<i4", (2,)), ("reserved", "<i4"), ("model", S.RESULT_DTYPE)])
MUTUAL_DTYPE = np.dtype([("n_prior", "<i4"), ("n_new", "<i4")])
UPSTREAM = dict(chi2=10.0, lambda_=1e-6, step_eps=1e-10, iterations0=5, iterations_more=10, iterations_same=5, min_corr=10, min_inliers=10,
                fix_scale=False)
H_PAIRS = [(a, b) for a in range(7) for b in range(a, 7)]


# ---- step 1 -------------------------------------------------------------------------------------------------------------------------
def correspondences(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale):
    """-> dict rows (query rows, ascending), float64 x1, x2 [N, 3], u1 v1 u2 v2 w1 w2 [N]"""
    c = S.correspondences(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale, 1.0)
    rows, cols = c["rows"], c["cols"]
    sc = np.asarray(scale, f32)
    s1 = sc[q_kp["octave"][rows]].astype(f64)
    s2 = sc[t_kp["octave"][cols]].astype(f64) if len(cols) else np.zeros(0, f64)
    kp = lambda a, r: np.asarray(a, f32)[r].astype(f64)  # noqa: E731
    with np.errstate(all="ignore"):
        return dict(rows=rows, x1=c["x1"].astype(f64), x2=c["x2"].astype(f64), u1=kp(q_kp["x"], rows), v1=kp(q_kp["y"], rows),
                    u2=kp(t_kp["x"], cols) if len(cols) else np.zeros(0, f64), v2=kp(t_kp["y"], cols) if len(cols) else np.zeros(0, f64),
                    w1=1.0 / (s1 * s1), w2=1.0 / (s2 * s2))


def cameras(view1, view2, chi2):
    k = {n + "1": f64(f32(view1[n])) for n in ("fx", "fy", "cx", "cy")}
    k.update({n + "2": f64(f32(view2[n])) for n in ("fx", "fy", "cx", "cy")})
    k["chi2"] = f64(chi2)
    k["delta"] = np.sqrt(k["chi2"])
    return k


# ---- step 2 -------------------------------------------------------------------------------------------------------------------------
def start(model, fix_scale):
    """a sim3 RESULT_DTYPE record -> (R as nine float64, t as three, s, usable?)"""
    a = [f64(f32(v)) for v in model["sr12"]]
    st = a + [f64(f32(v)) for v in model["t12"]]
    with np.errstate(all="ignore"):
        n0 = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    R, t, ok = PR.start_pose(st)
    s = f64(1.0) if fix_scale else n0
    ok = bool(ok and s > 0.0 and np.isfinite(s))
    if not ok:
        return [f64(1.0 if k % 4 == 0 else 0.0) for k in range(9)], [f64(0.0)] * 3, f64(1.0), False
    return R, t, s, True


# ---- step 3 -------------------------------------------------------------------------------------------------------------------------
def map12(c, R, t, s):
    X = c["x2"]
    return tuple(s * ((R[3 * i] * X[:, 0] + R[3 * i + 1] * X[:, 1]) + R[3 * i + 2] * X[:, 2]) + t[i] for i in range(3))


def map21(c, R, t, s):
    """-> (M as nine scalars, Z as three arrays)"""
    inv = 1.0 / s
    M = [inv * R[3 * j + i] for i in range(3) for j in range(3)]
    d = [c["x1"][:, i] - t[i] for i in range(3)]
    return M, tuple((M[3 * i] * d[0] + M[3 * i + 1] * d[1]) + M[3 * i + 2] * d[2] for i in range(3))


def edge12(c, k, R, t, s):
    """-> (takes part?, rx, ry, J0, J1, w); a structural zero is the factor +0.0"""
    x, y, z = map12(c, R, t, s)
    iz = 1.0 / z
    iz2 = iz * iz
    fx, fy = k["fx1"], k["fy1"]
    zero = np.zeros_like(z)
    rx, ry = c["u1"] - (fx * x * iz + k["cx1"]), c["v1"] - (fy * y * iz + k["cy1"])
    J0 = [x * y * iz2 * fx, -(1.0 + x * x * iz2) * fx, y * iz * fx, -iz * fx, zero, x * iz2 * fx, zero]
    J1 = [(1.0 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, zero, -iz * fy, y * iz2 * fy, zero]
    return z > 0.0, rx, ry, J0, J1, c["w1"]


def edge21(c, k, R, t, s):
    M, (x, y, z) = map21(c, R, t, s)
    iz = 1.0 / z
    iz2 = iz * iz
    fx, fy = k["fx2"], k["fy2"]
    rx, ry = c["u2"] - (fx * x * iz + k["cx2"]), c["v2"] - (fy * y * iz + k["cy2"])
    px, pxz, py, pyz = fx * iz, fx * x * iz2, fy * iz, fy * y * iz2
    a, b, g = c["x1"][:, 0], c["x1"][:, 1], c["x1"][:, 2]
    D = []
    for i in range(3):
        m0, m1, m2 = M[3 * i], M[3 * i + 1], M[3 * i + 2]
        D.append([m1 * g - m2 * b, m2 * a - m0 * g, m0 * b - m1 * a, -m0, -m1, -m2, -((m0 * a + m1 * b) + m2 * g)])
    J0 = [pxz * D[2][q] - px * D[0][q] for q in range(7)]
    J1 = [pyz * D[2][q] - py * D[1][q] for q in range(7)]
    return z > 0.0, rx, ry, J0, J1, c["w2"]


def terms(edge, k, robust):
    """one edge of every correspondence -> float64 [35][n]"""
    _, rx, ry, J0, J1, w = edge
    e2 = w * (rx * rx + ry * ry)
    d = k["delta"]
    wq = np.where((e2 > d * d) & bool(robust), w * d / np.sqrt(e2), w)
    out = np.empty((SUMS, len(rx)), f64)
    w0, w1 = [wq * v for v in J0], [wq * v for v in J1]
    for n, (a, b) in enumerate(H_PAIRS):
        out[n] = w0[a] * J0[b] + w1[a] * J1[b]
    for a in range(7):
        out[28 + a] = w0[a] * rx + w1[a] * ry
    return out


def interleave(v12, v21, m12, m21):
    """values [..., n] and masks [n] of both edges -> one array whose rounds of 256 alternate: e12 of correspondences 256 j .., then e21
    of the same, so that pose_ref.tree adds, in every slot, correspondence by correspondence the e12 term and then the e21 term"""
    n = v12.shape[-1]
    rounds = max(1, -(-n // PR.SLOTS))
    lead = v12.shape[:-1]
    V = np.zeros(lead + (rounds, 2, PR.SLOTS), f64)
    Mk = np.zeros((rounds, 2, PR.SLOTS), bool)
    pad = rounds * PR.SLOTS
    for e, (v, m) in enumerate(((v12, m12), (v21, m21))):
        vv, mm = np.zeros(lead + (pad,), f64), np.zeros(pad, bool)
        vv[..., :n], mm[:n] = v, m
        V[..., :, e, :] = vv.reshape(lead + (rounds, PR.SLOTS))
        Mk[:, e, :] = mm.reshape(rounds, PR.SLOTS)
    return V.reshape(lead + (-1,)), Mk.reshape(-1)


def sums(c, k, R, t, s, robust, active):
    with np.errstate(all="ignore"):
        e12, e21 = edge12(c, k, R, t, s), edge21(c, k, R, t, s)
        V, M = interleave(terms(e12, k, robust), terms(e21, k, robust), active & e12[0], active & e21[0])
    return PR.tree(V, M)


def solve(total, lam, n):
    """the 35 sums -> (delta as n float64, or None when a pivot is not > 0): pose_ref.solve over n unknowns"""
    H = [[f64(0.0)] * n for _ in range(n)]
    for q, (a, b) in enumerate(H_PAIRS):
        if b < n:
            H[a][b] = H[b][a] = f64(total[q])
    lam = f64(lam)
    d = [-f64(total[28 + a]) for a in range(n)]
    with np.errstate(all="ignore"):
        for a in range(n):
            H[a][a] = H[a][a] + lam * (1.0 + H[a][a])
        for j in range(n):
            v = H[j][j]
            for q in range(j):
                v = v - H[j][q] * H[j][q]
            if not v > 0.0:
                return None
            H[j][j] = np.sqrt(v)
            for i in range(j + 1, n):
                v = H[i][j]
                for q in range(j):
                    v = v - H[i][q] * H[j][q]
                H[i][j] = v / H[j][j]
        for i in range(n):
            v = d[i]
            for q in range(i):
                v = v - H[i][q] * d[q]
            d[i] = v / H[i][i]
        for i in range(n - 1, -1, -1):
            v = d[i]
            for q in range(i + 1, n):
                v = v - H[q][i] * d[q]
            d[i] = v / H[i][i]
    return d


def exp_scale(sigma):
    v = f64(PR.INV_FACT[SERIES - 1])
    sigma = f64(sigma)
    with np.errstate(all="ignore"):
        for q in range(SERIES - 2, -1, -1):
            v = v * sigma + PR.INV_FACT[q]
    return v


def retract(d, R, t, s, fix_scale):
    """-> (R, t, s) or None when the step is too large"""
    e = PR.exp(list(d[:6]))
    if e is None:
        return None
    if not fix_scale and not abs(d[6]) <= 1.0:
        return None
    dR = e[0]
    ds = f64(1.0) if fix_scale else exp_scale(d[6])
    with np.errstate(all="ignore"):
        Rn = [(dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
        tn = [ds * ((dR[3 * i] * t[0] + dR[3 * i + 1] * t[1]) + dR[3 * i + 2] * t[2]) + d[3 + i] for i in range(3)]
        sn = s if fix_scale else ds * s
    return Rn, tn, sn


# ---- step 4 -------------------------------------------------------------------------------------------------------------------------
def chi2(c, k, R, t, s):
    """-> (chi2_12, chi2_21)"""
    with np.errstate(all="ignore"):
        x, y, z = map12(c, R, t, s)
        ex, ey = c["u1"] - (k["fx1"] * x / z + k["cx1"]), c["v1"] - (k["fy1"] * y / z + k["cy1"])
        c12 = np.where(z > 0.0, c["w1"] * (ex * ex + ey * ey), BEHIND)
        _, (x, y, z) = map21(c, R, t, s)
        ex, ey = c["u2"] - (k["fx2"] * x / z + k["cx2"]), c["v2"] - (k["fy2"] * y / z + k["cy2"])
        c21 = np.where(z > 0.0, c["w2"] * (ex * ex + ey * ey), BEHIND)
    return c12, c21


# ---- step 5 -------------------------------------------------------------------------------------------------------------------------
def floats(R, t, s):
    """-> (dict of the 25 floats, all finite?)"""
    with np.errstate(all="ignore"):
        s21 = 1.0 / s
        m = {"sr12": np.array([f32(s * R[k]) for k in range(9)], f32),
             "sr21": np.array([f32(s21 * R[3 * j + i]) for i in range(3) for j in range(3)], f32),
             "t12": np.array([f32(v) for v in t], f32),
             "t21": np.array([f32(-(s21 * ((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]))) for i in range(3)], f32),
             "s12": f32(s)}
    ok = all(np.isfinite(v) for v in list(R) + list(t) + [s]) and all(np.all(np.isfinite(v)) for v in m.values())
    return m, bool(ok)


# ---- the pair -----------------------------------------------------------------------------------------------------------------------
def optimise(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale, start_model, params=None, status=0, trace=None):
    """-> (RESULT_DTYPE record, uint8 flag per query row).  params: fields of UPSTREAM.  status != 0: a frame voided the pair.  trace: a
    list that receives the inlier mask after every classification"""
    p = dict(UPSTREAM, **(params or {}))
    fix = bool(p["fix_scale"])
    start_model = np.asarray(start_model, S.RESULT_DTYPE).reshape(())
    status = status if status else int(start_model["status"])
    usable = status == 0 and int(start_model["state"]) == 0
    if usable:
        c = correspondences(view1, q_xyz, q_kp, q_skip, view2, t_xyz, t_kp, t_skip, idx, scale)
    else:
        c = correspondences(view1, q_xyz[:0], q_kp[:0], None, view2, t_xyz, t_kp, None, np.zeros(0, np.int64), scale)
    n = len(c["rows"])
    k = cameras(view1, view2, p["chi2"])
    R, t, s, ok = start(start_model, fix)
    R0, t0, s0 = list(R), list(t), s
    active = np.ones(n, bool)
    state = 1 if not usable else 2 if not ok else 1 if n < p["min_corr"] else 0
    n_in, n_removed, cost, steps = n, 0, f64(0.0), [0, 0]
    nu = 6 if fix else 7
    for rnd in range(2):
        if state:
            break
        iterations = p["iterations0"] if rnd == 0 else p["iterations_more"] if n_removed > 0 else p["iterations_same"]
        for _ in range(iterations):
            d = solve(sums(c, k, R, t, s, rnd == 0, active), p["lambda_"], nu)
            if d is None:
                state = 2
                break
            d7 = list(d) + [f64(0.0)] * (7 - nu)
            new = retract(d7, R, t, s, fix)
            if new is None:
                state = 4
                break
            R, t, s = new
            steps[rnd] += 1
            if all(abs(v) < p["step_eps"] for v in d):
                break
        if state:
            break
        c12, c21 = chi2(c, k, R, t, s)
        with np.errstate(invalid="ignore"):
            active = active & (c12 <= k["chi2"]) & (c21 <= k["chi2"])
        if trace is not None:
            trace.append(active.copy())
        n_in = int(active.sum())
        with np.errstate(all="ignore"):
            cost = PR.tree(c12 + c21, active)
        if rnd == 0:
            n_removed = n - n_in
            if n_in < p["min_inliers"]:
                state = 3
    m, finite = floats(R, t, s)
    if not finite:
        state, R, t, s = 2, R0, t0, s0
    flags = np.full(len(q_xyz), 2, np.uint8)
    flags[c["rows"]] = np.where(active, 0, 1)
    res = np.zeros((), RESULT_DTYPE)
    res["r12"], res["t12"], res["s12"], res["cost"] = np.array(R, f64), np.array(t, f64), s, cost
    res["state"], res["status"], res["n_corr"], res["n_removed"], res["n_inliers"] = state, status, n, n_removed, n_in
    res["steps"] = steps
    if state == 0:
        for name, v in m.items():
            res["model"][name] = v
    res["model"]["state"], res["model"]["n_corr"], res["model"]["n_inliers"] = state, n, n_in if state == 0 else 0
    res["model"]["iteration"], res["model"]["status"] = -1, status
    return res, flags


# ---- the bookkeeping of SearchBySim3 ---------------------------------------------------------------------------------------------------
def _valid(i, j, nq, nt):
    return i < nq and 0 <= j < nt


def marks(idx, q_skip, t_skip, nq, nt):
    """one pair of len(idx) rows -> (skip1, skip2), uint8 each"""
    rows = len(idx)
    nq, nt = min(max(int(nq), 0), rows), min(max(int(nt), 0), rows)
    s1, s2 = np.zeros(rows, np.uint8), np.zeros(rows, np.uint8)
    for i in range(rows):
        s1[i] = 1 if (q_skip is not None and q_skip[i] != 0) or _valid(i, int(idx[i]), nq, nt) else 0
        s2[i] = 1 if t_skip is not None and t_skip[i] != 0 else 0
    for i in range(rows):
        if _valid(i, int(idx[i]), nq, nt):
            s2[int(idx[i])] = 1
    return s1, s2


def mutual(idx, idx12, idx21, nq, nt):
    """one pair -> (idx_out int32, MUTUAL_DTYPE record)"""
    rows = len(idx)
    nq, nt = min(max(int(nq), 0), rows), min(max(int(nt), 0), rows)
    taken = {int(idx[i]) for i in range(rows) if _valid(i, int(idx[i]), nq, nt)}
    out = np.full(rows, -1, np.int32)
    res = np.zeros((), MUTUAL_DTYPE)
    for i in range(rows):
        if _valid(i, int(idx[i]), nq, nt):
            out[i] = idx[i]
            res["n_prior"] += 1
        elif i < nq:
            j = int(idx12[i])
            if 0 <= j < nt and int(idx21[j]) == i and j not in taken:
                out[i] = j
                res["n_new"] += 1
    return out, res


def to_s21w(res, rcw1, tcw1):
    """ss_sim3_to_view21's Sim3 in double: (srcw 3 x 3, t)"""
    a = [float(v) for v in res["sr21"]]
    r = [float(v) for v in np.asarray(rcw1, np.float64).reshape(9)]
    tc = [float(v) for v in np.asarray(tcw1, np.float64).reshape(3)]
    m = [[(a[3 * i] * r[j] + a[3 * i + 1] * r[3 + j]) + a[3 * i + 2] * r[6 + j] for j in range(3)] for i in range(3)]
    t = [((a[3 * i] * tc[0] + a[3 * i + 1] * tc[1]) + a[3 * i + 2] * tc[2]) + float(res["t21"][i]) for i in range(3)]
    return np.array(m), np.array(t)
