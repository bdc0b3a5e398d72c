"""The pose-only optimisation of include/sendslam_orb.h (Optimizer::PoseOptimization as the tracking threads run it on the matches
of a search), restated in numpy: the NORMATIVE statement of the rule (test infrastructure, plain module).  It is the rule of ss_track's
host step with the stereo row added and the order of every sum fixed; every deviation from upstream is listed in the header.

    observations()   step 1: the slots that are observations, in slot order, and their numbers widened to double
    start_pose()     step 2: the Gram-Schmidt rotation next to the start rotation
    terms()          step 3: the 26 terms of every observation, vectorised over observations
    tree()           step 3: one sum -- 256 slot sums in ascending order, four groups of 64 folded by halving, (r0 + r1) + (r2 + r3)
    solve()          step 3: the damped 6 x 6 Cholesky solve, scalar
    exp()            step 3: the exponential by three Horner sums over INV_FACT
    update()         step 3: R <- dR.R, t <- dR.t + dt
    chi2()           step 4: the chi-square of every observation
    optimise()       steps 1 - 5 of one frame -> (RESULT_DTYPE record, uint8 flag per slot)

Every step is one numpy float64 operation (elementwise operations and sqrt are IEEE and correctly rounded; nothing is summed by numpy),
left to right as the header writes them.  The terms are built from the structure of the three Jacobian rows, not copied from the list
the C text spells out.
"""
from __future__ import annotations

import numpy as np

f64 = np.float64
SLOTS = 256
SUMS = 26
SERIES = 15
PI2 = float.fromhex("0x1.3bd3cc9be45dep+3")
BEHIND = 1e30
# INV_FACT[n]: the double next to 1 / n!, n = 0 .. 2 * SERIES + 1 (csrc/ss_pose_steps.h holds the same table)
INV_FACT = [float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "0x1.0000000000000p+0", "0x1.0000000000000p-1", "0x1.5555555555555p-3", "0x1.5555555555555p-5",
    "0x1.1111111111111p-7", "0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-13", "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19",
    "0x1.27e4fb7789f5cp-22", "0x1.ae64567f544e4p-26", "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33", "0x1.93974a8c07c9dp-37",
    "0x1.ae7f3e733b81fp-41", "0x1.ae7f3e733b81fp-45", "0x1.952c77030ad4ap-49", "0x1.6827863b97d97p-53", "0x1.2f49b46814157p-57",
    "0x1.e542ba4020225p-62", "0x1.71b8ef6dcf572p-66", "0x1.0ce396db7f853p-70", "0x1.761b41316381ap-75", "0x1.f2cf01972f578p-80",
    "0x1.3f3ccdd165fa9p-84", "0x1.88e85fc6a4e5ap-89", "0x1.d1ab1c2dccea3p-94", "0x1.0a18a2635085dp-98", "0x1.259f98b4358adp-103",
    "0x1.3932c5047d60ep-108", "0x1.434d2e783f5bcp-113")]
RESULT_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,)), ("cost", "<f8")] +
                        [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers")] + [("steps", "<i4", (8,)), ("reserved", "<i4")])
UPSTREAM = dict(chi2_mono=5.991, chi2_stereo=7.815, lambda_=1e-6, step_eps=1e-10, n_rounds=4, iterations=10, robust_rounds=2, min_obs=3,
                check_right=False, idx_by_row=False)
# the pairs (a, b) of the 20 sums of H, in order; H34 has no term
H_PAIRS = [(a, b) for a in range(6) for b in range(a, 6) if (a, b) != (3, 4)]


# ---- step 1 -------------------------------------------------------------------------------------------------------------------------
def observations(points, kp, idx, scale, skip=None, right=None, check_right=False, idx_by_row=False):
    """-> a dict of float64 arrays X Y Z u v ur w, bool stereo and int slot, one entry per observation in slot order, plus n_slots"""
    n_p, n_k = len(points), len(kp)
    idx = np.asarray(idx, np.int64)
    n_slots = n_k if idx_by_row else n_p
    assert len(idx) == n_slots
    slot = np.arange(n_slots, dtype=np.int64)
    prow, krow = (idx, slot) if idx_by_row else (slot, idx)
    keep = (prow >= 0) & (prow < n_p) & (krow >= 0) & (krow < n_k)
    prow, krow, slot = prow[keep], krow[keep], slot[keep]
    octave = np.asarray(kp["octave"], np.int64)[krow]
    ok = (octave >= 0) & (octave < len(scale))
    if skip is not None:
        ok &= np.asarray(skip)[prow] == 0
    prow, krow, slot, octave = prow[ok], krow[ok], slot[ok], octave[ok]
    wide = lambda a, rows: np.asarray(a, np.float32)[rows].astype(f64)  # noqa: E731
    s = np.asarray(scale, np.float32)[octave].astype(f64)
    o = {"X": wide(points["x"], prow), "Y": wide(points["y"], prow), "Z": wide(points["z"], prow), "u": wide(kp["x"], krow), "v": wide(kp["y"], krow),
         "w": 1.0 / (s * s), "slot": slot, "n_slots": n_slots}
    if check_right and right is not None:
        r = np.asarray(right, np.float32)[krow]
        with np.errstate(invalid="ignore"):
            o["stereo"] = r > np.float32(0)
        o["ur"] = np.where(o["stereo"], r.astype(f64), 0.0)
    else:
        o["stereo"] = np.zeros(len(slot), bool)
        o["ur"] = np.zeros(len(slot), f64)
    return o


def camera(view, chi2_mono, chi2_stereo):
    c = {k: f64(np.float32(view[k])) for k in ("fx", "fy", "cx", "cy", "bf")}
    c["chi2_mono"], c["chi2_stereo"] = f64(chi2_mono), f64(chi2_stereo)
    c["delta_mono"], c["delta_stereo"] = np.sqrt(c["chi2_mono"]), np.sqrt(c["chi2_stereo"])
    return c


# ---- step 2 -------------------------------------------------------------------------------------------------------------------------
def start_pose(start):
    """twelve doubles -> (R as nine float64, t as three, finite?); the identity and zero when an entry is not finite"""
    s = [f64(v) for v in np.asarray(start, f64).reshape(12)]
    with np.errstate(all="ignore"):
        n0 = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        a = [s[0] / n0, s[1] / n0, s[2] / n0]
        d = (s[3] * a[0] + s[4] * a[1]) + s[5] * a[2]
        b = [s[3] - d * a[0], s[4] - d * a[1], s[5] - d * a[2]]
        n1 = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        c = [b[0] / n1, b[1] / n1, b[2] / n1]
        R = a + c + [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]]
    t = s[9:12]
    if not all(np.isfinite(v) for v in R + t):
        return [f64(1.0 if k % 4 == 0 else 0.0) for k in range(9)], [f64(0.0)] * 3, False
    return R, t, True


# ---- step 3 -------------------------------------------------------------------------------------------------------------------------
def transform(o, R, t):
    x = ((R[0] * o["X"] + R[1] * o["Y"]) + R[2] * o["Z"]) + t[0]
    y = ((R[3] * o["X"] + R[4] * o["Y"]) + R[5] * o["Z"]) + t[1]
    z = ((R[6] * o["X"] + R[7] * o["Y"]) + R[8] * o["Z"]) + t[2]
    return x, y, z


def jacobians(o, c, R, t):
    """-> (contributes?, residuals [rx, ry, rr], rows [J0, J1, J2], each six entries or None for a structural zero)"""
    x, y, z = transform(o, R, t)
    front = z > 0.0
    iz = 1.0 / z
    iz2 = iz * iz
    fx, fy, bf = c["fx"], c["fy"], c["bf"]
    up = fx * x * iz + c["cx"]
    rx, ry = o["u"] - up, o["v"] - (fy * y * iz + c["cy"])
    rr = o["ur"] - (up - bf * iz)
    J0 = [x * y * iz2 * fx, -(1.0 + x * x * iz2) * fx, y * iz * fx, -iz * fx, None, x * iz2 * fx]
    J1 = [(1.0 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, None, -iz * fy, y * iz2 * fy]
    J2 = [J0[0] - bf * y * iz2, J0[1] + bf * x * iz2, J0[2], J0[3], None, J0[5] - bf * iz2]
    return front, [rx, ry, rr], [J0, J1, J2]


def terms(o, c, R, t, robust):
    """-> (bool [n]: the observation contributes, float64 [26][n]: its terms)"""
    n = len(o["X"])
    with np.errstate(all="ignore"):
        front, res, J = jacobians(o, c, R, t)
        st, w = o["stereo"], o["w"]
        sq = res[0] * res[0] + res[1] * res[1]
        e2 = np.where(st, w * (sq + res[2] * res[2]), w * sq)
        d = np.where(st, c["delta_stereo"], c["delta_mono"])
        wq = np.where((e2 > d * d) & bool(robust), w * d / np.sqrt(e2), w)
        wJ = [[None if v is None else wq * v for v in row] for row in J]

        def term(left, right):
            """left[r], right[r]: the factors of row r or None; (row0 + row1) + row2, absent rows left out, row 2 for stereo only"""
            mono = None
            for r in (0, 1):
                if left[r] is not None and right[r] is not None:
                    p = left[r] * right[r]
                    mono = p if mono is None else mono + p
            if left[2] is None or right[2] is None:
                return mono
            p = left[2] * right[2]
            return np.where(st, p if mono is None else mono + p, 0.0 if mono is None else mono)

        out = np.empty((SUMS, n), f64)
        for k, (a, b) in enumerate(H_PAIRS):
            out[k] = term([wJ[r][a] for r in range(3)], [J[r][b] for r in range(3)])
        for a in range(6):
            out[20 + a] = term([wJ[r][a] for r in range(3)], res)
    return front, out


def tree(values, mask):
    """the sum of values[..., k] over the k with mask[k]: slot s adds k = s, s + 256, ... in ascending order from +0.0, groups of 64
    slots fold by halving, the four results combine as (r0 + r1) + (r2 + r3)"""
    values = np.asarray(values, f64)
    lead, n = values.shape[:-1], values.shape[-1]
    rounds = max(1, -(-n // SLOTS))
    v = np.zeros(lead + (rounds * SLOTS,), f64)
    m = np.zeros(rounds * SLOTS, bool)
    v[..., :n], m[:n] = values, mask
    v = v.reshape(lead + (rounds, SLOTS))
    m = m.reshape(rounds, SLOTS)
    acc = np.zeros(lead + (SLOTS,), f64)
    with np.errstate(all="ignore"):
        for j in range(rounds):
            acc = np.where(m[j], acc + v[..., j, :], acc)
        a = acc.reshape(lead + (4, 64)).copy()
        for h in (32, 16, 8, 4, 2, 1):
            a[..., :h] = a[..., :h] + a[..., h:2 * h]
        return (a[..., 0, 0] + a[..., 1, 0]) + (a[..., 2, 0] + a[..., 3, 0])


def solve(total, lam):
    """the 26 sums -> (delta as six float64, or None when a pivot is not > 0)"""
    H = [[f64(0.0)] * 6 for _ in range(6)]
    for k, (a, b) in enumerate(H_PAIRS):
        H[a][b] = H[b][a] = f64(total[k])
    lam = f64(lam)
    d = [-f64(total[20 + a]) for a in range(6)]
    with np.errstate(all="ignore"):
        for a in range(6):
            H[a][a] = H[a][a] + lam * (1.0 + H[a][a])
        for j in range(6):
            s = H[j][j]
            for k in range(j):
                s = s - H[j][k] * H[j][k]
            if not s > 0.0:
                return None
            H[j][j] = np.sqrt(s)
            for i in range(j + 1, 6):
                v = H[i][j]
                for k in range(j):
                    v = v - H[i][k] * H[j][k]
                H[i][j] = v / H[j][j]
        for i in range(6):
            v = d[i]
            for k in range(i):
                v = v - H[i][k] * d[k]
            d[i] = v / H[i][i]
        for i in range(5, -1, -1):
            v = d[i]
            for k in range(i + 1, 6):
                v = v - H[k][i] * d[k]
            d[i] = v / H[i][i]
    return d


def series(q):
    """-> (A, B, C) at q = |omega|^2"""
    mq = -f64(q)
    A, B, C = f64(INV_FACT[2 * SERIES - 1]), f64(INV_FACT[2 * SERIES]), f64(INV_FACT[2 * SERIES + 1])
    for k in range(SERIES - 2, -1, -1):
        A = A * mq + INV_FACT[2 * k + 1]
        B = B * mq + INV_FACT[2 * k + 2]
        C = C * mq + INV_FACT[2 * k + 3]
    return A, B, C


def exp(d):
    """delta -> (dR as nine, dt as three), or None when q > pi^2"""
    with np.errstate(all="ignore"):
        w0, w1, w2 = d[0], d[1], d[2]
        s00, s11, s22 = w0 * w0, w1 * w1, w2 * w2
        q = (s00 + s11) + s22
        if q > PI2:  # a NaN q passes: the pose is then not finite, which ends the frame in state 2
            return None
        A, B, C = series(q)
        p01, p02, p12 = w0 * w1, w0 * w2, w1 * w2
        m00, m11, m22 = -(s11 + s22), -(s00 + s22), -(s00 + s11)

        def mat(a, b):  # I + a.W + b.W2
            return [1.0 + b * m00, b * p01 - a * w2, b * p02 + a * w1,
                    b * p01 + a * w2, 1.0 + b * m11, b * p12 - a * w0,
                    b * p02 - a * w1, b * p12 + a * w0, 1.0 + b * m22]
        dR, V = mat(A, B), mat(B, C)
        dt = [(V[3 * i] * d[3] + V[3 * i + 1] * d[4]) + V[3 * i + 2] * d[5] for i in range(3)]
    return dR, dt


def update(dR, dt, R, t):
    with np.errstate(all="ignore"):
        Rn = [(dR[3 * i] * R[j] + dR[3 * i + 1] * R[3 + j]) + dR[3 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
        tn = [((dR[3 * i] * t[0] + dR[3 * i + 1] * t[1]) + dR[3 * i + 2] * t[2]) + dt[i] for i in range(3)]
    return Rn, tn


# ---- step 4 -------------------------------------------------------------------------------------------------------------------------
def chi2(o, c, R, t):
    with np.errstate(all="ignore"):
        x, y, z = transform(o, R, t)
        up = c["fx"] * x / z + c["cx"]
        ex, ey = o["u"] - up, o["v"] - (c["fy"] * y / z + c["cy"])
        er = o["ur"] - (up - c["bf"] / z)
        sq = ex * ex + ey * ey
        v = np.where(o["stereo"], o["w"] * (sq + er * er), o["w"] * sq)
        return np.where(z > 0.0, v, BEHIND)


def inliers(o, c, values):
    with np.errstate(invalid="ignore"):
        return values <= np.where(o["stereo"], c["chi2_stereo"], c["chi2_mono"])


# ---- the frame ------------------------------------------------------------------------------------------------------------------------
def optimise(view, start, scale, points, kp, idx, params, skip=None, right=None, status=0, trace=None):
    """-> (RESULT_DTYPE record, uint8 flag per slot).  params: the fields of UPSTREAM.  status != 0: the frame is void (no observations).
    trace: a list that receives the inlier mask after every round that ended"""
    p = dict(UPSTREAM, **params)
    if status:
        o = observations(points[:0], kp[:0], np.zeros(0, np.int64), scale)
        o["n_slots"] = len(idx)
    else:
        o = observations(points, kp, idx, scale, skip, right, p["check_right"], p["idx_by_row"])
    n = len(o["X"])
    c = camera(view, p["chi2_mono"], p["chi2_stereo"])
    R, t, ok = start_pose(start)
    R0, t0 = list(R), list(t)
    active = np.ones(n, bool)
    state = 2 if not ok else 1 if n < p["min_obs"] else 0
    n_in, cost, steps = n, f64(0.0), [0] * 8
    for rnd in range(p["n_rounds"]):
        if state:
            break
        for _ in range(p["iterations"]):
            front, T = terms(o, c, R, t, rnd < p["robust_rounds"])
            total = tree(T, active & front)
            d = solve(total, p["lambda_"])
            if d is None:
                state = 2
                break
            e = exp(d)
            if e is None:
                state = 4
                break
            R, t = update(e[0], e[1], R, t)
            steps[rnd] += 1
            if all(abs(v) < p["step_eps"] for v in d):
                break
        if state:
            break
        values = chi2(o, c, R, t)
        active = inliers(o, c, values)
        if trace is not None:
            trace.append(active.copy())
        n_in = int(active.sum())
        cost = tree(values, active)
        if n_in < p["min_obs"]:
            state = 3
    if not all(np.isfinite(v) for v in list(R) + list(t)):
        state, R, t = 2, R0, t0
    flags = np.full(o["n_slots"], 2, np.uint8)
    flags[o["slot"]] = np.where(active, 0, 1)
    res = np.zeros((), RESULT_DTYPE)
    res["rcw"], res["tcw"], res["cost"] = np.array(R, f64), np.array(t, f64), cost
    res["state"], res["status"], res["n_obs"], res["n_stereo"], res["n_inliers"] = state, status, n, int(o["stereo"].sum()), n_in
    res["steps"] = steps
    return res, flags
