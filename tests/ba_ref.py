"""The local bundle adjustment of include/sendslam_orb.h (Optimizer::LocalBundleAdjustment as LocalMapping runs it after the map-building
chain), restated in numpy: the NORMATIVE statement of the rule (test infrastructure, plain module).  The observation's residuals,
Jacobian rows, Huber weight, pose terms, chi-square, the start rotation, the exponential, the update and the tree of a sum are
tests/pose_ref.py's; everything the coupled problem adds is here.

    gather()         step 1: the points, the observations of every (keyframe, point row) and their numbers widened to double
    linearise()      step 2: the terms of V, b and W of every point row in one keyframe
    factor3()        step 3: the damped 3 x 3 Cholesky factor of every point, and subst3() its two triangular solves
    chol_n()         step 5: Cholesky by columns in its right-looking schedule, subst_n() the two triangular solves
    cost()           step 7: the sum over the keyframes of the trees of the chi-terms
    optimise()       steps 1 - 9 of one problem

Every step is one numpy float64 operation (elementwise operations and sqrt are IEEE and correctly rounded; the only sums numpy forms
are ufunc.accumulate ones, which are sequential), left to right as the header writes them.
"""
from __future__ import annotations

import numpy as np

import pose_ref as PR

f64 = np.float64
RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                        [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers", "n_points_active", "n_frozen_max")] +
                        [("steps", "<i4", (4,)), ("accepted", "<i4", (4,)), ("reserved", "<i4")])
DEFAULTS = dict(chi2_mono=5.991, chi2_stereo=7.815, lambda_=1e-4, lambda_factor=10.0, lambda_min=1e-9, step_eps=1e-10, n_rounds=2,
                iterations=(5, 10, 0, 0), robust_rounds=1, min_point_obs=2, check_right=False)
# the pairs (a, b) of the upper triangle of a 6 x 6 block, row by row, and of a 3 x 3 one
UPPER6 = [(a, b) for a in range(6) for b in range(a, 6)]
UPPER3 = [(a, b) for a in range(3) for b in range(a, 3)]


# ---- step 1 -------------------------------------------------------------------------------------------------------------------------
def gather(points, kp, idx, n_kp, scale, skip=None, right=None, check_right=False):
    """points [P], kp [n_kf][rows], idx [n_kf][P] -> (X float64 [P][3] with +0.0 where the row is no point, bool is_point [P], a list
    of one dict per keyframe with float64 u v ur w [P], bool stereo [P] and bool obs [P])"""
    P, n_kf, rows = len(points), len(kp), kp.shape[1]
    X = np.stack([np.asarray(points[n], np.float32).astype(f64) for n in ("x", "y", "z")], axis=1).reshape(P, 3)
    is_point = np.isfinite(X).all(axis=1)
    if skip is not None:
        is_point &= np.asarray(skip) == 0
    X = np.where(is_point[:, None], X, 0.0)
    idx = np.asarray(idx, np.int64).reshape(n_kf, P)
    frames = []
    for k in range(n_kf):
        nk = min(max(int(n_kp[k]), 0), rows)
        ok = is_point & (idx[k] >= 0) & (idx[k] < nk)
        row = np.where(ok, idx[k], 0)
        octave = np.asarray(kp[k]["octave"], np.int64)[row]
        ok &= (octave >= 0) & (octave < len(scale))
        s = np.asarray(scale, np.float32)[np.where(ok, octave, 0)].astype(f64)
        o = {"u": np.asarray(kp[k]["x"], np.float32)[row].astype(f64), "v": np.asarray(kp[k]["y"], np.float32)[row].astype(f64), "w": 1.0 / (s * s), "obs": ok}
        if check_right and right is not None:
            r = np.asarray(right[k], np.float32)[row]
            with np.errstate(invalid="ignore"):
                o["stereo"] = ok & (r > np.float32(0))
            o["ur"] = np.where(o["stereo"], r.astype(f64), 0.0)
        else:
            o["stereo"], o["ur"] = np.zeros(P, bool), np.zeros(P, f64)
        frames.append(o)
    return X, is_point, frames


def with_points(o, X):
    return dict(o, X=X[:, 0], Y=X[:, 1], Z=X[:, 2])


# ---- step 2 -------------------------------------------------------------------------------------------------------------------------
def point_rows(J, R):
    """the rows of the pose Jacobian -> the three rows of the point Jacobian, Jp = -Jproj.R from the translation entries of J"""
    a3, a5, c4, c5, d5 = J[0][3], J[0][5], J[1][4], J[1][5], J[2][5]
    return [[a3 * R[b] + a5 * R[6 + b] for b in range(3)], [c4 * R[3 + b] + c5 * R[6 + b] for b in range(3)], [a3 * R[b] + d5 * R[6 + b] for b in range(3)]]


def linearise(o, c, R, t, robust):
    """-> (bool [P]: z > 0, V [6][P], b [3][P], W [18][P]) of every point row under the keyframe's (R, t)"""
    with np.errstate(all="ignore"):
        front, res, J = PR.jacobians(o, c, R, t)
        st, w = o["stereo"], o["w"]
        zero = np.zeros_like(w)
        J = [[zero if v is None else v for v in row] for row in J]  # the structural zeros are +0.0 factors here
        sq = res[0] * res[0] + res[1] * res[1]
        e2 = np.where(st, w * (sq + res[2] * res[2]), w * sq)
        d = np.where(st, c["delta_stereo"], c["delta_mono"])
        q = np.where((e2 > d * d) & bool(robust), w * d / np.sqrt(e2), w)
        Jp = point_rows(J, R)
        qJp = [[q * v for v in row] for row in Jp]
        qJ = [[q * v for v in row] for row in J]

        def term(left, right):  # (row0 + row1) [+ row2], the bracket for stereo only
            mono = left[0] * right[0] + left[1] * right[1]
            return np.where(st, mono + left[2] * right[2], mono)

        V = np.stack([term([qJp[r][a] for r in range(3)], [Jp[r][b] for r in range(3)]) for a, b in UPPER3])
        b = np.stack([term([qJp[r][a] for r in range(3)], res) for a in range(3)])
        W = np.stack([term([qJ[r][a] for r in range(3)], [Jp[r][b] for r in range(3)]) for a in range(6) for b in range(3)])
    return front, V, b, W


# ---- step 3 -------------------------------------------------------------------------------------------------------------------------
def factor3(V, lam):
    """V [6][P] (V00 V01 V02 V11 V12 V22) -> (bool [P]: every pivot > 0, L [6][P]: L00 L10 L11 L20 L21 L22)"""
    lam = f64(lam)
    with np.errstate(all="ignore"):
        h00, h10, h20, h11, h21, h22 = V[0], V[1], V[2], V[3], V[4], V[5]
        h00 = h00 + lam * (1.0 + h00)
        h11 = h11 + lam * (1.0 + h11)
        h22 = h22 + lam * (1.0 + h22)
        ok = h00 > 0.0
        l00 = np.sqrt(h00)
        l10, l20 = h10 / l00, h20 / l00
        s = h11 - l10 * l10
        ok = ok & (s > 0.0)
        l11 = np.sqrt(s)
        l21 = (h21 - l20 * l10) / l11
        s = (h22 - l20 * l20) - l21 * l21
        ok = ok & (s > 0.0)
        l22 = np.sqrt(s)
    return ok, np.stack([l00, l10, l11, l20, l21, l22])


def subst3(L, v):
    """v [3][...] -> V^-1.v by the two triangular solves"""
    with np.errstate(all="ignore"):
        v0 = v[0] / L[0]
        v1 = (v[1] - L[1] * v0) / L[2]
        v2 = ((v[2] - L[3] * v0) - L[4] * v1) / L[5]
        v2 = v2 / L[5]
        v1 = (v1 - L[4] * v2) / L[2]
        v0 = ((v0 - L[1] * v1) - L[3] * v2) / L[0]
    return [v0, v1, v2]


# ---- step 5 -------------------------------------------------------------------------------------------------------------------------
def chol_n(S):
    """S symmetric [n][n] -> (every pivot > 0, L in the lower triangle).  Right-looking: once column k is final it is taken off every
    later entry, so each entry's subtractions run in ascending k, as in the column form"""
    H = np.array(S, f64)
    n = len(H)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            ok = ok and bool(H[k, k] > 0.0)
            H[k, k] = np.sqrt(H[k, k])
            H[k + 1:, k] = H[k + 1:, k] / H[k, k]
            col = H[k + 1:, k]
            H[k + 1:, k + 1:] = H[k + 1:, k + 1:] - col[:, None] * col[None, :]
    return ok, H


def subst_n(L, rhs):
    d = np.array(rhs, f64)
    n = len(d)
    with np.errstate(all="ignore"):
        for k in range(n):
            d[k] = d[k] / L[k, k]
            d[k + 1:] = d[k + 1:] - L[k + 1:, k] * d[k]
        for i in range(n - 1, -1, -1):
            chain = np.concatenate(([d[i]], L[i + 1:, i] * d[i + 1:]))
            d[i] = np.subtract.accumulate(chain)[-1] / L[i, i]
    return d


# ---- step 7 -------------------------------------------------------------------------------------------------------------------------
def cost_terms(o, c, R, t, robust):
    with np.errstate(all="ignore"):
        e2 = PR.chi2(o, c, R, t)
        if not robust:
            return e2
        d = np.where(o["stereo"], c["delta_stereo"], c["delta_mono"])
        return np.where(e2 <= d * d, e2, 2.0 * d * np.sqrt(e2) - d * d)


def cost(frames, cams, poses, X, active, robust):
    total = f64(0.0)
    with np.errstate(all="ignore"):
        for k, o in enumerate(frames):
            total = total + PR.tree(cost_terms(with_points(o, X), cams[k], poses[k][0], poses[k][1], robust), o["obs"] & active)
    return total


def next_lambda(lam, accepted, factor, lam_min):
    with np.errstate(all="ignore"):
        if not accepted:
            return lam * f64(factor)
        l = lam / f64(factor)
        return l if l > lam_min else f64(lam_min)


# ---- the problem ---------------------------------------------------------------------------------------------------------------------
def optimise(views, start, n_free, scale, points, kp, idx, params, n_kp=None, skip=None, right=None, status=0, trace=None):
    """-> (poses float64 [n_kf][12], xyz float64 [P][3], uint8 point flags [P], uint8 observation flags [n_kf][P], RESULT_DTYPE record).
    params: the fields of DEFAULTS.  status != 0: the problem is void.  trace: a list that receives one dict per step (the state it
    was linearised at, dc, dp, lambda, whether it was accepted) and one per classification"""
    p = dict(DEFAULTS, **params)
    n_kf, P = len(views), len(points)
    n_kp = np.full(n_kf, kp.shape[1]) if n_kp is None else n_kp
    X, is_point, frames = gather(points, kp, idx, n_kp, scale, skip, right, p["check_right"])
    if status:
        is_point[:] = False
        X[:] = 0.0
        for o in frames:
            o["obs"][:] = False
            o["stereo"][:] = False
    cams = [PR.camera(v, p["chi2_mono"], p["chi2_stereo"]) for v in views]
    poses, ok = [], True
    for k in range(n_kf):
        R, t, good = PR.start_pose(np.asarray(start, f64).reshape(n_kf, 12)[k])
        poses.append((R, t))
        ok = ok and good
    oflag = np.stack([np.where(o["obs"], 0, 2).astype(np.uint8) for o in frames]) if n_kf else np.zeros((0, P), np.uint8)
    count = sum(o["obs"].astype(np.int64) for o in frames)
    n_obs, n_stereo = int(count.sum()), int(sum(o["stereo"].sum() for o in frames))
    pflag = np.where(~is_point, 2, np.where(count < p["min_point_obs"], 1, 0)).astype(np.uint8)
    state = 2 if not ok else 1 if not (pflag == 0).any() else 0
    lam, cost0, cost_before = f64(p["lambda_"]), f64(0.0), f64(0.0)
    steps, accepted_n, frozen_max = [0] * 4, [0] * 4, 0
    n = 6 * n_free
    for rnd in range(p["n_rounds"]):
        if state:
            break
        robust = rnd < p["robust_rounds"]
        cost_now = cost(frames, cams, poses, X, pflag == 0, robust)
        if not np.isfinite(cost_now):
            state = 2
            break
        cost0 = cost_now
        if rnd == 0:
            cost_before = cost0
        for _ in range(p["iterations"][rnd]):
            active = pflag == 0
            # steps 2 and 3
            V, b = np.zeros((6, P), f64), np.zeros((3, P), f64)
            lin, W = [], []
            with np.errstate(all="ignore"):
                for k, o in enumerate(frames):
                    front, tV, tb, tW = linearise(with_points(o, X), cams[k], poses[k][0], poses[k][1], robust)
                    part = front & o["obs"] & active
                    V, b = np.where(part, V + tV, V), np.where(part, b + tb, b)
                    lin.append(part)
                    W.append(tW if k < n_free else None)
            good, L = factor3(V, lam)
            solved = active & good
            frozen_max = max(frozen_max, int((active & ~good).sum()))
            Y = [np.stack([v for a in range(6) for v in subst3(L, W[k][3 * a:3 * a + 3])]) for k in range(n_free)]
            # step 4
            S, r = np.zeros((n, n), f64), np.zeros(n, f64)
            with np.errstate(all="ignore"):
                for k in range(n_free):
                    o = with_points(frames[k], X)
                    _, T = PR.terms(o, cams[k], poses[k][0], poses[k][1], robust)
                    total = PR.tree(T, lin[k])
                    U = np.zeros((6, 6), f64)
                    for m, (a, c) in enumerate(PR.H_PAIRS):
                        U[a, c] = total[m]
                    for a in range(6):
                        U[a, a] = U[a, a] + lam * (1.0 + U[a, a])
                    both = lin[k] & solved
                    yb = PR.tree(np.stack([(Y[k][3 * a] * b[0] + Y[k][3 * a + 1] * b[1]) + Y[k][3 * a + 2] * b[2] for a in range(6)]), both)
                    r[6 * k:6 * k + 6] = total[20:26] - yb
                    for l in range(k, n_free):
                        pairs = UPPER6 if k == l else [(a, c) for a in range(6) for c in range(6)]
                        C = PR.tree(np.stack([(Y[k][3 * a] * W[l][3 * c] + Y[k][3 * a + 1] * W[l][3 * c + 1]) + Y[k][3 * a + 2] * W[l][3 * c + 2]
                                              for a, c in pairs]), both & lin[l])
                        for m, (a, c) in enumerate(pairs):
                            v = U[a, c] - C[m] if k == l else 0.0 - C[m]
                            S[6 * k + a, 6 * l + c] = S[6 * l + c, 6 * k + a] = v
            # step 5
            pos, Lc = chol_n(S)
            if not pos:
                state = 2
                break
            dc = subst_n(Lc, -r)
            # step 6
            trial, large, small, finite = list(poses), False, True, True
            for k in range(n_free):
                d = [dc[6 * k + a] for a in range(6)]
                e = PR.exp(d)
                if e is None:
                    large = True
                    continue
                trial[k] = PR.update(e[0], e[1], poses[k][0], poses[k][1])
                with np.errstate(invalid="ignore"):
                    small = small and all(abs(v) < p["step_eps"] for v in d)
                finite = finite and all(np.isfinite(v) for v in list(trial[k][0]) + list(trial[k][1]))
            if large:
                state = 4
                break
            with np.errstate(all="ignore"):
                v = [-b[0], -b[1], -b[2]]
                for k in range(n_free):
                    for e in range(3):
                        s = ((((W[k][e] * dc[6 * k] + W[k][3 + e] * dc[6 * k + 1]) + W[k][6 + e] * dc[6 * k + 2]) + W[k][9 + e] * dc[6 * k + 3]) +
                             W[k][12 + e] * dc[6 * k + 4]) + W[k][15 + e] * dc[6 * k + 5]
                        v[e] = np.where(lin[k], v[e] - s, v[e])
                dp = np.stack(subst3(L, v), axis=1)
                Xt = np.where(solved[:, None], X + dp, X)
                small = small and bool((np.abs(dp[solved]) < p["step_eps"]).all())
                finite = finite and bool(np.isfinite(Xt[solved]).all())
            # step 7
            cost1 = cost(frames, cams, trial, Xt, active, robust)
            with np.errstate(invalid="ignore"):
                accepted = bool(finite and np.isfinite(cost1) and cost1 <= cost0)
            if trace is not None:
                trace.append(dict(kind="step", round=rnd, robust=robust, lam=lam, poses=list(poses), X=X.copy(), active=active.copy(), solved=solved.copy(),
                                  lin=[m.copy() for m in lin], dc=dc.copy(), dp=np.where(solved[:, None], dp, 0.0), accepted=accepted, cost0=cost0, cost1=cost1,
                                  small=small))
            steps[rnd] += 1
            lam = next_lambda(lam, accepted, p["lambda_factor"], p["lambda_min"])
            if not accepted:
                continue
            accepted_n[rnd] += 1
            cost0, poses, X = cost1, trial, Xt
            if small:
                break
        if state:
            break
        # step 8
        removed = 0
        for k, o in enumerate(frames):
            ow = with_points(o, X)
            keep = PR.inliers(ow, cams[k], PR.chi2(ow, cams[k], poses[k][0], poses[k][1]))
            out = o["obs"] & (pflag == 0) & ~keep
            removed += int(out.sum())
            o["obs"] = o["obs"] & ~out
            oflag[k][out] = 1
        count = sum(o["obs"].astype(np.int64) for o in frames)
        pflag = np.where((pflag == 0) & (count < p["min_point_obs"]), 1, pflag).astype(np.uint8)
        if trace is not None:
            trace.append(dict(kind="classify", round=rnd, removed=removed))
    res = np.zeros((), RESULT_DTYPE)
    res["lambda_"], res["cost_before"], res["cost_after"] = lam, cost_before, cost0
    res["state"], res["status"], res["n_obs"], res["n_stereo"] = state, status, n_obs, n_stereo
    res["n_inliers"], res["n_points_active"], res["n_frozen_max"] = int((oflag == 0).sum()), int((pflag == 0).sum()), frozen_max
    res["steps"], res["accepted"] = steps, accepted_n
    out_poses = np.array([list(R) + list(t) for R, t in poses], f64).reshape(n_kf, 12)
    return out_poses, np.where((pflag == 2)[:, None], 0.0, X), pflag, oflag, res
