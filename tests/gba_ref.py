"""The global bundle adjustment of include/sendslam_orb.h (Optimizer::BundleAdjustment as LoopClosing::RunGlobalBundleAdjustment and
CreateInitialMapMonocular run it over a whole map), restated in numpy: the NORMATIVE statement of the rule (test infrastructure, plain
module).  The observation's terms, the point's factor and its solves, the chi-terms and the lambda schedule are tests/ba_ref.py's and
tests/pose_ref.py's; what the whole-map problem adds is here: the sorted record table and its two incidence lists, the per-keyframe
trees in list order, the blocks of the free keyframes and the matrix-free preconditioned conjugate gradients on the reduced system.

    tables()         the records sorted by (point, kf), the points' runs, the keyframes' lists padded to whole tree rounds
    tree_lists()     one tree per keyframe over its list in list order, all keyframes at once
    chol6(), subst6() the Cholesky by columns of order 6 and its two triangular solves, every keyframe at once
    optimise()       steps 1 - 9 of one problem

Every step is one numpy float64 operation (elementwise operations and sqrt are IEEE and correctly rounded; nothing is summed by numpy),
left to right as the header writes them.  The arrays run over the sorted records, the points or the keyframes.
"""
from __future__ import annotations

import numpy as np

import ba_ref as BR
import pose_ref as PR

f64 = np.float64
SLOTS = PR.SLOTS
OBS_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("right", "<f4"), ("octave", "<i4")])
RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                        [(n, "<i4") for n in ("state", "status", "n_obs", "n_stereo", "n_inliers", "n_points_active", "n_frozen_max")] +
                        [("steps", "<i4", (4,)), ("accepted", "<i4", (4,))] + [(n, "<i4") for n in ("pcg_iterations", "n_free", "n_fixed")] +
                        [("reserved", "<i4", (2,))])
DEFAULTS = dict(chi2_mono=5.991, chi2_stereo=7.815, lambda_=1e-4, lambda_factor=10.0, lambda_min=1e-9, step_eps=1e-10, pcg_tol=1e-2, n_rounds=1,
                iterations=(10, 0, 0, 0), robust_rounds=1, min_point_obs=2, check_right=False, pcg_iterations=64)


class Tables:
    """the records of one problem sorted by (point, kf) and both incidence lists"""

    def __init__(self, n_kf, n_points, obs):
        obs = np.asarray(obs, OBS_DTYPE).reshape(-1)
        kf, pt = obs["kf"].astype(np.int64), obs["point"].astype(np.int64)
        if ((kf < 0) | (kf >= n_kf)).any():
            raise ValueError("a kf outside the problem")
        if ((pt < 0) | (pt >= n_points)).any():
            raise ValueError("a point outside the problem")
        order = np.lexsort((kf, pt))
        self.orig = order
        self.rec = obs[order]
        self.kf, self.pt = kf[order], pt[order]
        if len(order) > 1 and ((self.kf[1:] == self.kf[:-1]) & (self.pt[1:] == self.pt[:-1])).any():
            raise ValueError("a (kf, point) pair twice")
        S = len(order)
        self.n_kf, self.n_points, self.n = n_kf, n_points, S
        cnt = np.bincount(self.pt, minlength=n_points)
        off = np.concatenate(([0], np.cumsum(cnt)[:-1])) if n_points else np.zeros(0, np.int64)
        self.rank = np.arange(S) - off[self.pt] if S else np.zeros(0, np.int64)
        self.max_rank = int(cnt.max()) if n_points and S else 0
        # the keyframes' lists: ascending record number is ascending point; padded with the dummy record S to whole rounds of 256
        lists = [np.flatnonzero(self.kf == k) for k in range(n_kf)]
        longest = max([len(l) for l in lists] + [1])
        rounds = -(-longest // SLOTS)
        self.KL = np.full((n_kf, rounds * SLOTS), S, np.int64)
        for k, l in enumerate(lists):
            self.KL[k, :len(l)] = l
        self.rounds = rounds

    def tree_lists(self, values, mask):
        """values [..., S], mask [S] -> [..., n_kf]: per keyframe the tree over its list of the items with mask: slot s adds the items j =
        s, s + 256, ... in ascending j from +0.0, groups of 64 slots fold by halving, (r0 + r1) + (r2 + r3)"""
        values = np.asarray(values, f64)
        lead = values.shape[:-1]
        v = np.concatenate([values, np.zeros(lead + (1,), f64)], axis=-1)
        m = np.concatenate([np.asarray(mask, bool), [False]])
        KL = self.KL.reshape(self.n_kf, self.rounds, SLOTS)
        acc = np.zeros(lead + (self.n_kf, SLOTS), f64)
        with np.errstate(all="ignore"):
            for j in range(self.rounds):
                acc = np.where(m[KL[:, j, :]], acc + v[..., KL[:, j, :]], acc)
            a = acc.reshape(lead + (self.n_kf, 4, 64)).copy()
            for h in (32, 16, 8, 4, 2, 1):
                a[..., :h] = a[..., :h] + a[..., h:2 * h]
            return (a[..., 0, 0] + a[..., 1, 0]) + (a[..., 2, 0] + a[..., 3, 0])


def chol6(H):
    """H[i][j], i >= j: arrays over the keyframes (overwritten by the factor) -> bool per keyframe: every pivot > 0.  Cholesky by
    columns, every inner sum subtracting in ascending k"""
    ok = np.ones(np.shape(H[0][0]), bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = H[j][j]
            for k in range(j):
                s = s - H[j][k] * H[j][k]
            ok = ok & (s > 0.0)
            H[j][j] = np.sqrt(s)
            for i in range(j + 1, 6):
                v = H[i][j]
                for k in range(j):
                    v = v - H[i][k] * H[j][k]
                H[i][j] = v / H[j][j]
    return ok


def subst6(L, d):
    """d [6] arrays over the keyframes -> L^-T.L^-1.d by the two triangular solves"""
    d = list(d)
    with np.errstate(all="ignore"):
        for i in range(6):
            v = d[i]
            for k in range(i):
                v = v - L[i][k] * d[k]
            d[i] = v / L[i][i]
        for i in range(5, -1, -1):
            v = d[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * d[k]
            d[i] = v / L[i][i]
    return d


def dot(x, y):
    """x, y [n_kf][6] -> the tree over the 6 n_kf products in keyframe-major order"""
    with np.errstate(all="ignore"):
        prod = (x * y).reshape(-1)
    return PR.tree(prod, np.ones(len(prod), bool))


def gather(tab, scale, points, skip, check_right):
    """-> (X float64 [P][3] with +0.0 where the row is no point, bool is_point [P], the records' dict of float64 u v ur w, bool stereo
    and bool valid [S])"""
    P = len(points)
    X = np.stack([np.asarray(points[n], np.float32).astype(f64) for n in ("x", "y", "z")], axis=1).reshape(P, 3)
    is_point = np.isfinite(X).all(axis=1)
    if skip is not None:
        is_point &= np.asarray(skip) == 0
    X = np.where(is_point[:, None], X, 0.0)
    rec = tab.rec
    octave = rec["octave"].astype(np.int64)
    valid = (octave >= 0) & (octave < len(scale))
    s = np.asarray(scale, np.float32)[np.where(valid, octave, 0)].astype(f64)
    s = np.where(valid, s, 1.0)
    o = {"u": rec["u"].astype(f64), "v": rec["v"].astype(f64), "w": 1.0 / (s * s), "valid": valid}
    with np.errstate(invalid="ignore"):
        o["stereo"] = (rec["right"] > np.float32(0)) & bool(check_right)
    o["ur"] = np.where(o["stereo"], rec["right"].astype(f64), 0.0)
    return X, is_point, o


def optimise(views, start, fixed, scale, points, obs, params, skip=None, trace=None):
    """-> (poses float64 [n_kf][12], xyz float64 [P][3], uint8 point flags [P], uint8 observation flags [n_obs] in the order of obs,
    RESULT_DTYPE record).  params: the fields of DEFAULTS.  trace: a list that receives one dict per step (the state it was linearised
    at, dc, dp, lambda, the PCG's iterations and exit, whether it was accepted) and one per classification"""
    p = dict(DEFAULTS, **params)
    n_kf, P = len(views), len(points)
    fixed = np.asarray(fixed, np.uint8).reshape(n_kf) != 0
    free = ~fixed
    tab = Tables(n_kf, P, obs)
    S, kf, pt, rank = tab.n, tab.kf, tab.pt, tab.rank
    X, is_point, o = gather(tab, scale, points, skip, p["check_right"])
    cams = [PR.camera(v, p["chi2_mono"], p["chi2_stereo"]) for v in views]
    c = {n: np.array([cam[n] for cam in cams], f64)[kf] for n in cams[0]} if n_kf else {}
    Rm, tm, ok = np.empty((n_kf, 9), f64), np.empty((n_kf, 3), f64), True
    for k in range(n_kf):
        R, t, good = PR.start_pose(np.asarray(start, f64).reshape(n_kf, 12)[k])
        Rm[k], tm[k] = R, t
        ok = ok and good
    # step 1
    is_obs = o["valid"] & is_point[pt]
    ob = np.where(is_obs, 0, 2).astype(np.uint8)
    count = np.bincount(pt[is_obs], minlength=P)
    n_obs, n_stereo = int(is_obs.sum()), int((is_obs & o["stereo"]).sum())
    pflag = np.where(~is_point, 2, np.where(count < p["min_point_obs"], 1, 0)).astype(np.uint8)
    n_free = int(free.sum())
    state = 2 if not ok else 1 if (not (pflag == 0).any() or n_free == 0) else 0
    lam, cost0, cost_before = f64(p["lambda_"]), f64(0.0), f64(0.0)
    steps, accepted_n, frozen_max, pcg_total = [0] * 4, [0] * 4, 0, 0

    def at(Rs, ts, Xs):
        """the records' observation dict, rotations and translations under a state"""
        return dict(o, X=Xs[pt, 0], Y=Xs[pt, 1], Z=Xs[pt, 2]), [Rs[kf, i] for i in range(9)], [ts[kf, i] for i in range(3)]

    def cost(Rs, ts, Xs, robust):
        ow, R, t = at(Rs, ts, Xs)
        with np.errstate(all="ignore"):
            per_kf = tab.tree_lists(BR.cost_terms(ow, c, R, t, robust), (ob == 0) & (pflag[pt] == 0))
            return PR.tree(per_kf, np.ones(n_kf, bool))

    for rnd in range(p["n_rounds"]):
        if state:
            break
        robust = rnd < p["robust_rounds"]
        cost_now = cost(Rm, tm, X, robust)
        if not np.isfinite(cost_now):
            state = 2
            break
        cost0 = cost_now
        if rnd == 0:
            cost_before = cost0
        for _ in range(p["iterations"][rnd]):
            active = pflag == 0
            ow, R, t = at(Rm, tm, X)
            with np.errstate(all="ignore"):
                # steps 2 and 3: the points, their lists in ascending kf
                front, tV, tb, W = BR.linearise(ow, c, R, t, robust)
                lin = front & (ob == 0) & active[pt]
                V, b = np.zeros((6, P), f64), np.zeros((3, P), f64)
                for j in range(tab.max_rank):
                    sel = lin & (rank == j)
                    V[:, pt[sel]] = V[:, pt[sel]] + tV[:, sel]
                    b[:, pt[sel]] = b[:, pt[sel]] + tb[:, sel]
                good, L = BR.factor3(V, lam)
                solved = active & good
                frozen_max = max(frozen_max, int((active & ~good).sum()))
                # step 4: the blocks of the free keyframes, their lists in list order
                Lr = L[:, pt]
                Y = np.stack([v for a in range(6) for v in BR.subst3(Lr, W[3 * a:3 * a + 3])])
                both = lin & solved[pt]
                Csum = tab.tree_lists(np.stack([(Y[3 * a] * W[3 * d] + Y[3 * a + 1] * W[3 * d + 1]) + Y[3 * a + 2] * W[3 * d + 2] for a, d in BR.UPPER6]), both)
                Ysum = tab.tree_lists(np.stack([(Y[3 * a] * b[0][pt] + Y[3 * a + 1] * b[1][pt]) + Y[3 * a + 2] * b[2][pt] for a in range(6)]), both)
                _, T = PR.terms(ow, c, R, t, robust)
                Usum = tab.tree_lists(T, lin)
                U = [[None] * 6 for _ in range(6)]
                for m, (a, d) in enumerate(PR.H_PAIRS):
                    U[a][d] = U[d][a] = Usum[m]
                U[3][4] = U[4][3] = np.zeros(n_kf, f64)
                for a in range(6):
                    U[a][a] = U[a][a] + lam * (1.0 + U[a][a])
                M = [[None] * 6 for _ in range(6)]
                for m, (a, d) in enumerate(BR.UPPER6):
                    M[d][a] = U[a][d] - Csum[m]
                r = np.stack([np.where(free, -(Usum[20 + a] - Ysum[a]), 0.0) for a in range(6)], axis=1)
                pos = chol6(M)
            if (free & ~pos).any():
                state = 2
                break

            def precondition(r):
                z = subst6(M, [r[:, a] for a in range(6)])
                return np.stack([np.where(free, z[a], r[:, a]) for a in range(6)], axis=1)

            def operator(pv):
                with np.errstate(all="ignore"):
                    a3 = np.zeros((3, P), f64)
                    pr = [pv[kf, a] for a in range(6)]
                    for j in range(tab.max_rank):
                        sel = lin & free[kf] & (rank == j)
                        for e in range(3):
                            s = ((((W[e] * pr[0] + W[3 + e] * pr[1]) + W[6 + e] * pr[2]) + W[9 + e] * pr[3]) + W[12 + e] * pr[4]) + W[15 + e] * pr[5]
                            a3[e, pt[sel]] = a3[e, pt[sel]] + s[sel]
                    cc = BR.subst3(L, [a3[0], a3[1], a3[2]])
                    Tk = tab.tree_lists(np.stack([(W[3 * a] * cc[0][pt] + W[3 * a + 1] * cc[1][pt]) + W[3 * a + 2] * cc[2][pt] for a in range(6)]), both)
                    q = np.zeros((n_kf, 6), f64)
                    for a in range(6):
                        up = U[a][0] * pv[:, 0]
                        for d in range(1, 6):
                            up = up + U[a][d] * pv[:, d]
                        q[:, a] = np.where(free, up - Tk[a], 0.0)
                return q

            # step 5: preconditioned conjugate gradients on S.dc = r
            with np.errstate(all="ignore"):
                x = np.zeros((n_kf, 6), f64)
                z = precondition(r)
                pv = z.copy()
                rho = dot(r, z)
                stop = (f64(p["pcg_tol"]) * f64(p["pcg_tol"])) * rho
                done, left = 0, "cap"
                while done < p["pcg_iterations"]:
                    q = operator(pv)
                    pq = dot(pv, q)
                    if not pq > 0.0:
                        left = "curvature"
                        break
                    alpha = rho / pq
                    x, r = x + alpha * pv, r - alpha * q
                    done += 1
                    z = precondition(r)
                    rho1 = dot(r, z)
                    if rho1 <= stop:
                        left = "tolerance"
                        break
                    beta = rho1 / rho
                    pv = z + beta * pv
                    rho = rho1
            pcg_total += done
            dc = x
            # step 6
            Rt, tt, large, small, finite = Rm.copy(), tm.copy(), False, True, True
            for k in np.flatnonzero(free):
                d = [dc[k, a] for a in range(6)]
                e = PR.exp(d)
                if e is None:
                    large = True
                    continue
                Rn, tn = PR.update(e[0], e[1], list(Rm[k]), list(tm[k]))
                Rt[k], tt[k] = Rn, tn
                with np.errstate(invalid="ignore"):
                    small = small and all(abs(v) < p["step_eps"] for v in d)
                finite = finite and bool(np.isfinite(Rt[k]).all() and np.isfinite(tt[k]).all())
            if large:
                state = 4
                break
            with np.errstate(all="ignore"):
                v = np.stack([-b[0], -b[1], -b[2]])
                dr = [dc[kf, a] for a in range(6)]
                for j in range(tab.max_rank):
                    sel = lin & free[kf] & (rank == j)
                    for e in range(3):
                        s = ((((W[e] * dr[0] + W[3 + e] * dr[1]) + W[6 + e] * dr[2]) + W[9 + e] * dr[3]) + W[12 + e] * dr[4]) + W[15 + e] * dr[5]
                        v[e, pt[sel]] = v[e, pt[sel]] - s[sel]
                dp = np.stack(BR.subst3(L, [v[0], v[1], v[2]]), axis=1)
                Xt = np.where(solved[:, None], X + dp, X)
                small = small and bool((np.abs(dp[solved]) < p["step_eps"]).all())
                finite = finite and bool(np.isfinite(Xt[solved]).all())
            # step 7
            cost1 = cost(Rt, tt, Xt, robust)
            with np.errstate(invalid="ignore"):
                accepted = bool(finite and np.isfinite(cost1) and cost1 <= cost0)
            if trace is not None:
                trace.append(dict(kind="step", round=rnd, robust=robust, lam=lam, R=Rm.copy(), t=tm.copy(), X=X.copy(), active=active.copy(), solved=solved.copy(),
                                  lin=lin.copy(), dc=dc.copy(), dp=np.where(solved[:, None], dp, 0.0), accepted=accepted, cost0=cost0, cost1=cost1, small=small,
                                  pcg=done, left=left, ob=ob.copy()))
            steps[rnd] += 1
            lam = BR.next_lambda(lam, accepted, p["lambda_factor"], p["lambda_min"])
            if not accepted:
                continue
            accepted_n[rnd] += 1
            cost0, Rm, tm, X = cost1, Rt, tt, Xt
            if small:
                break
        if state:
            break
        # step 8
        ow, R, t = at(Rm, tm, X)
        keep = PR.inliers(ow, c, PR.chi2(ow, c, R, t))
        out = (ob == 0) & (pflag[pt] == 0) & ~keep
        ob[out] = 1
        count = np.bincount(pt[ob == 0], minlength=P)
        pflag = np.where((pflag == 0) & (count < p["min_point_obs"]), 1, pflag).astype(np.uint8)
        if trace is not None:
            trace.append(dict(kind="classify", round=rnd, removed=int(out.sum())))
    res = np.zeros((), RESULT_DTYPE)
    res["lambda_"], res["cost_before"], res["cost_after"] = lam, cost_before, cost0
    res["state"], res["status"], res["n_obs"], res["n_stereo"] = state, 0, n_obs, n_stereo
    res["n_inliers"], res["n_points_active"], res["n_frozen_max"] = int((ob == 0).sum()), int((pflag == 0).sum()), frozen_max
    res["steps"], res["accepted"] = steps, accepted_n
    res["pcg_iterations"], res["n_free"], res["n_fixed"] = pcg_total, n_free, n_kf - n_free
    oflag = np.empty(S, np.uint8)
    oflag[tab.orig] = ob
    return np.concatenate([Rm, tm], axis=1).reshape(n_kf, 12), np.where((pflag == 2)[:, None], 0.0, X), pflag, oflag, res


def obs_from_idx(kp, idx, n_kp=None, right=None):
    """the stack the projection searches leave -> OBS_DTYPE records in ascending (point, kf) order"""
    n_kf, rows = kp.shape
    idx = np.asarray(idx, np.int64).reshape(n_kf, -1)
    nk = np.full(n_kf, rows) if n_kp is None else np.clip(np.asarray(n_kp, np.int64), 0, rows)
    out = []
    for i in range(idx.shape[1]):
        for k in range(n_kf):
            row = idx[k, i]
            if 0 <= row < nk[k]:
                out.append((k, i, kp["x"][k, row], kp["y"][k, row], -1.0 if right is None else right[k, row], kp["octave"][k, row]))
    return np.array(out, OBS_DTYPE)
