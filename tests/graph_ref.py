"""The essential-graph optimisation of include/sendslam_orb.h (Optimizer::OptimizeEssentialGraph as LoopClosing::CorrectLoop runs it, and
the map-point correction after it), restated in numpy: the NORMATIVE statement of the rule (test infrastructure, plain module).  The
rotation's series, the table of 1 / n! and the tree of a sum are tests/pose_ref.py's, the scale's series is tests/sim3opt_ref.py's;
everything the pose graph adds is here.

    atan2(), ln()    the two series
    inv(), mul()     Sim3 as thirteen rows: R row-major, t, s; every function works on columns (one per edge or keyframe) at once
    log(), error()   step 2: e = (omega, upsilon, sigma) of E = (M . S_i) . S_j^-1
    retract()        step 3
    jacobian()       step 4: central differences through the retraction
    blocks()         step 5: H_vv, g_v, the damping terms and the factor of every free keyframe
    pcg()            step 6
    optimise()       steps 1 - 7 of one problem
    points()         the map-point correction

Every step is one numpy float64 operation (elementwise operations and sqrt are IEEE and correctly rounded; numpy forms no sum here),
left to right as the header writes them.
"""
from __future__ import annotations

import numpy as np

import pose_ref as PR
import sim3opt_ref as SR

f64 = np.float64
RESULT_DTYPE = np.dtype([("lambda_", "<f8"), ("cost_before", "<f8"), ("cost_after", "<f8")] +
                        [(n, "<i4") for n in ("state", "n_edges", "n_free", "steps", "accepted", "pcg_iterations")])
DEFAULTS = dict(lambda_=1e-16, lambda_factor=10.0, lambda_min=0.0, pcg_tol=1e-2, iterations=20, pcg_iterations=128, fix_scale=False)
INV_ODD = [f64(1.0) / f64(2 * k + 1) for k in range(26)]
ATAN_TERMS, LN_TERMS = 24, 13
H, H2 = f64(1e-9), f64(2e-9)
SMALL_N, NEAR_PI_N = f64(2.0 ** -26), f64(2.0 ** -20)
ATAN_HALF = (float.fromhex("0x1.dac670561bb4fp-2"), float.fromhex("0x1.a2b7f222f65e2p-56"))
PI_4 = (float.fromhex("0x1.921fb54442d18p-1"), float.fromhex("0x1.1a62633145c07p-55"))
PI_2 = (float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54"))
PI = (float.fromhex("0x1.921fb54442d18p+1"), float.fromhex("0x1.1a62633145c07p-53"))
LN2 = (float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33"))
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")


# ---- the two series -----------------------------------------------------------------------------------------------------------------
def atan01(r):
    """atan(r), 0 <= r <= 1: three ranges, z + z*(mw*P) with P the Horner sum of 1/3, 1/5, ... in mw = -(z*z)"""
    r = np.asarray(r, f64)
    with np.errstate(all="ignore"):
        low, mid = r < 0.4375, r < 0.6875
        z = np.where(low, r, np.where(mid, (2.0 * r - 1.0) / (2.0 + r), (r - 1.0) / (r + 1.0)))
        hi = np.where(low, 0.0, np.where(mid, ATAN_HALF[0], PI_4[0]))
        lo = np.where(low, 0.0, np.where(mid, ATAN_HALF[1], PI_4[1]))
        mw = -(z * z)
        P = np.full_like(z, INV_ODD[ATAN_TERMS - 1])
        for k in range(ATAN_TERMS - 2, 0, -1):
            P = P * mw + INV_ODD[k]
        return hi + ((z * (mw * P) + lo) + z)


def atan2(y, x):
    """finite y >= 0, finite x -> the angle in 0 .. pi; NaN outside"""
    y, x = np.broadcast_arrays(np.asarray(y, f64), np.asarray(x, f64))
    with np.errstate(all="ignore"):
        bad = ~(y >= 0.0) | ~np.isfinite(x) | ~np.isfinite(y)
        ax = np.abs(x)
        wide = ax >= y
        a = atan01(np.where(wide, y / ax, ax / y))
        flat = np.where(x > 0.0, a, PI[0] - (a - PI[1]))
        steep = np.where(x >= 0.0, PI_2[0] - (a - PI_2[1]), PI_2[0] + (a + PI_2[1]))
        out = np.where(y == 0.0, np.where(x < 0.0, PI[0], 0.0), np.where(wide, flat, steep))
        return np.where(bad, np.nan, out)


def ln(s):
    """finite s > 0 -> ln s; NaN outside"""
    s = np.asarray(s, f64)
    with np.errstate(all="ignore"):
        bad = ~(s > 0.0) | ~np.isfinite(s)
        mant, ex = np.frexp(np.where(bad, 1.0, s))
        m, e = mant * 2.0, ex - 1  # 1 <= m < 2, exact
        big = m > SQRT2
        m, e = np.where(big, m * 0.5, m), np.where(big, e + 1, e)
        f = m - 1.0
        z = f / (2.0 + f)
        w, z2, de = z * z, 2.0 * z, e.astype(f64)
        P = np.full_like(z, INV_ODD[LN_TERMS - 1])
        for k in range(LN_TERMS - 2, 0, -1):
            P = P * w + INV_ODD[k]
        return np.where(bad, np.nan, de * LN2[0] + ((z2 * (w * P) + de * LN2[1]) + z2))


# ---- Sim3: an array [13][n] ------------------------------------------------------------------------------------------------------------
def cols(S):
    """[n][13] -> [13][n]"""
    return np.ascontiguousarray(np.asarray(S, f64).reshape(-1, 13).T)


def inv(S):
    with np.errstate(all="ignore"):
        o = np.empty_like(S)
        is_ = 1.0 / S[12]
        for i in range(3):
            for j in range(3):
                o[3 * i + j] = S[3 * j + i]
            o[9 + i] = -(is_ * ((S[i] * S[9] + S[3 + i] * S[10]) + S[6 + i] * S[11]))
        o[12] = is_
    return o


def mul(A, B):
    with np.errstate(all="ignore"):
        o = np.empty(np.broadcast(A, B).shape, f64)
        for i in range(3):
            for j in range(3):
                o[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j]
            o[9 + i] = A[12] * ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i]
        o[12] = A[12] * B[12]
    return o


def usable(S):
    with np.errstate(all="ignore"):
        return (S[12] > 0.0) & np.isfinite(S).all(axis=0)


def log(E):
    """[13][n] -> e [7][n]"""
    with np.errstate(all="ignore"):
        v0, v1, v2 = 0.5 * (E[7] - E[5]), 0.5 * (E[2] - E[6]), 0.5 * (E[3] - E[1])
        c = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0)
        n = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
        th = atan2(n, c)
        f = th / n
        plain = [v0 * f, v1 * f, v2 * f]
        # next to pi
        d = 1.0 - c
        b01, b02, b12 = 0.5 * (E[1] + E[3]), 0.5 * (E[2] + E[6]), 0.5 * (E[5] + E[7])
        k0 = (E[0] >= E[4]) & (E[0] >= E[8])
        k1 = ~k0 & (E[4] >= E[8])
        p0, p1, p2 = np.sqrt((E[0] - c) / d), np.sqrt((E[4] - c) / d), np.sqrt((E[8] - c) / d)
        a0 = np.where(k0, p0, np.where(k1, b01 / (d * p1), b02 / (d * p2)))
        a1 = np.where(k0, b01 / (d * p0), np.where(k1, p1, b12 / (d * p2)))
        a2 = np.where(k0, b02 / (d * p0), np.where(k1, b12 / (d * p1), p2))
        neg = (a0 * v0 + a1 * v1) + a2 * v2 < 0.0
        a0, a1, a2 = np.where(neg, -a0, a0), np.where(neg, -a1, a1), np.where(neg, -a2, a2)
        near_pi = (c < 0.0) & (n < NEAR_PI_N)
        small = ~near_pi & (n < SMALL_N)
        w = [np.where(near_pi, a * th, np.where(small, v, p)) for a, v, p in zip((a0, a1, a2), (v0, v1, v2), plain)]
        return np.stack(w + [E[9], E[10], E[11], ln(E[12])])


def error(M, Si, Sj):
    return log(mul(mul(M, Si), inv(Sj)))


def dot7(a, b):
    with np.errstate(all="ignore"):
        return (((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5]) + a[6] * b[6]


def rotation_series(q):
    """pose_ref.series for a column of q: A and B of the rotation's exponential"""
    mq = -q
    A, B = np.full_like(q, PR.INV_FACT[2 * PR.SERIES - 1]), np.full_like(q, PR.INV_FACT[2 * PR.SERIES])
    for k in range(PR.SERIES - 2, -1, -1):
        A = A * mq + PR.INV_FACT[2 * k + 1]
        B = B * mq + PR.INV_FACT[2 * k + 2]
    return A, B


def scale_series(sigma):
    """sim3opt_ref.exp_scale for a column of sigma"""
    v = np.full_like(sigma, PR.INV_FACT[SR.SERIES - 1])
    for k in range(SR.SERIES - 2, -1, -1):
        v = v * sigma + PR.INV_FACT[k]
    return v


def retract(d, S, fix_scale):
    """d [7][n], S [13][n] -> (the retracted S, bool [n]: the step is not too large; a refused column keeps its S)"""
    with np.errstate(all="ignore"):
        w0, w1, w2 = d[0], d[1], d[2]
        s00, s11, s22 = w0 * w0, w1 * w1, w2 * w2
        q = (s00 + s11) + s22
        ok = ~(q > PR.PI2)
        if not fix_scale:
            ok &= np.abs(d[6]) <= 1.0
        A, B = rotation_series(q)
        p01, p02, p12 = w0 * w1, w0 * w2, w1 * w2
        m00, m11, m22 = -(s11 + s22), -(s00 + s22), -(s00 + s11)
        dR = [1.0 + B * m00, B * p01 - A * w2, B * p02 + A * w1, B * p01 + A * w2, 1.0 + B * m11, B * p12 - A * w0, B * p02 - A * w1, B * p12 + A * w0,
              1.0 + B * m22]
        ds = np.ones_like(q) if fix_scale else scale_series(d[6])
        o = np.empty_like(S)
        for i in range(3):
            for j in range(3):
                o[3 * i + j] = (dR[3 * i] * S[j] + dR[3 * i + 1] * S[3 + j]) + dR[3 * i + 2] * S[6 + j]
            o[9 + i] = ds * ((dR[3 * i] * S[9] + dR[3 * i + 1] * S[10]) + dR[3 * i + 2] * S[11]) + d[3 + i]
        o[12] = S[12] if fix_scale else ds * S[12]
        return np.where(ok, o, S), ok


def jacobian(M, Si, Sj, fixed_i, fixed_j, fix_scale, h=H, h2=H2):
    """-> J [14][7][n]: J[c] is column c of the 7 x 14 block, endpoint i first.  h, h2: the rule's step and its double; the tests
    form a second estimate with another step"""
    n = M.shape[1]
    J = np.zeros((14, 7, n), f64)
    with np.errstate(all="ignore"):
        for c in range(14):
            side, a = divmod(c, 7)
            zero = (fixed_j if side else fixed_i) | (fix_scale and a == 6)
            e = []
            for step in (h, -h):
                d = np.zeros((7, n), f64)
                d[a] = step
                P, _ = retract(d, Sj if side else Si, fix_scale)
                e.append(error(M, Si, P) if side else error(M, P, Sj))
            J[c] = np.where(zero, 0.0, (e[0] - e[1]) / h2)
    return J


def edge(nc_i, nc_j, s_i, s_j, fixed_i=False, fixed_j=False, fix_scale=False):
    """one edge -> (e [7], J [14][7])"""
    M = mul(cols(nc_j), inv(cols(nc_i)))
    Si, Sj = cols(s_i), cols(s_j)
    e = error(M, Si, Sj)
    J = jacobian(M, Si, Sj, np.array([bool(fixed_i)]), np.array([bool(fixed_j)]), bool(fix_scale))
    return e[:, 0], J[:, :, 0]


# ---- steps 5 and 6 ----------------------------------------------------------------------------------------------------------------------
def incidence(n_kf, edges):
    """-> (cnt [n_kf], inc [n_kf][max degree] of 2 * edge + side in ascending order, -1 beyond cnt)"""
    lists = [[] for _ in range(n_kf)]
    for e, (i, j) in enumerate(np.asarray(edges).reshape(-1, 2).tolist()):
        lists[i].append(2 * e)
        lists[j].append(2 * e + 1)
    cnt = np.array([len(v) for v in lists], np.int64)
    inc = np.full((n_kf, max(1, int(cnt.max()) if n_kf else 1)), -1, np.int64)
    for v, l in enumerate(lists):
        inc[v, :len(l)] = l
    return cnt, inc


def chol(Hm, n):
    """Hm [7][7][K], its lower triangle filled -> (the factor over it, bool [K]: every pivot > 0): ss_gn_chol_n"""
    L = Hm.copy()
    ok = np.ones(Hm.shape[2], bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = L[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            ok &= s > 0.0
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, n):
                v = L[i][j]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / L[j][j]
    return L, ok


def subst(L, n, d):
    """d [7][K] <- L^-T L^-1 d over the leading n: ss_gn_subst_n"""
    d = d.copy()
    with np.errstate(all="ignore"):
        for i in range(n):
            v = d[i]
            for k in range(i):
                v = v - L[i][k] * d[k]
            d[i] = v / L[i][i]
        for i in range(n - 1, -1, -1):
            v = d[i]
            for k in range(i + 1, n):
                v = v - L[k][i] * d[k]
            d[i] = v / L[i][i]
    return d


def blocks(J, err, cnt, inc, free, n, lam):
    """-> (L [7][7][K], dd [7][K], g [7][K], bool: every pivot of every free keyframe > 0)"""
    K = len(cnt)
    Hm, g = np.zeros((7, 7, K), f64), np.zeros((7, K), f64)
    with np.errstate(all="ignore"):
        for m in range(inc.shape[1]):
            live = free & (cnt > m)
            if not live.any():
                break
            e, side = np.where(live, inc[:, m], 0) >> 1, np.where(live, inc[:, m], 0) & 1
            Jc = [J[7 * side + a, :, e].T for a in range(7)]  # column a of the keyframe's side: [7][K]
            ee = err[:, e]
            for a in range(7):
                for b in range(a + 1):
                    Hm[a][b] = np.where(live, Hm[a][b] + dot7(Jc[a], Jc[b]), Hm[a][b])
                g[a] = np.where(live, g[a] + dot7(Jc[a], ee), g[a])
        dd = np.zeros((7, K), f64)
        for a in range(7):
            if a < n:
                dd[a] = np.where(free, f64(lam) * (1.0 + Hm[a][a]), 0.0)
            else:
                g[a] = 0.0
            Hm[a][a] = Hm[a][a] + dd[a]
        g = np.where(free, g, 0.0)
        L, ok = chol(Hm, n)
    return L, dd, g, bool((ok | ~free).all())


def dot(a, b):
    """the tree over the 7 * n_kf entries in keyframe-major order; a, b [7][K]"""
    with np.errstate(all="ignore"):
        prod = (a * b).T.reshape(-1)
    return PR.tree(prod, np.ones(len(prod), bool))


def product(J, edges, cnt, inc, free, n, dd, p):
    """q = (H + diag dd).p, matrix-free"""
    i, j = edges[:, 0], edges[:, 1]
    K = len(cnt)
    with np.errstate(all="ignore"):
        pi, pj = p[:, i], p[:, j]
        u = []
        for r in range(7):
            v = J[0, r] * pi[0]
            for c in range(1, 7):
                v = v + J[c, r] * pi[c]
            for c in range(7):
                v = v + J[7 + c, r] * pj[c]
            u.append(v)
        u = np.stack(u)
        acc = np.zeros((7, K), f64)
        for m in range(inc.shape[1]):
            live = free & (cnt > m)
            if not live.any():
                break
            e, side = np.where(live, inc[:, m], 0) >> 1, np.where(live, inc[:, m], 0) & 1
            ue = u[:, e]
            for a in range(7):
                acc[a] = np.where(live, acc[a] + dot7(J[7 * side + a, :, e].T, ue), acc[a])
        q = np.zeros((7, K), f64)
        for a in range(n):
            q[a] = np.where(free, acc[a] + dd[a] * p[a], 0.0)
    return q


def pcg(J, edges, cnt, inc, free, n, L, dd, g, tol, max_it):
    """-> (x [7][K], iterations, why it stopped: "cap", "curvature" or "tolerance")"""
    K = len(cnt)

    def precondition(r):
        return np.where(free, subst(L, n, r), r)

    with np.errstate(all="ignore"):
        x = np.zeros((7, K), f64)
        r = np.where(free, -g, 0.0)
        r[n:] = 0.0
        z = precondition(r)
        p = z.copy()
        rho = dot(r, z)
        stop = (f64(tol) * f64(tol)) * rho
        done, why = 0, "cap"
        while done < max_it:
            q = product(J, edges, cnt, inc, free, n, dd, p)
            pq = dot(p, q)
            if not pq > 0.0:
                why = "curvature"
                break
            alpha = rho / pq
            x = x + alpha * p
            r = r - alpha * q
            done += 1
            z = precondition(r)
            rho1 = dot(r, z)
            if rho1 <= stop:
                why = "tolerance"
                break
            beta = rho1 / rho
            p = z + beta * p
            rho = rho1
    return x, done, why


def cost(M, S, edges):
    e = error(M, S[:, edges[:, 0]], S[:, edges[:, 1]])
    terms = dot7(e, e)
    return PR.tree(terms, np.ones(len(terms), bool))


def pose(S):
    """[13][K] -> [K][12]: R and t / s"""
    with np.errstate(all="ignore"):
        return np.concatenate([S[:9], S[9:12] / S[12]]).T.copy()


def optimise(nc, start, fixed, edges, params=None, trace=None, solver=None):
    """one problem: nc, start [n_kf][13], fixed [n_kf], edges [n_edges][2] -> (sim3 [n_kf][13], poses [n_kf][12], one RESULT_DTYPE
    record).  trace, a list, receives one dict per step.  solver(J, err, lam) -> x replaces blocks() and pcg(): the independent
    optimiser of the tests"""
    p = dict(DEFAULTS, **(params or {}))
    N, S = cols(nc), cols(start)
    K = N.shape[1]
    free = np.asarray(fixed).reshape(-1) == 0
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    fix, n = bool(p["fix_scale"]), 6 if p["fix_scale"] else 7
    res = np.zeros(1, RESULT_DTYPE)[0]
    ok = bool((usable(N) & usable(S)).all())
    state = 2 if not ok else 1 if (not free.any() or len(edges) == 0) else 0
    lam, cost0, cost_before, steps, accepted, n_pcg = f64(p["lambda_"]), f64(0.0), f64(0.0), 0, 0, 0
    if state == 0:
        i, j = edges[:, 0], edges[:, 1]
        cnt, inc = incidence(K, edges)
        M = mul(N[:, j], inv(N[:, i]))
        cost0 = cost(M, S, edges)
        if not np.isfinite(cost0):
            state, cost0 = 2, f64(0.0)
        cost_before = cost0
    for _ in range(p["iterations"]):
        if state != 0:
            break
        Si, Sj = S[:, i], S[:, j]
        err = error(M, Si, Sj)
        J = jacobian(M, Si, Sj, ~free[i], ~free[j], fix)
        if solver is None:
            L, dd, g, pivots = blocks(J, err, cnt, inc, free, n, lam)
            if not pivots:
                state = 2
                break
            x, done, why = pcg(J, edges, cnt, inc, free, n, L, dd, g, p["pcg_tol"], p["pcg_iterations"])
        else:
            x, done, why = solver(J, err, lam), 0, "direct"
        n_pcg += done
        T, fits = retract(x, S, fix)
        T = np.where(free, T, S)
        if not (fits | ~free).all():
            state = 4
            break
        cost1 = cost(M, T, edges)
        accept = bool(np.isfinite(T).all() and np.isfinite(cost1) and cost1 <= cost0)
        steps += 1
        lam_before = lam
        with np.errstate(all="ignore"):
            lam = max(lam / f64(p["lambda_factor"]), f64(p["lambda_min"])) if accept else lam * f64(p["lambda_factor"])
        if trace is not None:
            trace.append(dict(accepted=accept, cost=cost1, lambda_=lam, lambda_before=lam_before, pcg=done, why=why, x=x.T.copy(), before=S.T.copy()))
        if accept:
            accepted, cost0, S = accepted + 1, cost1, T
    res["lambda_"], res["cost_before"], res["cost_after"] = lam, cost_before, cost0
    res["state"], res["n_edges"], res["n_free"], res["steps"], res["accepted"], res["pcg_iterations"] = state, len(edges), int(free.sum()), steps, accepted, n_pcg
    return S.T.copy(), pose(S), res


def points(xyz, ref, nc, sim3):
    """xyz float32 [P][3], ref [P] -> float32 [P][3]: x <- S_r^-1(N_r(x)) where 0 <= ref < n_kf, in double, rounded once"""
    xyz = np.asarray(xyz, np.float32)
    ref = np.asarray(ref, np.int64).reshape(-1)
    N, S = cols(nc), cols(sim3)
    live = (ref >= 0) & (ref < N.shape[1])
    r = np.where(live, ref, 0)
    N, S = N[:, r], S[:, r]
    x = [xyz[:, k].astype(f64) for k in range(3)]
    with np.errstate(all="ignore"):
        d = [(N[12] * ((N[3 * i] * x[0] + N[3 * i + 1] * x[1]) + N[3 * i + 2] * x[2]) + N[9 + i]) - S[9 + i] for i in range(3)]
        is_ = 1.0 / S[12]
        out = np.stack([is_ * ((S[i] * d[0] + S[3 + i] * d[1]) + S[6 + i] * d[2]) for i in range(3)], axis=1).astype(np.float32)
    return np.where(live[:, None], out, xyz)
