"""The two-view initialisation restated in numpy scalars, one IEEE double operation per step in the order include/sendslam_orb.h
writes them (test infrastructure, plain module; the normative statement of the rule).  Nothing here calls the library: the host twins
and, through them, the kernels are held to this text bit for bit by tests/test_two_view_ref.py.

    tree_sum      THE TREE of step 2: chunks of 256, halving folds of 64, (g0 + g1) + (g2 + g3), chunks in ascending order
    normalise     step 2
    model_of      step 3 of one octuple -> (H21, H12, F21, ok_h, ok_f)
    term_h/term_f step 4 of one correspondence
    svd3, decompose_f, decompose_h   step 7
    check_rt, map_point              step 8
    pick, accept                     steps 8 and 9 on counts
    solve         the whole rule for one problem -> (flags per row, points, point rows, result record, per-hypothesis scores)
"""
from __future__ import annotations

import struct

import numpy as np

import pnp_ref

F = np.float64
f32 = np.float32
ZERO, ONE = F(0.0), F(1.0)
DRAWS, SWEEPS3, SWEEPS4, INVERSE_STEPS = 8, 8, 6, 6
SHIFT, COS_TRI, TH2, MIN_DET = F(1e-13), F(0.99998), F(4.0), F(1e-300)
MAX_ITERATIONS = 1024
COS_1DEG = 0.9998476951563913
RESULT_DTYPE = np.dtype([("r21", "<f8", (9,)), ("t21", "<f8", (3,)), ("score_h", "<f8"), ("score_f", "<f8"), ("cos_parallax", "<f8")] +
                        [(n, "<i4") for n in ("state", "reason", "status", "model", "iteration_h", "iteration_f", "n_corr", "n_inliers", "n_good",
                                              "n_triangulated")] + [("reserved", "<i4", (8,))])
MAP_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
UPSTREAM = dict(chi2_h=5.991, chi2_f=3.841, chi2_score=5.991, rh_threshold=0.45, cos_min_parallax=COS_1DEG, min_triangulated=50, max_iterations=200, seed=0)


def finite(x):
    return x - x == 0.0


def draw(seed, problem, t, n):
    return pnp_ref.draw(seed, problem, t, n, DRAWS)


def tree_sum(terms):
    """terms: a list of np.float64"""
    n = len(terms)
    total = ZERO
    c0 = 0
    while c0 < n or c0 == 0:
        a = [terms[c0 + s] if c0 + s < n else ZERO for s in range(256)]
        for g in range(0, 256, 64):
            h = 32
            while h >= 1:
                for lane in range(h):
                    a[g + lane] = a[g + lane] + a[g + lane + h]
                h >>= 1
        v = (a[0] + a[64]) + (a[128] + a[192])
        total = v if c0 == 0 else total + v
        c0 += 256
    return total


def normalise(corr):
    """corr: n x 4 float32 -> (m[4], d[4])"""
    n = len(corr)
    m, d = [], []
    for c in range(4):
        col = [F(x) for x in corr[:, c]]
        mc = tree_sum(col) / F(n)
        m.append(mc)
        d.append(tree_sum([abs(x - mc) for x in col]) / F(n))
    return m, d


def norm_ok(m, d):
    return all(d[k] > 0.0 and finite(d[k]) and finite(m[k]) for k in range(4))


def tri(i, j):
    return i * (i + 1) // 2 + j


def chol(w, n):
    ok = True
    for j in range(n):
        s = w[tri(j, j)]
        for k in range(j):
            s = s - w[tri(j, k)] * w[tri(j, k)]
        ok = ok and bool(s > 0.0)
        d = np.sqrt(s)
        w[tri(j, j)] = d
        for i in range(j + 1, n):
            v = w[tri(i, j)]
            for k in range(j):
                v = v - w[tri(i, k)] * w[tri(j, k)]
            w[tri(i, j)] = v / d
    return ok


def inverse_step(w, x, n):
    for i in range(n):
        v = x[i]
        for k in range(i):
            v = v - w[tri(i, k)] * x[k]
        x[i] = v / w[tri(i, i)]
    for i in range(n - 1, -1, -1):
        v = x[i]
        for k in range(i + 1, n):
            v = v - w[tri(k, i)] * x[k]
        x[i] = v / w[tri(i, i)]
    s = x[0] * x[0]
    for k in range(1, n):
        s = s + x[k] * x[k]
    nrm = np.sqrt(s)
    for k in range(n):
        x[k] = x[k] / nrm


def null9(w):
    trace = w[0]
    for k in range(1, 9):
        trace = trace + w[tri(k, k)]
    shift = SHIFT * trace
    for k in range(9):
        w[tri(k, k)] = w[tri(k, k)] + shift
    ok = chol(w, 9)
    x = [ONE / F(3.0)] * 9
    for _ in range(INVERSE_STEPS):
        inverse_step(w, x, 9)
    return ok, x


def mul3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def t3(a):
    return [a[3 * j + i] for i in range(3) for j in range(3)]


def det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def inv3(m):
    d = det3(m)
    i = ONE / d
    o = [(m[4] * m[8] - m[5] * m[7]) * i, (m[2] * m[7] - m[1] * m[8]) * i, (m[1] * m[5] - m[2] * m[4]) * i,
         (m[5] * m[6] - m[3] * m[8]) * i, (m[0] * m[8] - m[2] * m[6]) * i, (m[2] * m[3] - m[0] * m[5]) * i,
         (m[3] * m[7] - m[4] * m[6]) * i, (m[1] * m[6] - m[0] * m[7]) * i, (m[0] * m[4] - m[1] * m[3]) * i]
    return bool(abs(d) > MIN_DET), o


def rotate(M, V, p, q, n):
    """one Jacobi rotation on the symmetric n x n M and the vectors V (ss_tri_rotate)"""
    apq = M[p][q]
    if apq != 0.0:
        theta = (M[q][q] - M[p][p]) / (F(2.0) * apq)
        t = (ONE if theta >= 0.0 else -ONE) / (abs(theta) + np.sqrt(theta * theta + ONE))
        c = ONE / np.sqrt(t * t + ONE)
        s = t * c
        for k in range(n):
            if k == p or k == q:
                continue
            akp, akq = M[k][p], M[k][q]
            M[k][p] = M[p][k] = c * akp - s * akq
            M[k][q] = M[q][k] = s * akp + c * akq
        M[p][p] = M[p][p] - t * apq
        M[q][q] = M[q][q] + t * apq
        M[p][q] = M[q][p] = ZERO
        for k in range(n):
            vkp, vkq = V[k][p], V[k][q]
            V[k][p] = c * vkp - s * vkq
            V[k][q] = s * vkp + c * vkq


def eig_ata(A):
    """A: 9 entries row-major -> (e[3], V 3 x 3 with the eigenvectors in its columns)"""
    M = [[ZERO] * 3 for _ in range(3)]
    V = [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(i, 3):
            M[i][j] = M[j][i] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j]
    for _ in range(SWEEPS3):
        rotate(M, V, 0, 1, 3)
        rotate(M, V, 0, 2, 3)
        rotate(M, V, 1, 2, 3)
    return [M[0][0], M[1][1], M[2][2]], V


def smallest(e):
    best, low = 0, e[0]
    for k in range(1, len(e)):
        if e[k] < low:
            best, low = k, e[k]
    return best


def model_of(uv, pick, m, d):
    """uv: 8 x 4 float32 in draw order, pick: their correspondence numbers -> (h21, h12, f21, ok_h, ok_f), lists of 9"""
    with np.errstate(all="ignore"):
        s = [ONE / d[c] for c in range(4)]
        p = [[(F(uv[k][c]) - m[c]) * s[c] for c in range(4)] for k in range(DRAWS)]
        T1 = [s[0], ZERO, -m[0] * s[0], ZERO, s[1], -m[1] * s[1], ZERO, ZERO, ONE]
        T2 = [s[2], ZERO, -m[2] * s[2], ZERO, s[3], -m[3] * s[3], ZERO, ZERO, ONE]
        T2inv = [d[2], ZERO, m[2], ZERO, d[3], m[3], ZERO, ZERO, ONE]
        distinct = len(set(int(v) for v in pick)) == DRAWS
        w = [ZERO] * 45
        for k in range(DRAWS):
            u1, v1, u2, v2 = p[k]
            ra = [ZERO, ZERO, ZERO, -u1, -v1, -ONE, v2 * u1, v2 * v1, v2]
            rb = [u1, v1, ONE, ZERO, ZERO, ZERO, -(u2 * u1), -(u2 * v1), -u2]
            for i in range(9):
                for j in range(i + 1):
                    term = ra[i] * ra[j] + rb[i] * rb[j]
                    w[tri(i, j)] = term if k == 0 else w[tri(i, j)] + term
        ok, x = null9(w)
        h21 = mul3(mul3(T2inv, x), T1)
        inv_ok, h12 = inv3(h21)
        ok_h = inv_ok and ok and distinct and all(finite(v) for v in h21) and all(finite(v) for v in h12)
        w = [ZERO] * 45
        for k in range(DRAWS):
            u1, v1, u2, v2 = p[k]
            r = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, ONE]
            for i in range(9):
                for j in range(i + 1):
                    term = r[i] * r[j]
                    w[tri(i, j)] = term if k == 0 else w[tri(i, j)] + term
        ok, x = null9(w)
        e, V = eig_ata(x)
        b = smallest(e)
        v = [V[r_][b] for r_ in range(3)]
        for r_ in range(3):
            fv = (x[3 * r_] * v[0] + x[3 * r_ + 1] * v[1]) + x[3 * r_ + 2] * v[2]
            for c in range(3):
                x[3 * r_ + c] = x[3 * r_ + c] - fv * v[c]
        f21 = mul3(mul3(t3(T2), x), T1)
        ok_f = ok and distinct and all(finite(v_) for v_ in f21)
    zero = [ZERO] * 9
    return (h21 if ok_h else zero, h12 if ok_h else zero, f21 if ok_f else zero, int(bool(ok_h)), int(bool(ok_f)))


def term_h(H21, H12, u1, v1, u2, v2, th):
    """-> (contribution, inlier, chi_a, chi_b)"""
    with np.errstate(all="ignore"):
        w21 = ONE / ((H12[6] * u2 + H12[7] * v2) + H12[8])
        a, b = ((H12[0] * u2 + H12[1] * v2) + H12[2]) * w21, ((H12[3] * u2 + H12[4] * v2) + H12[5]) * w21
        chi0 = (u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)
        w12 = ONE / ((H21[6] * u1 + H21[7] * v1) + H21[8])
        c, d = ((H21[0] * u1 + H21[1] * v1) + H21[2]) * w12, ((H21[3] * u1 + H21[4] * v1) + H21[5]) * w12
        chi1 = (u2 - c) * (u2 - c) + (v2 - d) * (v2 - d)
        in0, in1 = bool(chi0 <= th), bool(chi1 <= th)
        return ((th - chi0 if in0 else ZERO) + (th - chi1 if in1 else ZERO)), in0 and in1, chi0, chi1


def term_f(Fm, u1, v1, u2, v2, th, th_score):
    with np.errstate(all="ignore"):
        a2, b2, c2 = (Fm[0] * u1 + Fm[1] * v1) + Fm[2], (Fm[3] * u1 + Fm[4] * v1) + Fm[5], (Fm[6] * u1 + Fm[7] * v1) + Fm[8]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi0 = (num2 * num2) / (a2 * a2 + b2 * b2)
        a1, b1, c1 = (Fm[0] * u2 + Fm[3] * v2) + Fm[6], (Fm[1] * u2 + Fm[4] * v2) + Fm[7], (Fm[2] * u2 + Fm[5] * v2) + Fm[8]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi1 = (num1 * num1) / (a1 * a1 + b1 * b1)
        in0, in1 = bool(chi0 <= th), bool(chi1 <= th)
        return ((th_score - chi0 if in0 else ZERO) + (th_score - chi1 if in1 else ZERO)), in0 and in1, chi0, chi1


def beats(score, t, best, best_t):
    return bool(score > best) or (bool(score == best) and t < best_t)


def choose(sh, sf, rh_threshold):
    if not sh > 0.0 and not sf > 0.0:
        return 0
    h, f = (sh if sh > 0.0 else ZERO), (sf if sf > 0.0 else ZERO)
    return 2 if h / (h + f) > rh_threshold else 1


def svd3(A):
    """-> (U[9], s[3], V[9]) row-major"""
    with np.errstate(all="ignore"):
        e, Ve = eig_ata(A)
        order = [(e[0], 0), (e[1], 1), (e[2], 2)]
        for a, b in ((0, 1), (1, 2), (0, 1)):
            if order[b][0] > order[a][0]:
                order[a], order[b] = order[b], order[a]
        s = [np.sqrt(v if v > 0.0 else ZERO) for v, _ in order]
        v = [[Ve[r][i] for r in range(3)] for _, i in order]
        V, U = [ZERO] * 9, [ZERO] * 9
        u = [[(A[3 * r] * v[k][0] + A[3 * r + 1] * v[k][1]) + A[3 * r + 2] * v[k][2] for r in range(3)] for k in range(3)]
        for k in range(3):
            for r in range(3):
                V[3 * r + k] = v[k][r]
        for k in range(2):
            n = np.sqrt((u[k][0] * u[k][0] + u[k][1] * u[k][1]) + u[k][2] * u[k][2])
            for r in range(3):
                U[3 * r + k] = u[k][r] / n
        c0, c1, c2 = U[3] * U[7] - U[6] * U[4], U[6] * U[1] - U[0] * U[7], U[0] * U[4] - U[3] * U[1]
        if (c0 * u[2][0] + c1 * u[2][1]) + c2 * u[2][2] < 0.0:
            c0, c1, c2 = -c0, -c1, -c2
        U[2], U[5], U[8] = c0, c1, c2
        return U, s, V


def _K(cam):
    fx, fy, cx, cy = (F(f32(v)) for v in cam)
    return fx, fy, cx, cy


def decompose_f(Fm, cam):
    """-> the four (R[9], t[3])"""
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _K(cam)
        K = [fx, ZERO, cx, ZERO, fy, cy, ZERO, ZERO, ONE]
        E = mul3(mul3(t3(K), Fm), K)
        U, s, V = svd3(E)
        Vt = t3(V)
        tn = np.sqrt((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8])
        t = [U[2] / tn, U[5] / tn, U[8] / tn]
        W = [ZERO, -ONE, ZERO, ONE, ZERO, ZERO, ZERO, ZERO, ONE]
        Wt = [ZERO, ONE, ZERO, -ONE, ZERO, ZERO, ZERO, ZERO, ONE]
        R1, R2 = mul3(mul3(U, W), Vt), mul3(mul3(U, Wt), Vt)
        if det3(R1) < 0.0:
            R1 = [-v for v in R1]
        if det3(R2) < 0.0:
            R2 = [-v for v in R2]
        nt = [-v for v in t]
        return [(R1, t), (R2, t), (R1, nt), (R2, nt)]


def decompose_h(H, cam):
    """-> the eight (R, t), or [] when the singular values refuse"""
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _K(cam)
        K = [fx, ZERO, cx, ZERO, fy, cy, ZERO, ZERO, ONE]
        ifx, ify = ONE / fx, ONE / fy
        Kinv = [ifx, ZERO, -cx * ifx, ZERO, ify, -cy * ify, ZERO, ZERO, ONE]
        A = mul3(mul3(Kinv, H), K)
        U, w, V = svd3(A)
        Vt = t3(V)
        sgn = det3(U) * det3(Vt)
        d1, d2, d3 = w
        if not (d1 / d2 >= 1.00001 and d2 / d3 >= 1.00001):
            return []
        q12, q23, q13 = d1 * d1 - d2 * d2, d2 * d2 - d3 * d3, d1 * d1 - d3 * d3
        aux1, aux3 = np.sqrt(q12 / q13), np.sqrt(q23 / q13)
        root = np.sqrt(q12 * q23)
        aux_st, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        aux_sp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        out = []
        for i in range(8):
            j, pos = i & 3, i < 4
            x1 = aux1 if j < 2 else -aux1
            x3 = -aux3 if j & 1 else aux3
            st = aux_st if j in (0, 3) else -aux_st
            sp = aux_sp if j in (0, 3) else -aux_sp
            Rp = [ct if pos else cp, ZERO, -st if pos else sp, ZERO, ONE if pos else -ONE, ZERO, st if pos else sp, ZERO, ct if pos else -cp]
            R = [sgn * v for v in mul3(mul3(U, Rp), Vt)]
            scale = d1 - d3 if pos else d1 + d3
            tp0, tp2 = x1 * scale, (-x3 if pos else x3) * scale
            tt = [(U[3 * r] * tp0 + U[3 * r + 1] * ZERO) + U[3 * r + 2] * tp2 for r in range(3)]
            n = np.sqrt((tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2])
            out.append((R, [v / n for v in tt]))
        return out


def null4(A):
    M = [[ZERO] * 4 for _ in range(4)]
    V = [[ONE if i == j else ZERO for j in range(4)] for i in range(4)]
    for i in range(4):
        for j in range(i, 4):
            M[i][j] = M[j][i] = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j]
    for _ in range(SWEEPS4):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            rotate(M, V, p, q, 4)
    b = smallest([M[k][k] for k in range(4)])
    return [V[k][b] for k in range(4)]


def check_rt(R, t, cam, u1, v1, u2, v2):
    """-> (good, dict X n2 d1 d2 cos e1 e2); e1, e2: the squared reprojection errors where they were formed, else None"""
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _K(cam)
        a1, b1, a2, b2 = (u1 - cx) / fx, (v1 - cy) / fy, (u2 - cx) / fx, (v2 - cy) / fy
        A = [[-ONE, ZERO, a1, ZERO], [ZERO, -ONE, b1, ZERO], [ZERO] * 4, [ZERO] * 4]
        for k in range(4):
            p0, p1, p2 = (R[k], R[3 + k], R[6 + k]) if k < 3 else (t[0], t[1], t[2])
            A[2][k] = a2 * p2 - p0
            A[3][k] = b2 * p2 - p1
        v = null4(A)
        o = dict(X=[ZERO] * 3, n2=[ZERO] * 3, d1=ZERO, d2=ZERO, cos=ZERO, e1=None, e2=None)
        if not (abs(v[3]) <= 1.7976931348623157e308 and v[3] != 0.0):
            return False, o
        X0, X1, X2 = v[0] / v[3], v[1] / v[3], v[2] / v[3]
        if not (finite(X0) and finite(X1) and finite(X2)):
            return False, o
        O2 = [-((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]) for k in range(3)]
        n0, n1, n2 = X0 - O2[0], X1 - O2[1], X2 - O2[2]
        d1, d2 = np.sqrt((X0 * X0 + X1 * X1) + X2 * X2), np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        cosp = ((X0 * n0 + X1 * n1) + X2 * n2) / (d1 * d2)
        if not finite(cosp):
            return False, o
        o.update(X=[X0, X1, X2], n2=[n0, n1, n2], d1=d1, d2=d2, cos=cosp)
        if not (X2 > 0.0 or cosp >= COS_TRI):
            return False, o
        Y0, Y1 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0], ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1]
        Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2]
        if not (Y2 > 0.0 or cosp >= COS_TRI):
            return False, o
        e1x, e1y = ((fx * X0) / X2 + cx) - u1, ((fy * X1) / X2 + cy) - v1
        o["e1"] = e1x * e1x + e1y * e1y
        if not o["e1"] <= TH2:
            return False, o
        e2x, e2y = ((fx * Y0) / Y2 + cx) - u2, ((fy * Y1) / Y2 + cy) - v2
        o["e2"] = e2x * e2x + e2y * e2y
        if not o["e2"] <= TH2:
            return False, o
        return True, o


def triangulated(cosp):
    return bool(cosp < COS_TRI)


def map_point(o, s1, s_last):
    with np.errstate(all="ignore"):
        X, n2, d1, d2 = o["X"], o["n2"], o["d1"], o["d2"]
        max_dist = d1 * F(f32(s1))
        nrm = [(X[k] / d1 + n2[k] / d2) / F(2.0) for k in range(3)]
        return tuple(f32(v) for v in (X[0], X[1], X[2], nrm[0], nrm[1], nrm[2], max_dist / F(f32(s_last)), max_dist))


def key(x):
    b = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | 0x8000000000000000)


def parallax(cosines):
    """the element at index min(50, n - 1) of the ascending cosines (-0.0 below +0.0)"""
    s = sorted(cosines, key=key)
    return s[min(50, len(s) - 1)]


def pick(good):
    best, best_good, second = -1, 0, 0
    for k, g in enumerate(good):
        if g > best_good:
            second, best_good, best = best_good, g, k
        elif g > second:
            second = g
    return best, best_good, second


def accept(model, good, best_good, second_good, n_in, cosp, p):
    """0 accepted, else the reason"""
    if best_good < 1:
        return 2
    if model == 2:
        if not (best_good > p["min_triangulated"] and F(best_good) > F(0.9) * F(n_in)):
            return 2
        if not F(second_good) < F(0.75) * F(best_good):
            return 3
        return 0 if cosp <= F(p["cos_min_parallax"]) else 4
    floor_n = max(int(F(0.9) * F(n_in)), p["min_triangulated"])
    if not best_good >= floor_n:
        return 2
    if not sum(1 for g in good if F(g) > F(0.7) * F(best_good)) <= 1:
        return 3
    return 0 if cosp < F(p["cos_min_parallax"]) else 4


def correspondences(kp1, kp2, idx, n_levels):
    """step 1 -> (corr n x 4 float32, the rows of frame 1)"""
    rows = [i for i in range(len(kp1)) if 0 <= idx[i] < len(kp2) and 0 <= kp1["octave"][i] < n_levels]
    corr = np.array([[kp1["x"][i], kp1["y"][i], kp2["x"][idx[i]], kp2["y"][idx[i]]] for i in rows], f32).reshape(len(rows), 4)
    return corr, rows


def hypothesis(corr, m, d, seed, problem, t):
    pk = draw(seed, problem, t, len(corr))
    return model_of(corr[pk], pk, m, d)


def solve(view, kp1, kp2, idx, scale, problem=0, status=0, **params):
    """the whole rule -> (flag uint8 [n1], points, point rows (k x 2 int32), one RESULT_DTYPE record, [(score_h, score_f)] per t)"""
    p = dict(UPSTREAM, **params)
    cam = (view["fx"], view["fy"], view["cx"], view["cy"])
    cam = tuple(np.asarray(v).reshape(-1)[0] for v in cam)
    corr, rows = correspondences(kp1, kp2, idx, len(scale)) if status == 0 else (np.zeros((0, 4), f32), [])
    n = len(rows)
    res = np.zeros(1, RESULT_DTYPE)[0]
    res["state"], res["status"], res["n_corr"], res["iteration_h"], res["iteration_f"] = 1, status, n, -1, -1
    flag = np.zeros(len(kp1), np.uint8)
    flag[rows] = 1
    none = (np.zeros(0, MAP_POINT_DTYPE), np.zeros((0, 2), np.int32))
    if n < DRAWS:
        return (flag,) + none + (res, [])
    res["state"] = 2
    m, d = normalise(corr)
    if not norm_ok(m, d):
        return (flag,) + none + (res, [])
    c64 = [[F(v) for v in row] for row in corr]
    th_h, th_f, th_s = F(p["chi2_h"]), F(p["chi2_f"]), F(p["chi2_score"])
    sh, sf, it_h, it_f, scores = F(-1.0), F(-1.0), -1, -1, []
    for t in range(p["max_iterations"]):
        h21, h12, f21, ok_h, ok_f = hypothesis(corr, m, d, p["seed"], problem, t)
        h = tree_sum([term_h(h21, h12, *c, th_h)[0] for c in c64]) if ok_h else F(-1.0)
        f = tree_sum([term_f(f21, *c, th_f, th_s)[0] for c in c64]) if ok_f else F(-1.0)
        scores.append((float(h), float(f)))
        if it_h < 0 or beats(h, t, sh, it_h):
            sh, it_h = h, t
        if it_f < 0 or beats(f, t, sf, it_f):
            sf, it_f = f, t
    res["score_h"], res["score_f"], res["iteration_h"], res["iteration_f"] = sh, sf, it_h, it_f
    model = choose(sh, sf, F(p["rh_threshold"]))
    if model == 0:
        return (flag,) + none + (res, scores)
    res["model"], res["state"] = model, 3
    h21, h12, f21, _, _ = hypothesis(corr, m, d, p["seed"], problem, it_h if model == 2 else it_f)
    inl = [term_h(h21, h12, *c, th_h)[1] if model == 2 else term_f(f21, *c, th_f, th_s)[1] for c in c64]
    n_in = sum(inl)
    res["n_inliers"] = n_in
    reason, hyps, good, best, best_good, second, cosp = 0, [], [], -1, 0, 0, ZERO
    if n_in < DRAWS:
        reason = 2
    else:
        hyps = decompose_h(h21, cam) if model == 2 else decompose_f(f21, cam)
        if not hyps:
            reason = 1
        else:
            good = [sum(1 for k in range(n) if inl[k] and check_rt(R, t, cam, *c64[k])[0]) for R, t in hyps]
            best, best_good, second = pick(good)
    checked = {}
    if best >= 0:
        checked = {k: check_rt(hyps[best][0], hyps[best][1], cam, *c64[k]) for k in range(n) if inl[k]}
        cosp = parallax([o["cos"] for g, o in checked.values() if g])
    if reason == 0:
        reason = accept(model, good, best_good, second, n_in, cosp, p)
    res["reason"], res["n_good"], res["cos_parallax"] = reason, best_good, cosp
    if reason != 0:
        return (flag,) + none + (res, scores)
    res["state"] = 0
    res["r21"], res["t21"] = hyps[best][0], hyps[best][1]
    pts, prow = [], []
    for k in range(n):
        if inl[k]:
            g, o = checked[k]
            tri_ = g and triangulated(o["cos"])
            flag[rows[k]] = 3 if tri_ else 2
            if tri_:
                pts.append(map_point(o, scale[kp1["octave"][rows[k]]], scale[len(scale) - 1]))
                prow.append((rows[k], idx[rows[k]]))
    res["n_triangulated"] = len(pts)
    return flag, np.array(pts, MAP_POINT_DTYPE).reshape(len(pts)), np.array(prow, np.int32).reshape(len(pts), 2), res, scores
