"""Synthetic pose graphs for the essential-graph optimisation (test infrastructure, plain module): ground-truth Sim3s, a drifted start, the
shared cases of the CPU and the GPU suite, the ladders, and the stacking of several problems into one call.  A problem is a dict: nc,
start [n_kf][13] float64, fixed uint8 [n_kf], edges int32 [n_edges][2], truth [n_kf][13] or None."""
from __future__ import annotations

import functools

import numpy as np

import graph_ref as GR

f64 = np.float64


def rotation(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def sim3(w, t, s=1.0):
    return np.concatenate([rotation(w).reshape(-1), np.asarray(t, f64), [f64(s)]])


def ring(n, chords=()):
    return [(v, (v + 1) % n) for v in range(n if n > 2 else 1)] + list(chords)


def make_problem(seed, n_kf, edges, drift=0.02, scale_drift=0.01, fixed=(0,), fix_scale=False, clash=0.0):
    """ground truth G, nc = G (consistent measurements), the start drifting away from G along the keyframe numbers (a random walk in the
    increment of the retraction), the fixed keyframes at their truth.  clash: the fixed keyframes after the first get a start that
    disagrees with the measurements by about that much, so no state has cost 0 (truth: None)"""
    rng = np.random.default_rng(seed)
    G = np.stack([sim3(rng.normal(0, 0.6, 3), rng.normal(0, 3.0, 3), 1.0 if fix_scale else np.exp(rng.normal(0, 0.15))) for _ in range(n_kf)])
    start, walk = G.copy(), np.zeros(7)
    for v in range(n_kf):
        walk = walk + rng.normal(0, 1.0, 7) * np.array([drift] * 6 + [0.0 if fix_scale else scale_drift])
        if v not in fixed:
            start[v] = GR.retract(walk.reshape(7, 1), GR.cols(G[v]), fix_scale)[0][:, 0]
        elif clash and v != fixed[0]:
            d = rng.normal(0, clash, 7) * np.array([1] * 6 + [0.0 if fix_scale else 0.5])
            start[v] = GR.retract(d.reshape(7, 1), GR.cols(G[v]), fix_scale)[0][:, 0]
    fx = np.zeros(n_kf, np.uint8)
    fx[list(fixed)] = 1
    return dict(nc=G.copy(), start=start, fixed=fx, edges=np.asarray(edges, np.int32).reshape(-1, 2), truth=None if clash else G, fix_scale=fix_scale)


def random_edges(seed, n_kf, n_edges):
    """a chain first (as far as the count goes), then random pairs, duplicates allowed"""
    rng = np.random.default_rng(seed)
    edges = [(v, v + 1) for v in range(min(n_kf - 1, n_edges))]
    while len(edges) < n_edges:
        i, j = rng.integers(0, n_kf, 2)
        if i != j:
            edges.append((int(i), int(j)))
    return edges


CASES = [
    dict(name="ring40_two_chords", make=lambda: make_problem(1, 40, ring(40, [(3, 22), (11, 31)])), params={}),
    dict(name="chain30_one_loop_edge", make=lambda: make_problem(2, 30, [(v, v + 1) for v in range(29)] + [(29, 0)], fixed=(29,)), params={}),
    dict(name="two_loops_sharing_keyframes", make=lambda: make_problem(3, 24, ring(14) + [(v, v + 1) for v in range(10, 23)] + [(23, 10)], fixed=(12,)), params={}),
    dict(name="fix_scale_ring20", make=lambda: make_problem(4, 20, ring(20, [(2, 12)]), fix_scale=True), params=dict(fix_scale=True)),
    dict(name="noisy_ring20_two_fixed", make=lambda: make_problem(5, 20, ring(20, [(4, 15)]), fixed=(0, 10), clash=0.05), params={}),
]
CASE_NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_problem(k):
    return CASES[k]["make"]()


def solve(pr, params=None, trace=None):
    return GR.optimise(pr["nc"], pr["start"], pr["fixed"], pr["edges"], params, trace)


@functools.lru_cache(maxsize=None)
def reference(k):
    trace = []
    return solve(case_problem(k), CASES[k]["params"], trace) + (trace,)


def vertex_ladder(n_kf):
    return make_problem(100 + n_kf, n_kf, ring(n_kf, [(0, n_kf // 2)] if n_kf > 4 else []), drift=0.01)


def edge_ladder(n_edges):
    n_kf = max(2, min(n_edges + 1, 40))
    return make_problem(200 + n_edges, n_kf, random_edges(300 + n_edges, n_kf, n_edges), drift=0.01)


def star(degree=300):
    """a hub of the given degree, free; leaf 1 is fixed"""
    return make_problem(400, degree + 1, [(0, v) if v % 2 else (v, 0) for v in range(1, degree + 1)], drift=0.002, scale_drift=0.001, fixed=(1,))


def failure_cases():
    """the odd problems of both suites by name: what each one is for stands next to it"""
    base = make_problem(21, 12, ring(12, [(2, 7)]), drift=0.01)
    all_fixed = dict(base, fixed=np.ones(12, np.uint8))
    two_fixed = make_problem(22, 12, ring(12), fixed=(0, 6), drift=0.01)
    dup = dict(base, edges=np.concatenate([base["edges"], base["edges"][:3]]))
    nan_start = dict(base, start=base["start"].copy())
    nan_start["start"][5, 10] = np.nan
    bad_scale = dict(base, nc=base["nc"].copy())
    bad_scale["nc"][3, 12] = 0.0
    half = dict(base, start=base["start"].copy())  # the error rotation of edge (0, 1) is exactly pi
    turn = GR.cols(sim3((0, 0, 0), (0, 0, 0), 1.0))
    turn[[0, 4]] = -1.0
    half["start"][1] = GR.mul(turn, GR.cols(half["nc"][1]))[:, 0]
    far = dict(base, start=base["start"].copy())  # a start so far off that the first step exceeds pi
    far["start"][4] = sim3((0.3, 2.9, -0.4), (40.0, -30.0, 20.0), 3.0)
    far["start"][8] = sim3((-2.7, 0.1, 1.0), (-30.0, 10.0, 5.0), 0.2)
    no_edges = dict(base, edges=np.zeros((0, 2), np.int32))
    return dict(all_fixed=all_fixed, two_fixed=two_fixed, duplicate_edges=dup, nan_start=nan_start, bad_scale=bad_scale, half_turn=half, far_start=far,
                no_edges=no_edges)


def correct_loop(seed=50, n_kf=24, group=3, fix_group=True):
    """A problem built the way INTEGRATION.md N prescribes for LoopClosing::CorrectLoop: a trajectory whose odometry drifted, so that
    the current keyframe c = n_kf - 1 meets the loop keyframe m = 0 again with a non-corrected pose that disagrees with what the loop
    detection measured (S_cm, scale 1.03).  nc: every pose before the correction, s = 1.  corrected[c] = S_cm . nc[m]; the last `group`
    keyframes (c's covisibility group) start at (nc[v] . nc[c]^-1) . corrected[c], the others at nc.  Edges: the chain, the loop edge
    (c, m) and a few covisibility chords.  fix_group: m AND the corrected group are fixed, as the section says; without it only m
    is, and the zero-cost state is the non-corrected map.  -> the problem, with "corrected" [n_kf][13] (the group's rows filled)"""
    rng = np.random.default_rng(seed)
    G = np.stack([sim3((0.0, 2 * np.pi * v / n_kf, 0.05 * np.sin(v)), (3.0 * np.cos(2 * np.pi * v / n_kf), 0.1 * v, 3.0 * np.sin(2 * np.pi * v / n_kf))) for v in range(n_kf)])
    nc, walk = G.copy(), np.zeros(7)
    for v in range(1, n_kf):
        walk = walk + rng.normal(0, 1.0, 7) * np.array([0.004] * 3 + [0.02] * 3 + [0.0])
        nc[v] = GR.retract(walk.reshape(7, 1), GR.cols(G[v]), True)[0][:, 0]
    c, m = n_kf - 1, 0
    s_cm = GR.mul(GR.cols(G[c]), GR.inv(GR.cols(G[m])))
    s_cm[9:12] *= 1.03  # a monocular map: the loop also measures the scale the odometry lost
    s_cm[12] = 1.03
    corrected = np.zeros_like(nc)
    corrected[c] = GR.mul(s_cm, GR.cols(nc[m]))[:, 0]
    start = nc.copy()
    members = list(range(n_kf - group, n_kf))
    for v in members:
        corrected[v] = GR.mul(GR.mul(GR.cols(nc[v]), GR.inv(GR.cols(nc[c]))), GR.cols(corrected[c]))[:, 0]
        start[v] = corrected[v]
    fixed = np.zeros(n_kf, np.uint8)
    fixed[[m] + (members if fix_group else [])] = 1
    edges = [(v, v + 1) for v in range(n_kf - 1)] + [(c, m)] + [(v, v + 3) for v in range(0, n_kf - 3, 4)]
    return dict(nc=nc, start=start, fixed=fixed, edges=np.asarray(edges, np.int32), truth=None, fix_scale=False, corrected=corrected, members=members)


def stack(problems, order=None, gaps=0):
    """several problems as one call -> (nc, start, fixed, edges in the call's numbers, problems table GRAPH_PROBLEM_DTYPE rows as tuples,
    the keyframe ranges in table order).  order: the table's order (the arrays keep theirs); gaps: that many keyframes of no problem
    ahead of each problem's"""
    nc, start, fixed, edges, table, at, e_at = [], [], [], [], [], 0, 0
    rng = np.random.default_rng(7)
    for pr in problems:
        for _ in range(gaps):
            nc.append(sim3(rng.normal(0, 1, 3), rng.normal(0, 1, 3), 1.3)[None])
            start.append(sim3(rng.normal(0, 1, 3), rng.normal(0, 1, 3), 0.7)[None])
            fixed.append(np.zeros(1, np.uint8))
            at += 1
        n_kf, n_e = len(pr["nc"]), len(pr["edges"])
        nc.append(pr["nc"]), start.append(pr["start"]), fixed.append(pr["fixed"]), edges.append(pr["edges"] + at)
        table.append((at, n_kf, e_at, n_e))
        at, e_at = at + n_kf, e_at + n_e
    order = list(range(len(problems))) if order is None else list(order)
    return (np.concatenate(nc), np.concatenate(start), np.concatenate(fixed), np.concatenate(edges).astype(np.int32).reshape(-1, 2),
            [table[k] for k in order], order)
