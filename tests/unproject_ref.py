"""The normative statement of the map points from depth (include/sendslam_orb.h, "map points from depth") in
numpy (test infrastructure, plain module).

Upstream's loops are stated literally: `select_literal` is the sort of (depth, row) pairs and the sequential loop with its break
of Tracking::CreateNewKeyFrame / UpdateLastFrame (and the loop without a break of Tracking::StereoInitialization); `select_closed`
is the closed form the library computes, rank <= max(n_not_far, max_points).  `frame` is the whole rule of one frame.  Every
floating-point step of the map point is one float64 operation, left to right, rounded to float32 once at the end."""
from __future__ import annotations

import numpy as np

ALL, CLOSE = 0, 1
CREATED, KEPT, FAR, NO_DEPTH, OCTAVE, DEGENERATE = range(6)
SUMMARY_FIELDS = ("status", "n_kp", "n_depth", "n_close", "n_not_far", "n_processed", "n_created", "n_kept", "n_tracked_close", "n_untracked_close")
VIEW_DTYPE = np.dtype([("rcw", "<f8", (9,)), ("tcw", "<f8", (3,))] + [(n, "<f8") for n in ("fx", "fy", "cx", "cy", "invfx", "invfy")] + [("ow", "<f8", (3,))])
MAP_POINT_FIELDS = ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")
MAP_POINT_DTYPE = np.dtype([(n, "<f4") for n in MAP_POINT_FIELDS])

f64 = np.float64


def view_init(fx, fy, cx, cy, rcw, tcw) -> np.ndarray:
    """ss_unproject_view_init: ow[k] = -((r[k]*t[0] + r[3+k]*t[1]) + r[6+k]*t[2])"""
    v = np.zeros((), VIEW_DTYPE)
    r, t = np.asarray(rcw, f64).reshape(9), np.asarray(tcw, f64).reshape(3)
    with np.errstate(all="ignore"):
        v["rcw"], v["tcw"] = r, t
        v["fx"], v["fy"], v["cx"], v["cy"] = fx, fy, cx, cy
        v["invfx"], v["invfy"] = f64(1.0) / f64(fx), f64(1.0) / f64(fy)
        v["ow"] = [-((r[k] * t[0] + r[3 + k] * t[1]) + r[6 + k] * t[2]) for k in range(3)]
    return v


def clamp(n: int, rows: int) -> int:
    return min(max(int(n), 0), rows)


def ranked_rows(depth, octave, n: int, n_levels: int) -> list:
    """the rows that have a key: i < n, depth > 0 (a NaN fails), octave inside the table"""
    return [i for i in range(n) if depth[i] > 0 and 0 <= int(octave[i]) < n_levels]


def select_literal(depth, rows, mode: int, max_points: int, close_limit) -> set:
    """upstream: vDepthIdx of (z, i) with z > 0, std::sort, then the loop; `rows`: the rows that enter vDepthIdx"""
    pairs = sorted((np.float32(depth[i]), i) for i in rows)  # pair<float, int>: by depth, then by row
    processed, n_points = set(), 0
    for z, i in pairs:
        processed.add(i)  # the row is either given a new point or keeps its own; both count
        n_points += 1
        if mode == CLOSE and z > np.float32(close_limit) and n_points > max_points:
            break
    return processed


def select_closed(depth, rows, mode: int, max_points: int, close_limit) -> set:
    """the library's form: the key bits(depth) << 32 | row, rank = the number of lower keys"""
    d32 = np.asarray(depth, np.float32)
    keys = sorted((int(d32[i:i + 1].view(np.uint32)[0]) << 32) | i for i in rows)
    if mode == ALL:
        return set(rows)
    n_not_far = sum(1 for i in rows if d32[i] <= np.float32(close_limit))
    bound = max(n_not_far, max_points)
    return {k & 0xFFFFFFFF for rank, k in enumerate(keys) if rank <= bound}


def map_point(view, scale, x, y, octave: int, depth):
    """step 5 -> the eight float32 numbers, or None (state 5)"""
    sc = np.asarray(scale, np.float32)
    r, ow = view["rcw"], view["ow"]
    with np.errstate(all="ignore"):
        z = f64(np.float32(depth))
        xc = ((f64(np.float32(x)) - view["cx"]) * z) * view["invfx"]
        yc = ((f64(np.float32(y)) - view["cy"]) * z) * view["invfy"]
        X = [((r[k] * xc + r[3 + k] * yc) + r[6 + k] * z) + ow[k] for k in range(3)]
        n = [X[k] - ow[k] for k in range(3)]
        d = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if not (d > 0 and np.isfinite(d)):
            return None
        max_dist = d * f64(sc[octave])
        min_dist = max_dist / f64(sc[len(sc) - 1])
        return tuple(np.float32(v) for v in (X[0], X[1], X[2], n[0] / d, n[1] / d, n[2] / d, min_dist, max_dist))


def frame(view, mode: int, max_points: int, close_limit, scale, kp, desc, depth, n=None, has_point=None, outlier=None, literal: bool = True):
    """the rule of one frame -> dict(state int32 [rows], points MAP_POINT_DTYPE [n_points], desc uint8 [n_points][32], rows int32
    [n_points][2], summary dict).  literal: the selection by upstream's loop, else by the closed form"""
    rows = len(kp)
    nk = clamp(rows if n is None else n, rows)
    depth = np.asarray(depth, np.float32)
    limit = np.float32(close_limit)
    n_levels = len(scale)
    ranked = ranked_rows(depth, kp["octave"], nk, n_levels)
    is_ranked = set(ranked)
    select = select_literal if literal else select_closed
    processed = select(depth, ranked, mode, max_points, limit)
    has = (lambda i: False) if has_point is None else (lambda i: has_point[i] != 0)
    out = (lambda i: False) if outlier is None else (lambda i: outlier[i] != 0)
    state = np.full(rows, -1, np.int32)
    pts, pdesc, prow = [], [], []
    for i in range(nk):
        if not depth[i] > 0:
            state[i] = NO_DEPTH
        elif i not in is_ranked:
            state[i] = OCTAVE
        elif i not in processed:
            state[i] = FAR
        elif has(i):
            state[i] = KEPT
        else:
            p = map_point(view, scale, kp["x"][i], kp["y"][i], int(kp["octave"][i]), depth[i])
            state[i] = DEGENERATE if p is None else CREATED
            if p is not None:
                pts.append(p), pdesc.append(np.asarray(desc[i], np.uint8)), prow.append((i, -1))
    close = [i for i in ranked if depth[i] < limit]
    tracked = sum(1 for i in close if has(i) and not out(i))
    summary = dict(status=0, n_kp=nk, n_depth=int(sum(1 for i in range(nk) if depth[i] > 0)), n_close=len(close),
                   n_not_far=sum(1 for i in ranked if depth[i] <= limit), n_processed=len(processed), n_created=len(pts),
                   n_kept=int((state == KEPT).sum()), n_tracked_close=tracked, n_untracked_close=len(close) - tracked)
    return dict(state=state, points=np.array(pts, MAP_POINT_DTYPE).reshape(-1), desc=np.array(pdesc, np.uint8).reshape(-1, 32),
                rows=np.array(prow, np.int32).reshape(-1, 2), summary=summary)
