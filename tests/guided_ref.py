"""numpy restatement of the guided matching rule (test infrastructure, plain module).

Written from the rule's description (include/sendslam_orb.h, DESIGN.md "Guided matching"), not from the kernels: serial loops
over the queries and their candidates, float32 at every step (every operation rounded once), `stereo_ref.c_round` for the
rounding of the rotation bin.  The device code must reproduce idx, d1, d2 and every summary field bit for bit.

    candidates   train rows inside the query's window: octave range, |dx| < radius and |dy| < radius, both strict
                 (`box_candidates`; `grid_candidates` is the literal upstream form, Frame::GetFeaturesInArea on its 64 x 48 grid)
    search       d1 = lowest distance, idx = lowest row among those, d2 = lowest distance over the other candidates
    accept       d1 <= th and (ratio_den == 0 or d1 * ratio_den < d2 * ratio_num)
    one_to_one   per train row the accepted query with the lowest d1 << 20 | i keeps it
    orientation  30-bin histogram of angle_query - angle_train, ComputeThreeMaxima, matches outside the kept bins dropped
"""
from __future__ import annotations

import numpy as np

from stereo_ref import c_round

f32 = np.float32
HISTO_LENGTH = 30
ROT_FACTOR = {1: f32(1.0) / f32(HISTO_LENGTH), 2: f32(HISTO_LENGTH) / f32(360.0)}
NONE = 0xFFFF
FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48

WINDOW_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("oct_lo", "<i2"), ("oct_hi", "<i2")])
SUMMARY_FIELDS = ("status", "n_query", "n_train", "n_candidates", "n_accepted", "n_unique", "n_final", "rot_bins")

_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint16)


def make_windows(x, y, radius, oct_lo, oct_hi) -> np.ndarray:
    x = np.asarray(x, np.float32)
    w = np.empty(len(x), WINDOW_DTYPE)
    w["x"], w["y"], w["radius"], w["oct_lo"], w["oct_hi"] = x, y, radius, oct_lo, oct_hi
    return w


def own_windows(kp, radius, radius_by_octave: bool, octave_span: int, scale) -> np.ndarray:
    """the NULL-window form of the batch call: a query's window is its own position; radius, or radius * scale[octave] (one
    float32 product); octaves octave -+ octave_span"""
    octv = kp["octave"].astype(np.int64)
    sc = np.array([f32(s) for s in scale], np.float32)
    r = f32(radius) * sc[octv] if radius_by_octave else np.full(len(kp), f32(radius), np.float32)
    return make_windows(kp["x"], kp["y"], r.astype(np.float32), octv - octave_span, octv + octave_span)


def whole_windows(n: int) -> np.ndarray:
    """windows that hold every train row with finite coordinates"""
    return make_windows(np.zeros(n), np.zeros(n), 1e9, 0, 15)


def box_candidates(win, t_kp) -> list:
    """ascending train rows inside one window: the membership test of GetFeaturesInArea, in closed form"""
    x, y, r = f32(win["x"]), f32(win["y"]), f32(win["radius"])
    if not r > 0:  # zero, negative, NaN
        return []
    lo, hi = int(win["oct_lo"]), int(win["oct_hi"])
    out = []
    with np.errstate(all="ignore"):
        for j in range(len(t_kp)):
            o = int(t_kp["octave"][j])
            if o < lo or o > hi:
                continue
            if np.abs(f32(f32(t_kp["x"][j]) - x)) < r and np.abs(f32(f32(t_kp["y"][j]) - y)) < r:
                out.append(j)
    return out


def _box_mask(windows, t_kp) -> np.ndarray:
    """box_candidates for every query at once: the same float32 operations, element-wise"""
    with np.errstate(all="ignore"):
        tx, ty, to = t_kp["x"].astype(np.float32), t_kp["y"].astype(np.float32), t_kp["octave"].astype(np.int64)
        r = windows["radius"][:, None]
        m = (np.abs(tx[None, :] - windows["x"][:, None]) < r) & (np.abs(ty[None, :] - windows["y"][:, None]) < r)
        m &= (to[None, :] >= windows["oct_lo"].astype(np.int64)[:, None]) & (to[None, :] <= windows["oct_hi"].astype(np.int64)[:, None])
        m &= (windows["radius"] > 0)[:, None]
    return m


class UpstreamGrid:
    """Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea, as written upstream, for an undistorted image
    (mnMinX = mnMinY = 0, mnMaxX = width, mnMaxY = height)."""

    def __init__(self, kp, width: int, height: int):
        self.kp = kp
        self.inv_w = f32(FRAME_GRID_COLS) / f32(width)
        self.inv_h = f32(FRAME_GRID_ROWS) / f32(height)
        self.cells = [[[] for _ in range(FRAME_GRID_ROWS)] for _ in range(FRAME_GRID_COLS)]
        self.dropped = 0
        for j in range(len(kp)):
            px, py = c_round(f32(f32(kp["x"][j]) * self.inv_w)), c_round(f32(f32(kp["y"][j]) * self.inv_h))
            if px < 0 or px >= FRAME_GRID_COLS or py < 0 or py >= FRAME_GRID_ROWS:
                self.dropped += 1  # upstream leaves such a keypoint out of its grid
                continue
            self.cells[px][py].append(j)

    def features_in_area(self, x, y, r, min_level: int, max_level: int) -> list:
        x, y, r = f32(x), f32(y), f32(r)
        x0 = max(0, int(np.floor(f32(f32(x - r) * self.inv_w))))
        x1 = min(FRAME_GRID_COLS - 1, int(np.ceil(f32(f32(x + r) * self.inv_w))))
        y0 = max(0, int(np.floor(f32(f32(y - r) * self.inv_h))))
        y1 = min(FRAME_GRID_ROWS - 1, int(np.ceil(f32(f32(y + r) * self.inv_h))))
        if x0 >= FRAME_GRID_COLS or x1 < 0 or y0 >= FRAME_GRID_ROWS or y1 < 0:
            return []
        out = []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for j in self.cells[ix][iy]:
                    o = int(self.kp["octave"][j])
                    if o < min_level or o > max_level:
                        continue
                    if np.abs(f32(f32(self.kp["x"][j]) - x)) < r and np.abs(f32(f32(self.kp["y"][j]) - y)) < r:
                        out.append(j)
        return out


def grid_candidates(windows, t_kp, width: int, height: int):
    """-> (per-query sorted candidate lists through the upstream grid, keypoints the grid dropped)"""
    g = UpstreamGrid(t_kp, width, height)
    return [sorted(g.features_in_area(w["x"], w["y"], w["radius"], int(w["oct_lo"]), int(w["oct_hi"]))) for w in windows], g.dropped


def distances(q_desc, t_desc, chunk: int = 256) -> np.ndarray:
    """Hamming distances [nq, nt] uint16, the queries taken `chunk` at a time"""
    q = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
    out = np.empty((len(q), len(t)), np.uint16)
    if hasattr(np, "bitwise_count"):  # numpy >= 2: eight bytes at a time
        q, t = q.view(np.uint64), t.view(np.uint64)
    for a in range(0, len(q), chunk):
        x = q[a:a + chunk, None, :] ^ t[None, :, :]
        out[a:a + chunk] = (np.bitwise_count(x) if x.dtype == np.uint64 else _POPCOUNT[x]).sum(axis=2, dtype=np.uint16)
    return out


def rot_bin(angle_q, angle_t, orientation: int) -> int:
    """-> bin 0..29, or -1 when it falls outside (angles outside [0, 360), NaN)"""
    with np.errstate(all="ignore"):
        rot = f32(f32(angle_q) - f32(angle_t))
        if rot < 0:
            rot = f32(rot + f32(360.0))
        v = f32(rot * ROT_FACTOR[orientation])
    if not (v == v) or v < -1 or v > HISTO_LENGTH + 1:
        return -1
    b = c_round(v)
    if b < 0 or b > HISTO_LENGTH:
        return -1
    return 0 if b == HISTO_LENGTH else b


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima on the bin counts -> (ind1, ind2, ind3), -1 = none"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    cut = f32(f32(0.1) * f32(max1))
    if f32(max2) < cut:
        ind2 = ind3 = -1
    elif f32(max3) < cut:
        ind3 = -1
    return ind1, ind2, ind3


def pack_bins(inds) -> int:
    return sum((i & 0xFF) << (8 * k) for k, i in enumerate(inds))


def none_result(n: int):
    return np.full(n, -1, np.int32), np.full(n, NONE, np.uint16), np.full(n, NONE, np.uint16)


def search(q_desc, t_kp, t_desc, windows, exclude_self=False):
    """The window search of every query: -> (best row or -1, d1, d2, candidate lists), before any test.  t_kp None = no train
    frame."""
    nq = len(windows)
    best_row, d1, d2 = none_result(nq)
    nt = 0 if t_kp is None else len(t_kp)
    cands = [[] for _ in range(nq)]
    if nq and nt:
        dist = distances(q_desc, t_desc)
        mask = _box_mask(windows, t_kp)
        for i in range(nq):
            best, second, best_j = NONE, NONE, -1
            for j in np.flatnonzero(mask[i]):  # ascending j
                if exclude_self and j == i:
                    continue
                cands[i].append(int(j))
                d = int(dist[i, j])
                if d < best:
                    second, best, best_j = best, d, int(j)
                elif d < second:
                    second = d
            best_row[i], d1[i], d2[i] = best_j, best, second
    return best_row, d1, d2, cands


def finish(found, q_kp, t_kp, th=50, ratio_num=9, ratio_den=10, one_to_one=False, orientation=0):
    """The acceptance test and the two filters on the result of search() -> (idx, d1, d2, summary dict, candidate lists)"""
    best_row, d1, d2, cands = found
    nq = len(best_row)
    nt = 0 if t_kp is None else len(t_kp)
    idx = np.full(nq, -1, np.int32)
    for i in range(nq):
        best, second = int(d1[i]), int(d2[i])
        if best_row[i] >= 0 and best <= th and (ratio_den == 0 or best * ratio_den < second * ratio_num):
            idx[i] = best_row[i]
    n_acc = int((idx >= 0).sum())
    if one_to_one:
        owner = {}
        for i in range(nq):
            if idx[i] >= 0:
                key = (int(d1[i]) << 20) | i
                j = int(idx[i])
                if j not in owner or key < owner[j]:
                    owner[j] = key
        for i in range(nq):
            if idx[i] >= 0 and owner[int(idx[i])] != ((int(d1[i]) << 20) | i):
                idx[i] = -1
    n_uni = int((idx >= 0).sum())
    bins = 0xFFFFFF
    if orientation:
        hist = [0] * HISTO_LENGTH
        which = {}
        for i in range(nq):
            if idx[i] >= 0:
                b = rot_bin(q_kp["angle"][i], t_kp["angle"][idx[i]], orientation)
                which[i] = b
                if b >= 0:
                    hist[b] += 1
        inds = three_maxima(hist)
        for i, b in which.items():
            if b < 0 or b not in inds:
                idx[i] = -1
        bins = pack_bins(inds)
    summary = {"status": 0, "n_query": nq, "n_train": nt, "n_candidates": sum(len(c) for c in cands), "n_accepted": n_acc,
               "n_unique": n_uni, "n_final": int((idx >= 0).sum()), "rot_bins": bins}
    return idx, d1.copy(), d2.copy(), summary, cands


def match(q_kp, q_desc, t_kp, t_desc, windows, th=50, ratio_num=9, ratio_den=10, one_to_one=False, orientation=0,
          exclude_self=False):
    """One (query frame, train frame) pair.  t_kp None = no train frame.  -> (idx, d1, d2, summary dict, candidate lists)"""
    return finish(search(q_desc, t_kp, t_desc, windows, exclude_self), q_kp, t_kp, th, ratio_num, ratio_den, one_to_one, orientation)
