"""The map-point refresh of include/sendslam_orb.h restated in numpy and plain Python: its normative statement.
MapPoint::UpdateNormalAndDepth in Python floats (IEEE double, one operation per step) from float32 inputs widened, with the normal's sum
as a tree of 64 slots; MapPoint::ComputeDistinctiveDescriptors as a sorted row of Hamming distances per observation.  Written from the
rule, not from the library's text: a dictionary per point, numpy's sort for the median, no halving and no incidence list of the library's
shape."""
import math

import numpy as np

OBS_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("right", "<f4"), ("octave", "<i4")])
PROBLEM_DTYPE = np.dtype([(n, "<i4") for n in ("first_kf", "n_kf", "first_block", "n_blocks", "first_obs", "n_obs")] + [("reserved", "<i4", (2,))])
MAP_POINT_DTYPE = np.dtype([(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
INFO_DTYPE = np.dtype([(n, "<i4") for n in ("state", "n_obs", "count", "ref_kf", "level", "best_kf", "best_median", "reserved")])
SUMMARY_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_rows", "n_selected", "n_refreshed", "n_no_obs", "n_degenerate", "max_obs", "reserved")])
SLOTS = 64
POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def scale_table(scale_factor=1.2, n_levels=8):
    """the context's table: scale[0] = 1, scale[i] = (float)(scale[i - 1] * (double)factor)"""
    sc = [np.float32(1)]
    for _ in range(1, n_levels):
        sc.append(np.float32(float(sc[-1]) * float(np.float32(scale_factor))))
    return np.array(sc, np.float32)


def tree(terms):
    """slot s adds the terms s, s + 64, ... in ascending order from +0.0; the slots fold by halving"""
    a = [0.0] * SLOTS
    for j, t in enumerate(terms):
        a[j % SLOTS] = a[j % SLOTS] + t
    h = SLOTS // 2
    while h >= 1:
        for s in range(h):
            a[s] = a[s] + a[s + h]
        h //= 2
    return a[0]


def observations(call, n_levels):
    """{(block, row): [(kf relative to the problem, octave, stereo, keypoint row)] in ascending kf} of the records that are observations"""
    out = {}
    rows = call["obs_row"]
    for pr in np.asarray(call["table"], PROBLEM_DTYPE).reshape(-1):
        for m in range(pr["first_obs"], pr["first_obs"] + pr["n_obs"]):
            o = call["obs"][m]
            if not 0 <= int(o["octave"]) < n_levels:
                continue
            b, i = divmod(int(o["point"]), call["point_rows"])
            out.setdefault((int(pr["first_block"]) + b, i), []).append(
                (int(o["kf"]), int(o["octave"]), bool(call["check_right"] and o["right"] > 0), -1 if rows is None else int(rows[m])))
    for lst in out.values():
        lst.sort()
    return out


def medians(d):
    """the Hamming matrix of the descriptors d [n][32] and, per row, the element of rank (n - 1) // 2 in ascending order"""
    D = POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2)
    return D, np.sort(D, axis=1)[:, (len(d) - 1) // 2]


def refresh(call, geometry=1, descriptor=1, scale=None, rank_shift=0, tie_last=False):
    """-> (points, point_desc, info, summary), the inputs copied.  rank_shift and tie_last exist for the liveness tests only: the
    neighbouring rank, and a tie decided for the highest observation"""
    scale = scale_table() if scale is None else scale
    n_levels = len(scale)
    B, R = call["n_blocks"], call["point_rows"]
    pts = np.array(call["points"], MAP_POINT_DTYPE).reshape(B, R).copy()
    pd = None if call["point_desc"] is None else np.array(call["point_desc"], np.uint8).reshape(B, R, 32).copy()
    info, summary = np.zeros((B, R), INFO_DTYPE), np.zeros(B, SUMMARY_DTYPE)
    for name in ("ref_kf", "level", "best_kf", "best_median"):
        info[name] = -1
    info["state"] = -1
    seen = observations(call, n_levels)
    ow = np.asarray(call["views"]["ow"], np.float32)
    table = np.asarray(call["table"], PROBLEM_DTYPE).reshape(-1)
    for pr in table:
        for b in range(pr["first_block"], pr["first_block"] + pr["n_blocks"]):
            n_rows = min(max(int(call["n_points"][b]), 0), R)
            summary[b]["n_rows"] = n_rows
            for i in range(n_rows):
                P = pts[b, i]
                if call["select"] is not None and call["select"][b][i] != 0:
                    continue
                if not (np.isfinite(P["x"]) and np.isfinite(P["y"]) and np.isfinite(P["z"])):
                    continue
                r = info[b, i]
                lst = seen.get((b, i), [])
                n = len(lst)
                r["n_obs"], r["count"] = n, n + sum(1 for o in lst if o[2])
                if n == 0:
                    r["state"] = 1
                    continue
                if geometry:
                    terms, lens = [], []
                    for kf, _, _, _ in lst:
                        c = ow[pr["first_kf"] + kf]
                        d = [float(P["x"]) - float(c[0]), float(P["y"]) - float(c[1]), float(P["z"]) - float(c[2])]
                        ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                        lens.append(ln)
                        terms.append([d[k] / ln if ln != 0 else math.nan for k in range(3)])
                    if not all(ln > 0 and math.isfinite(ln) for ln in lens):
                        r["state"] = 2
                        continue
                    given = -1 if call["ref_kf"] is None else int(call["ref_kf"][b][i])
                    ref = next((a for a, o in enumerate(lst) if o[0] == given), 0)
                    mx = lens[ref] * float(scale[lst[ref][1]])
                    mn = mx / float(scale[n_levels - 1])
                    geo = [np.float32(tree([t[k] for t in terms]) / float(n)) for k in range(3)] + [np.float32(mn), np.float32(mx)]
                if descriptor:
                    d = np.stack([call["desc"][pr["first_kf"] + kf][row] for kf, _, _, row in lst])
                    _, med = medians(d)
                    if rank_shift:
                        med = np.sort(POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2), axis=1)[:, min(max((n - 1) // 2 + rank_shift, 0), n - 1)]
                    best = min(range(n), key=lambda a: (int(med[a]), -a if tie_last else a))
                    r["best_kf"], r["best_median"] = lst[best][0], int(med[best])
                    pd[b, i] = d[best]
                if geometry:
                    r["ref_kf"], r["level"] = lst[ref][0], lst[ref][1]
                    P["nx"], P["ny"], P["nz"], P["min_dist"], P["max_dist"] = geo
                r["state"] = 0
    for b in range(B):
        st = info[b]["state"]
        s = summary[b]
        s["n_selected"], s["n_refreshed"], s["n_no_obs"], s["n_degenerate"] = (st >= 0).sum(), (st == 0).sum(), (st == 1).sum(), (st == 2).sum()
        s["max_obs"] = info[b]["n_obs"][st >= 0].max(initial=0)
    return pts, pd, info, summary
