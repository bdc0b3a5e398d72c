"""numpy restatement of ORB-SLAM3's Frame::ComputeStereoMatches (test infrastructure, plain module).

Written from the routine's description (include/sendslam_orb.h, DESIGN.md "Stereo depth"), not from the kernels: upstream's
row table and serial loops, float32 at every step (every operation rounded once), keypoints / descriptors / pyramids
from the CPU oracle.  The device code must reproduce every field bit for bit.

    stage A  ORB search: right keypoints of the left keypoint's row (row table), octave +-1, u inside [uL - maxD, uL - minD],
             lowest Hamming distance (ties: lowest right index), rejected at >= (TH_HIGH + TH_LOW) / 2 = 75
    stage B  11 x 11 SAD window slid -5 .. +5 px at the left keypoint's octave on the unblurred pyramids (ties: lowest
             shift), parabola fit, disparity test, depth = bf / disparity
    stage C  median of the accepted SADs, points at >= 1.5 * 1.4 * median lose their depth

Two deviations from upstream, both counted in `stats` so that tests can assert they stay theoretical: "guard" (a window
that would leave the level image rejects the point) and an empty accepted list is a no-op.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from oracle import orb_oracle as O

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50
W_HALF, SLIDE = 5, 5

POINT_DTYPE = np.dtype([("u_right", "<f4"), ("depth", "<f4"), ("right_idx", "<i4"), ("orb_dist", "<u2"), ("sad", "<u2")])
SUMMARY_FIELDS = ("status", "n_left", "n_right", "n_matched", "n_refined", "n_depth", "n_close", "sad_median")


def c_round(x) -> int:
    """std::round of a float32: half away from zero"""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def level_scales(p, width: int, height: int):
    """the context's per-level scale (the oracle's geometry: scale[i] = (float)(scale[i - 1] * (double)scaleFactor))"""
    g = O.geometry(p, width, height)
    return [f32(g.scale[l]) for l in range(g.n_levels)]


def none_points(n: int) -> np.ndarray:
    pts = np.empty(n, POINT_DTYPE)
    pts["u_right"] = -1
    pts["depth"] = -1
    pts["right_idx"] = -1
    pts["orb_dist"] = 0xFFFF
    pts["sad"] = 0xFFFF
    return pts


def compute(kpL, dL, pyrL, kpR, dR, pyrR, scale, fx, baseline, th_depth=35.0, stats: Counter | None = None):
    """-> (points POINT_DTYPE[len(kpL)], summary dict).  scale: per-level float32 scales; pyr*: unblurred level images."""
    st = stats if stats is not None else Counter()
    N = len(kpL)
    inv = [f32(1.0) / s for s in scale]
    n_rows = pyrL[0].shape[0]
    fx = f32(fx)
    bf = f32(f32(baseline) * fx)
    mb = f32(bf / fx)
    min_d = f32(0)
    max_d = f32(bf / mb)
    th_close = f32(f32(bf * f32(th_depth)) / fx)

    # upstream's row table: right keypoint iR is a candidate of every row of its band
    rows = [[] for _ in range(n_rows)]
    for iR in range(len(kpR)):
        y = f32(kpR["y"][iR])
        r = f32(f32(2.0) * scale[int(kpR["octave"][iR])])
        lo, hi = int(np.floor(f32(y - r))), int(np.ceil(f32(y + r)))
        assert 0 <= lo and hi < n_rows, "a band leaves the image (upstream would write outside its table)"
        for yi in range(lo, hi + 1):
            rows[yi].append(iR)

    pts = none_points(N)
    bitsL = np.unpackbits(np.ascontiguousarray(dL).reshape(-1, 32), axis=1)
    bitsR = np.unpackbits(np.ascontiguousarray(dR).reshape(-1, 32), axis=1)
    accepted = []  # (bestSad, iL)
    for iL in range(N):
        lv = int(kpL["octave"][iL])
        uL, vL = f32(kpL["x"][iL]), f32(kpL["y"][iL])
        cand = rows[int(vL)]
        if not cand:
            st["no_candidates"] += 1
            continue
        min_u, max_u = f32(uL - max_d), f32(uL - min_d)
        if max_u < 0:
            st["max_u_negative"] += 1
            continue
        best, best_r = TH_HIGH, 0
        for iR in cand:  # ascending iR
            o = int(kpR["octave"][iR])
            if o < lv - 1 or o > lv + 1:
                continue
            uR = f32(kpR["x"][iR])
            if uR >= min_u and uR <= max_u:
                d = int(np.count_nonzero(bitsL[iL] != bitsR[iR]))
                if d < best:
                    best, best_r = d, iR
        if best >= (TH_HIGH + TH_LOW) // 2:
            st["orb_reject"] += 1
            continue
        pts["right_idx"][iL] = best_r
        pts["orb_dist"][iL] = best

        s = inv[lv]
        su, sv, sr = c_round(f32(uL * s)), c_round(f32(vL * s)), c_round(f32(f32(kpR["x"][best_r]) * s))
        w, L = W_HALF, SLIDE
        h_l, cols = pyrR[lv].shape
        if sr + L - w < 0 or sr + L + w + 1 >= cols:  # upstream's test, as written
            st["edge"] += 1
            continue
        if sr - L - w < 0 or sr + L + w > cols - 1 or su - w < 0 or su + w > cols - 1 or sv - w < 0 or sv + w > h_l - 1:
            st["guard"] += 1  # deviation: upstream would read outside the image
            continue
        IL = pyrL[lv][sv - w:sv + w + 1, su - w:su + w + 1].astype(np.int64)
        best_sad, best_inc, dist = 2 ** 31 - 1, 0, []
        for inc in range(-L, L + 1):
            IR = pyrR[lv][sv - w:sv + w + 1, sr + inc - w:sr + inc + w + 1].astype(np.int64)
            d = int(np.abs(IL - IR).sum())
            if d < best_sad:
                best_sad, best_inc = d, inc
            dist.append(d)
        pts["sad"][iL] = best_sad
        if best_inc == -L or best_inc == L:
            st["slide_end"] += 1
            continue
        d1, d2, d3 = f32(dist[L + best_inc - 1]), f32(dist[L + best_inc]), f32(dist[L + best_inc + 1])
        with np.errstate(all="ignore"):
            den = f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2)))
            delta = f32(f32(d1 - d3) / den)
            if delta < -1 or delta > 1:
                st["delta"] += 1
                continue
            if np.isnan(delta):
                st["nan"] += 1
            best_u = f32(scale[lv] * f32(f32(f32(sr) + f32(best_inc)) + delta))
            disp = f32(uL - best_u)
            if not (disp >= min_d and disp < max_d):
                st["disp_negative" if disp < min_d else "disp_reject"] += 1
                continue
            if disp <= 0:
                disp = f32(0.01)
                best_u = f32(uL - f32(0.01))
                st["disp_clamped"] += 1
            pts["depth"][iL] = f32(bf / disp)
            pts["u_right"][iL] = best_u
        accepted.append((best_sad, iL))

    median = -1
    if accepted:
        accepted.sort()
        median = accepted[len(accepted) // 2][0]
        th_dist = f32(f32(f32(1.5) * f32(1.4)) * f32(median))
        for sad, i in accepted:
            if f32(sad) >= th_dist:
                pts["u_right"][i] = -1
                pts["depth"][i] = -1
                st["median_cut"] += 1
    st["refined"] += len(accepted)
    depth = pts["depth"]
    summary = {"status": 0, "n_left": N, "n_right": len(kpR), "n_matched": int((pts["right_idx"] >= 0).sum()),
               "n_refined": len(accepted), "n_depth": int((depth > 0).sum()),
               "n_close": int(((depth > 0) & (depth < th_close)).sum()), "sad_median": int(median)}
    return pts, summary


def stereo_pair(left: np.ndarray, right: np.ndarray, p, fx, baseline, th_depth=35.0, stats: Counter | None = None):
    """Extraction of both eyes with the CPU oracle, then compute().  -> (kL, dL, kR, dR, points, summary)"""
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    kL, dL, _ = O.extract(left, p)
    kR, dR, _ = O.extract(right, p)
    pts, summary = compute(kL, dL, O.pyramid(left, p), kR, dR, O.pyramid(right, p), level_scales(p, w, h), fx, baseline, th_depth, stats)
    return kL, dL, kR, dR, pts, summary
