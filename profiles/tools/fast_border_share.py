"""What k_fast_score queues outside the rectangle any cell window can use.  ComputeKeyPointsOctTree's windows start at
minBorder = 16 and end at w - 16, and FAST leaves a 3-px rim inside each, so a level is evaluated in 19 <= x < w - 19,
19 <= y < h - 19 only; the kernel's compass test, ring and arc search run on 3 <= x < w - 3, 3 <= y < h - 3.  Per level and
per kind of block (64 x 64 region of two stacked tiles, or the lone half that ends a level; ss_geometry.cpp's block records) this
prints the queue entries (region pixels and ring pixels that pass the compass test, and the ring's four untested corner pixels)
and the 64-entry chunks of phase 2 a block holds with the bound at 3 and at 19.  The frames are the bench's
(synth.frame_from_scene of scene s, seed s, time step 0, for s = 0, 1, 1000, 2003), the pyramid the oracle's.  CPU only.
1280 x 720: 11.9 % of the pixels outside (8.1 % at level 0, 27.5 % at level 7), 12.9 % of 1 019 973 entries, chunks
17 481 -> 15 353 (-12.2 %); 640 x 480: 22.2 % of the entries, -20.8 % of the chunks.
usage: python profiles/tools/fast_border_share.py [--json]          (1280 x 720 / 2000 and 640 x 480 / 1250, 8 levels)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
from oracle import orb_oracle as O  # noqa: E402
from send_slam_amd import synth  # noqa: E402

SEEDS = (0, 1, 1000, 2003)
KINDS = ("interior", "top_bottom", "left_right", "corner")
EDGE = 19  # SS_EDGE_THRESHOLD


def compass(lv, min_th):
    """the kernel's compass rule on every pixel whose ring is inside the level (3 <= x < w - 3, 3 <= y < h - 3)"""
    a = lv.astype(np.int32)
    v = a[3:-3, 3:-3]
    p0, p8, p4, p12 = a[6:, 3:-3], a[:-6, 3:-3], a[3:-3, 6:], a[3:-3, :-6]
    dark = v - np.maximum(np.minimum(p0, p8), np.minimum(p4, p12))
    bright = np.minimum(np.maximum(p0, p8), np.maximum(p4, p12)) - v
    out = np.zeros(lv.shape, bool)
    out[3:-3, 3:-3] = np.maximum(dark, bright) > min_th
    return out


def inside(w, h, b):
    m = np.zeros((h, w), bool)
    m[b:h - b, b:w - b] = True
    return m


def level_blocks(passed, w, h, b):
    """(kind, entries) of every block of a level with the bound at b"""
    live = passed & inside(w, h, b)
    # a frame of 1 px so that ring rows / columns outside the level read False
    pad = np.zeros((h + 66, w + 66), bool)
    pad[1:h + 1, 1:w + 1] = live
    box = np.zeros((h + 66, w + 66), bool)
    box[1:h + 1, 1:w + 1] = inside(w, h, b)
    tiles_y = (h + 31) // 32
    out = []
    for y0 in range(0, 32 * tiles_y, 64):
        hrows = 64 if y0 + 32 < 32 * tiles_y else 32
        for x0 in range(0, w, 64):
            inner_x = x0 >= 4 and x0 + 68 <= w
            inner_y = y0 >= 4 and y0 + hrows + 4 <= h
            kind = 0 if inner_x and inner_y else 1 if inner_x else 2 if inner_y else 3
            X, Y = x0 + 1, y0 + 1  # in pad
            n = int(pad[Y:Y + hrows, X:X + 64].sum())
            n += int(pad[Y - 1, X:X + 64].sum()) + int(pad[Y + hrows, X:X + 64].sum())
            n += int(pad[Y:Y + hrows, X - 1].sum()) + int(pad[Y:Y + hrows, X + 64].sum())
            n += int(box[Y - 1, X - 1]) + int(box[Y - 1, X + 64]) + int(box[Y + hrows, X - 1]) + int(box[Y + hrows, X + 64])
            out.append((kind, n))
    return out


def table(w, h, n_features):
    p = O.default_params(n_features=n_features)
    g = O.geometry(p, w, h)
    rows = [{"level": l, "size": f"{g.w[l]}x{g.h[l]}", "pixels_3": 0, "pixels_19": 0,
             "blocks": [0] * 4, "entries_3": [0] * 4, "entries_19": [0] * 4, "chunks_3": [0] * 4, "chunks_19": [0] * 4}
            for l in range(g.n_levels)]
    for s in SEEDS:
        img = np.ascontiguousarray(synth.frame_from_scene(synth.scene(s, w, h), s, w, h, 0))
        for l, lv in enumerate(O.pyramid(img, p)):
            lh, lw = lv.shape
            passed = compass(lv, p.min_th_fast)
            r = rows[l]
            r["pixels_3"] += lw * lh  # of all the level's pixels
            r["pixels_19"] += (lw - 2 * EDGE) * (lh - 2 * EDGE)
            for b, tag in ((3, "3"), (EDGE, "19")):
                for kind, n in level_blocks(passed, lw, lh, b):
                    r["entries_" + tag][kind] += n
                    r["chunks_" + tag][kind] += (n + 63) // 64
                    if b == 3:
                        r["blocks"][kind] += 1
    return rows


def total(rows, key):
    return sum(sum(r[key]) if isinstance(r[key], list) else r[key] for r in rows)


def main():
    result = {}
    for w, h, nf in ((1280, 720, 2000), (640, 480, 1250)):
        rows = table(w, h, nf)
        print(f"{w}x{h} / {nf}, {len(SEEDS)} frames: per level and kind of block ({' / '.join(KINDS)})")
        print("level size pixels-outside% | blocks | entries bound 3 | entries bound 19 | chunks bound 3 | chunks bound 19")
        for r in rows:
            out = 100.0 * (r["pixels_3"] - r["pixels_19"]) / r["pixels_3"]
            print(f"{r['level']} {r['size']} {out:.1f} | " + " | ".join(" ".join(str(v) for v in r[k]) for k in
                                                                       ("blocks", "entries_3", "entries_19", "chunks_3", "chunks_19")))
        e3, e19, c3, c19 = (total(rows, k) for k in ("entries_3", "entries_19", "chunks_3", "chunks_19"))
        p3, p19 = total(rows, "pixels_3"), total(rows, "pixels_19")
        by_kind = {KINDS[k]: {"blocks": sum(r["blocks"][k] for r in rows), "entries_3": sum(r["entries_3"][k] for r in rows),
                              "entries_19": sum(r["entries_19"][k] for r in rows), "chunks_3": sum(r["chunks_3"][k] for r in rows),
                              "chunks_19": sum(r["chunks_19"][k] for r in rows)} for k in range(4)}
        for k, d in by_kind.items():
            gone = 100.0 * (d["entries_3"] - d["entries_19"]) / max(d["entries_3"], 1)
            print(f"  {k:11s} blocks {d['blocks']:5d}  entries {d['entries_3']:7d} -> {d['entries_19']:7d} (-{gone:.1f} %)  "
                  f"chunks {d['chunks_3']:6d} -> {d['chunks_19']:6d}")
        print(f"all: pixels outside the rectangle {100.0 * (p3 - p19) / p3:.1f} %, queue entries outside it "
              f"{100.0 * (e3 - e19) / e3:.1f} % of {e3}, chunks {c3} -> {c19} ({100.0 * (c19 - c3) / c3:+.1f} %)\n")
        result[f"{w}x{h}_{nf}"] = {
            "pixels_outside_pct": round(100.0 * (p3 - p19) / p3, 1),
            "pixels_outside_pct_by_level": [round(100.0 * (r["pixels_3"] - r["pixels_19"]) / r["pixels_3"], 1) for r in rows],
            "entries_bound_3": e3, "entries_bound_19": e19, "entries_outside_pct": round(100.0 * (e3 - e19) / e3, 1),
            "chunks_bound_3": c3, "chunks_bound_19": c19, "chunks_pct": round(100.0 * (c19 - c3) / c3, 1), "by_kind": by_kind}
    if "--json" in sys.argv:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
