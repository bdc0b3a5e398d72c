"""How often the loop that writes k_fast_score's queue runs.  After the compass test a thread holds the verdicts of four pixels
(columns 4 tx + i) of four rows (region rows 32 hf + 2 ty + rr): eight per half.  A wave (ty = 4 wave .. 4 wave + 3, every tx)
writes its candidates in a `while (bits)` loop that runs as often as its fullest lane has candidates.  As built before the
merged loop there were two loops, one per half: max over the lanes of the upper half's count + max of the lower half's; the
merged loop runs max over the lanes of the sum.  Per configuration this prints, per block (64 x 64 region of two stacked tiles, or
the lone half that ends a level; ss_geometry.cpp's block records): the queued region pixels, the loop iterations as built and
merged (summed over the block's four waves), the histogram of the per-wave maximum of either form, and the share of the
wave-halves with candidates that hold a lane with all eight flags set.  The bound is the kernel's without the response map (19 px,
SS_EDGE_THRESHOLD); the frames are the bench's (synth.frame_from_scene of scene s, seed s, time step 0), the pyramid the oracle's.
CPU only.
1280 x 720, scenes 0, 1, 1000, 2003: 3 052 blocks, 271.5 region entries per block, 33.67 -> 26.65 iterations per block;
640 x 480, scenes 0 and 1000 (the two the figures of DESIGN.md section 11 were taken on): 552 blocks, 250.3 entries, 30.59 -> 24.22;
640 x 480 on all four scenes: 1 104 blocks, 239.2 entries, 30.37 -> 23.99.
usage: python profiles/tools/fast_queue_share.py [--json]          (1280 x 720 / 2000 and 640 x 480 / 1250, 8 levels)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import orb_oracle as O  # noqa: E402
from send_slam_amd import synth  # noqa: E402
from fast_border_share import EDGE, SEEDS, compass, inside  # noqa: E402

CONFIGS = ((1280, 720, 2000, SEEDS), (640, 480, 1250, (0, 1000)), (640, 480, 1250, SEEDS))


def lane_counts(live):
    """live: (h, w) bool, the pixels a level queues.  -> counts[by, hf, wave, t4, bx, tx]: the candidates of lane
    (ty = 4 wave + t4, tx) of block (bx, by) in half hf (eight verdicts: two rows, four columns)"""
    h, w = live.shape
    nby, nbx = (((h + 31) // 32) + 1) // 2, (w + 63) // 64
    pad = np.zeros((64 * nby, 64 * nbx), np.int32)
    pad[:h, :w] = live
    # y = 64 by + 32 hf + 8 wave + 2 t4 + rr, x = 64 bx + 4 tx + i
    return pad.reshape(nby, 2, 4, 4, 2, nbx, 16, 4).sum(axis=(4, 7))


def table(w, h, n_features, seeds):
    p = O.default_params(n_features=n_features)
    blocks = entries = it_built = it_merged = halves_live = halves_full = 0
    hist_built, hist_merged = np.zeros(9, np.int64), np.zeros(17, np.int64)
    for s in seeds:
        img = np.ascontiguousarray(synth.frame_from_scene(synth.scene(s, w, h), s, w, h, 0))
        for lv in O.pyramid(img, p):
            lh, lw = lv.shape
            c = lane_counts(compass(lv, p.min_th_fast) & inside(lw, lh, EDGE))
            blocks += c.shape[0] * c.shape[4]
            entries += int(c.sum())
            half_max = c.max(axis=(3, 5))                # [by, hf, wave, bx]
            merged_max = c.sum(axis=1).max(axis=(2, 4))  # [by, wave, bx]
            it_built += int(half_max.sum())
            it_merged += int(merged_max.sum())
            hist_built += np.bincount(half_max.reshape(-1), minlength=9)
            hist_merged += np.bincount(merged_max.reshape(-1), minlength=17)
            halves_live += int((half_max > 0).sum())
            halves_full += int((half_max == 8).sum())
    return {"blocks": blocks, "region_entries_per_block": round(entries / blocks, 1),
            "iterations_per_block_two_loops": round(it_built / blocks, 2), "iterations_per_block_merged": round(it_merged / blocks, 2),
            "wave_halves_with_candidates": halves_live, "of_those_with_a_full_lane_pct": round(100.0 * halves_full / halves_live, 1),
            "wave_half_maximum_histogram_0_to_8": hist_built.tolist(), "wave_merged_maximum_histogram_0_to_16": hist_merged.tolist()}


def main():
    result = {}
    for w, h, nf, seeds in CONFIGS:
        r = table(w, h, nf, seeds)
        print(f"{w}x{h} / {nf}, scenes {seeds}: {r['blocks']} blocks, {r['region_entries_per_block']} queued region pixels per block")
        print(f"  loop iterations per block: two loops {r['iterations_per_block_two_loops']}, one merged loop {r['iterations_per_block_merged']}")
        print(f"  wave-halves with candidates {r['wave_halves_with_candidates']}, a lane with all 8 flags in {r['of_those_with_a_full_lane_pct']} % of them")
        print("  per-wave maximum of a half (0 .. 8):   " + " ".join(str(v) for v in r["wave_half_maximum_histogram_0_to_8"]))
        print("  per-wave maximum, merged (0 .. 16):    " + " ".join(str(v) for v in r["wave_merged_maximum_histogram_0_to_16"]) + "\n")
        result[f"{w}x{h}_{nf}_scenes_{'_'.join(str(s) for s in seeds)}"] = r
    if "--json" in sys.argv:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
