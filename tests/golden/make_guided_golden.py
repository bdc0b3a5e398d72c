"""Regenerates tests/golden/guided/*.npz: the guided-matching reference (tests/guided_ref.py) frozen on three pairs of 320 x 240
frames / 500 features.  Each file holds the inputs as arrays (keypoints and descriptors of both frames from the CPU oracle, the
windows: the query's own position, radius 15 * scale[octave], octave -+ 1), and for each of the twelve parameter sets
(guided_cases.COMBOS) the expected idx / d1 / d2 and summary.

usage: python tests/golden/make_guided_golden.py   (from the repository root, after the oracle has been built)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import guided_cases as G  # noqa: E402
import guided_ref as R  # noqa: E402

PAIRS = [("synth_t1", "synth_t0"), ("dots_shift", "dots"), ("checker_shift", "checker")]


def main():
    out_dir = os.path.join(HERE, "guided")
    os.makedirs(out_dir, exist_ok=True)
    for query, train in PAIRS:
        qk, qd = G.features(query)
        tk, td = G.features(train)
        win = G.own_windows(qk)
        arrays = {"q_kp": qk, "q_desc": qd, "t_kp": tk, "t_desc": td, "windows": win, "size": np.array([G.W, G.H, G.NF], np.int32),
                  "radius": np.float32(G.RADIUS), "octave_span": np.int32(G.SPAN)}
        for c in G.COMBOS:
            idx, d1, d2, summ, _ = R.match(qk, qd, tk, td, win, **c)
            n = G.combo_name(c)
            arrays[n + "_idx"], arrays[n + "_d1"], arrays[n + "_d2"] = idx, d1, d2
            arrays[n + "_summary"] = np.array([summ[f] for f in R.SUMMARY_FIELDS], np.int32)
            print(query, n, summ)
        path = os.path.join(out_dir, f"{query}_vs_{train}.npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
