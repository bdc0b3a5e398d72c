"""Writes tests/golden/bow/: the k3 vocabulary of tests/bow_cases.py in DBoW2's text format and, per frame, the reference
transform (tests/bow_ref.py) of its oracle descriptors for several levelsup, plus its L1 score against another frame.

    python tests/golden/make_bow_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bow_cases as BC  # noqa: E402
import bow_ref as B  # noqa: E402
import guided_cases as G  # noqa: E402

OUT = os.path.join(HERE, "bow")
LEVELSUPS = (0, 2, 4, 9)
PAIRS = [("synth_t0", "synth_t1"), ("checker", "synth_t0")]


def main():
    os.makedirs(OUT, exist_ok=True)
    voc = BC.vocab("k3")
    BC.write(os.path.join(OUT, "k3_vocabulary.txt"), voc)
    for frame, other in PAIRS:
        desc = G.features(frame)[1]
        _, _, ow, ov, _ = B.transform(voc, G.features(other)[1], 2)
        out = {"desc": desc, "levelsups": np.array(LEVELSUPS, np.int32), "other_word": ow, "other_value": ov}
        for lu in LEVELSUPS:
            word, node, bw, bv, summ = B.transform(voc, desc, lu)
            out.update({f"lu{lu}_word": word, f"lu{lu}_node": node, f"lu{lu}_bow_word": bw, f"lu{lu}_bow_value_bits": B.bits(bv),
                        f"lu{lu}_norm_bits": B.bits([summ["norm"]])[0]})
        out["score_bits"] = B.bits([B.score(bw, bv, ow, ov)])
        np.savez_compressed(os.path.join(OUT, frame + ".npz"), **out)
        print(frame, len(desc), "rows,", len(bw), "words")


if __name__ == "__main__":
    main()
