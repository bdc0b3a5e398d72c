"""Writer for DBoW2's vocabulary text format, the one `binding.Vocabulary.load_text` (ss_vocab_load_text) reads.

    k L scoring weighting
    parent_id is_leaf b0 ... b31 weight        one line per node; line n (from 0) is node n + 1, the root is node 0

Weights are written with repr(), the shortest decimal that reads back to the same double.
"""
from __future__ import annotations

import numpy as np


def write_text(path: str, k: int, L: int, parent, is_leaf, desc, weight, scoring: int = 0, weighting: int = 0) -> None:
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    with open(path, "w") as f:
        f.write(f"{int(k)} {int(L)} {int(scoring)} {int(weighting)}\n")
        for p, leaf, d, w in zip(parent, is_leaf, desc, weight):
            f.write(f"{int(p)} {int(leaf)} {' '.join(str(int(b)) for b in d)} {float(w)!r}\n")
