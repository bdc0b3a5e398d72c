"""The seeded vocabularies, frames and cached references the bag-of-words tests share (test infrastructure, plain module).

Vocabularies, by name (VOCABS):
    k10      random tree, k = 10, L = 3, depth-first file order (so the file's ids are not the device's breadth-first positions)
    k2_l8    random tree, k = 2, L = 8
    k3       random tree, k = 3, L = 6: nodes with fewer than k children, leaves at every depth from 1 on (a depth-1 leaf is
             shallower than L - levelsup for levelsup <= 4), children with DUPLICATE descriptors (the tie), words of weight 0.0
    l1       k = 10, L = 1: the root's children are the words
    cluster  hierarchical k-majority clustering (k = 6, L = 3) of the oracle descriptors of synth.frame images, idf weights
             ln(N / n_i): related frames share words, a word every training frame has weighs 0.0
"""
from __future__ import annotations

import functools
import math

import numpy as np

import bow_ref as B
import guided_cases as G

BATCH = ["synth_t0", "synth_t1", "synth_t2", "synth_t3", "dots", "checker", "noise", "flat"]  # flat: no keypoints
LEVELSUPS = (0, 2, 4, 9)  # 9 >= every L here


def random_tree(seed: int, k: int, L: int, p_leaf: float = 0.0, p_few: float = 0.0, p_zero: float = 0.0, p_dup: float = 0.0,
                depth_first: bool = False) -> B.Vocab:
    """A seeded tree: a node above depth L becomes a leaf with p_leaf, has 1 .. k - 1 children with p_few (else k), a child copies
    an earlier sibling's descriptor with p_dup, a word weighs 0.0 with p_zero.  File order: breadth first, or depth first."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, leaf, desc, weight = [], [], [], []

    def add(p, d, depth):
        parent.append(p)
        is_leaf = depth == L or (depth >= 1 and rng.random() < p_leaf)
        leaf.append(int(is_leaf))
        desc.append(d)
        weight.append((0.0 if rng.random() < p_zero else float(rng.random() * 8 + 1e-3)) if is_leaf else 0.0)
        return len(parent), is_leaf  # the node's id

    def children_of(depth):
        n = int(rng.integers(1, k)) if (k > 1 and rng.random() < p_few) else k
        ds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        for c in range(1, n):
            if rng.random() < p_dup:
                ds[c] = ds[int(rng.integers(0, c))]
        return ds

    if depth_first:
        def grow(pid, depth):
            for d in children_of(depth):
                cid, is_leaf = add(pid, d, depth + 1)
                if not is_leaf:
                    grow(cid, depth + 1)
        grow(0, 0)
    else:
        level = [(0, 0)]
        while level:
            nxt = []
            for pid, depth in level:
                for d in children_of(depth):
                    cid, is_leaf = add(pid, d, depth + 1)
                    if not is_leaf:
                        nxt.append((cid, depth + 1))
            level = nxt
    return B.Vocab(k, L, parent, leaf, np.array(desc, np.uint8), weight)


def _majority(rows: np.ndarray) -> np.ndarray:
    bits = np.unpackbits(rows, axis=1)
    return np.packbits((bits.sum(axis=0) * 2 > len(rows)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def cluster_vocab(k: int = 6, L: int = 3, seed: int = 0xB0C) -> B.Vocab:
    train = ["synth_t0", "synth_t2", "synth_t4", "parallax_t0", "parallax_t3", "dots", "checker"]
    descs = [G.features(n)[1] for n in train]
    rows = np.concatenate(descs)
    frame_of = np.concatenate([np.full(len(d), i) for i, d in enumerate(descs)])
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, leaf, desc, weight = [], [], [], []

    def split(pid, members, depth):
        sub = rows[members]
        uniq = np.unique(sub, axis=0)
        kk = min(k, len(uniq))
        centres = uniq[rng.choice(len(uniq), kk, replace=False)]
        for _ in range(3):
            own = R_dist(sub, centres).argmin(axis=1)
            centres = np.array([_majority(sub[own == c]) if (own == c).any() else centres[c] for c in range(kk)])
        own = R_dist(sub, centres).argmin(axis=1)
        for c in range(kk):
            m = members[own == c]
            if len(m) == 0:
                continue
            is_leaf = depth + 1 == L or len(np.unique(rows[m], axis=0)) <= 1
            parent.append(pid)
            leaf.append(int(is_leaf))
            desc.append(centres[c])
            n_i = len(set(frame_of[m]))
            weight.append(math.log(len(train) / n_i) if is_leaf else 0.0)
            cid = len(parent)
            if not is_leaf:
                split(cid, m, depth + 1)

    split(0, np.arange(len(rows)), 0)
    return B.Vocab(k, L, parent, leaf, np.array(desc, np.uint8), weight)


def R_dist(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    import guided_ref
    return guided_ref.distances(a, b).astype(np.int64)


VOCABS = {
    "k10": lambda: random_tree(0xB001, 10, 3, p_zero=0.05, depth_first=True),
    "k2_l8": lambda: random_tree(0xB002, 2, 8, p_leaf=0.05, p_zero=0.05),
    "k3": lambda: random_tree(0xB126, 3, 6, p_leaf=0.15, p_few=0.3, p_zero=0.15, p_dup=0.25, depth_first=True),
    "l1": lambda: random_tree(0xB004, 10, 1, p_zero=0.2, p_dup=0.3),
    "cluster": cluster_vocab,
}


@functools.lru_cache(maxsize=None)
def vocab(name: str) -> B.Vocab:
    return VOCABS[name]()


@functools.lru_cache(maxsize=None)
def paths(voc_name: str, frame: str):
    """the descent of every oracle descriptor of a named 320 x 240 / 500 frame: computed once, whatever levelsup"""
    voc = vocab(voc_name)
    return tuple(tuple(B.descend(voc, r)) for r in G.features(frame)[1])


@functools.lru_cache(maxsize=None)
def frame_transform(voc_name: str, frame: str, levelsup: int):
    """-> (word, node, bow_word, bow_value, summary) of a named frame"""
    return B.transform_paths(vocab(voc_name), paths(voc_name, frame), levelsup)


@functools.lru_cache(maxsize=None)
def _found(voc_name: str, levelsup: int, query: str, train, exclude_self: bool):
    qn = frame_transform(voc_name, query, levelsup)[1]
    if train is None:
        return B.search(G.features(query)[1], qn, None, [], exclude_self)
    return B.search(G.features(query)[1], qn, G.features(train)[1], frame_transform(voc_name, train, levelsup)[1], exclude_self)


def reference_pair(voc_name: str, levelsup: int, query: str, train, combo, exclude_self: bool = False):
    qk = G.features(query)[0]
    tk = G.features(train)[0] if train is not None else None
    return G.R.finish(_found(voc_name, levelsup, query, train, exclude_self), qk, tk, **combo)


def write(path: str, voc: B.Vocab, **kw) -> None:
    from send_slam_amd import bow
    bow.write_text(path, voc.k, voc.L, *voc.arrays(), **kw)


def library_vocab(voc: B.Vocab):
    from send_slam_amd import binding
    return binding.Vocabulary.from_arrays(*voc.arrays(), voc.k, voc.L)
