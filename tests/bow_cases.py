"""The seeded vocabularies, frames and cached references the bag-of-words tests share (test infrastructure, plain module).

Vocabularies, by name (VOCABS):
    k10      random tree, k = 10, L = 3, depth-first file order (so the file's ids are not the device's breadth-first positions)
    k2_l8    random tree, k = 2, L = 8
    k3       random tree, k = 3, L = 6: nodes with fewer than k children, leaves at every depth from 1 on (a depth-1 leaf is
             shallower than L - levelsup for levelsup <= 4), children with DUPLICATE descriptors (the tie), words of weight 0.0
    l1       k = 10, L = 1: the root's children are the words
    cluster  hierarchical k-majority clustering (k = 6, L = 3) of the oracle descriptors of synth.frame images, idf weights
             ln(N / n_i): related frames share words, a word every training frame has weighs 0.0

The limits (further down): BIG_VOCABS / big_transform (SS_BOW_MAX_ROWS rows per frame), BOUND_CASES (k = 256, 9, 17 and 1, depth 32),
the 640 x 480 / 2000-feature batch (kp_capacity above 1024) and long_score_case (a query of more than 8192 words).
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


# ---- the limits: transforms above 1024 rows, the vocabulary's bounds, long vectors (tests/test_bow.py, tests/test_bow_ref.py) ------
BIG_ROWS = 16384                       # SS_BOW_MAX_ROWS: thread t of k_bow_vector owns 16 sorted positions
BIG_COUNTS = (1025, 2048, 2049, 5000, 16383)  # paddings on both sides of a power of two, all above the 1024 threads
BIG_VOCABS = {
    "k4_l8": lambda: random_tree(0xB008, 4, 8, p_zero=0.05),  # 87380 nodes, 65536 words: thousands of distinct words per frame
    "k10": lambda: vocab("k10"),                              # 1000 words: runs of about 16 equal words
}


@functools.lru_cache(maxsize=None)
def big_vocab(name: str) -> B.Vocab:
    return BIG_VOCABS[name]()


@functools.lru_cache(maxsize=None)
def big_rows() -> np.ndarray:
    return np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(BIG_ROWS, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def big_paths(name: str):
    voc = big_vocab(name)
    return tuple(tuple(B.descend(voc, r)) for r in big_rows())


@functools.lru_cache(maxsize=None)
def big_transform(name: str, levelsup: int, count: int = BIG_ROWS):
    """the first `count` rows of big_rows() under a BIG_VOCABS entry -> (word, node, bow_word, bow_value, summary)"""
    return B.transform_paths(big_vocab(name), big_paths(name)[:count], levelsup)


@functools.lru_cache(maxsize=None)
def one_word_index(name: str = "k10") -> int:
    """the first row of big_rows() whose word has a weight"""
    voc = big_vocab(name)
    return next(i for i, p in enumerate(big_paths(name)) if voc.weight[p[-1]] > 0)


@functools.lru_cache(maxsize=None)
def one_word_transform(name: str, levelsup: int):
    """BIG_ROWS copies of that row: one word, its weight added to itself BIG_ROWS - 1 times"""
    return B.transform_paths(big_vocab(name), (big_paths(name)[one_word_index(name)],) * BIG_ROWS, levelsup)


def longest_run(words) -> int:
    """the most rows one word has among the used rows"""
    return int(np.unique(np.asarray(words), return_counts=True)[1].max()) if len(words) else 0


def _complement(d) -> np.ndarray:
    return np.bitwise_xor(np.asarray(d, np.uint8), np.uint8(255))


# ordinals of the children of a 256-ary node that hold the descriptor of an EARLIER child: (earlier, later)
K256_SAME_LANE = [(3, 43), (7, 255 - 8), (100, 228)]   # later = earlier + 8 m: the same lane of the eight, a later stride
K256_OTHER_LANE = [(21, 100 + 4), (15, 16), (200, 201)]  # another lane; 15 -> 16 is lane 7 against lane 0 of the next stride
K256_INNER = (0, 3, 43, 254, 255)                     # root children of k256_l2 that have 256 children of their own


def _k256_children(rng, around=None) -> np.ndarray:
    """256 random descriptors, or `around` with eight random bits flipped in each (a row equal to one of those is 8 or less from
    `around` and about 128 from unrelated descriptors); the later ordinals of the K256 pairs copy the earlier ones"""
    if around is None:
        d = rng.integers(0, 256, size=(256, 32), dtype=np.uint8)
    else:
        d = np.tile(np.asarray(around, np.uint8), (256, 1))
        for c in range(256):
            for bit in rng.integers(0, 256, 8):
                d[c, bit >> 3] ^= np.uint8(1 << (bit & 7))
    for a, b in K256_SAME_LANE + K256_OTHER_LANE:
        d[b] = d[a]
    return d


@functools.lru_cache(maxsize=None)
def k256_vocab(L: int) -> B.Vocab:
    """k = SS_VOCAB_MAX_K.  L = 1: the root's 256 children are the words.  L = 2: the children K256_INNER of the root have 256
    children each, lying around it (the others are depth-1 leaves); the children of root child 0 all hold ONE descriptor, so a row
    there is equally far from all 256 and ordinal 0 must win.  One word in sixteen weighs 0.0."""
    rng = np.random.Generator(np.random.PCG64(0xB256 + L))
    parent, leaf, desc, weight = [], [], [], []
    top = _k256_children(rng)
    for c in range(256):
        inner = L == 2 and c in K256_INNER
        parent.append(0), leaf.append(int(not inner)), desc.append(top[c])
        weight.append(0.0 if inner or c % 16 == 5 else float(rng.random() * 8 + 1e-3))
    if L == 2:
        for c in K256_INNER:
            sub = _k256_children(rng, top[c])
            if c == 0:
                sub[:] = sub[0]
            for s in range(256):
                parent.append(c + 1), leaf.append(1), desc.append(sub[s])
                weight.append(0.0 if s % 16 == 9 else float(rng.random() * 8 + 1e-3))
    return B.Vocab(256, L, parent, leaf, np.array(desc, np.uint8), weight)


@functools.lru_cache(maxsize=None)
def k256_one_vocab() -> B.Vocab:
    """256 words that all hold ONE descriptor: every row is equally far from all of them, its complement 256 from all of them, and
    ordinal 0 wins every time"""
    d = np.random.Generator(np.random.PCG64(0xB2561)).integers(0, 256, size=(1, 32), dtype=np.uint8)
    return B.Vocab(256, 1, [0] * 256, [1] * 256, np.tile(d, (256, 1)), [1.5] + [2.5] * 255)


@functools.lru_cache(maxsize=None)
def k256_rows(L: int) -> np.ndarray:
    """every child of the root, the complements of some, random rows; L = 2: the one descriptor under root child 0 and root child 0
    itself (8 from all 256), every child of two inner nodes"""
    voc = k256_vocab(L)
    rng = np.random.Generator(np.random.PCG64(0xB2F6 + L))
    top = voc.desc[voc.children[0]]
    rows = [top, _complement(top[[0, 3, 43, 255]]), rng.integers(0, 256, size=(40, 32), dtype=np.uint8)]
    if L == 2:
        under0 = voc.desc[voc.children[1]]
        rows += [under0[:1], voc.desc[1:2]]
        for c in (255, 3):  # the children of an inner node lie around it: a row equal to one goes to c first, then to it
            rows.append(voc.desc[voc.children[c + 1]])
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def spine_vocab() -> B.Vocab:
    """Depth SS_VOCAB_MAX_DEPTH: 32 inner levels (the root and the spine nodes at depths 1 .. 31), each with one leaf sibling; at
    depth 32 both children are leaves.  The spine descriptors are all zero, the leaf at depth d has byte d - 1 set to 0xFF: a row
    equal to that leaf is 8 from the spine and 16 from every earlier leaf, so it leaves the spine exactly at depth d.  The leaf comes
    first at odd depths, the spine node first at even ones (a tie takes the first).  The leaves at depths 5 and 20 weigh 0.0."""
    parent, leaf, desc, weight = [], [], [], []
    spine = 0
    for d in range(1, 33):
        f = np.zeros(32, np.uint8)
        f[d - 1] = 255
        kids = [(1, f, 0.0 if d in (5, 20) else 0.25 + d), (int(d == 32), np.zeros(32, np.uint8), 40.0 if d == 32 else 0.0)]
        if d % 2 == 0:
            kids.reverse()
        ids = []
        for is_leaf, dd, w in kids:
            parent.append(spine), leaf.append(is_leaf), desc.append(dd), weight.append(w)
            ids.append(len(parent))
        spine = ids[0] if d % 2 == 0 else ids[1]
    return B.Vocab(2, 32, parent, leaf, np.array(desc, np.uint8), weight)


SPINE_DEPTHS = (1, 2, 16, 31, 32)
SPINE_LEVELSUPS = (0, 1, 16, 31, 32, 40)


@functools.lru_cache(maxsize=None)
def spine_rows() -> np.ndarray:
    """rows that leave the spine at SPINE_DEPTHS (the leaf itself), at every other depth, ties (four of the leaf's eight bits: 4 from
    both children), the all-zero row (down the spine to depth 32) and random rows"""
    rng = np.random.Generator(np.random.PCG64(0xB5B1))
    rows = []
    for d in list(SPINE_DEPTHS) + list(range(1, 33)):
        f = np.zeros(32, np.uint8)
        f[d - 1] = 255
        rows.append(f)
    for d in (1, 2, 15, 16, 31, 32):
        f = np.zeros(32, np.uint8)
        f[d - 1] = 0x0F
        rows.append(f)
    rows.append(np.zeros(32, np.uint8))
    return np.concatenate([np.array(rows, np.uint8), rng.integers(0, 256, size=(60, 32), dtype=np.uint8),
                           (rng.integers(0, 256, size=(60, 32), dtype=np.uint8) & rng.integers(0, 256, size=(60, 32), dtype=np.uint8)
                            & rng.integers(0, 256, size=(60, 32), dtype=np.uint8))])


def _with_children_as_rows(voc: B.Vocab, seed: int, n_random: int = 150) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([voc.desc[1:][:200], _complement(voc.desc[1:][:20]), rng.integers(0, 256, size=(n_random, 32), dtype=np.uint8)])


# name -> (vocabulary, rows, levelsups): the crafted trees of the descent's bounds
BOUND_CASES = {
    "k256_l1": lambda: (k256_vocab(1), k256_rows(1), (0, 1)),
    "k256_l2": lambda: (k256_vocab(2), k256_rows(2), (0, 1, 2)),
    "k256_one": lambda: (k256_one_vocab(), np.concatenate([k256_one_vocab().desc[1:2], _complement(k256_one_vocab().desc[1:2]),
                                                          big_rows()[:30]]), (0,)),
    "k9": lambda: _bound_random(0xB009, 9),
    "k17": lambda: _bound_random(0xB011, 17),
    "k1_chain": lambda: _bound_random(0xB00C, 1, L=5),
    "spine32": lambda: (spine_vocab(), spine_rows(), SPINE_LEVELSUPS),
}


def _bound_random(seed: int, k: int, L: int = 2):
    voc = random_tree(seed, k, L, p_zero=0.1, p_dup=0.3 if k > 1 else 0.0)
    return voc, _with_children_as_rows(voc, seed + 1), (0, 1, L)


@functools.lru_cache(maxsize=None)
def bound_case(name: str):
    return BOUND_CASES[name]()


@functools.lru_cache(maxsize=None)
def bound_paths(name: str):
    voc, rows, _ = bound_case(name)
    return tuple(tuple(B.descend(voc, r)) for r in rows)


@functools.lru_cache(maxsize=None)
def bound_transform(name: str, levelsup: int):
    return B.transform_paths(bound_case(name)[0], bound_paths(name), levelsup)


# ---- a batch whose kp_capacity is above 1024: 640 x 480 at 2000 features ----------------------------------------------------------
WIDE = ("synth_t0", "synth_t1")
WIDE_SIZE = (640, 480, 2000)  # width, height, n_features


def wide_features(frame: str):
    return G.features(frame, *WIDE_SIZE)


@functools.lru_cache(maxsize=None)
def wide_transform(voc_name: str, frame: str, levelsup: int):
    return B.transform(vocab(voc_name), wide_features(frame)[1], levelsup)


@functools.lru_cache(maxsize=None)
def _wide_found(voc_name: str, levelsup: int, query: str, train):
    qn = wide_transform(voc_name, query, levelsup)[1]
    if train is None:
        return B.search(wide_features(query)[1], qn, None, [])
    return B.search(wide_features(query)[1], qn, wide_features(train)[1], wide_transform(voc_name, train, levelsup)[1])


def wide_reference_pair(voc_name: str, levelsup: int, query: str, train, combo):
    tk = wide_features(train)[0] if train is not None else None
    return G.R.finish(_wide_found(voc_name, levelsup, query, train), wide_features(query)[0], tk, **combo)


# ---- the score at its edges: a query of more than 8192 words ----------------------------------------------------------------------
SCORE_N_DB = (1, 2, 3, 5, 7)


@functools.lru_cache(maxsize=None)
def long_score_case():
    """-> (q_word, q_value, [(word, value)] database vectors, want scores).  The query is the vector of the first frame of the
    k4_l8 transform (more than 8192 words).  The database: the query itself; 1, 63, 64 and 65 words of which every other one is the
    query's; more than 8192 words, half of them the query's; a vector sharing only the query's first word; one sharing only its
    last."""
    rng = np.random.Generator(np.random.PCG64(0x5C1))
    _, _, qw, qv, _ = big_transform("k4_l8", 2)
    others = np.setdiff1d(np.arange(big_vocab("k4_l8").n_words, dtype=np.int32), qw)
    inside = others[(others > qw[0]) & (others < qw[-1])]

    def mixed(m):
        w = np.sort(np.concatenate([rng.choice(qw, (m + 1) // 2, replace=False), rng.choice(others, m // 2, replace=False)])).astype(np.int32)
        v = rng.random(m) + 1e-3
        return w, v / v.sum()

    def sharing(word):
        w = np.sort(np.concatenate([[word], rng.choice(inside, 200, replace=False)])).astype(np.int32)
        return w, np.full(len(w), 1.0 / len(w))

    db = [(qw, qv), mixed(1), mixed(63), mixed(64), mixed(65), mixed(9000), sharing(qw[0]), sharing(qw[-1])]
    want = np.array([B.score(qw, qv, w, v) for w, v in db], np.float64)
    return qw, qv, db, want
