"""numpy / plain-Python restatement of the bag-of-words rules (test infrastructure, plain module).

Written from the rule's description (include/sendslam_orb.h, DESIGN.md "Bag of words"), not from the kernels: serial loops, Python
floats (IEEE doubles, every operation rounded once).  The device code must reproduce words, nodes, vector words, the bit patterns
of values / norm / scores, idx / d1 / d2 and every summary field.

    parse_text   DBoW2's text format -> Vocab (node ids are the file's, word ids count the leaves in file order)
    descend      root -> leaf, the nearest child at every node, ties to the earliest child; the path of node ids
    transform    word / node of every row, the BoW vector (addWeight, normalize(L1)) and the summary of one frame
    search       SearchByBoW's candidate sets (train rows of the query's node) -> what guided_ref.finish takes
    score        L1Scoring::score of two vectors
"""
from __future__ import annotations

import math
import re

import numpy as np

import guided_ref as R

MAX_K, MAX_DEPTH, MAX_NODES = 256, 32, 1 << 24
SUMMARY_FIELDS = ("status", "n_rows", "n_used", "n_words", "n_nodes", "reserved", "norm")
_INT = re.compile(r"-?[0-9]{1,9}\Z")
_FLOAT_CHARS = set("0123456789+-.eE")
_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)


class Vocab:
    """the linked tree: arrays indexed by node id (0 = the root)"""

    def __init__(self, k, L, parent, is_leaf, desc, weight):
        n = len(parent)
        if not 1 <= k <= MAX_K or not 1 <= L <= MAX_DEPTH:
            raise ValueError("k or L outside its bounds")
        if n < 1:
            raise ValueError("no nodes")
        if n >= MAX_NODES:
            raise ValueError("too many nodes")
        self.k, self.L, self.n_nodes = int(k), int(L), n
        self.parent = np.concatenate([[-1], np.asarray(parent, np.int64)])
        self.leaf = np.concatenate([[0], np.asarray(is_leaf, np.int64)]).astype(bool)
        self.desc = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(desc, np.uint8).reshape(n, 32)])
        self.children = [[] for _ in range(n + 1)]
        self.depth = np.zeros(n + 1, np.int32)
        for i in range(1, n + 1):
            p = int(self.parent[i])
            if p < 0 or p >= i:
                raise ValueError(f"node {i}: parent {p} is no earlier node")
            if self.leaf[p]:
                raise ValueError(f"leaf {p} has a child")
            self.children[p].append(i)
            if len(self.children[p]) > k:
                raise ValueError(f"node {p} has more than k children")
            self.depth[i] = self.depth[p] + 1
            if self.depth[i] > MAX_DEPTH:
                raise ValueError("too deep")
        self.word = np.full(n + 1, -1, np.int32)
        self.weight = np.zeros(n + 1, np.float64)
        w = 0
        for i in range(1, n + 1):
            if self.leaf[i]:
                self.word[i] = w
                self.weight[i] = weight[i - 1]
                w += 1
            elif not self.children[i]:
                raise ValueError(f"inner node {i} has no children")
        self.n_words = w
        self.max_depth = int(self.depth[self.leaf].max())
        self.word_weight = self.weight[self.leaf]  # by word id
        self.first_child = np.array([c[0] if c else -1 for c in self.children], np.int32)
        self.n_children = np.array([len(c) for c in self.children], np.int32)

    def info(self) -> dict:
        return {"k": self.k, "L": self.L, "n_nodes": self.n_nodes, "n_words": self.n_words, "max_depth": self.max_depth}

    def arrays(self):
        """-> parent, is_leaf, desc, weight of the nodes 1 .. n, what the file holds"""
        return self.parent[1:].astype(np.int32), self.leaf[1:].astype(np.uint8), self.desc[1:], self.weight[1:].copy()


def _weight(tok: str) -> float:
    if not tok or len(tok) >= 64 or not set(tok) <= _FLOAT_CHARS or not any(ch.isdigit() for ch in tok):
        raise ValueError("the weight is no number")
    return float(tok)  # correctly rounded, like strtod


def parse_text(path: str) -> Vocab:
    """ValueError for everything ss_vocab_load_text answers with SS_ERR_INVALID_ARG"""
    header = None
    parent, leaf, desc, weight = [], [], [], []
    with open(path, "rb") as f:
        text = f.read().decode("latin-1")
    for ln, line in enumerate(text.split("\n"), 1):
        toks = [t for t in re.split(r"[ \t\r]+", line) if t]
        if not toks:
            continue
        want = 4 if header is None else 34
        ints = toks[:want]
        for t in ints:
            if not _INT.match(t):
                raise ValueError(f"line {ln}: {t!r} is no integer")
        if len(ints) < want:
            raise ValueError(f"line {ln}: truncated")
        vals = [int(t) for t in ints]
        if header is None:
            if len(toks) != 4:
                raise ValueError(f"line {ln}: header with {len(toks)} tokens")
            if vals[2] != 0 or vals[3] != 0:
                raise ValueError("only L1 scoring with TF-IDF weighting")
            header = vals
            continue
        if len(toks) < 35:
            raise ValueError(f"line {ln}: truncated")
        w = _weight(toks[34])
        if len(toks) > 35:
            raise ValueError(f"line {ln}: too many tokens")
        if vals[1] not in (0, 1):
            raise ValueError(f"line {ln}: is_leaf")
        if any(b < 0 or b > 255 for b in vals[2:]):
            raise ValueError(f"line {ln}: byte outside 0 .. 255")
        parent.append(vals[0])
        leaf.append(vals[1])
        desc.append(vals[2:])
        weight.append(w)
    if header is None:
        raise ValueError("no header")
    return Vocab(header[0], header[1], parent, leaf, np.array(desc, np.uint8).reshape(-1, 32), weight)


def descend(voc: Vocab, row) -> list:
    """the node ids from the first level down to the leaf"""
    row = np.asarray(row, np.uint8)
    cur, path = 0, []
    while not voc.leaf[cur]:
        best, best_d = -1, 1 << 30
        for ch in voc.children[cur]:  # file order; strict <: the earliest of equally near children
            d = int(_POP[voc.desc[ch] ^ row].sum())
            if d < best_d:
                best, best_d = ch, d
        cur = best
        path.append(cur)
    return path


def node_of(voc: Vocab, path, levelsup: int) -> int:
    """the path's node at depth L - levelsup; 0 when that is <= 0; the leaf when the path is shorter (the documented deviation);
    -1 when the leaf's weight is not > 0"""
    if not voc.weight[path[-1]] > 0:
        return -1
    target = voc.L - levelsup
    if target <= 0:
        return 0
    return path[target - 1] if target <= len(path) else path[-1]


def bow_vector(words, weights):
    """BowVector::addWeight per used row, then normalize(L1) -> (ascending words, values, norm)"""
    seen = {}
    for wd, w in zip(words, weights):
        w = float(w)
        if not w > 0:
            continue
        seen[int(wd)] = seen[int(wd)] + w if int(wd) in seen else w  # all addends of a word are equal: the order cannot matter
    ids = sorted(seen)
    vals = [seen[i] for i in ids]
    norm = 0.0
    for v in vals:  # one serial chain, ascending word id
        norm += math.fabs(v)
    if norm > 0.0:
        vals = [v / norm for v in vals]
    return np.array(ids, np.int32), np.array(vals, np.float64), norm


def transform_paths(voc: Vocab, paths, levelsup: int, status: int = 0):
    """one frame from the paths of its rows -> (word, node, bow_word, bow_value, summary dict)"""
    n = len(paths)
    word = np.array([voc.word[p[-1]] for p in paths], np.int32).reshape(n)
    node = np.array([node_of(voc, p, levelsup) for p in paths], np.int32).reshape(n)
    bw, bv, norm = bow_vector(word, [voc.weight[p[-1]] for p in paths])
    summary = {"status": status, "n_rows": n, "n_used": int((node >= 0).sum()), "n_words": len(bw),
               "n_nodes": len(set(int(v) for v in node if v >= 0)), "reserved": 0, "norm": norm}
    return word, node, bw, bv, summary


def transform(voc: Vocab, desc, levelsup: int):
    return transform_paths(voc, [descend(voc, r) for r in np.asarray(desc, np.uint8).reshape(-1, 32)], levelsup)


def node_candidates(q_node, t_node, exclude_self: bool = False) -> list:
    """per query the ascending train rows of its node; a query without a node (-1) has none"""
    rows = {}
    for j, nd in enumerate(t_node):
        if nd >= 0:
            rows.setdefault(int(nd), []).append(j)
    return [[j for j in rows.get(int(nd), []) if not (exclude_self and j == i)] if nd >= 0 else [] for i, nd in enumerate(q_node)]


def search(q_desc, q_node, t_desc, t_node, exclude_self: bool = False):
    """guided_ref.search with the node sets in place of the windows -> (best row or -1, d1, d2, candidate lists); t_desc None =
    no train frame"""
    nq = len(q_node)
    best_row, d1, d2 = R.none_result(nq)
    cands = [[] for _ in range(nq)]
    if nq and t_desc is not None and len(t_node):
        cands = node_candidates(q_node, t_node, exclude_self)
        q = np.asarray(q_desc, np.uint8).reshape(-1, 32)
        t = np.asarray(t_desc, np.uint8).reshape(-1, 32)
        for i, cs in enumerate(cands):
            if not cs:
                continue
            dist = _POP[t[cs] ^ q[i]].sum(axis=1)
            best, second, best_j = R.NONE, R.NONE, -1
            for j, d in zip(cs, dist):  # ascending j
                d = int(d)
                if d < best:
                    second, best, best_j = best, d, j
                elif d < second:
                    second = d
            best_row[i], d1[i], d2[i] = best_j, best, second
    return best_row, d1, d2, cands


def match(q_kp, q_desc, q_node, t_kp, t_desc, t_node, th=50, ratio_num=7, ratio_den=10, one_to_one=False, orientation=0,
          exclude_self=False):
    """one (query frame, train frame) pair; t_kp None = no train frame -> (idx, d1, d2, summary dict, candidate lists)"""
    found = search(q_desc, q_node, None if t_kp is None else t_desc, [] if t_kp is None else t_node, exclude_self)
    return R.finish(found, q_kp, t_kp, th, ratio_num, ratio_den, one_to_one, orientation)


def score(q_word, q_value, d_word, d_value) -> float:
    """L1Scoring::score; an empty side gives 0.0, no common word -0.0"""
    if len(q_word) == 0 or len(d_word) == 0:
        return 0.0
    s, i, j = 0.0, 0, 0
    while i < len(q_word) and j < len(d_word):
        if q_word[i] == d_word[j]:
            v, w = float(q_value[i]), float(d_value[j])
            t = math.fabs(v - w)
            t = t - math.fabs(v)
            t = t - math.fabs(w)
            s += t
            i += 1
            j += 1
        elif q_word[i] < d_word[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0


def bits(x) -> np.ndarray:
    """the raw 64-bit patterns of doubles"""
    return np.ascontiguousarray(x, np.float64).view(np.uint64)
