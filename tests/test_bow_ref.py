"""CPU tests of the bag-of-words path: the C vocabulary loader against the Python parser of tests/bow_ref.py, the malformed
files, the ABI boundary, and properties of the reference rules the GPU tests (tests/test_bow.py) are compared with."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import bow_cases as BC
import bow_ref as B
import guided_cases as G
import guided_ref as R
from send_slam_amd import binding


def _same_tree(lib_voc, ref: B.Vocab):
    assert lib_voc.info() == ref.info()
    out = lib_voc.copy_out()
    for name, want in (("first_child", ref.first_child), ("n_children", ref.n_children), ("word", ref.word), ("depth", ref.depth)):
        assert np.array_equal(out[name], want), name
    assert np.array_equal(B.bits(out["weight"]), B.bits(ref.weight)), "weights differ in some bit"


@pytest.mark.parametrize("name", list(BC.VOCABS))
def test_loader_equals_the_python_parser_and_the_array_form(tmp_path, name):
    voc = BC.vocab(name)
    path = str(tmp_path / (name + ".txt"))
    BC.write(path, voc)
    ref = B.parse_text(path)
    assert ref.info() == voc.info() and np.array_equal(B.bits(ref.weight), B.bits(voc.weight)) and np.array_equal(ref.desc, voc.desc)
    with binding.Vocabulary.load_text(path) as lv, BC.library_vocab(voc) as av:
        _same_tree(lv, ref)
        _same_tree(av, ref)


def test_weights_are_correctly_rounded_and_blank_lines_are_skipped(tmp_path):
    path = str(tmp_path / "w.txt")
    ws = ["0.1", "1e-310", "2.2250738585072011e-308", "0.30000000000000004", "17", "1.7976931348623157e308", "+.5e1", "0", "-0.0", "3.00"]
    with open(path, "w") as f:
        f.write("10 1 0 0 \r\n\n")
        for i, w in enumerate(ws):
            f.write(f"0 1 {' '.join(str((i * 7 + b) % 256) for b in range(32))}  {w} \n")
        f.write("\n  \n")
    ref = B.parse_text(path)
    assert np.array_equal(B.bits(ref.weight[1:]), B.bits([float(w) for w in ws]))
    with binding.Vocabulary.load_text(path) as lv:
        _same_tree(lv, ref)


def _line(parent, leaf, weight="1.5", desc=None):
    return f"{parent} {leaf} {' '.join(str(b) for b in (desc or range(32)))} {weight}\n"


MALFORMED = {
    "truncated_line": "3 2 0 0\n" + _line(0, 1) + "0 1 1 2 3\n",
    "missing_weight": "3 2 0 0\n" + " ".join(["0", "1"] + ["7"] * 32) + "\n",
    "byte_above_255": "3 2 0 0\n" + _line(0, 1, desc=[256] + [0] * 31),
    "negative_byte": "3 2 0 0\n" + _line(0, 1, desc=[-1] + [0] * 31),
    "parent_is_itself": "3 2 0 0\n" + _line(0, 0) + _line(2, 1),
    "parent_later": "3 2 0 0\n" + _line(0, 0) + _line(3, 1) + _line(1, 1),
    "parent_unknown": "3 2 0 0\n" + _line(0, 0) + _line(40, 1),
    "parent_negative": "3 2 0 0\n" + _line(-1, 1),
    "more_than_k_children": "3 2 0 0\n" + _line(0, 1) * 4,
    "inner_node_without_children": "3 2 0 0\n" + _line(0, 1) + _line(0, 0),
    "leaf_with_children": "3 2 0 0\n" + _line(0, 1) + _line(1, 1),
    "zero_nodes": "3 2 0 0\n",
    "empty_file": "",
    "non_numeric_token": "3 2 0 0\n" + _line(0, 1, desc=["x"] + [0] * 31),
    "non_numeric_weight": "3 2 0 0\n" + _line(0, 1, weight="heavy"),
    "hex_weight": "3 2 0 0\n" + _line(0, 1, weight="0x10"),
    "non_numeric_header": "k 2 0 0\n" + _line(0, 1),
    "short_header": "3 2 0\n" + _line(0, 1),
    "long_line": "3 2 0 0\n" + _line(0, 1, weight="1.5 9"),
    "is_leaf_2": "3 2 0 0\n" + _line(0, 2),
    "scoring_1": "3 2 1 0\n" + _line(0, 1),
    "weighting_1": "3 2 0 1\n" + _line(0, 1),
    "k_0": "0 2 0 0\n" + _line(0, 1),
    "k_above_bound": "257 2 0 0\n" + _line(0, 1),
    "L_above_bound": "3 33 0 0\n" + _line(0, 1),
    "huge_number": "3 2 0 0\n" + _line(0, 1, desc=[10 ** 12] + [0] * 31),
    # L within its bound, the tree one level deeper than SS_VOCAB_MAX_DEPTH; k = SS_VOCAB_MAX_K with 257 children of the root
    "depth_33": "1 32 0 0\n" + "".join(_line(d, int(d == 32)) for d in range(33)),
    "child_257": "256 1 0 0\n" + _line(0, 1) * 257,
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_files_are_refused_with_a_message(tmp_path, case):
    path = str(tmp_path / (case + ".txt"))
    with open(path, "w") as f:
        f.write(MALFORMED[case])
    with pytest.raises(ValueError):
        B.parse_text(path)
    with pytest.raises(binding.OrbError) as e:
        binding.Vocabulary.load_text(path)
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "vocabulary" in e.value.message, e.value.message
    print(case, "->", e.value.message)


def test_missing_file_and_bad_arrays_are_refused():
    with pytest.raises(binding.OrbError) as e:
        binding.Vocabulary.load_text("/nonexistent/voc.txt")
    assert e.value.code == binding.SS_ERR_INVALID_ARG and "cannot open" in e.value.message
    d = np.zeros((2, 32), np.uint8)
    for parent, leaf, k, L in (([0, 2], [0, 1], 3, 2), ([0, 0], [1, 0], 3, 2), ([0, 0], [1, 1], 1, 2), ([0, 0], [1, 1], 3, 0)):
        with pytest.raises(binding.OrbError) as e:
            binding.Vocabulary.from_arrays(parent, leaf, d, [1.0, 1.0], k, L)
        assert e.value.code == binding.SS_ERR_INVALID_ARG
    # the bounds themselves pass, one past them does not: k = SS_VOCAB_MAX_K + 1, a chain of depth SS_VOCAB_MAX_DEPTH + 1 under L = 32
    chain = lambda n: (list(range(n)), [0] * (n - 1) + [1], np.zeros((n, 32), np.uint8), [1.0] * n)
    with binding.Vocabulary.from_arrays(*chain(32), 1, 32) as lv:
        assert lv.info()["max_depth"] == 32 == B.Vocab(1, 32, *chain(32)).max_depth
    with binding.Vocabulary.from_arrays([0] * 256, [1] * 256, np.zeros((256, 32), np.uint8), [1.0] * 256, 256, 1) as lv:
        assert lv.info()["n_words"] == 256
    for args in ((*chain(33), 1, 32), ([0] * 2, [1] * 2, d, [1.0] * 2, binding.SS_VOCAB_MAX_K + 1, 1),
                 ([0] * 257, [1] * 257, np.zeros((257, 32), np.uint8), [1.0] * 257, 256, 1)):
        with pytest.raises(binding.OrbError) as e:
            binding.Vocabulary.from_arrays(*args)
        assert e.value.code == binding.SS_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            B.Vocab(args[4], args[5], *args[:4])
    # a short error buffer is filled without overflow, a NULL one is allowed
    lib = binding.load()
    h, err = C.c_void_p(), C.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.ss_vocab_load_text(b"/nonexistent/voc.txt", C.byref(h), err, 8) == binding.SS_ERR_INVALID_ARG
    assert err.raw[7] == 0 and err.raw[8:] == b"\x7f" * 8 and not h.value
    assert lib.ss_vocab_load_text(b"/nonexistent/voc.txt", C.byref(h), None, 0) == binding.SS_ERR_INVALID_ARG


def test_symbols_are_declared_exported_and_bound_and_struct_sizes_match():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sendslam_orb.h")).read()
    lib = binding.load()
    names = ["ss_vocab_load_text", "ss_vocab_from_arrays", "ss_vocab_info", "ss_vocab_copy_out", "ss_vocab_destroy", "ss_bow_set_vocabulary",
             "ss_bow_transform_device", "ss_bow_transform_batch_device", "ss_match_bow_pairs_device", "ss_match_bow_batch_device",
             "ss_bow_score_device"]
    for n in names:
        assert ("int " + n + "(") in header and hasattr(lib, n) and n in binding.EXPORTS, n
    assert C.sizeof(binding.BowSummary) == binding.BOW_SUMMARY_DTYPE.itemsize == 32 and "/* 32 bytes, one per frame */" in header
    assert C.sizeof(binding.VocabShape) == 20
    assert lib.ss_abi_version() == 5
    for macro, val in (("SS_VOCAB_MAX_K", 256), ("SS_VOCAB_MAX_DEPTH", 32), ("SS_VOCAB_MAX_NODES", "(1 << 24)"), ("SS_BOW_MAX_ROWS", "SS_GUIDED_MAX_ROWS")):
        assert f"#define {macro} {val}" in header
    assert (binding.SS_VOCAB_MAX_K, binding.SS_VOCAB_MAX_DEPTH, binding.SS_VOCAB_MAX_NODES) == (B.MAX_K, B.MAX_DEPTH, B.MAX_NODES) == (256, 32, 1 << 24)
    assert B.MAX_K >= 32 and B.MAX_DEPTH >= 16 and B.MAX_NODES >= 1 << 21


def test_the_case_vocabularies_hold_what_they_claim():
    ks = {n: BC.vocab(n) for n in BC.VOCABS}
    assert (ks["k10"].k, ks["k2_l8"].k, ks["k2_l8"].L, ks["k3"].k, ks["l1"].L) == (10, 2, 8, 3, 1)
    assert ks["k2_l8"].max_depth == 8 and ks["l1"].max_depth == 1 and ks["l1"].n_words == 10
    v = ks["k3"]
    leaf_depths = set(int(d) for d in v.depth[v.leaf])
    assert min(leaf_depths) == 1 and max(leaf_depths) == v.L  # a depth-1 leaf is shallower than L - levelsup for levelsup 0, 2
    dup = [p for p in range(v.n_nodes + 1) if len(v.children[p]) > len(set(v.desc[c].tobytes() for c in v.children[p]))]
    assert 0 in dup or len(dup) > 3, "no node with duplicate children"
    assert any(len(c) not in (0, v.k) for c in v.children)
    for n, v in ks.items():
        assert (v.word_weight == 0.0).any(), f"{n}: no word of weight 0.0"
    # a row that reaches the depth-1 leaf of k3 keeps the leaf as its node
    v = ks["k3"]
    shallow = [i for i in v.children[0] if v.leaf[i] and v.weight[i] > 0]
    assert shallow
    word, node, *_ = B.transform(v, v.desc[shallow[0]][None], 0)
    assert node[0] == shallow[0] or v.desc[shallow[0]].tobytes() in [v.desc[c].tobytes() for c in v.children[0] if c < shallow[0]]
    # the tie: a row equal to duplicated children goes to the earliest of them
    p = dup[0]
    cs = v.children[p]
    later = next(c for i, c in enumerate(cs) if v.desc[c].tobytes() in [v.desc[o].tobytes() for o in cs[:i]])
    first = next(o for o in cs if v.desc[o].tobytes() == v.desc[later].tobytes())
    sub = B.Vocab(v.k, v.L, *_subtree(v, p))
    assert B.descend(sub, v.desc[later])[0] == cs.index(first) + 1


def _subtree(v: B.Vocab, p: int):
    """the children of p as a one-level vocabulary"""
    cs = v.children[p]
    return [0] * len(cs), [1] * len(cs), v.desc[cs], [1.0] * len(cs)


def test_vector_values_sum_to_one_and_words_ascend():
    for name in BC.VOCABS:
        for frame in ("synth_t0", "noise"):
            word, node, bw, bv, summ = BC.frame_transform(name, frame, 2)
            assert (np.diff(bw) > 0).all() and len(bw) == summ["n_words"] > 0
            assert abs(float(np.sum(bv)) - 1.0) <= len(bv) * np.finfo(np.float64).eps
            assert summ["n_used"] == int((node >= 0).sum()) <= summ["n_rows"] == len(word)
            assert set(bw) == set(int(w) for w, n in zip(word, node) if n >= 0)


def test_repeated_addition_is_visible():
    """0.1 added to itself 10 times is not 10 * 0.1 rounded once"""
    bw, bv, norm = B.bow_vector([3] * 10 + [5], [0.1] * 10 + [0.7])
    acc = 0.1
    for _ in range(9):
        acc += 0.1
    assert acc != 0.1 * 10 and norm == acc + 0.7 and list(bw) == [3, 5] and bv[0] == acc / norm
    bw, bv, norm = B.bow_vector([3, 4], [0.0, -1.0])
    assert len(bw) == 0 and norm == 0.0


def test_score_properties():
    a = BC.frame_transform("cluster", "synth_t0", 2)
    b = BC.frame_transform("cluster", "noise", 2)
    assert abs(B.score(a[2], a[3], a[2], a[3]) - 1.0) <= len(a[2]) * np.finfo(np.float64).eps
    disjoint = B.score([1, 3, 5], [0.2, 0.3, 0.5], [0, 2, 4, 6], [0.25] * 4)
    assert disjoint == 0.0
    assert B.score([], [], a[2], a[3]) == 0.0 and B.score(a[2], a[3], [], []) == 0.0
    assert 0.0 <= B.score(a[2], a[3], b[2], b[3]) <= 1.0
    assert B.score([1, 4], [0.5, 0.5], [4, 9], [0.5, 0.5]) == 0.5


def test_levelsup_at_least_L_is_guided_matching_with_an_all_covering_window():
    combo = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=1)
    for name in ("k3", "cluster"):
        voc = BC.vocab(name)
        qn = BC.frame_transform(name, "synth_t1", voc.L)[1]
        tn = BC.frame_transform(name, "synth_t0", voc.L + 3)[1]
        assert set(qn) <= {0, -1} and set(tn) <= {0, -1} and (qn == 0).sum() > 100
        (qk, qd), (tk, td) = G.features("synth_t1"), G.features("synth_t0")
        qu, tu = np.flatnonzero(qn == 0), np.flatnonzero(tn == 0)
        got = B.match(qk[qu], qd[qu], qn[qu], tk[tu], td[tu], tn[tu], **combo)
        want = R.match(qk[qu], qd[qu], tk[tu], td[tu], R.whole_windows(len(qu)), **combo)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3] and got[3]["n_final"] > 20


def test_related_frames_score_higher_and_node_sets_are_smaller_than_all_pairs():
    t0, t1, noise = (BC.frame_transform("cluster", f, 1) for f in ("synth_t0", "synth_t1", "noise"))
    s_seq, s_noise = B.score(t1[2], t1[3], t0[2], t0[3]), B.score(t1[2], t1[3], noise[2], noise[3])
    print(f"score synth_t1 vs synth_t0 {s_seq:.4f}, vs noise {s_noise:.4f}")
    assert s_seq > s_noise
    cands = B.node_candidates(t1[1], t0[1])
    n_node, n_all = sum(len(c) for c in cands), len(t1[1]) * len(t0[1])
    print(f"candidates: node sets {n_node}, all pairs {n_all}")
    assert 0 < n_node < n_all
    # and the matches they give are mostly the all-pairs matcher's: the same best train row where both accept
    combo = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=False, orientation=0)
    (qk, qd), (tk, td) = G.features("synth_t1"), G.features("synth_t0")
    got = B.match(qk, qd, t1[1], tk, td, t0[1], **combo)
    want = R.match(qk, qd, tk, td, R.whole_windows(len(qk)), **combo)
    both = (got[0] >= 0) & (want[0] >= 0)
    assert both.sum() > 50 and (got[0][both] == want[0][both]).mean() > 0.9


def test_goldens_equal_the_reference(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "bow", "*.npz")))
    assert files
    voc = B.parse_text(os.path.join(golden_dir, "bow", "k3_vocabulary.txt"))
    with binding.Vocabulary.load_text(os.path.join(golden_dir, "bow", "k3_vocabulary.txt")) as lv:
        _same_tree(lv, voc)
    for path in files:
        g = np.load(path)
        for lu in (int(v) for v in g["levelsups"]):
            word, node, bw, bv, summ = B.transform(voc, g["desc"], lu)
            assert np.array_equal(word, g[f"lu{lu}_word"]) and np.array_equal(node, g[f"lu{lu}_node"]) and np.array_equal(bw, g[f"lu{lu}_bow_word"])
            assert np.array_equal(B.bits(bv), g[f"lu{lu}_bow_value_bits"]) and B.bits([summ["norm"]])[0] == g[f"lu{lu}_norm_bits"]
        assert np.array_equal(B.bits([B.score(bw, bv, g["other_word"], g["other_value"])]), g["score_bits"])


# ---- the limit cases of tests/bow_cases.py reach what they are meant for ----------------------------------------------------------
def test_big_transforms_give_every_thread_several_positions():
    """k_bow_vector's thread t owns ceil(n2 / 1024) sorted positions, n2 the count rounded up to a power of two: every count is
    above 1024, on both sides of a power of two; k4_l8 gives more than 8192 distinct words, k10 runs longer than the 16 positions a
    thread owns at 16384 rows, and one row repeated gives one run over everything"""
    assert BC.BIG_ROWS == binding.SS_BOW_MAX_ROWS == 16384 and BC.big_vocab("k4_l8").info() == {"k": 4, "L": 8, "n_nodes": 87380, "n_words": 65536, "max_depth": 8}
    full = BC.big_transform("k4_l8", 2)
    print(full[4])
    assert full[4]["n_words"] > 8192 and full[4]["n_used"] < full[4]["n_rows"] == BC.BIG_ROWS and full[4]["n_nodes"] > 1024
    assert set(BC.big_transform("k4_l8", 9)[1]) == {0, -1}  # levelsup >= L: the root
    pow2 = lambda n: 1 << (n - 1).bit_length()
    assert [pow2(c) for c in BC.BIG_COUNTS] == [2048, 2048, 4096, 8192, 16384] and min(BC.BIG_COUNTS) > 1024
    for c in BC.BIG_COUNTS:
        part = BC.big_transform("k4_l8", 2, c)
        assert c // 2 < part[4]["n_words"] < part[4]["n_used"] < part[4]["n_rows"] == c  # per counts the padded size, not the used rows
    runs = BC.big_transform("k10", 2)
    used = runs[0][runs[1] >= 0]
    per = BC.BIG_ROWS // 1024
    print(runs[4], "longest run", BC.longest_run(used))
    assert BC.longest_run(used) > per == 16 and runs[4]["n_words"] < runs[4]["n_used"] / 4
    one = BC.one_word_transform("k10", 2)
    assert one[4]["n_words"] == 1 and one[4]["n_used"] == BC.BIG_ROWS and one[3][0] == 1.0
    w = float(BC.big_vocab("k10").weight[BC.big_paths("k10")[BC.one_word_index("k10")][-1]])
    assert one[4]["norm"] != w * BC.BIG_ROWS or w * BC.BIG_ROWS == sum([w] * BC.BIG_ROWS)


@pytest.mark.parametrize("name", list(BC.BOUND_CASES))
def test_library_links_the_bound_vocabularies_as_the_reference_does(name):
    voc = BC.bound_case(name)[0]
    with BC.library_vocab(voc) as lv:
        _same_tree(lv, voc)
        if name == "spine32":
            assert lv.info()["max_depth"] == 32


def _ordinals(voc, path):
    """the child ordinal taken at every step of a path"""
    out, cur = [], 0
    for nd in path:
        out.append(voc.children[cur].index(nd))
        cur = nd
    return out


def _dist(a, b) -> int:
    return int(R.distances(np.asarray(a, np.uint8).reshape(1, 32), np.asarray(b, np.uint8).reshape(1, 32))[0, 0])


@pytest.mark.parametrize("L", (1, 2))
def test_k256_cases_reach_ordinal_255_both_tie_placements_and_distance_256(L):
    voc, rows = BC.k256_vocab(L), BC.k256_rows(L)
    assert voc.k == binding.SS_VOCAB_MAX_K == 256 and len(voc.children[0]) == 256 and voc.max_depth == L
    paths = BC.bound_paths(f"k256_l{L}")
    first = [_ordinals(voc, p)[0] for p in paths]
    assert 255 in first and max(first) == 255
    top = voc.children[0]
    for pairs, same_lane in ((BC.K256_SAME_LANE, True), (BC.K256_OTHER_LANE, False)):
        for a, b in pairs:
            assert a < b and ((b - a) % 8 == 0) == same_lane and voc.desc[top[a]].tobytes() == voc.desc[top[b]].tobytes()
            assert first[b] == a and first[a] == a, "the row equal to both children goes to the earlier one"  # rows 0 .. 255 are the children
    assert any(a % 8 > b % 8 for a, b in BC.K256_OTHER_LANE)  # the earlier child in a later lane
    # the complement of a child is 256 from it
    assert _dist(rows[256], voc.desc[top[0]]) == 256
    if L == 2:
        assert [len(voc.children[c + 1]) for c in BC.K256_INNER] == [256] * len(BC.K256_INNER)
        second = [_ordinals(voc, p) for p in paths if len(p) == 2]
        assert any(o == [255, 255] for o in second) and any(o[0] == 3 and o[1] > 127 for o in second)
        for a, b in BC.K256_SAME_LANE + BC.K256_OTHER_LANE:  # the same placements one level down
            assert [255, a] in second and [255, b] not in second
        # under root child 0 all 256 children are one descriptor: ordinal 0 wins
        under0 = voc.desc[voc.children[1][0]]
        hits = [(r, p) for r, p in zip(rows, paths) if len(p) == 2 and p[0] == top[0]]
        assert {_dist(r, under0) for r, p in hits} >= {0, 8} and all(_ordinals(voc, p) == [0, 0] for r, p in hits)
        depth1 = [p for p in paths if len(p) == 1]
        assert len(depth1) > 100  # leaves shallower than L


def test_small_bound_cases_reach_one_past_a_stride_a_chain_and_depth_32():
    voc, rows, _ = BC.bound_case("k256_one")  # a winning distance of 256 among 256 children
    assert _dist(rows[1], voc.desc[1]) == 256 and _dist(rows[1], voc.desc[256]) == 256 and set(BC.bound_transform("k256_one", 0)[0]) == {0}
    for name, k in (("k9", 9), ("k17", 17)):
        voc, rows, _ = BC.bound_case(name)
        ords = [o for p in BC.bound_paths(name) for o in _ordinals(voc, p)]
        assert voc.k == k and max(len(c) for c in voc.children) == k and max(ords) == k - 1 and {8} <= set(ords), name
        dup = [p for p in range(voc.n_nodes + 1) if len(voc.children[p]) > len(set(voc.desc[c].tobytes() for c in voc.children[p]))]
        assert dup, name
    voc, rows, lus = BC.bound_case("k1_chain")
    assert voc.k == 1 and voc.n_words == 1 and voc.max_depth == 5 and all(len(p) == 5 for p in BC.bound_paths("k1_chain"))
    assert any(_dist(r, voc.desc[1]) == 256 for r in rows)  # the only child, as far as a descriptor can be
    for lu, node in ((0, 5), (1, 4), (5, 0)):
        assert set(BC.bound_transform("k1_chain", lu)[1]) == {node}
    voc, rows, lus = BC.bound_case("spine32")
    assert voc.info()["max_depth"] == 32 == binding.SS_VOCAB_MAX_DEPTH == voc.L and voc.n_nodes == 64
    paths = BC.bound_paths("spine32")
    assert [len(p) for p in paths[:len(BC.SPINE_DEPTHS)]] == list(BC.SPINE_DEPTHS)
    assert {len(p) for p in paths} == set(range(1, 33)) and lus == (0, 1, 16, 31, 32, 40)
    for i, d in enumerate(BC.SPINE_DEPTHS):  # the row's node at depth L - levelsup: its own leaf where the path is shorter
        for lu in lus:
            target = 32 - lu
            want = 0 if target <= 0 else paths[i][min(target, d) - 1]
            assert BC.bound_transform("spine32", lu)[1][i] == want
    ties = [p for r, p in zip(rows, paths) if r.sum() == 0x0F and (r != 0).sum() == 1]
    assert len(ties) == 6 and {len(p) for p in ties} == {1, 15, 31, 32}  # odd depths: the leaf first; even: on down the spine
    assert (BC.bound_transform("spine32", 0)[1] == -1).sum() >= 2  # the leaves of weight 0.0


def test_wide_batch_and_long_score_cases():
    used = [BC.wide_transform("cluster", f, 1)[4]["n_used"] for f in BC.WIDE]
    print("used rows at 640 x 480 / 2000:", used, [len(BC.wide_features(f)[0]) for f in BC.WIDE])
    assert max(used) > 1024
    combo = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=1)
    assert BC.wide_reference_pair("cluster", 1, BC.WIDE[1], BC.WIDE[0], combo)[3]["n_final"] > 100
    qw, qv, db, want = BC.long_score_case()
    assert len(qw) > 8192 and [len(w) for w, _ in db] == [len(qw), 1, 63, 64, 65, 9000, 201, 201]
    assert abs(want[0] - 1.0) <= len(qw) * np.finfo(np.float64).eps and (want[1:] > 0).all() and (want[1:] < 1).all()
    for (w, v), word in ((db[6], qw[0]), (db[7], qw[-1])):
        assert set(w) & set(qw) == {word} and (np.diff(w) > 0).all()
    assert len(set(db[5][0]) & set(qw)) == 4500 and (np.diff(db[5][0]) > 0).all()
    assert all(n % 4 != 0 for n in BC.SCORE_N_DB)
