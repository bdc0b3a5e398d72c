"""GPU parity of the bag-of-words path (ss_bow_transform*_device, ss_match_bow_*_device, ss_bow_score_device) against
tests/bow_ref.py: bit for bit, no tolerance -- words, nodes, vector words, the raw 64-bit patterns of values / norm / scores,
idx / d1 / d2 and every summary field.  Outputs are prefilled with a pattern no result has."""
import numpy as np
import pytest

import bow_cases as BC
import bow_ref as B
import guided_cases as G
import guided_ref as R
from test_guided import Outputs, _check, _extract, _kp

pytestmark = pytest.mark.gpu

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(len(a), -1) if a.dtype.fields else a).to(_dev())
    torch.cuda.synchronize()
    return t


def _filled(*shape_fill_dtype):
    """a prefilled device tensor, complete before it is handed out: the library's stream does not wait for torch's"""
    import torch
    shape, fill, dtype = shape_fill_dtype
    t = torch.full(shape, fill, dtype=dtype, device=_dev())
    torch.cuda.synchronize()
    return t


def _outputs(n, rows):
    import torch
    out = Outputs(n, rows)
    torch.cuda.synchronize()
    return out


class Transformed:
    """device outputs of a transform of n frames of `rows` rows, prefilled"""

    def __init__(self, n, rows):
        import torch
        self.n, self.rows = n, rows
        self.word, self.node, self.bow_word = (torch.full((n, rows), FILL32, dtype=torch.int32, device=_dev()) for _ in range(3))
        self.bow_value = torch.full((n, rows), FILL64, dtype=torch.int64, device=_dev())
        self.summary = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()  # the library's stream does not wait for torch's

    def ptrs(self):
        return self.word.data_ptr(), self.node.data_ptr(), self.bow_word.data_ptr(), self.bow_value.data_ptr(), self.summary.data_ptr()

    def host(self):
        from send_slam_amd import binding
        summ = self.summary.cpu().numpy().copy().view(binding.BOW_SUMMARY_DTYPE).reshape(self.n)
        return (self.word.cpu().numpy(), self.node.cpu().numpy(), self.bow_word.cpu().numpy(), self.bow_value.cpu().numpy().view(np.uint64), summ)


def _check_transform(tag, got, f, want):
    """frame f of a transform's host outputs against (word, node, bow_word, bow_value, summary) of the reference"""
    word, node, bw, bv, summ = got
    wword, wnode, wbw, wbv, wsumm = want
    n, m = len(wword), len(wbw)
    for name in B.SUMMARY_FIELDS[:-1]:
        assert int(summ[f][name]) == wsumm[name], f"{tag}: summary.{name} {int(summ[f][name])} != {wsumm[name]}"
    assert B.bits([summ[f]["norm"]])[0] == B.bits([wsumm["norm"]])[0], f"{tag}: norm {summ[f]['norm']!r} != {wsumm['norm']!r}"
    for name, g, w in (("word", word[f], wword), ("node", node[f], wnode)):
        bad = np.flatnonzero(g[:n] != w)
        assert len(bad) == 0, f"{tag}: {name} differs at rows {bad[:8]}: {g[:n][bad[:8]]} != {w[bad[:8]]}"
        assert (g[n:] == -1).all(), f"{tag}: {name} past the count is not -1"
    assert np.array_equal(bw[f][:m], wbw) and (bw[f][m:] == -1).all(), f"{tag}: vector words differ"
    bad = np.flatnonzero(bv[f][:m] != B.bits(wbv))
    assert len(bad) == 0, f"{tag}: vector values differ at {bad[:8]}: {bv[f][:m][bad[:8]].view(np.float64)} != {wbv[bad[:8]]}"
    assert (bv[f][m:] == 0).all(), f"{tag}: values past the vector are not 0.0"


@pytest.fixture(scope="module")
def batch_ctx():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(BC.BATCH)) as ctx:
        pixels, kcap = _extract(ctx, BC.BATCH)
        yield ctx, kcap, pixels


def _set(ctx, voc: B.Vocab):
    with BC.library_vocab(voc) as lv:
        ctx.set_vocabulary(lv)  # the context keeps its own copy


def test_calls_before_a_vocabulary_return_state():
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF, max_batch=2) as ctx:
        _, kcap = _extract(ctx, ["synth_t0", "synth_t1"])
        out, m = Transformed(2, kcap), _outputs(2, kcap)
        with pytest.raises(binding.OrbError) as e:
            ctx.bow_transform_batch_device(2, *out.ptrs())
        assert e.value.code == binding.SS_ERR_STATE and "vocabulary" in e.value.message
        with pytest.raises(binding.OrbError) as e:
            ctx.bow_transform_device(ctx.batch_view().descriptors, ctx.batch_view().n_keypoints, 2, kcap, 2, *out.ptrs())
        assert e.value.code == binding.SS_ERR_STATE
        with pytest.raises(binding.OrbError) as e:
            ctx.match_bow_batch_device(binding.guided_params(), *m.ptrs())
        assert e.value.code == binding.SS_ERR_STATE
        # with a vocabulary the match still wants a transform of THIS batch
        _set(ctx, BC.vocab("k3"))
        with pytest.raises(binding.OrbError) as e:
            ctx.match_bow_batch_device(binding.guided_params(), *m.ptrs())
        assert e.value.code == binding.SS_ERR_STATE and "ss_bow_transform_batch_device" in e.value.message
        ctx.bow_transform_batch_device(2, *out.ptrs())
        ctx.match_bow_batch_device(binding.guided_params(), *m.ptrs())
        _extract(ctx, ["synth_t2", "synth_t3"])
        with pytest.raises(binding.OrbError) as e:
            ctx.match_bow_batch_device(binding.guided_params(), *m.ptrs())
        assert e.value.code == binding.SS_ERR_STATE
        with pytest.raises(binding.OrbError) as e:
            ctx.bow_transform_batch_device(-1, *out.ptrs())
        assert e.value.code == binding.SS_ERR_INVALID_ARG


@pytest.mark.parametrize("name", list(BC.VOCABS))
def test_batch_transform(batch_ctx, name):
    """every vocabulary in turn on ONE context (each call of ss_bow_set_vocabulary replaces the one before), levelsup 0, 2, 4, >= L"""
    ctx, kcap, _ = batch_ctx
    _set(ctx, BC.vocab(name))
    for lu in BC.LEVELSUPS:
        out = Transformed(len(BC.BATCH), kcap)
        ctx.bow_transform_batch_device(lu, *out.ptrs())
        ctx.synchronize()
        got = out.host()
        for f, frame in enumerate(BC.BATCH):
            want = BC.frame_transform(name, frame, lu)
            if lu == 2:
                print(name, frame, want[4])
            _check_transform(f"{name} levelsup {lu} frame {f} ({frame})", got, f, want)
    assert BC.frame_transform(name, "flat", 2)[4]["n_rows"] == 0 and BC.frame_transform(name, "synth_t0", 9)[4]["n_nodes"] == 1


def _transform_arrays(ctx, descs, rows, lu):
    """the device-array form on a list of per-frame descriptor arrays"""
    n = len(descs)
    host = np.full((n, rows, 32), 0xA5, np.uint8)  # rows past the count hold a pattern; they must not matter
    for f, d in enumerate(descs):
        host[f, :len(d)] = d
    d_desc, d_n = _to_dev(host), _to_dev(np.array([len(d) for d in descs], np.int32))
    out = Transformed(n, rows)
    ctx.bow_transform_device(d_desc.data_ptr(), d_n.data_ptr(), n, rows, lu, *out.ptrs())
    ctx.synchronize()
    return out.host()


def test_device_array_form_counts_ties_repeats_and_zero_weights():
    from send_slam_amd import binding
    rng = np.random.Generator(np.random.PCG64(0xB0A))
    voc = BC.vocab("k3")
    rows = 300
    real = G.features("synth_t0")[1]
    # rows equidistant from two children: a parent whose children differ, a row that is child a with half of the differing bits
    # of child b flipped in -- and rows EQUAL to duplicated children
    crafted = []
    for p in range(voc.n_nodes + 1):
        cs = voc.children[p]
        for a in range(len(cs)):
            for b in range(a + 1, len(cs)):
                x, y = voc.desc[cs[a]], voc.desc[cs[b]]
                diff = np.flatnonzero(np.unpackbits(x ^ y))
                if len(diff) == 0:
                    crafted.append(x.copy())
                elif len(diff) % 2 == 0:
                    bits = np.unpackbits(x)
                    bits[diff[:len(diff) // 2]] ^= 1
                    crafted.append(np.packbits(bits))
    crafted = np.array(crafted[:rows], np.uint8)
    assert len(crafted) > 50
    used = np.flatnonzero(BC.frame_transform("k3", "synth_t0", 0)[1] >= 0)
    same = np.tile(real[used[0]], (rows, 1))  # one word, seen `rows` times
    frames = [real[:0], real[:1], real[:rows], crafted, same, rng.integers(0, 256, size=(rows, 32), dtype=np.uint8)]
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        _set(ctx, voc)
        for lu in (0, 4):
            got = _transform_arrays(ctx, frames, rows, lu)
            for f, d in enumerate(frames):
                _check_transform(f"k3 levelsup {lu} array frame {f}", got, f, B.transform(voc, d, lu))
        want = B.transform(voc, same, 0)
        assert want[4]["n_words"] == 1 and want[4]["n_used"] == rows and want[3][0] == 1.0
        # all weights 0: empty vector, norm 0.0, nothing divided
        zero = B.Vocab(voc.k, voc.L, *voc.arrays()[:3], np.zeros(voc.n_nodes))
        _set(ctx, zero)
        got = _transform_arrays(ctx, frames, rows, 2)
        for f, d in enumerate(frames):
            want = B.transform(zero, d, 2)
            assert want[4]["n_used"] == 0 and want[4]["n_words"] == 0 and want[4]["norm"] == 0.0 and (want[1] == -1).all()
            _check_transform(f"zero weights frame {f}", got, f, want)
        # refused calls leave the context usable
        out = Transformed(1, 8)
        for kw in (dict(rows=binding.SS_BOW_MAX_ROWS + 1, lu=0), dict(rows=8, lu=-1), dict(rows=0, lu=0)):
            with pytest.raises(binding.OrbError) as e:
                ctx.bow_transform_device(1, 1, 1, kw["rows"], kw["lu"], *out.ptrs())
            assert e.value.code == binding.SS_ERR_INVALID_ARG
        _set(ctx, voc)
        got = _transform_arrays(ctx, frames[2:3], rows, 2)
        _check_transform("after the refused calls", got, 0, B.transform(voc, frames[2], 2))


def test_repeated_word_adds_the_weight_to_itself():
    """a two-word vocabulary with weights 0.1 and 0.3: six rows on the first word give 0.1 + ... + 0.1 = 0.6 (five additions), which
    is not 6 * 0.1 = 0.6000000000000001 rounded once; the norm and the normalised value show it"""
    from send_slam_amd import binding
    d = np.zeros((2, 32), np.uint8)
    d[1] = 255
    voc = B.Vocab(2, 1, [0, 0], [1, 1], d, [0.1, 0.3])
    rows = np.concatenate([np.tile(d[0], (6, 1)), d[1:2]])
    want = B.transform(voc, rows, 0)
    acc = 0.1
    for _ in range(5):
        acc += 0.1
    assert acc != 0.1 * 6 and want[4]["norm"] == acc + 0.3 != 0.1 * 6 + 0.3
    assert want[3][0] == acc / (acc + 0.3) != (0.1 * 6) / (0.1 * 6 + 0.3) and list(want[2]) == [0, 1]
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        _set(ctx, voc)
        _check_transform("repeated word", _transform_arrays(ctx, [rows], 16, 0), 0, want)


def test_orbvoc_shaped_tree():
    """k = 10, L = 6, 1 111 110 nodes (ORBvoc.txt's shape), generated here: breadth-first ids, so node i has the children
    10 i + 1 .. 10 i + 10; 500 real descriptors; the reference descent is written on that closed form"""
    from send_slam_amd import binding
    k, L = 10, 6
    n = sum(k ** d for d in range(1, L + 1))
    rng = np.random.Generator(np.random.PCG64(0x0B0C))
    ids = np.arange(1, n + 1, dtype=np.int64)
    parent = ((ids - 1) // k).astype(np.int32)
    first_leaf = n - k ** L + 1
    is_leaf = (ids >= first_leaf).astype(np.uint8)
    desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    weight = np.where(is_leaf == 1, rng.random(n) * 9 + 0.01, 0.0)
    weight[first_leaf - 1 + rng.integers(0, k ** L, 40000)] = 0.0
    rows = np.concatenate([G.features("synth_t0")[1], G.features("noise")[1]])[:500]
    pop = np.array([bin(v).count("1") for v in range(256)], np.int64)
    lu = 4
    word, node, ws = [], [], []
    for r in rows:
        cur, path = 0, []
        for _ in range(L):
            ch = cur * k + 1 + np.arange(k)
            cur = int(ch[int(np.argmin(pop[desc[ch - 1] ^ r].sum(axis=1)))])  # argmin: the first of equal minima
            path.append(cur)
        w = float(weight[cur - 1])
        word.append(cur - first_leaf)
        ws.append(w)
        node.append(path[L - lu - 1] if w > 0 else -1)
    bw, bv, norm = B.bow_vector(word, ws)
    want = (np.array(word, np.int32), np.array(node, np.int32), bw, bv,
            {"status": 0, "n_rows": len(rows), "n_used": int(sum(w > 0 for w in ws)), "n_words": len(bw),
             "n_nodes": len(set(v for v in node if v >= 0)), "reserved": 0, "norm": norm})
    with binding.Vocabulary.from_arrays(parent, is_leaf, desc, weight, k, L) as lv:
        assert lv.info() == {"k": k, "L": L, "n_nodes": n, "n_words": k ** L, "max_depth": L}
        with binding.OrbContext(0, n_features=G.NF) as ctx:
            ctx.set_vocabulary(lv)
            got = _transform_arrays(ctx, [rows], 512, lu)
    print(want[4])
    _check_transform("ORBvoc-shaped tree", got, 0, want)
    assert 0 < want[4]["n_used"] < 500 and want[4]["n_nodes"] > 50


# ---- SearchByBoW ----------------------------------------------------------------------------------------------------------
UPSTREAM = dict(th=50, ratio_num=7, ratio_den=10)
MATCH_RULES = [UPSTREAM, dict(th=100, ratio_num=0, ratio_den=0)]
MATCH_COMBOS = [dict(r, one_to_one=bool(o), orientation=k) for r in MATCH_RULES for o in (0, 1) for k in (0, 1, 2)]
MATCH_VOC, MATCH_LU = "cluster", 1


@pytest.fixture(scope="module")
def transformed_ctx(batch_ctx):
    ctx, kcap, _ = batch_ctx
    return ctx, kcap


def _transform_batch(ctx, kcap, name, lu):
    _set(ctx, BC.vocab(name))
    out = Transformed(len(BC.BATCH), kcap)
    ctx.bow_transform_batch_device(lu, *out.ptrs())
    ctx.synchronize()  # the call is asynchronous on the context's own stream: a caller may drop `out` only after it has run
    return out


@pytest.mark.parametrize("combo", MATCH_COMBOS, ids=G.combo_name)
def test_batch_match(transformed_ctx, combo):
    """frame b against b - 1 on the nodes of the clustered vocabulary"""
    from send_slam_amd import binding
    ctx, kcap = transformed_ctx
    _transform_batch(ctx, kcap, MATCH_VOC, MATCH_LU)
    out = _outputs(len(BC.BATCH), kcap)
    ctx.match_bow_batch_device(binding.guided_params(**combo), *out.ptrs())
    ctx.synchronize()
    got = out.host()
    total = 0
    for b, name in enumerate(BC.BATCH):
        want = BC.reference_pair(MATCH_VOC, MATCH_LU, name, BC.BATCH[b - 1] if b else None, combo)
        print(b, name, want[3])
        _check(f"frame {b} ({name}) {G.combo_name(combo)}", got, b, want)
        total += want[3]["n_final"]
    assert total > 100


def test_batch_match_table_form(transformed_ctx):
    """t == b (the self pair is excluded), t == -1, an earlier and a later frame, on few large nodes; bad entries are refused"""
    from send_slam_amd import binding
    ctx, kcap = transformed_ctx
    n = len(BC.BATCH)
    _transform_batch(ctx, kcap, "k3", 4)
    table = np.array([0, -1, 3, 2, 4, 0, 6, 1], np.int32)  # self: 0 4 6; later: 2 <- 3; none: 1; flat <- synth_t1
    combo = dict(th=100, ratio_num=0, ratio_den=0, one_to_one=True, orientation=1)
    out = _outputs(n, kcap)
    ctx.match_bow_batch_device(binding.guided_params(**combo), *out.ptrs(), train_src=table)
    ctx.synchronize()
    got = out.host()
    selfs = 0
    for b, t in enumerate(table):
        want = BC.reference_pair("k3", 4, BC.BATCH[b], BC.BATCH[t] if t >= 0 else None, combo, exclude_self=bool(t == b))
        _check(f"frame {b} against {t}", got, b, want)
        if t == b:
            nq = want[3]["n_query"]
            assert not (got[0][b][:nq] == np.arange(nq)).any()
            selfs += want[3]["n_accepted"]
    assert selfs > 0
    for bad in (-2, n):
        t2 = table.copy()
        t2[5] = bad
        with pytest.raises(binding.OrbError) as e:
            ctx.match_bow_batch_device(binding.guided_params(**combo), *out.ptrs(), train_src=t2)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "train_src[5]" in e.value.message


def _upload_pairs(frames, rows):
    """frames: dicts q_kp q_desc q_node t_kp t_desc t_node -> device arrays [n][rows] of the pairs form (plus whole windows)"""
    from send_slam_amd import binding
    n = len(frames)
    host = {"q_desc": np.zeros((n, rows, 32), np.uint8), "t_desc": np.zeros((n, rows, 32), np.uint8),
            "q_kp": np.zeros((n, rows), binding.KP_DTYPE), "t_kp": np.zeros((n, rows), binding.KP_DTYPE),
            "q_node": np.full((n, rows), 7, np.int32), "t_node": np.full((n, rows), 7, np.int32),  # rows past the counts: a live node
            "windows": np.zeros((n, rows), binding.GUIDED_WINDOW_DTYPE), "nq": np.zeros(n, np.int32), "nt": np.zeros(n, np.int32)}
    for b, f in enumerate(frames):
        nq, nt = len(f["q_kp"]), len(f["t_kp"])
        host["nq"][b], host["nt"][b] = nq, nt
        host["q_desc"][b, :nq], host["q_kp"][b, :nq], host["q_node"][b, :nq] = f["q_desc"], f["q_kp"], f["q_node"]
        host["t_desc"][b, :nt], host["t_kp"][b, :nt], host["t_node"][b, :nt] = f["t_desc"], f["t_kp"], f["t_node"]
        host["windows"][b, :nq] = R.whole_windows(nq)
    return {k: _to_dev(v) for k, v in host.items()}


def _run_bow_pairs(ctx, dev, n, rows, params):
    out = _outputs(n, rows)
    ctx.match_bow_pairs_device(dev["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), dev["q_node"].data_ptr(), dev["nq"].data_ptr(),
                               dev["t_desc"].data_ptr(), dev["t_kp"].data_ptr(), dev["t_node"].data_ptr(), dev["nt"].data_ptr(), n, rows, params,
                               *out.ptrs())
    ctx.synchronize()
    return out


def test_pairs_form_with_caller_made_nodes():
    from send_slam_amd import binding
    rng = np.random.Generator(np.random.PCG64(0xB0B))
    (qk, qd), (tk, td) = G.features("synth_t1"), G.features("synth_t0")
    nq, nt = len(qk), len(tk)
    big = (1 << 31) - 1  # any non-negative int32 is a node
    frames = {
        "all_minus_one": dict(q_node=np.full(nq, -1), t_node=np.full(nt, -1)),
        "one_node": dict(q_node=np.full(nq, big), t_node=np.full(nt, big)),
        "one_side_only": dict(q_node=rng.integers(0, 4, nq) * 2, t_node=rng.integers(0, 4, nt) * 2 + 1),
        "mixed": dict(q_node=rng.integers(-1, 12, nq) * 100003, t_node=rng.integers(-1, 12, nt) * 100003),
        "no_train": dict(q_node=rng.integers(0, 3, nq), t_node=np.zeros(0, np.int64), t_kp=tk[:0], t_desc=td[:0]),
        "no_query": dict(q_node=np.zeros(0, np.int64), t_node=rng.integers(0, 3, nt), q_kp=qk[:0], q_desc=qd[:0]),
    }
    for f in frames.values():
        for k, v in (("q_kp", qk), ("q_desc", qd), ("t_kp", tk), ("t_desc", td)):
            f.setdefault(k, v)
        f["q_node"] = np.where(np.asarray(f["q_node"]) < 0, -1, f["q_node"]).astype(np.int32)
        f["t_node"] = np.where(np.asarray(f["t_node"]) < 0, -1, f["t_node"]).astype(np.int32)
    names, rows = list(frames), 512
    dev = _upload_pairs([frames[k] for k in names], rows)
    combos = [dict(UPSTREAM, one_to_one=False, orientation=0), dict(UPSTREAM, one_to_one=True, orientation=1),
              dict(MATCH_RULES[1], one_to_one=True, orientation=2)]
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        for c in combos:
            p = binding.guided_params(**c, extent_w=G.W, extent_h=G.H)
            out = _run_bow_pairs(ctx, dev, len(names), rows, p)
            got = out.host()
            for i, k in enumerate(names):
                f = frames[k]
                want = B.match(f["q_kp"], f["q_desc"], f["q_node"], f["t_kp"] if len(f["t_kp"]) else None, f["t_desc"], f["t_node"], **c)
                _check(f"{k} {G.combo_name(c)}", got, i, want)
                if k in ("all_minus_one", "one_side_only"):
                    assert want[3]["n_candidates"] == 0 and (want[0] == -1).all() and (want[1] == R.NONE).all()
            # one node holding every row = the guided search with an all-covering window, on the same device arrays
            guided = _outputs(len(names), rows)
            ctx.match_guided_pairs_device(dev["q_desc"].data_ptr(), dev["q_kp"].data_ptr(), dev["nq"].data_ptr(), dev["t_desc"].data_ptr(),
                                          dev["t_kp"].data_ptr(), dev["nt"].data_ptr(), dev["windows"].data_ptr(), len(names), rows, p, *guided.ptrs())
            ctx.synchronize()
            i = names.index("one_node")
            a, b = got, guided.host()
            assert all(np.array_equal(a[j][i], b[j][i]) for j in range(3)) and a[3][i] == b[3][i] and a[3][i]["n_candidates"] == nq * nt
        with pytest.raises(binding.OrbError) as e:
            _run_bow_pairs(ctx, dev, 1, binding.SS_GUIDED_MAX_ROWS + 1, binding.guided_params())
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "SS_GUIDED_MAX_ROWS" in e.value.message


def _capacity_nodes():
    """nodes for guided_cases.capacity_frames: 96 nodes spread over both sides (about 170 train rows each), node ids up to 2^30;
    the planted queries carry the node of their planted train row, so the rows 8191, 8192 and 16383 are contested"""
    rng = np.random.Generator(np.random.PCG64(0xCAB0))
    frames = G.capacity_frames()
    ids = rng.choice(1 << 30, 96, replace=False).astype(np.int32)
    t_node = ids[rng.integers(0, 96, len(frames[0]["t_kp"]))]
    q_node = ids[rng.integers(0, 96, len(frames[0]["q_kp"]))]
    t_node[rng.integers(0, len(t_node), 500)] = -1
    for k, row in enumerate(G.CAP_PLANTED):
        t_node[row] = ids[k]
        q_node[len(q_node) - 2 * len(G.CAP_PLANTED) + 2 * k:][:2] = ids[k]
    return [dict(frames[0], q_node=q_node, t_node=t_node), dict(frames[1], q_node=t_node, t_node=q_node)]


def test_full_capacity_pairs():
    """SS_GUIDED_MAX_ROWS rows per frame: the LDS sort at its full size, both passes of the finish's conflict table with contested
    train rows at 8191, 8192 and 16383"""
    from send_slam_amd import binding
    frames = _capacity_nodes()
    rows = G.CAP_ROWS
    dev = _upload_pairs(frames, rows)
    found = [B.search(f["q_desc"], f["q_node"], f["t_desc"], f["t_node"]) for f in frames]
    # each planted row is the best of its two queries, at distance 0
    assert (found[0][0][-6:] == np.repeat(G.CAP_PLANTED, 2)).all() and (found[0][1][-6:] == 0).all()
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        for c in G.CAP_COMBOS:
            got = _run_bow_pairs(ctx, dev, 2, rows, binding.guided_params(**c)).host()
            for b, f in enumerate(frames):
                want = R.finish(found[b], f["q_kp"], f["t_kp"], **c)
                print(b, G.combo_name(c), want[3])
                _check(f"capacity frame {b} {G.combo_name(c)}", got, b, want)
                assert (want[0][-6:][1::2] == -1).all() if b == 0 else True  # the later query of a contested row loses it
                assert want[3]["n_unique"] < want[3]["n_accepted"]


# ---- L1 score -------------------------------------------------------------------------------------------------------------
def test_score_against_a_kept_database():
    from send_slam_amd import binding
    rng = np.random.Generator(np.random.PCG64(0x5C0))
    vecs = []
    for name in ("cluster", "k10"):
        for frame in BC.BATCH + ["parallax_t0", "parallax_t3", "synth_t4"]:
            for lu in (0, 2):
                _, _, bw, bv, _ = BC.frame_transform(name, frame, lu)
                vecs.append((bw, bv))
    q = BC.frame_transform("cluster", "synth_t1", 2)
    qw, qv = q[2], q[3]
    stride = max(max(len(w) for w, _ in vecs), len(qw)) + 3
    full = np.sort(rng.choice(5000, stride, replace=False)).astype(np.int32)
    crafted = [(qw[:0], qv[:0]), (qw, qv), (qw + 1 if len(set(qw + 1) & set(qw)) == 0 else qw + 100000, qv),
               (np.array([qw[0]], np.int32), np.array([0.25])), (np.array([qw[-1]], np.int32), np.array([1.0])),
               (np.concatenate([[qw[0]], qw[-1:] + 5]).astype(np.int32), np.array([0.5, 0.5])),
               (full, rng.random(stride) / stride), (np.union1d(qw, full)[:stride].astype(np.int32), np.full(stride, 1.0 / stride))]
    vecs += crafted
    for _ in range(200):  # random sub-vectors of the query's words mixed with others
        m = int(rng.integers(1, stride))
        w = np.sort(rng.choice(np.union1d(qw, full), min(m, len(np.union1d(qw, full))), replace=False)).astype(np.int32)
        v = rng.random(len(w))
        vecs.append((w, v / v.sum()))
    n = len(vecs)
    assert n >= 250
    want = np.array([B.score(qw, qv, w, v) for w, v in vecs], np.float64)
    assert abs(want[len(vecs) - 200 - len(crafted) + 1] - 1.0) < 1e-12 and want[len(vecs) - 200 - len(crafted)] == 0.0
    assert (want > 0).sum() > 100 and np.signbit(want[len(vecs) - 200 - len(crafted) + 2])  # no common word: -0.0
    import torch
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        for st, q_rows in ((stride, len(qw)), (stride + 29, len(qw) + 7)):
            dbw, dbv, cnt = np.full((n, st), -1, np.int32), np.zeros((n, st)), np.zeros(n, np.int32)
            for i, (w, v) in enumerate(vecs):
                dbw[i, :len(w)], dbv[i, :len(w)], cnt[i] = w, v, len(w)
            dbw = np.where(np.arange(st)[None, :] < cnt[:, None], dbw, qw[0]).astype(np.int32)  # past the count: a word of the query
            hq_w, hq_v = np.full(q_rows, qw[-1], np.int32), np.full(q_rows, 0.5)
            hq_w[:len(qw)], hq_v[:len(qw)] = qw, qv
            d = [_to_dev(a) for a in (hq_w, hq_v, np.array([len(qw)], np.int32), dbw, dbv, cnt)]
            score = _filled((n,), FILL64, torch.int64)
            ctx.bow_score_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), q_rows, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), n, st,
                                 score.data_ptr())
            ctx.synchronize()
            got = score.cpu().numpy().view(np.uint64)
            bad = np.flatnonzero(got != B.bits(want))
            assert len(bad) == 0, f"stride {st}: scores differ at {bad[:8]}: {got[bad[:8]].view(np.float64)} != {want[bad[:8]]}"
            # an empty query scores 0.0 against everything
            zero = _to_dev(np.zeros(1, np.int32))
            ctx.bow_score_device(d[0].data_ptr(), d[1].data_ptr(), zero.data_ptr(), q_rows, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), n, st,
                                 score.data_ptr())
            ctx.synchronize()
            assert (score.cpu().numpy() == 0).all()


def test_scores_of_transformed_frames_rank_the_sequence_first(batch_ctx):
    """the database kept from a device transform, as a caller would: row f of the transform's outputs is vector f"""
    import torch
    ctx, kcap, _ = batch_ctx
    out = _transform_batch(ctx, kcap, "cluster", 1)
    n = len(BC.BATCH)
    counts = out.summary.view(torch.int32)[:, 3].contiguous()  # n_words
    torch.cuda.synchronize()
    score = _filled((n,), FILL64, torch.int64)
    ctx.bow_score_device(out.bow_word[1].data_ptr(), out.bow_value[1].data_ptr(), counts[1:].data_ptr(), kcap, out.bow_word.data_ptr(),
                         out.bow_value.data_ptr(), counts.data_ptr(), n, kcap, score.data_ptr())
    ctx.synchronize()
    got = score.cpu().numpy().view(np.float64)
    q = BC.frame_transform("cluster", "synth_t1", 1)
    want = np.array([B.score(q[2], q[3], *BC.frame_transform("cluster", f, 1)[2:4]) for f in BC.BATCH])
    assert np.array_equal(B.bits(got), B.bits(want)), (got, want)
    print(dict(zip(BC.BATCH, got)))
    assert got[0] > got[BC.BATCH.index("noise")] and got[2] > got[BC.BATCH.index("noise")] and got[BC.BATCH.index("flat")] == 0.0
