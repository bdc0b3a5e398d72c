"""GPU parity of the bag-of-words path (ss_bow_transform*_device, ss_match_bow_*_device, ss_bow_score_device) against
tests/bow_ref.py: bit for bit, no tolerance -- words, nodes, vector words, the raw 64-bit patterns of values / norm / scores,
idx / d1 / d2 and every summary field.  Outputs are prefilled with a pattern no result has."""
import numpy as np
import pytest

import bow_cases as BC
import bow_ref as B
import guided_cases as G
import guided_ref as R
import proj_cases as PC
import proj_ref
from test_guided import Outputs, _check, _extract, _kp
from test_guided import _params as _guided_params
from test_guided import _upload as _upload_guided
from test_proj import Outputs as ProjOutputs
from test_proj import _upload as _upload_proj

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


def _transform_host(ctx, host, counts, lu):
    """the device-array form on descriptors [n][rows][32] and counts [n] as the caller holds them"""
    n, rows = host.shape[:2]
    d_desc, d_n = _to_dev(host), _to_dev(np.asarray(counts, np.int32))
    out = Transformed(n, rows)
    ctx.bow_transform_device(d_desc.data_ptr(), d_n.data_ptr(), n, rows, lu, *out.ptrs())
    ctx.synchronize()
    return out.host()


def _transform_arrays(ctx, descs, rows, lu):
    """the device-array form on a list of per-frame descriptor arrays"""
    n = len(descs)
    host = np.full((n, rows, 32), 0xA5, np.uint8)  # rows past the count hold a pattern; they must not matter
    for f, d in enumerate(descs):
        host[f, :len(d)] = d
    return _transform_host(ctx, host, [len(d) for d in descs], lu)


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


# ---- above 1024 rows: thread t of k_bow_vector owns ceil(n2 / 1024) sorted positions -------------------------------------------
def _big_frames(name):
    """-> (descriptors [n][BIG_ROWS][32], counts as given to the device, (rows, count) the reference sees).  Rows past a count stay
    live (the first frame's own rows) except in the last frame, which holds 0xA5 there."""
    rows = BC.big_rows()
    frames = [(rows, BC.BIG_ROWS, BC.BIG_ROWS)]
    if name == "k4_l8":
        frames += [(rows, c, c) for c in BC.BIG_COUNTS]
        frames += [(rows, BC.BIG_ROWS + 3616, BC.BIG_ROWS), (rows, 0, 0), (rows, -7, 0)]  # a count above rows_per_frame is clamped
        masked = np.full_like(rows, 0xA5)
        masked[:5000] = rows[:5000]
        frames.append((masked, 5000, 5000))
    else:
        frames += [(np.tile(rows[BC.one_word_index(name)], (BC.BIG_ROWS, 1)), BC.BIG_ROWS, None), (rows, 2049, 2049)]
    return np.stack([f[0] for f in frames]), [f[1] for f in frames], [f[2] for f in frames]


@pytest.mark.parametrize("name,levelsups", [("k4_l8", (2, 9)), ("k10", (2, 0))])
def test_transform_above_1024_rows(name, levelsups):
    """SS_BOW_MAX_ROWS rows per frame in the device-array form: many distinct words (k4_l8: more than 8192), long runs that cross
    the sixteen positions a thread owns (k10), one word 16384 times, counts on both sides of a power of two, clamped counts"""
    from send_slam_amd import binding
    voc = BC.big_vocab(name)
    host, counts, seen = _big_frames(name)
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        _set(ctx, voc)
        for lu in levelsups:
            got = _transform_host(ctx, host, counts, lu)
            for f, c in enumerate(seen):
                want = BC.big_transform(name, lu, c) if c is not None else BC.one_word_transform(name, lu)
                print(name, "levelsup", lu, "frame", f, "count", counts[f], want[4])
                _check_transform(f"{name} levelsup {lu} frame {f} (count {counts[f]})", got, f, want)
                if c is None:  # w added to itself 16383 times, then divided by itself
                    acc = w = float(voc.weight[BC.big_paths(name)[BC.one_word_index(name)][-1]])
                    for _ in range(BC.BIG_ROWS - 1):
                        acc += w
                    assert want[4]["n_words"] == 1 and want[4]["n_used"] == BC.BIG_ROWS and want[4]["norm"] == acc and want[3][0] == 1.0
    full = BC.big_transform(name, levelsups[0])
    if name == "k4_l8":
        assert full[4]["n_words"] > 8192 and full[4]["n_used"] < full[4]["n_rows"] == BC.BIG_ROWS
    else:
        assert BC.longest_run(full[0][full[1] >= 0]) > 16 and full[4]["n_words"] < full[4]["n_used"] / 4


@pytest.mark.parametrize("name", list(BC.BOUND_CASES))
def test_descent_at_the_vocabulary_bounds(name):
    """k = SS_VOCAB_MAX_K with equal children in one lane's strides and in different lanes, k one past a stride of eight lanes,
    k = 1, depth SS_VOCAB_MAX_DEPTH, a distance of 256 (tests/test_bow_ref.py asserts what each case reaches)"""
    from send_slam_amd import binding
    voc, rows, levelsups = BC.bound_case(name)
    n = len(rows) + 5
    with BC.library_vocab(voc) as lv:
        assert lv.info() == voc.info()
        with binding.OrbContext(0, n_features=G.NF) as ctx:
            ctx.set_vocabulary(lv)
            for lu in levelsups:
                got = _transform_arrays(ctx, [rows, rows[::-1], rows[:1]], n, lu)
                want = BC.bound_transform(name, lu)
                _check_transform(f"{name} levelsup {lu}", got, 0, want)
                _check_transform(f"{name} levelsup {lu}, one row", got, 2, B.transform_paths(voc, BC.bound_paths(name)[:1], lu))
                back = B.transform_paths(voc, BC.bound_paths(name)[::-1], lu)  # the same vector from another row order
                _check_transform(f"{name} levelsup {lu}, rows reversed", got, 1, back)
                assert np.array_equal(back[2], want[2]) and np.array_equal(B.bits(back[3]), B.bits(want[3]))


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


def test_batch_forms_above_1024_rows():
    """two frames at 640 x 480 / 2000 features: kp_capacity and the used rows are above the 1024 threads of k_bow_vector; the
    transform, then the match under both rules with one_to_one on"""
    from send_slam_amd import binding
    name, lu = MATCH_VOC, MATCH_LU
    w, h, nf = BC.WIDE_SIZE
    with binding.OrbContext(0, n_features=nf, max_batch=len(BC.WIDE)) as ctx:
        _, kcap = _extract(ctx, list(BC.WIDE), w, h, nf)  # asserts that the extraction is the oracle's
        assert kcap > 1024
        _set(ctx, BC.vocab(name))
        out = Transformed(len(BC.WIDE), kcap)
        ctx.bow_transform_batch_device(lu, *out.ptrs())
        ctx.synchronize()
        got = out.host()
        for f, frame in enumerate(BC.WIDE):
            want = BC.wide_transform(name, frame, lu)
            print(frame, want[4])
            _check_transform(f"{frame} at {w} x {h}", got, f, want)
        assert max(BC.wide_transform(name, frame, lu)[4]["n_used"] for frame in BC.WIDE) > 1024
        for rule in MATCH_RULES:
            combo = dict(rule, one_to_one=True, orientation=1)
            m = _outputs(len(BC.WIDE), kcap)
            ctx.match_bow_batch_device(binding.guided_params(**combo), *m.ptrs())
            ctx.synchronize()
            mg = m.host()
            for b, frame in enumerate(BC.WIDE):
                want = BC.wide_reference_pair(name, lu, frame, BC.WIDE[b - 1] if b else None, combo)
                print(b, frame, want[3])
                _check(f"{frame} at {w} x {h} {G.combo_name(combo)}", mg, b, want)
            assert want[3]["n_final"] > 100


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


@pytest.mark.parametrize("n_db", BC.SCORE_N_DB)
def test_score_partial_blocks_and_long_vectors(n_db):
    """n_db no multiple of the four waves of a block, a query of more than 8192 words against itself and against vectors of 1, 63,
    64, 65 and 9000 words and vectors sharing only its first or its last word; the scores past n_db stay as they were"""
    import torch
    from send_slam_amd import binding
    qw, qv, db, want = BC.long_score_case()
    assert len(qw) > 8192 and [len(w) for w, _ in db[1:6]] == [1, 63, 64, 65, 9000]
    first = len(db) - n_db if n_db > 1 else 0  # n_db 7 scores vectors 1 .. 7, 5: 3 .. 7, ...; n_db 1 the query itself
    part = db[first:first + n_db]
    stride = max(len(w) for w, _ in part) + 3
    dbw, dbv, cnt = np.full((n_db, stride), qw[0], np.int32), np.full((n_db, stride), 0.5), np.zeros(n_db, np.int32)  # past a count: a word of the query
    for i, (w, v) in enumerate(part):
        dbw[i, :len(w)], dbv[i, :len(w)], cnt[i] = w, v, len(w)
    q_rows = len(qw) + 7
    hq_w, hq_v = np.full(q_rows, qw[-1], np.int32), np.full(q_rows, 0.5)
    hq_w[:len(qw)], hq_v[:len(qw)] = qw, qv
    d = [_to_dev(a) for a in (hq_w, hq_v, np.array([len(qw)], np.int32), dbw, dbv, cnt)]
    score = _filled((n_db + 9,), FILL64, torch.int64)
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        ctx.bow_score_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), q_rows, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), n_db, stride,
                             score.data_ptr())
        ctx.synchronize()
    got = score.cpu().numpy().view(np.uint64)
    exp = B.bits(want[first:first + n_db])
    assert np.array_equal(got[:n_db], exp), f"n_db {n_db}: {got[:n_db].view(np.float64)} != {want[first:first + n_db]}"
    assert (got[n_db:] == FILL64).all(), "a score past n_db was written"
    if first == 0:
        assert abs(want[0] - 1.0) <= len(qw) * np.finfo(np.float64).eps


# ---- stages interleaved on one context ---------------------------------------------------------------------------------------------
def _raw(out):
    """every device array of an outputs object, on the host"""
    import torch
    return {k: v.cpu().numpy().copy() for k, v in vars(out).items() if isinstance(v, torch.Tensor)}


def _interleaved_steps():
    """-> [(name, alloc() -> outputs object, launch(ctx, outputs))]: calls that share d_guided_ws and the bow workspaces at changing
    sizes; every device input is uploaded here, every launch only enqueues"""
    import torch
    from send_slam_amd import binding
    (qk, qd), (tk, td) = G.features("synth_t1"), G.features("synth_t0")
    g_rows = 512
    g_dev = _upload_guided([{"q_kp": qk, "q_desc": qd, "t_kp": tk, "t_desc": td, "windows": G.own_windows(qk)}], g_rows)
    g_par = binding.guided_params(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1, extent_w=G.W, extent_h=G.H)
    scenes = PC.scenes()
    p_rows, t_rows = 470, 483
    p_dev = _upload_proj(scenes, p_rows, t_rows)
    combo = PC.EXTENT_COMBOS[0]
    rng = np.random.Generator(np.random.PCG64(0x1C7E))
    b_frames = [dict(q_kp=qk, q_desc=qd, t_kp=tk, t_desc=td, q_node=rng.integers(-1, 9, len(qk)).astype(np.int32), t_node=rng.integers(-1, 9, len(tk)).astype(np.int32)),
                dict(q_kp=tk, q_desc=td, t_kp=qk, t_desc=qd, q_node=rng.integers(0, 3, len(tk)).astype(np.int32), t_node=rng.integers(0, 3, len(qk)).astype(np.int32))]
    b_rows = 600
    b_dev = _upload_pairs(b_frames, b_rows)
    b_par = binding.guided_params(**UPSTREAM, one_to_one=True, orientation=2)
    x_rows = 2100
    x_host = np.full((3, x_rows, 32), 0xA5, np.uint8)
    x_host[:, :2049] = BC.big_rows()[:2049]
    x_dev, x_n = _to_dev(x_host), _to_dev(np.array([2049, 500, 0], np.int32))

    def guided(ctx, out):
        ctx.match_guided_pairs_device(g_dev["q_desc"].data_ptr(), g_dev["q_kp"].data_ptr(), g_dev["nq"].data_ptr(), g_dev["t_desc"].data_ptr(),
                                      g_dev["t_kp"].data_ptr(), g_dev["nt"].data_ptr(), g_dev["windows"].data_ptr(), 1, g_rows, g_par, *out.ptrs())

    def proj(extent):
        def run(ctx, out):
            ctx.match_proj_pairs_device(p_dev["points"].data_ptr(), p_dev["p_desc"].data_ptr(), p_dev["np"].data_ptr(), len(scenes), p_rows,
                                        p_dev["t_desc"].data_ptr(), p_dev["t_kp"].data_ptr(), p_dev["nt"].data_ptr(), len(scenes), t_rows, p_dev["views"],
                                        PC.combo_params(binding, combo, extent_w=extent[0], extent_h=extent[1]), *out.ptrs(),
                                        d_train_right=p_dev["right"].data_ptr(), d_train_taken=p_dev["taken"].data_ptr())
        return run

    def bow(ctx, out):
        ctx.match_bow_pairs_device(b_dev["q_desc"].data_ptr(), b_dev["q_kp"].data_ptr(), b_dev["q_node"].data_ptr(), b_dev["nq"].data_ptr(),
                                   b_dev["t_desc"].data_ptr(), b_dev["t_kp"].data_ptr(), b_dev["t_node"].data_ptr(), b_dev["nt"].data_ptr(), 2, b_rows, b_par,
                                   *out.ptrs())

    def transform(ctx, out):
        ctx.bow_transform_device(x_dev.data_ptr(), x_n.data_ptr(), 3, x_rows, 1, *out.ptrs())

    g_out, p_out, b_out = (lambda: Outputs(1, g_rows)), (lambda: ProjOutputs(len(scenes), p_rows)), (lambda: Outputs(2, b_rows))
    steps = [("guided", g_out, guided), ("proj 320 x 240", p_out, proj((G.W, G.H))), ("bow pairs", b_out, bow),
             ("bow transform", lambda: Transformed(3, x_rows), transform), ("guided again", g_out, guided),
             ("proj 16000 x 12000", p_out, proj(PC.EXTENTS[0])), ("bow pairs again", b_out, bow), ("proj 1 x 1", p_out, proj((1, 1)))]
    return steps


def test_stages_interleaved_on_one_context_equal_the_stages_alone():
    """guided, projection and bag-of-words calls back to back on one context, no synchronise in between, at sizes that make the
    shared workspaces grow and then be reused at another layout; twice (the second round grows nothing).  Every output equals what
    the same call gives alone on a fresh context, and the first proj call equals the reference."""
    import torch
    from send_slam_amd import binding
    steps = _interleaved_steps()
    voc = BC.vocab("k10")
    torch.cuda.synchronize()
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        _set(ctx, voc)
        rounds = []
        for _ in range(2):
            outs = [alloc() for _, alloc, _ in steps]
            torch.cuda.synchronize()  # the prefills are complete; from here on the calls only enqueue
            for (_, _, launch), out in zip(steps, outs):
                launch(ctx, out)
            ctx.synchronize()
            rounds.append([_raw(o) for o in outs])
    for k, (name, alloc, launch) in enumerate(steps):
        with binding.OrbContext(0, n_features=G.NF) as ctx:
            _set(ctx, voc)
            out = alloc()
            torch.cuda.synchronize()
            launch(ctx, out)
            ctx.synchronize()
            alone = _raw(out)
        for r, got in enumerate(rounds):
            for field, want in alone.items():
                assert np.array_equal(got[k][field], want), f"round {r}, step {k} ({name}): {field} differs from the call alone"
    summ = rounds[0][1]["summary"].view(binding.PROJ_SUMMARY_DTYPE).reshape(-1)
    for k in range(len(PC.SCENES)):
        want = PC.scene_reference(k, PC.EXTENT_COMBOS[0])
        assert {f: int(summ[k][f]) for f in proj_ref.SUMMARY_FIELDS} == want[4] and np.array_equal(rounds[0][1]["idx"][k][:len(want[0])], want[0])
    assert int(rounds[0][0]["summary"].view(binding.GUIDED_SUMMARY_DTYPE)[0]["n_final"][0]) > 50
    want = BC.big_transform("k10", 1, 2049)
    assert np.array_equal(rounds[1][3]["bow_word"][0][:len(want[2])], want[2])


# ---- flagged frames in the batch forms -----------------------------------------------------------------------------------------------
FLAG_BATCH = ["synth_t0", "synth_t1", "synth_t2", "synth_t3"]
FLAG_TABLE = [-1, 0, 3, 0]  # frame 3 against frame 0: a pair the flags leave alone; by default (b - 1) its train frame is flagged
FLAG_COMBO = dict(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1)
FLAG_BOW = dict(UPSTREAM, one_to_one=True, orientation=1)


def _flag_run(binding):
    """the guided, transform and bow-match batch forms on FLAG_BATCH, with the default pairs and with FLAG_TABLE"""
    with binding.OrbContext(0, n_features=G.NF, max_batch=len(FLAG_BATCH)) as ctx:
        _, kcap = _extract(ctx, FLAG_BATCH)
        n = len(FLAG_BATCH)
        got = {}
        for key, table in (("guided", None), ("guided_table", FLAG_TABLE)):
            out = _outputs(n, kcap)
            ctx.match_guided_batch_device(_guided_params(binding, FLAG_COMBO), *out.ptrs(), train_src=table)
            ctx.synchronize()
            got[key] = out.host()
        _set(ctx, BC.vocab(MATCH_VOC))
        t = Transformed(n, kcap)
        ctx.bow_transform_batch_device(MATCH_LU, *t.ptrs())
        ctx.synchronize()
        got["transform"] = t.host()
        for key, table in (("bow", None), ("bow_table", FLAG_TABLE)):
            out = _outputs(n, kcap)
            ctx.match_bow_batch_device(binding.guided_params(**FLAG_BOW), *out.ptrs(), train_src=table)
            ctx.synchronize()  # raises nothing: the extraction's own frame_error is clean
            got[key] = out.host()
    return got


def test_flagged_frames_void_their_rows_in_the_batch_forms(monkeypatch):
    """SENDSLAM_TEST_FLAG_BATCH=1,2: frames 1 and 2 are flagged although they have keypoints.  Their summaries carry the status with
    zero counts, their rows are "none", their vectors empty; a query whose train frame is flagged is voided; everything else is
    what the unflagged run and the reference give"""
    from send_slam_amd import binding
    monkeypatch.delenv("SENDSLAM_TEST_FLAG_BATCH", raising=False)
    plain = _flag_run(binding)
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_BATCH", "1,2")
    flagged = _flag_run(binding)
    void = lambda want: want[:3] + (dict(want[3], status=binding.SS_ERR_OVERFLOW),)
    none_g = void(G.reference_pair("flat", None, FLAG_COMBO))
    none_b = void(BC.reference_pair(MATCH_VOC, MATCH_LU, "flat", None, FLAG_BOW))
    assert none_g[3]["n_query"] == 0 and len(none_g[0]) == 0
    for key, table, ref, none in (("guided", None, lambda q, t: G.reference_pair(q, t, FLAG_COMBO), none_g),
                                  ("guided_table", FLAG_TABLE, lambda q, t: G.reference_pair(q, t, FLAG_COMBO), none_g),
                                  ("bow", None, lambda q, t: BC.reference_pair(MATCH_VOC, MATCH_LU, q, t, FLAG_BOW), none_b),
                                  ("bow_table", FLAG_TABLE, lambda q, t: BC.reference_pair(MATCH_VOC, MATCH_LU, q, t, FLAG_BOW), none_b)):
        kept = 0
        for b, name in enumerate(FLAG_BATCH):
            t = (b - 1) if table is None else table[b]
            want = ref(name, FLAG_BATCH[t] if t >= 0 else None)
            _check(f"{key}, unflagged, frame {b}", plain[key], b, want)
            if b in (1, 2) or t in (1, 2):
                _check(f"{key}, frame {b} voided", flagged[key], b, none)
                assert want[3]["n_query"] > 100  # it had rows
            else:
                _check(f"{key}, flagged run, frame {b}", flagged[key], b, want)
                assert all(np.array_equal(flagged[key][j][b], plain[key][j][b]) for j in range(3)) and flagged[key][3][b] == plain[key][3][b]
                kept += want[3]["n_final"]
        assert kept > 50 if table else kept == 0, key  # by default only frame 0 is left, and it has no train frame
    voc = BC.vocab(MATCH_VOC)
    for b, name in enumerate(FLAG_BATCH):
        want = BC.frame_transform(MATCH_VOC, name, MATCH_LU)
        _check_transform(f"transform, unflagged, frame {b}", plain["transform"], b, want)
        if b in (1, 2):
            empty = B.transform_paths(voc, [], MATCH_LU, status=binding.SS_ERR_OVERFLOW)
            _check_transform(f"transform, frame {b} flagged", flagged["transform"], b, empty)
            assert want[4]["n_words"] > 10 and empty[4]["n_rows"] == 0 and empty[4]["norm"] == 0.0
        else:
            _check_transform(f"transform, flagged run, frame {b}", flagged["transform"], b, want)
            assert all(np.array_equal(flagged["transform"][j][b], plain["transform"][j][b]) for j in range(4))
