"""GPU parity of the place recognition (ss_place_set_database, ss_place_query_device, ss_place) against tests/place_ref.py: byte for byte
on d_cand, d_summary, d_words and d_score, every output prefilled with a pattern no result has.  tests/test_place_ref.py asserts on the
reference that the scenes are live.  Every test ends its context before the next; the out-of-range words and counts are the rule's
defined inputs."""
import os

import numpy as np
import pytest

import bow_ref as B
import guided_cases as G
import place_cases as PC
import place_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = PC.shared_cases()
U = PC.U


def _dev():
    import torch
    return torch.device("cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()  # the library's stream does not wait for torch's


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(len(a), -1) if a.dtype.fields else a).to(_dev())
    _sync()
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class Database:
    """a case's database arrays on the device"""

    def __init__(self, k):
        self.k = k
        self.word, self.value, self.count, self.nb = _to_dev(k["db_word"]), _to_dev(k["db_value"]), _to_dev(k["db_count"]), _to_dev(k["nb"])
        self.skip = None if k["db_skip"] is None else _to_dev(k["db_skip"])
        self.n_db, self.stride = k["db_word"].shape

    def set(self, ctx):
        ctx.place_set_database(self.word.data_ptr(), self.value.data_ptr(), self.count.data_ptr(), self.n_db, self.stride, self.k["n_words"], self.k["problems"],
                               d_db_skip=_ptr(self.skip))


def query(ctx, db, k, words=True, score=True):
    """the queries of case k against the context's database -> (cand, summary, words, score) as the reference returns them"""
    import torch
    from send_slam_amd import binding
    n_q, q_stride = k["q_word"].shape
    qw, qv, qc = _to_dev(k["q_word"]), _to_dev(k["q_value"]), _to_dev(k["q_count"])
    q_nb = None if k["q_nb"] is None else _to_dev(k["q_nb"])
    q_row = None if k["q_nb"] is None else _to_dev(k["q_row"])
    cap = k["cand_cap"]
    d_cand = torch.full((n_q, cap * 24), 0x5A, dtype=torch.uint8, device=_dev())
    d_sum = torch.full((n_q, 48), 0x5A, dtype=torch.uint8, device=_dev())
    d_words = torch.full((n_q, db.n_db), 0x5A5A5A5A, dtype=torch.int32, device=_dev()) if words else None
    d_score = torch.full((n_q, db.n_db), 0x5A5A5A5A, dtype=torch.int32, device=_dev()) if score else None
    _sync()
    ctx.place_query_device(qw.data_ptr(), qv.data_ptr(), qc.data_ptr(), q_stride, k["q_kf"], k["q_problem"], db.nb.data_ptr(), k["nb"].shape[1],
                           binding.place_params(**k["params"]), cap, d_cand.data_ptr(), d_sum.data_ptr(), d_words=_ptr(d_words), d_score=_ptr(d_score),
                           d_q_nb=_ptr(q_nb), d_q_row=_ptr(q_row), q_cap=0 if q_nb is None else k["q_nb"].shape[1])
    ctx.synchronize()
    return (d_cand.cpu().numpy().copy().view(PR.CAND_DTYPE).reshape(n_q, cap), d_sum.cpu().numpy().copy().view(PR.SUMMARY_DTYPE).reshape(n_q),
            None if d_words is None else d_words.cpu().numpy(), None if d_score is None else d_score.cpu().numpy().view(np.float32))


def same(tag, got, want):
    (cand, summary, words, score), (wcand, wsummary, wwords, wscore) = got, want
    for name in PR.SUMMARY_DTYPE.names:
        a, b = np.ascontiguousarray(summary[name]), np.ascontiguousarray(wsummary[name])
        assert a.tobytes() == b.tobytes(), f"{tag}: summary.{name} {a.tolist()[:16]} != {b.tolist()[:16]}"
    for name in PR.CAND_DTYPE.names:
        a, b = np.ascontiguousarray(cand[name]), np.ascontiguousarray(wcand[name])
        assert a.tobytes() == b.tobytes(), f"{tag}: cand.{name} {a.tolist()[:4]} != {b.tolist()[:4]}"
    assert cand.tobytes() == wcand.tobytes() and summary.tobytes() == wsummary.tobytes(), tag
    if words is not None:
        assert np.array_equal(words, wwords), f"{tag}: words differ at {np.argwhere(words != wwords)[:6].tolist()}"
    if score is not None:
        assert score.tobytes() == np.ascontiguousarray(wscore).tobytes(), f"{tag}: score differs at {np.argwhere(score.view(np.uint32) != wscore.view(np.uint32))[:6].tolist()}"


def run(k, **kw):
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        db = Database(k)
        db.set(ctx)
        return query(ctx, db, k, **kw)


def test_scenes_against_the_reference():
    """every scene of the CPU tests, each its own database, on one context"""
    from send_slam_amd import binding
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        for name in sorted(SHARED):
            db = Database(SHARED[name])
            db.set(ctx)
            same(name, query(ctx, db, SHARED[name]), PR.run(SHARED[name]))


@pytest.mark.parametrize("n_db", [1, 63, 64, 65, 257])
def test_database_sizes_across_wave_and_block_edges(n_db):
    """five queries in one call; stride 12 against q_stride 9"""
    for kw in (dict(mode=1), dict(mode=0, n_best=2, n_problems=3)):
        k = PC.random_case(100 + n_db, n_db, 5, **kw)
        assert k["db_word"].shape[1] != k["q_word"].shape[1]
        same(f"n_db {n_db} {kw}", run(k), PR.run(k))


def long_list_case():
    """word 0 held by all of 3000 rows, words 1 .. 40 by one row each: the split of a long list and the short lists in one launch"""
    rows = [{0: 4 * U, 1 + r: (1 + r % 8) * U} if r < 40 else {0: 4 * U} for r in range(3000)]
    queries = [dict(vec=PC.vec(range(0, 41), 8)), dict(vec={0: 8 * U}), dict(vec=PC.vec(range(1, 41), 8), kf=7)]
    return PC.case(rows, queries, n_words=64, nb={r: [r + 1, r + 2] for r in range(0, 60)}, cand_cap=12, params=dict(min_score=4 * U))


def test_one_long_list_and_forty_short_ones():
    k = long_list_case()
    want = PR.run(k)
    assert want[1]["n_sharing"].tolist() == [3000, 3000, 39] and want[1]["n_survivors"].tolist() == [40, 3000, 39] and want[1]["n_candidates"].tolist() == [15, 60, 9]
    same("long list", run(k), want)


def test_query_lengths():
    """queries of 1, 64, 65 and q_stride words in one call"""
    rng = np.random.default_rng(5)
    rows = [{int(w): int(rng.integers(1, 17)) * U for w in rng.choice(300, int(rng.integers(20, 100)), replace=False)} for _ in range(90)]
    queries = [dict(vec={int(w): int(rng.integers(1, 17)) * U for w in rng.choice(300, n, replace=False)}) for n in (1, 64, 65, 80)]
    k = PC.case(rows, queries, n_words=300, nb={r: [(r + 1) % 90, (r + 7) % 90] for r in range(90)}, q_stride=80, params=dict(min_score=8 * U))
    want = PR.run(k)
    assert k["q_count"].tolist() == [1, 64, 65, 80] and (want[1]["n_seeds"][1:] > 0).all() and want[1]["n_sharing"][0] > 0
    same("query lengths", run(k), want)


def sixteen():
    k = PC.random_case(77, 120, 16, mode=0, empty=(1, 5, 9))
    k["q_value"][[2, 6]] = U / 8.0  # at most 9 common words of U / 8 each: below the minimum score of 2 U
    return k


def test_sixteen_queries_some_empty_some_without_a_seed():
    k = sixteen()
    want = PR.run(k)
    assert (want[1]["n_sharing"][[1, 5, 9]] == 0).all() and (want[1]["n_survivors"][[2, 6]] > 0).all() and (want[1]["n_seeds"][[2, 6]] == 0).all()
    assert (want[1]["n_candidates"] > 0).sum() >= 8
    same("sixteen", run(k), want)


def test_small_database_after_a_large_one_and_a_repeated_query():
    from send_slam_amd import binding
    large, small = PC.random_case(31, 257, 3, n_words=997), PC.random_case(32, 9, 3)
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        a = Database(large)
        a.set(ctx)
        same("large", query(ctx, a, large), PR.run(large))
        b = Database(small)
        b.set(ctx)
        first, second = query(ctx, b, small), query(ctx, b, small)
        same("small", first, PR.run(small))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))
        ctx.place_set_database(0, 0, 0, 0, 1, 1, np.zeros(0, PR.PROBLEM_DTYPE))  # n_db 0 clears it
        with pytest.raises(binding.OrbError) as e:
            query(ctx, b, small)
        assert e.value.code == binding.SS_ERR_STATE and "ss_place_set_database" in e.value.message


def test_skip_bytes_change_between_queries_without_a_rebuild():
    from send_slam_amd import binding
    k = PC.random_case(41, 60, 6)
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        db = Database(k)
        db.set(ctx)
        before = PR.run(k)
        same("before", query(ctx, db, k), before)
        erased = k["db_skip"].copy()
        erased[before[0]["kf"][before[0]["kf"] >= 0]] = 1  # erase every candidate
        db.skip.copy_(_to_dev(erased))
        _sync()
        after = PR.run(k, db_skip=erased)
        assert after[0].tobytes() != before[0].tobytes()
        same("after", query(ctx, db, k), after)


def test_without_the_raw_tables():
    k = sixteen()
    same("no d_words, no d_score", run(k, words=False, score=False), PR.run(k))


def test_host_form_and_refusals():
    from send_slam_amd import binding
    k = PC.random_case(51, 40, 4, n_best=1, n_problems=2)
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        db = Database(k)
        with pytest.raises(binding.OrbError) as e:
            query(ctx, db, k)
        assert e.value.code == binding.SS_ERR_STATE
        got = ctx.place(k["db_word"], k["db_value"], k["db_count"], k["n_words"], k["problems"], k["q_word"], k["q_value"], k["q_count"], k["q_kf"], k["q_problem"],
                        k["nb"], binding.place_params(**k["params"]), k["cand_cap"], db_skip=k["db_skip"], q_nb=k["q_nb"], q_row=k["q_row"])
        same("ss_place", got, PR.run(k))
        db.set(ctx)
        with pytest.raises(binding.OrbError) as e:
            query(ctx, db, dict(k, q_kf=np.full(4, 40, np.int32)))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "q_kf" in e.value.message
        with pytest.raises(binding.OrbError) as e:
            ctx.place_set_database(db.word.data_ptr(), db.value.data_ptr(), db.count.data_ptr(), 40, db.stride, 0, k["problems"])
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "n_words" in e.value.message
        same("the database a refused call found", query(ctx, db, k), PR.run(k))


def test_chain_transform_database_covisibility_query_match():
    """ss_bow_transform_device on descriptors -> the rows copied device to device into the database -> ss_covis_set_map + ss_covis_kf_device
    (rows NULL, cap 10), d_nb fed without a round trip -> ss_place_query_device -> the candidates into ss_match_bow_pairs_device.  Twelve
    keyframes: 0 .. 2 see place A, 3 .. 8 place B, 9 .. 11 place A again through new map points, so 11 is connected to 9 and 10 and its
    loop candidates are among 0 .. 2.  The reference is fed the tables the device produced."""
    import torch
    from send_slam_amd import binding
    from test_guided import Outputs, _check
    rng = np.random.default_rng(9)
    n_kf, rows, cap = 12, 64, 10
    places = rng.integers(0, 256, (2, rows, 32), dtype=np.uint8)
    desc = np.zeros((n_kf, rows, 32), np.uint8)
    for kf in range(n_kf):
        place, flips = (0 if kf < 3 or kf >= 9 else 1), (24 if kf in (9, 10) else 3)
        bits = np.unpackbits(places[place], axis=1)
        for r in range(rows):
            bits[r, rng.choice(256, flips, replace=False)] ^= 1
        desc[kf] = np.packbits(bits, axis=1)
    first_point = [0] * 3 + [64] * 6 + [128] * 3
    obs = np.zeros(n_kf * rows, binding.GBA_OBS_DTYPE)
    obs["kf"], obs["point"] = np.repeat(np.arange(n_kf), rows), np.concatenate([np.arange(rows) + p for p in first_point])
    obs["right"] = -1.0
    problems = np.zeros(1, binding.GBA_PROBLEM_DTYPE)
    problems[0]["n_kf"], problems[0]["n_blocks"], problems[0]["n_obs"] = n_kf, 1, len(obs)
    voc = binding.Vocabulary.load_text(os.path.join(ROOT, "tests", "golden", "bow", "k3_vocabulary.txt"))
    n_words = voc.info()["n_words"]
    with binding.OrbContext(0, n_features=G.NF) as ctx:
        ctx.set_vocabulary(voc)
        d_desc, d_n = _to_dev(desc), _to_dev(np.full(n_kf, rows, np.int32))
        word, node, bow_word = (torch.full((n_kf, rows), -7, dtype=torch.int32, device=_dev()) for _ in range(3))
        bow_value = torch.zeros((n_kf, rows), dtype=torch.float64, device=_dev())
        t_sum = torch.zeros((n_kf, 32), dtype=torch.uint8, device=_dev())
        _sync()
        ctx.bow_transform_device(d_desc.data_ptr(), d_n.data_ptr(), n_kf, rows, 2, word.data_ptr(), node.data_ptr(), bow_word.data_ptr(), bow_value.data_ptr(), t_sum.data_ptr())
        ctx.synchronize()
        db_word, db_value = bow_word.clone(), bow_value.clone()  # device to device
        db_count = t_sum.view(torch.int32)[:, 3].contiguous()    # ss_bow_summary.n_words
        _sync()
        ctx.place_set_database(db_word.data_ptr(), db_value.data_ptr(), db_count.data_ptr(), n_kf, rows, n_words, problems)
        ctx.covis_set_map(problems, n_kf, 1, 192, obs)
        d_nb = torch.full((n_kf, cap, 2), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        d_row = torch.full((n_kf, 32), 0x5A, dtype=torch.uint8, device=_dev())
        d_cand = torch.full((1, 8 * 24), 0x5A, dtype=torch.uint8, device=_dev())
        d_sum = torch.full((1, 48), 0x5A, dtype=torch.uint8, device=_dev())
        _sync()
        ctx.covis_kf_device(None, n_kf, binding.covis_params(), cap, d_nb.data_ptr(), d_row.data_ptr())
        q = n_kf - 1
        params = dict(min_score_mode=1)
        ctx.place_query_device(db_word[q].data_ptr(), db_value[q].data_ptr(), db_count[q:].data_ptr(), rows, [q], [0], d_nb.data_ptr(), cap, binding.place_params(**params), 8,
                               d_cand.data_ptr(), d_sum.data_ptr(), d_q_nb=d_nb[q].data_ptr(), d_q_row=d_row[q].data_ptr(), q_cap=cap)
        ctx.synchronize()
        cand, summary = d_cand.cpu().numpy().copy().view(PR.CAND_DTYPE).reshape(8), d_sum.cpu().numpy().copy().view(PR.SUMMARY_DTYPE).reshape(-1)[0]
        nb, row = d_nb.cpu().numpy(), d_row.cpu().numpy().copy().view(PR.ROW_DTYPE).reshape(n_kf)
        assert sorted(nb[q, :row[q]["n_written"], 0].tolist()) == [9, 10]
        ref_db = PR.Database(db_word.cpu().numpy(), db_value.cpu().numpy(), db_count.cpu().numpy(), n_words, problems)
        qw, qv = ref_db.vector(q)
        wcand, wsummary, _, _ = PR.query(ref_db, qw, qv, q, 0, nb, params, 8, q_nb=nb[q], q_row=row[q])
        assert cand.tobytes() == wcand.tobytes() and summary.tobytes() == wsummary.tobytes(), (cand, wcand, summary, wsummary)
        found = cand["kf"][:int(summary["n_written"])].tolist()
        assert found and set(found) <= {0, 1, 2}, found
        # the candidates' rows, gathered on the device, against the query keyframe
        n = len(found)
        at = torch.tensor(found, device=_dev())
        kp = torch.zeros((n, rows, binding.KP_DTYPE.itemsize), dtype=torch.uint8, device=_dev())
        q_desc, q_node = d_desc[q:q + 1].expand(n, rows, 32).contiguous(), node[q:q + 1].expand(n, rows).contiguous()
        t_desc, t_node = d_desc[at].contiguous(), node[at].contiguous()
        counts = torch.full((n,), rows, dtype=torch.int32, device=_dev())
        out = Outputs(n, rows)
        _sync()
        combo = dict(th=50, ratio_num=7, ratio_den=10, one_to_one=False, orientation=0)
        ctx.match_bow_pairs_device(q_desc.data_ptr(), kp.data_ptr(), q_node.data_ptr(), counts.data_ptr(), t_desc.data_ptr(), kp.data_ptr(), t_node.data_ptr(),
                                   counts.data_ptr(), n, rows, binding.guided_params(**combo, extent_w=G.W, extent_h=G.H), *out.ptrs())
        ctx.synchronize()
        got, h_node, zero_kp = out.host(), node.cpu().numpy(), np.zeros(rows, binding.KP_DTYPE)
        for i, kf in enumerate(found):
            want = B.match(zero_kp, desc[q], h_node[q], zero_kp, desc[kf], h_node[kf], **combo)
            _check(f"candidate {kf}", got, i, want)
            assert (want[0] >= 0).sum() > rows // 4
