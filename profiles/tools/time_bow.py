"""Per-stage HIP-event times of the bag-of-words stages, one context alone on the chip: the batch of time_guided.py (64 frames of
1280x720 / 2000 features, eight scenes of eight consecutive frames, frame b against b - 1) with a generated k = 10, L = 6
vocabulary of random descriptors (1 111 110 nodes, ORBvoc.txt's shape), levelsup 4.  Timed: the descent, vector + index, the BoW
search and finish, and the L1 score of one query against 10 000 kept vectors.  Where the descent's time goes: the same rows
through the upper four levels of the same tree alone (a k = 10, L = 4 vocabulary).  What the serial norm chain costs: vector +
index with a 10-word vocabulary (L = 1), whose chains have at most 10 links.  Measured in the SAME run, on the same batch, as the
yardsticks: ss_match_batch_device mode 1 (all-pairs, the matrix-core matcher) and the guided call of DESIGN.md section 14.
usage: python profiles/tools/time_bow.py [frames] [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h, nf = 1280, 720, 2000
K, LEVELSUP, N_DB = 10, 4, 10000


def full_tree(L, desc, seed):
    """breadth-first ids: node i has the children K i + 1 .. K i + K; the first rows of `desc`; leaves weigh 0.01 .. 9"""
    n = sum(K ** d for d in range(1, L + 1))
    ids = np.arange(1, n + 1, dtype=np.int64)
    leaf = (ids > n - K ** L).astype(np.uint8)
    rng = np.random.Generator(np.random.PCG64(seed))
    return binding.Vocabulary.from_arrays(((ids - 1) // K).astype(np.int32), leaf, desc[:n], np.where(leaf == 1, rng.random(n) * 9 + 0.01, 0.0), K, L)


scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = np.stack([synth.frame_from_scene(scenes[(b // 8) % 8], 2000 + (b // 8) % 8, w, h, b % 8) for b in range(B)])
d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
ctx = binding.OrbContext(0, n_features=nf, max_batch=B)
ctx.extract_batch_device(d.data_ptr(), B, w, h)
kcap = ctx.batch_view().kp_capacity
n_full = sum(K ** lv for lv in range(1, 7))
tree_desc = np.random.Generator(np.random.PCG64(0x0B0C)).integers(0, 256, size=(n_full, 32), dtype=np.uint8)
d_idx = torch.empty((B, kcap), dtype=torch.int32, device="cuda")
d_d1 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_d2 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")
t_word, t_node, t_bw = (torch.empty((B, kcap), dtype=torch.int32, device="cuda") for _ in range(3))
t_bv = torch.empty((B, kcap), dtype=torch.float64, device="cuda")
t_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")


def stages(fn):
    """median ms per call of every stage `fn` launches (one call per repetition)"""
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(reps):
        fn()
        ctx.synchronize()
    ctx.profile(False)
    return {s["name"]: {"median_ms": round(s["median_ms"] * (s["launches"] // reps), 5), "mean_ms": round(s["total_ms"] / reps, 5),
                        "launches_per_call": s["launches"] // reps, "algorithmic_bytes": s["algorithmic_bytes"]}
            for s in ctx.stats() if s["launches"]}


def transform():
    ctx.bow_transform_batch_device(LEVELSUP, t_word.data_ptr(), t_node.data_ptr(), t_bw.data_ptr(), t_bv.data_ptr(), t_sum.data_ptr())


def bow_summaries():
    return t_sum.cpu().numpy().view(binding.BOW_SUMMARY_DTYPE).reshape(B)


result = {"frames": B, "size": [w, h], "n_features": nf, "kp_capacity": kcap, "reps": reps, "device": torch.cuda.get_device_name(0),
          "vocabulary": {"k": K, "L": 6, "n_nodes": n_full, "levelsup": LEVELSUP}}
for name, L in (("upper_four_levels", 4), ("ten_words", 1), ("transform", 6)):  # the full tree last: the match uses its nodes
    with full_tree(L, tree_desc, 0x0B0D) as voc:
        ctx.set_vocabulary(voc)
    st = stages(transform)
    s = bow_summaries()
    st["counts"] = {k: int(s[k].sum()) for k in ("n_rows", "n_used", "n_words", "n_nodes")}
    result[name] = st
    print(name, json.dumps(st))
upstream = binding.guided_params(th=50, ratio_num=7, ratio_den=10, one_to_one=True, orientation=1)
st = stages(lambda: ctx.match_bow_batch_device(upstream, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(), d_sum.data_ptr()))
summ = d_sum.cpu().numpy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(B)
st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
st["counts"] = {k: int(summ[k].sum()) for k in ("n_query", "n_candidates", "n_accepted", "n_unique", "n_final")}
st["candidates_per_query"] = round(st["counts"]["n_candidates"] / max(1, int(summ["n_query"][1:].sum())), 3)
result["match_bow"] = st
print("match_bow", json.dumps(st))
# one query against N_DB kept vectors: the batch's vectors over and over, at the transform's stride
rep = (N_DB + B - 1) // B
db_w, db_v = t_bw.repeat(rep, 1)[:N_DB].contiguous(), t_bv.repeat(rep, 1)[:N_DB].contiguous()
counts = t_sum.view(torch.int32)[:, 3].contiguous()
db_n = counts.repeat(rep)[:N_DB].contiguous()
d_score = torch.empty(N_DB, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()  # the context's stream does not wait for torch's
st = stages(lambda: ctx.bow_score_device(t_bw[1].data_ptr(), t_bv[1].data_ptr(), counts[1:].data_ptr(), kcap, db_w.data_ptr(), db_v.data_ptr(),
                                         db_n.data_ptr(), N_DB, kcap, d_score.data_ptr()))
st["n_db"], st["query_words"], st["mean_db_words"] = N_DB, int(counts[1]), round(float(db_n.double().mean()), 1)
sc = d_score.cpu().numpy()
st["best"] = [int(i) for i in np.argsort(-sc, kind="stable")[:3] % B]
result["score"] = st
print("score", json.dumps(st))
guided = binding.guided_params(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1, radius=15.0, radius_by_octave=True, octave_span=1)
st = stages(lambda: ctx.match_guided_batch_device(guided, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(), d_sum.data_ptr()))
summ = d_sum.cpu().numpy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(B)
st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
st["counts"] = {k: int(summ[k].sum()) for k in ("n_query", "n_candidates", "n_accepted", "n_unique", "n_final")}
result["guided_init"] = st
print("guided", json.dumps(st))
result["match_batch_mode1"] = stages(lambda: ctx.match_batch_device(1, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr()))
result["match_batch_mode1"]["n_accepted"] = int((d_idx.cpu().numpy() >= 0).sum())
print("match_batch_device mode 1", json.dumps(result["match_batch_mode1"]))
t = result["transform"]
print(f"descent {t['bow_descend']['median_ms']:.4f} ms (upper four levels alone {result['upper_four_levels']['bow_descend']['median_ms']:.4f}), "
      f"vector + index {t['bow_vector']['median_ms']:.4f} ms (ten words {result['ten_words']['bow_vector']['median_ms']:.4f}), "
      f"bow search + finish {result['match_bow']['total_ms']:.4f} ms, guided {result['guided_init']['total_ms']:.4f} ms, "
      f"all-pairs {result['match_batch_mode1']['match']['median_ms']:.4f} ms per {B} frames; score {result['score']['bow_score']['median_ms']:.4f} ms per {N_DB} vectors")
if out_path:
    json.dump(result, open(out_path, "w"), indent=1)
