"""Per-stage HIP-event times of the epipolar search and the triangulation, one context alone on the chip, on the batch of
time_proj.py: 64 frames of 1280x720 / 2000 features (eight scenes, eight consecutive frames each), every frame paired with the first
frame of its scene (one new keyframe against its neighbours).  Nodes: a k = 10, L = 4 vocabulary of random descriptors at levelsup 2
(100 nodes, unevenly filled: about 43 train rows per query).  The synthetic frames carry no poses: the pairs are tests/epi_cases.py's scaled pose
pairs, so the share of couples that passes the geometry is that of an arbitrary epipolar band, not of a tracked sequence.
The yardstick, in the SAME run on the same arrays, is ss_match_bow_pairs_device (SearchByBoW on the same nodes).  Timed: the pairs
form (index, search, finish), its coarse form, the triangulation of the search's matches, and the batch form after
ss_bow_transform_batch_device.  Prints the per-batch median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_epi.py [frames] [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import epi_cases as EC  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h, nf = 1280, 720, 2000
K, L, LEVELSUP = 10, 4, 2
cam = (900.0, 900.0, 640.0, 360.0)
scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = np.stack([synth.frame_from_scene(scenes[(b // 8) % 8], 2000 + (b // 8) % 8, w, h, b % 8) for b in range(B)])
d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
ctx = binding.OrbContext(0, n_features=nf, max_batch=B)
ctx.extract_batch_device(d.data_ptr(), B, w, h)
ctx.synchronize()
kcap = ctx.batch_view().kp_capacity
n_tree = sum(K ** lv for lv in range(1, L + 1))
ids = np.arange(1, n_tree + 1, dtype=np.int64)
leaf = (ids > n_tree - K ** L).astype(np.uint8)
rng = np.random.Generator(np.random.PCG64(0x0B0C))
tree_desc = rng.integers(0, 256, size=(n_tree, 32), dtype=np.uint8)
with binding.Vocabulary.from_arrays(((ids - 1) // K).astype(np.int32), leaf, tree_desc, np.where(leaf == 1, rng.random(n_tree) * 9 + 0.01, 0.0), K, L) as voc:
    ctx.set_vocabulary(voc)
t_word, t_node, t_bw = (torch.empty((B, kcap), dtype=torch.int32, device="cuda") for _ in range(3))
t_bv = torch.empty((B, kcap), dtype=torch.float64, device="cuda")
t_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ctx.bow_transform_batch_device(LEVELSUP, t_word.data_ptr(), t_node.data_ptr(), t_bw.data_ptr(), t_bv.data_ptr(), t_sum.data_ptr())
ctx.synchronize()
src = [8 * (b // 8) for b in range(B)]
pairs = np.concatenate([np.asarray(EC.make_pair(EC.pose(b % 3), EC.pose((b + 1) % 3), cam, cam)).reshape(1) for b in range(B)])

# the pairs form's arrays: the query side is the batch as it is, the train side the first frame of each scene, gathered on the host
node = t_node.cpu().numpy()
host = {"kp": np.zeros((B, kcap), binding.KP_DTYPE), "desc": np.zeros((B, kcap, 32), np.uint8), "n": np.zeros(B, np.int32)}
for b in range(B):
    kp, desc, _ = ctx.fetch_frame(b)
    host["kp"][b, :len(kp)], host["desc"][b, :len(kp)], host["n"][b] = kp, desc, len(kp)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else np.ascontiguousarray(a)).cuda()
q_kp, q_desc, q_node, q_n = up(host["kp"]), up(host["desc"]), up(node), up(host["n"])
t_kp, t_desc, t_nd, t_n = up(host["kp"][src]), up(host["desc"][src]), up(node[src]), up(host["n"][src])
d_idx = torch.empty((B, kcap), dtype=torch.int32, device="cuda")
d_d1 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_d2 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_sum = torch.empty(B * 40, dtype=torch.uint8, device="cuda")  # ss_epi_summary rows (40 bytes) or ss_guided_summary rows (32), contiguous
d_info = torch.empty((B, kcap * 16), dtype=torch.uint8, device="cuda")
d_pts, d_pd = (torch.empty((B, kcap * 32), dtype=torch.uint8, device="cuda") for _ in range(2))
d_rows = torch.empty((B, kcap * 2), dtype=torch.int32, device="cuda")
d_np = torch.empty(B, dtype=torch.int32, device="cuda")
d_tsum = torch.empty(B * 64, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()  # the context's stream does not wait for torch's


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
    st = {s["name"]: {"median_ms": round(s["median_ms"] * (s["launches"] // reps), 5), "mean_ms": round(s["total_ms"] / reps, 5),
                      "launches_per_call": s["launches"] // reps, "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"]}
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    return st


def epi_pairs(p):
    ctx.match_epi_pairs_device(q_desc.data_ptr(), q_kp.data_ptr(), q_node.data_ptr(), q_n.data_ptr(), t_desc.data_ptr(), t_kp.data_ptr(), t_nd.data_ptr(),
                               t_n.data_ptr(), B, kcap, pairs, p, d_idx.data_ptr(), d_d1.data_ptr(), d_sum.data_ptr())


def epi_counts():
    s = d_sum.cpu().numpy()[:B * 40].copy().view(binding.EPI_SUMMARY_DTYPE).reshape(B)
    return {k: int(s[k].sum()) for k in ("n_query", "n_candidates", "n_geometric", "n_near", "n_accepted", "n_unique", "n_final")}


result = {"frames": B, "size": [w, h], "n_features": nf, "kp_capacity": kcap, "reps": reps, "device": torch.cuda.get_device_name(0),
          "vocabulary": {"k": K, "L": L, "levelsup": LEVELSUP}, "train_src": "the first frame of the scene"}
for name, p in (("coarse", binding.epi_params(coarse=True)), ("fused", binding.epi_params())):  # the fused form last: its matches are triangulated
    st = stages(lambda: epi_pairs(p))
    st["counts"] = epi_counts()
    result["epi_" + name] = st
    print("epi", name, json.dumps(st))
st = stages(lambda: ctx.triangulate_pairs_device(q_desc.data_ptr(), q_kp.data_ptr(), q_n.data_ptr(), t_kp.data_ptr(), t_n.data_ptr(), d_idx.data_ptr(), B, kcap,
                                                 pairs, binding.tri_params(), d_info.data_ptr(), d_pts.data_ptr(), d_pd.data_ptr(), d_rows.data_ptr(),
                                                 d_np.data_ptr(), d_tsum.data_ptr()))
ts = d_tsum.cpu().numpy().copy().view(binding.TRI_SUMMARY_DTYPE).reshape(B)
st["counts"] = {"n_matches": int(ts["n_matches"].sum()), "n_points": int(ts["n_points"].sum()), "n_state": [int(v) for v in ts["n_state"].sum(axis=0)]}
result["triangulate"] = st
print("triangulate", json.dumps(st))
st = stages(lambda: ctx.match_epi_batch_device(pairs, binding.epi_params(), d_idx.data_ptr(), d_d1.data_ptr(), d_sum.data_ptr(), train_src=src))
st["counts"] = epi_counts()
result["epi_batch_form"] = st
print("epi batch form", json.dumps(st))
for name, p in (("no_ratio", binding.guided_params(th=50, ratio_num=0, ratio_den=0, orientation=1)),
                ("upstream", binding.guided_params(th=50, ratio_num=7, ratio_den=10, orientation=1))):
    st = stages(lambda: ctx.match_bow_pairs_device(q_desc.data_ptr(), q_kp.data_ptr(), q_node.data_ptr(), q_n.data_ptr(), t_desc.data_ptr(), t_kp.data_ptr(),
                                                   t_nd.data_ptr(), t_n.data_ptr(), B, kcap, p, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(),
                                                   d_sum.data_ptr()))
    s = d_sum.cpu().numpy()[:B * 32].copy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(B)
    st["counts"] = {k: int(s[k].sum()) for k in ("n_query", "n_candidates", "n_accepted", "n_unique", "n_final")}
    result["bow_" + name] = st
    print("bow", name, json.dumps(st))
f, c, y = result["epi_fused"], result["epi_coarse"], result["bow_no_ratio"]
couples = max(f["counts"]["n_candidates"], 1)
for r, key in ((f, "epi_search"), (c, "epi_search"), (y, "bow_search")):
    r["search_ns_per_couple"] = round(1e6 * r[key]["median_ms"] / max(r["counts"]["n_candidates"], 1), 4)
print(f"fused search {f['epi_search']['median_ms']:.4f} ms, coarse {c['epi_search']['median_ms']:.4f} ms, BoW search {y['bow_search']['median_ms']:.4f} ms per {B} pairs; "
      f"{couples} couples, {f['counts']['n_geometric']} geometric, {f['counts']['n_near']} near; per couple {f['search_ns_per_couple']} / "
      f"{c['search_ns_per_couple']} / {y['search_ns_per_couple']} ns; triangulation {result['triangulate']['total_ms']:.4f} ms")
if out_path:
    json.dump(result, open(out_path, "w"), indent=1)
