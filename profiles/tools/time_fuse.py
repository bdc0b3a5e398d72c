"""Per-stage HIP-event times of map-point fusion, one context alone on the chip, on the batch of time_proj.py: 64 frames of
1280x720 / 2000 features (eight scenes, eight consecutive frames each).  Each scene has one shared map: the keypoints of its first
frame back-projected at depths 2 .. 8 (tests/proj_cases.back_project), about 2000 points; frame b fuses the map of its scene under a
pose a few pixels away from identity (point_src[b] = scene); 40 % of the train rows carry a map-point id.  The yardstick, in the
SAME run on the same arrays, is ss_match_proj_pairs_device at th 1 and th 3.  Rows visited (train rows that
pass the octave and the window test, whatever comes after) are counted on the host from the call's own ss_fuse_point rows.
Prints the per-batch median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_fuse.py [frames] [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import fuse_ref as F  # noqa: E402
import guided_ref as R  # noqa: E402
import proj_cases as PC  # noqa: E402
import proj_ref as P  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h, nf = 1280, 720, 2000
fx, cx, cy, bf = 900.0, 640.0, 360.0, 45.0
n_scenes = min(8, (B + 7) // 8)
scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = np.stack([synth.frame_from_scene(scenes[(b // 8) % 8], 2000 + (b // 8) % 8, w, h, b % 8) for b in range(B)])
d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
ctx = binding.OrbContext(0, n_features=nf, max_batch=B)
ctx.extract_batch_device(d.data_ptr(), B, w, h)
ctx.synchronize()
bv = ctx.batch_view()
kcap = bv.kp_capacity
scale = [np.float32(1.0)]
for _ in range(7):
    scale.append(np.float32(float(scale[-1]) * float(np.float32(1.2))))

# the maps: block s = the first frame of scene s, back-projected
rng = np.random.Generator(np.random.PCG64(0x7140))
pts = np.zeros((n_scenes, kcap), binding.MAP_POINT_DTYPE)
pdesc = np.zeros((n_scenes, kcap, 32), np.uint8)
counts = np.zeros(n_scenes, np.int32)
for s in range(n_scenes):
    kp, desc, _ = ctx.fetch_frame(8 * s)
    block, _ = PC.back_project(rng, kp, scale, fx, fx, cx, cy)
    counts[s] = len(kp)
    pts[s, :len(kp)], pdesc[s, :len(kp)] = block, desc
train_kp = [ctx.fetch_frame(b)[0] for b in range(B)]
views = np.concatenate([np.asarray(P.view_init(fx, fx, cx, cy, w, h, *PC.POSES[b % 3], bf)).reshape(1) for b in range(B)])
point_src = [(b // 8) % 8 for b in range(B)]
ids = np.where(rng.random((B, kcap)) < 0.4, rng.integers(0, 1 << 30, (B, kcap)), -1).astype(np.int32)
d_pts = torch.from_numpy(pts.view(np.uint8).reshape(n_scenes, -1)).cuda()
d_pd = torch.from_numpy(pdesc).cuda()
d_n = torch.from_numpy(counts).cuda()
d_ids = torch.from_numpy(ids).cuda()
d_idx = torch.empty((B, kcap), dtype=torch.int32, device="cuda")
d_d1 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_d2 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_act = torch.empty((B, kcap * 8), dtype=torch.uint8, device="cuda")
d_point = torch.empty((B, kcap * 32), dtype=torch.uint8, device="cuda")
d_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ext = dict(extent_w=w, extent_h=h)
VARIANTS = {"local_mapping": binding.fuse_params(**F.LOCAL_MAPPING, **ext),
            "sim3_th4": binding.fuse_params(**F.SEARCH_AND_FUSE, **ext),
            "sim3_th8": binding.fuse_params(**F.CANDIDATE_CHECK, **ext),
            # what the order buys: local mapping's window with the chi-square test off, so every visited row costs a descriptor
            "th3_no_chi2": binding.fuse_params(**dict(F.LOCAL_MAPPING, chi2_mono=0.0), **ext)}
PROJ = {"local_points_th1": binding.proj_params(th=1.0, **ext), "local_points_th3": binding.proj_params(th=3.0, **ext)}
train = (bv.descriptors, bv.keypoints, bv.n_keypoints)


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


def visited(point_rows):
    """train rows inside the octave range and the window of every point, summed over the batch"""
    total = 0
    for b in range(B):
        o = point_rows[b][:counts[point_src[b]]]
        total += int(R._box_mask(F.windows_of(o), train_kp[b]).sum())
    return total


result = {"frames": B, "size": [w, h], "n_features": nf, "kp_capacity": kcap, "reps": reps, "device": torch.cuda.get_device_name(0),
          "map_points_per_block": [int(c) for c in counts], "occupied_rows": 0.4, "fuse": {}, "proj": {}}
for name, p in VARIANTS.items():
    st = stages(lambda: ctx.match_fuse_pairs_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_scenes, kcap, *train, B, kcap, views, p,
                                                    d_idx.data_ptr(), d_d1.data_ptr(), d_act.data_ptr(), d_point.data_ptr(), d_sum.data_ptr(),
                                                    point_src=point_src, d_train_point=d_ids.data_ptr()))
    summ = d_sum.cpu().numpy().view(binding.FUSE_SUMMARY_DTYPE).reshape(B)
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    st["counts"] = {k: int(summ[k].sum()) for k in ("n_points", "n_in_view", "n_candidates", "n_add", "n_replace", "n_duplicate")}
    st["rows_visited"] = visited(d_point.cpu().numpy().view(binding.FUSE_POINT_DTYPE).reshape(B, kcap))
    st["ns_per_visited_row"] = round(1e6 * st["fuse_search"]["median_ms"] / max(st["rows_visited"], 1), 3)
    result["fuse"][name] = st
    print(name, json.dumps(st))
for name, p in PROJ.items():
    st = stages(lambda: ctx.match_proj_pairs_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_scenes, kcap, *train, B, kcap, views, p,
                                                    d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(), d_point.data_ptr(), d_sum.data_ptr(),
                                                    point_src=point_src))
    summ = d_sum.cpu().numpy().view(binding.PROJ_SUMMARY_DTYPE).reshape(B)
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    st["counts"] = {k: int(summ[k].sum()) for k in ("n_points", "n_in_view", "n_candidates", "n_accepted", "n_unique")}
    st["ns_per_distance"] = round(1e6 * st["proj_search"]["median_ms"] / max(st["counts"]["n_candidates"], 1), 3)
    result["proj"][name] = st
    print("proj", name, json.dumps(st))
a, g = result["fuse"]["local_mapping"], result["proj"]["local_points_th3"]
print(f"fusion (local mapping) {a['total_ms']:.4f} ms per {B} frames, {a['rows_visited']} rows visited, {a['counts']['n_candidates']} distances; "
      f"projection search (th 3) {g['total_ms']:.4f} ms, {g['counts']['n_candidates']} distances")
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
