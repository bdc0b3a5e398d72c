"""Per-stage HIP-event times of the map-point projection search, one context alone on the chip, on the batch of
time_guided.py: 64 frames of 1280x720 / 2000 features (eight scenes, eight consecutive frames each).  Each scene has one shared
map: the keypoints of its first frame back-projected at depths 2 .. 8 (tests/proj_cases.back_project), about 2000 points; frame b
searches the map of its scene under a pose a few pixels away from identity (point_src[b] = scene).  The yardstick, in the SAME
run on the same batch, is the guided call of DESIGN.md section 14 (frame b against b - 1, radius 15 * scale[octave], octave -+ 1).
Prints the per-batch median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_proj.py [frames] [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
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
kcap = ctx.batch_view().kp_capacity
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
views = np.concatenate([np.asarray(P.view_init(fx, fx, cx, cy, w, h, *PC.POSES[b % 3], bf)).reshape(1) for b in range(B)])
point_src = [(b // 8) % 8 for b in range(B)]
d_pts = torch.from_numpy(pts.view(np.uint8).reshape(n_scenes, -1)).cuda()
d_pd = torch.from_numpy(pdesc).cuda()
d_n = torch.from_numpy(counts).cuda()
d_idx = torch.empty((B, kcap), dtype=torch.int32, device="cuda")
d_d1 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_d2 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_proj = torch.empty((B, kcap * 32), dtype=torch.uint8, device="cuda")
d_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")
VARIANTS = {"local_points_th1": binding.proj_params(th=1.0, one_to_one=False),
            "local_points_th3": binding.proj_params(th=3.0, one_to_one=False),
            "local_points_th3_one_to_one": binding.proj_params(th=3.0, one_to_one=True),
            # where the search's time goes: a window factor that holds nothing but the cell walk, and one of 16 x the candidates
            "empty_windows": binding.proj_params(th=1e-4),
            "th12": binding.proj_params(th=12.0)}
GUIDED = {"projection": binding.guided_params(th=100, ratio_num=0, ratio_den=0, radius=15.0, radius_by_octave=True, octave_span=1),
          "init": binding.guided_params(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1, radius=15.0, radius_by_octave=True,
                                        octave_span=1)}


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


result = {"frames": B, "size": [w, h], "n_features": nf, "kp_capacity": kcap, "reps": reps, "device": torch.cuda.get_device_name(0),
          "map_points_per_block": [int(c) for c in counts], "proj": {}, "guided": {}}
for name, p in VARIANTS.items():
    st = stages(lambda: ctx.match_proj_batch_device(d_pts.data_ptr(), d_pd.data_ptr(), d_n.data_ptr(), n_scenes, kcap, views, p, d_idx.data_ptr(),
                                                    d_d1.data_ptr(), d_d2.data_ptr(), d_proj.data_ptr(), d_sum.data_ptr(), point_src=point_src))
    summ = d_sum.cpu().numpy().view(binding.PROJ_SUMMARY_DTYPE).reshape(B)
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    st["counts"] = {k: int(summ[k].sum()) for k in ("n_points", "n_in_view", "n_candidates", "n_accepted", "n_unique")}
    st["candidates_per_point_in_view"] = round(st["counts"]["n_candidates"] / max(st["counts"]["n_in_view"], 1), 3)
    st["ns_per_distance"] = round(1e6 * st["total_ms"] / max(st["counts"]["n_candidates"], 1), 3)
    result["proj"][name] = st
    print(name, json.dumps(st))
for name, p in GUIDED.items():
    st = stages(lambda: ctx.match_guided_batch_device(p, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(), d_sum.data_ptr()))
    summ = d_sum.cpu().numpy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(B)
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    st["counts"] = {k: int(summ[k].sum()) for k in ("n_query", "n_candidates", "n_accepted", "n_unique", "n_final")}
    st["candidates_per_query"] = round(st["counts"]["n_candidates"] / max(st["counts"]["n_query"], 1), 3)
    st["ns_per_distance"] = round(1e6 * st["total_ms"] / max(st["counts"]["n_candidates"], 1), 3)
    result["guided"][name] = st
    print("guided", name, json.dumps(st))
a, g = result["proj"]["local_points_th1"], result["guided"]["projection"]
print(f"projection search (th 1) {a['total_ms']:.4f} ms per {B} frames, {a['candidates_per_point_in_view']} candidates per point in view; "
      f"guided yardstick {g['total_ms']:.4f} ms, {g['candidates_per_query']} candidates per query")
if out_path:
    json.dump(result, open(out_path, "w"), indent=1)
