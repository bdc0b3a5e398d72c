"""Times of Frame's keypoint post-processing at the benchmark's own shape, one context alone on the chip: 128 frames of 1280 x 720,
2000 features.  Per repetition one extraction, the out-of-place undistortion, the in-place undistortion and the depth lookup (uint16
frames), each stage by HIP events from ss_stats after warm-up calls; next to them the extraction's stages of the same batch in the
same run, and the byte floor of each new stage: the bytes it moves, computed from the shape and the counts, over the HBM peak.
usage: python profiles/tools/time_undistort.py [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
B, W, H, NF = 128, 1280, 720, 2000
HBM_PEAK = 8.0e12       # bytes/s, the datasheet's; 6.29e12 was measured with a float4 copy
HBM_MEASURED = 6.29e12
EXTRACT = ("ingest", "resize", "fast_blur_nms", "bucket_gather", "cells_emit", "quadtree", "slots", "orient_describe")
NEW = ("undistort", "undistort_in_place", "depth_lookup")

cam = binding.Camera(type=b"PinHole", fx=1040.0, fy=1030.0, cx=636.0, cy=363.0, k1=-0.28, k2=0.07, p1=1e-3, p2=-5e-4, width=W, height=H, fps=30.0,
                     th_depth=40.0, baseline=0.1, depth_map_factor=5000.0)
distinct = [synth.frame(0, W, H, t) for t in range(8)]
frames = np.stack([distinct[t % 8] for t in range(B)])
d_frames = torch.from_numpy(frames).cuda()
rng = np.random.default_rng(7)
d_depth = torch.from_numpy(rng.integers(0, 40000, (B, H, W)).astype(np.uint16).view(np.int16)).cuda()
ctx = binding.OrbContext(0, n_features=NF, max_batch=B)
ctx.set_calibration(1, cam)
ctx.extract_batch_device(d_frames.data_ptr(), B, W, H)
ctx.synchronize()
kcap = ctx.batch_view().kp_capacity
raw = [ctx.fetch_frame(b)[0] for b in range(B)]  # before any undistortion
counts = [len(k) for k in raw]
d_out = torch.empty((B, kcap * 24), dtype=torch.uint8, device="cuda")
d_right, d_dep = torch.empty((B, kcap), dtype=torch.float32, device="cuda"), torch.empty((B, kcap), dtype=torch.float32, device="cuda")
d_sum = torch.empty((B, 16), dtype=torch.uint8, device="cuda")
params = binding.depth_params_from_camera(cam, 1)
torch.cuda.synchronize()


def one():
    ctx.extract_batch_device(d_frames.data_ptr(), B, W, H)
    ctx.undistort_batch_device(cam, d_out.data_ptr())
    ctx.undistort_batch_device()
    ctx.depth_batch_device(params, d_depth.data_ptr(), W, H, W * 2, W * H * 2, d_right.data_ptr(), d_dep.data_ptr(), d_sum.data_ptr())
    ctx.synchronize()


for _ in range(3):
    one()
ctx.profile_reset()
ctx.profile(True)
for _ in range(reps):
    one()
ctx.profile(False)
stats = {s["name"]: s for s in ctx.stats() if s["launches"]}
# the device's results once more against the host twin, so that the figures are those of a correct run
un = binding.undistort_host(cam, raw[5])
got = d_out[5].cpu().numpy().view(binding.KP_DTYPE)[:counts[5]]
assert got.tobytes() == un.tobytes() and ctx.fetch_frame(5)[0].tobytes() == un.tobytes(), "the device and the host twin differ"

rows = int(np.sum(counts))
# the bytes a stage must move: live rows only; the frames' counts, errors, cameras and summaries are a few KB
floor_bytes = {"undistort": rows * (24 + 24), "undistort_in_place": rows * (8 + 8 + 8), "depth_lookup": rows * (8 + 4 + 2) + B * kcap * 8}
out = {"device": torch.cuda.get_device_name(0), "shape": {"frames": B, "width": W, "height": H, "n_features": NF, "kp_capacity": kcap, "keypoints": rows},
       "reps": reps, "warmup": 3,
       "note": "median_ms and mean_ms: HIP events around each stage's launches, per launch (the depth lookup is two launches under one pair of events); "
               "floor_us: bytes the stage must move (live rows; the depth planes over every row) over the HBM peak of 8.0 TB/s (datasheet) and over "
               "the 6.29 TB/s a float4 copy reaches; the extraction's stages are those of the same batch in the same run (resize: per launch, 7 a batch)",
       "stages": {}, "extraction": {}}
for name in NEW:
    s = stats[name]
    out["stages"][name] = {"median_ms": round(s["median_ms"], 5), "mean_ms": round(s["mean_ms"], 5), "launches": s["launches"], "floor_bytes": floor_bytes[name],
                           "counted_bytes": s["algorithmic_bytes"], "floor_us_at_8.0TBs": round(floor_bytes[name] / HBM_PEAK * 1e6, 3),
                           "floor_us_at_6.29TBs": round(floor_bytes[name] / HBM_MEASURED * 1e6, 3)}
total = 0.0
for name in EXTRACT:
    if name in stats:
        s = stats[name]
        per_batch = s["total_ms"] / reps
        total += per_batch
        out["extraction"][name] = {"median_ms": round(s["median_ms"], 5), "per_batch_ms": round(per_batch, 5), "launches": s["launches"]}
out["extraction_per_batch_ms"] = round(total, 4)
print(json.dumps(out))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
