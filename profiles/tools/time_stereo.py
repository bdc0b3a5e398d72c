"""Per-stage HIP-event times of the stereo depth stages next to the extraction stages of the same batch, one context alone
on the chip: 64 parallax pairs of 1280x720 / 2000 features = one 128-frame batch; each repetition runs the extraction and then
ss_stereo_batch_device.  Prints the per-batch median of every stage and, with an output path, writes the rows as JSON.
The CPU reference's time per pair on one host core is measured in the same run, for scale.
usage: python profiles/tools/time_stereo.py [pairs] [reps] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h, nf = 1280, 720, 2000
scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = []
for i in range(P):  # pair i: scene i % 8, left = frame t, right = frame 0, t = 2 .. 9
    s, t = i % 8, 2 + i // 8
    frames += [synth.parallax_frame(2000 + s, w, h, t, sc=scenes[s]), synth.parallax_frame(2000 + s, w, h, 0, sc=scenes[s])]
frames = np.stack(frames)
d = torch.from_numpy(frames).cuda()
ctx = binding.OrbContext(0, n_features=nf, max_batch=2 * P, lapping_x0=0, lapping_x1=0)
ctx.extract_batch_device(d.data_ptr(), 2 * P, w, h)
kcap = ctx.batch_view().kp_capacity
d_pts = torch.empty((P, kcap, 16), dtype=torch.uint8, device="cuda")
d_sum = torch.empty((P, 32), dtype=torch.uint8, device="cuda")


def one():
    ctx.extract_batch_device(d.data_ptr(), 2 * P, w, h)
    ctx.stereo_batch_device(d_pts.data_ptr(), d_sum.data_ptr(), 500.0, 0.1, 35.0)


for _ in range(3):
    one()
ctx.synchronize()
ctx.profile(True)
for _ in range(reps):
    one()
    ctx.synchronize()
rows, extract_ms, stereo_ms = [], 0.0, 0.0
for s in ctx.stats():
    if not s["launches"]:
        continue
    per_batch = s["launches"] // reps
    med = s["median_ms"] * per_batch  # median launch x launches per batch (resize: one launch per level)
    rows.append({"stage": s["name"], "launches_per_batch": per_batch, "median_ms_per_batch": round(med, 5),
                 "mean_ms_per_batch": round(s["total_ms"] / reps, 5), "algorithmic_bytes": s["algorithmic_bytes"]})
    if s["name"].startswith("stereo_"):
        stereo_ms += med
    else:
        extract_ms += med
    print(f"{s['name']:18s} {med:8.4f} ms/batch median  {s['total_ms'] / reps:8.4f} mean  ({per_batch} launches)")
summ = d_sum.cpu().numpy().view(binding.STEREO_SUMMARY_DTYPE).reshape(P)
print(f"extraction {extract_ms:.4f} ms, stereo {stereo_ms:.4f} ms per {2 * P}-frame batch = {100 * stereo_ms / extract_ms:.2f} % "
      f"({1e3 * stereo_ms / P:.2f} us per pair); depth on {summ['n_depth'].sum()} of {summ['n_left'].sum()} left keypoints")

# the CPU reference, one pair on one host core (extraction excluded)
import stereo_ref as R  # noqa: E402
from oracle import orb_oracle as O  # noqa: E402
p = O.default_params(n_features=nf, lapping_x0=0, lapping_x1=0)
kL, dL, _ = O.extract(frames[0], p)
kR, dR, _ = O.extract(frames[1], p)
pL, pR, scale = O.pyramid(frames[0], p), O.pyramid(frames[1], p), R.level_scales(p, w, h)
t0 = time.perf_counter()
pts, s0 = R.compute(kL, dL, pL, kR, dR, pR, scale, 500.0, 0.1, 35.0)
cpu_ms = 1e3 * (time.perf_counter() - t0)
same = pts.tobytes() == d_pts[0].cpu().numpy().view(binding.STEREO_POINT_DTYPE).reshape(kcap)[:len(pts)].tobytes()
print(f"CPU reference (numpy, one core): {cpu_ms:.1f} ms for pair 0; device points of pair 0 equal: {same}")
if out_path:
    json.dump({"pairs": P, "frames": 2 * P, "size": [w, h], "n_features": nf, "reps": reps, "stages": rows,
               "extraction_ms_per_batch": round(extract_ms, 5), "stereo_ms_per_batch": round(stereo_ms, 5),
               "stereo_percent_of_extraction": round(100 * stereo_ms / extract_ms, 3), "cpu_reference_ms_per_pair": round(cpu_ms, 2),
               "pair0_equals_reference": bool(same), "device": torch.cuda.get_device_name(0)}, open(out_path, "w"), indent=1)
