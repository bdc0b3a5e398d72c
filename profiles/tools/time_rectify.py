"""Per-stage HIP-event times of the rectification stage next to the extraction stages of the same batch, one context alone on
the chip: 64 raw pairs of 1280x720 gray = one 128-frame batch on two maps (model A's coefficients at that size, one map per
eye); each repetition remaps the batch and extracts the rectified frames in place.  Prints the per-batch median of every stage,
the stage's algorithmic GB/s next to that of `resize` (the yardstick: it moves a comparable number of image bytes) and its share
of the extraction sum; then times the same batch as 128 one-frame calls, the form that re-reads the map for every frame.  With
an output path, writes the rows as JSON.
usage: python profiles/tools/time_rectify.py [pairs] [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import rectify_ref as R  # noqa: E402
from oracle import orb_oracle as O  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h, nf = 1280, 720, 2000
scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = []
for i in range(P):  # pair i: scene i % 8, left = frame t, right = frame 0, t = 2 .. 9 (the batch of time_stereo.py, taken as raw)
    s, t = i % 8, 2 + i // 8
    frames += [synth.parallax_frame(2000 + s, w, h, t, sc=scenes[s]), synth.parallax_frame(2000 + s, w, h, 0, sc=scenes[s])]
frames = np.stack(frames)
n = 2 * P
left = R.scaled(R.model_a(), w, h, focal=4.0)
right = dict(left, R=R.rot_y(-0.02))
ids = [0, 1] * P
d_raw = torch.from_numpy(frames).cuda()
d_rect = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
ctx = binding.OrbContext(0, n_features=nf, max_batch=n, lapping_x0=0, lapping_x1=0)
for i, m in enumerate((left, right)):
    ctx.set_rectify_model(i, binding.rectify_model(**m))


def batch():
    ctx.rectify_batch_device(d_raw.data_ptr(), n, w, h, ids, d_rect.data_ptr())
    ctx.extract_batch_device(d_rect.data_ptr(), n, w, h)


def per_frame():
    for f in range(n):
        ctx.rectify_batch_device(d_raw.data_ptr() + f * w * h, 1, w, h, ids[f:f + 1], d_rect.data_ptr() + f * w * h)


def measure(fn):
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
        ctx.synchronize()
    ctx.profile(False)
    rows = []
    for s in ctx.stats():
        if not s["launches"]:
            continue
        per_batch = s["launches"] // reps
        med = s["median_ms"] * per_batch  # median launch x launches per batch (resize: one launch per level)
        rows.append({"stage": s["name"], "launches_per_batch": per_batch, "median_ms_per_batch": round(med, 5),
                     "mean_ms_per_batch": round(s["total_ms"] / reps, 5), "algorithmic_bytes": s["algorithmic_bytes"]})
    return rows


rows = measure(batch)
ok = all(np.array_equal(d_rect[f].cpu().numpy(), R.remap(frames[f], *R.build_map((left, right)[f % 2]))) for f in (0, 1, n - 1))
by = {r["stage"]: r for r in rows}
extract_ms = sum(r["median_ms_per_batch"] for r in rows if r["stage"] != "rectify")
rect = by["rectify"]
for r in rows:
    print(f"{r['stage']:18s} {r['median_ms_per_batch']:8.4f} ms/batch median  {r['mean_ms_per_batch']:8.4f} mean  ({r['launches_per_batch']} launches)")
# resize: its stage record keeps the bytes of the last launch only; the whole pyramid reads every level but the last and writes
# every level but the first
g = O.geometry(O.default_params(n_features=nf, lapping_x0=0, lapping_x1=0), w, h)
lv = [(g.w[l], g.h[l]) for l in range(g.n_levels)]
resize_bytes = n * sum(a[0] * a[1] + b[0] * b[1] for a, b in zip(lv[:-1], lv[1:]))
gbs = rect["algorithmic_bytes"] / rect["median_ms_per_batch"] / 1e6
resize_gbs = resize_bytes / by["resize"]["median_ms_per_batch"] / 1e6
print(f"rectify {rect['median_ms_per_batch']:.4f} ms per {n}-frame batch = {gbs:.0f} GB/s algorithmic "
      f"({rect['algorithmic_bytes']} B), {100 * rect['median_ms_per_batch'] / extract_ms:.2f} % of the extraction sum {extract_ms:.4f} ms; "
      f"resize {by['resize']['median_ms_per_batch']:.4f} ms = {resize_gbs:.0f} GB/s ({resize_bytes} B); "
      f"frames 0, 1, {n - 1} equal the reference: {ok}")

pf = [r for r in measure(per_frame) if r["stage"] == "rectify"][0]
pf_bytes = n * (w * h * 2 + w * h * 6)
pf_gbs = pf_bytes / pf["median_ms_per_batch"] / 1e6
print(f"one frame per call ({n} launches, the map re-read for every frame): {pf['median_ms_per_batch']:.4f} ms per batch, "
      f"{pf_gbs:.0f} GB/s over the {pf_bytes} B it moves")
if out_path:
    json.dump({"pairs": P, "frames": n, "size": [w, h], "channels": 1, "maps": 2, "n_features": nf, "reps": reps, "stages": rows,
               "extraction_ms_per_batch": round(extract_ms, 5), "rectify_ms_per_batch": rect["median_ms_per_batch"],
               "rectify_algorithmic_bytes": rect["algorithmic_bytes"], "rectify_algorithmic_gb_per_s": round(gbs, 1),
               "rectify_percent_of_extraction": round(100 * rect["median_ms_per_batch"] / extract_ms, 3),
               "resize_ms_per_batch": by["resize"]["median_ms_per_batch"], "resize_algorithmic_bytes": resize_bytes,
               "resize_algorithmic_gb_per_s": round(resize_gbs, 1), "fast_blur_nms_ms_per_batch": by["fast_blur_nms"]["median_ms_per_batch"],
               "one_frame_per_call": {"launches_per_batch": pf["launches_per_batch"], "median_ms_per_batch": pf["median_ms_per_batch"],
                                      "bytes_moved": pf_bytes, "gb_per_s": round(pf_gbs, 1)},
               "frames_equal_reference": bool(ok), "device": torch.cuda.get_device_name(0)}, open(out_path, "w"), indent=1)
