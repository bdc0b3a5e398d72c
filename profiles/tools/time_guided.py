"""Per-stage HIP-event times of the guided matching stages, one context alone on the chip: 64 frames of 1280x720 / 2000
features (eight scenes, eight consecutive frames each), frame b against b - 1, radius 15 * scale[octave], octave -+ 1.  Measured
in the SAME run, on the same batch, as two yardsticks: ss_match_batch_device mode 1 (all-pairs, the matrix-core matcher) and the
stereo_search stage (the brute-force walk of the same kind of problem: every left row tests every right row's band).
Prints the per-batch median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_guided.py [frames] [reps] [out.json]"""
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
scenes = [synth.scene(2000 + i, w, h) for i in range(8)]
frames = np.stack([synth.frame_from_scene(scenes[(b // 8) % 8], 2000 + (b // 8) % 8, w, h, b % 8) for b in range(B)])
d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
ctx = binding.OrbContext(0, n_features=nf, max_batch=B)
ctx.extract_batch_device(d.data_ptr(), B, w, h)
kcap = ctx.batch_view().kp_capacity
d_idx = torch.empty((B, kcap), dtype=torch.int32, device="cuda")
d_d1 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_d2 = torch.empty((B, kcap), dtype=torch.int16, device="cuda")
d_sum = torch.empty((B, 32), dtype=torch.uint8, device="cuda")
d_pts = torch.empty((B // 2, kcap, 16), dtype=torch.uint8, device="cuda")
d_ssum = torch.empty((B // 2, 32), dtype=torch.uint8, device="cuda")
VARIANTS = {"init": binding.guided_params(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=1, radius=15.0,
                                          radius_by_octave=True, octave_span=1),
            "projection": binding.guided_params(th=100, ratio_num=0, ratio_den=0, radius=15.0, radius_by_octave=True, octave_span=1),
            # where the search's time goes: windows that hold nothing (radius 1e-3: cell walk and record tests, no descriptor),
            # and 4 x the radius (16 x the candidates)
            "empty_windows": binding.guided_params(th=50, ratio_num=9, ratio_den=10, radius=1e-3, octave_span=1),
            "radius_x4": binding.guided_params(th=50, ratio_num=9, ratio_den=10, radius=60.0, radius_by_octave=True, octave_span=1)}


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


result = {"frames": B, "size": [w, h], "n_features": nf, "kp_capacity": kcap, "reps": reps, "device": torch.cuda.get_device_name(0), "guided": {}}
for name, p in VARIANTS.items():
    st = stages(lambda: ctx.match_guided_batch_device(p, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr(), d_sum.data_ptr()))
    summ = d_sum.cpu().numpy().view(binding.GUIDED_SUMMARY_DTYPE).reshape(B)
    st["total_ms"] = round(sum(v["median_ms"] for v in st.values()), 5)
    st["counts"] = {k: int(summ[k].sum()) for k in ("n_query", "n_candidates", "n_accepted", "n_unique", "n_final")}
    result["guided"][name] = st
    print(name, json.dumps(st))
result["match_batch_mode1"] = stages(lambda: ctx.match_batch_device(1, d_idx.data_ptr(), d_d1.data_ptr(), d_d2.data_ptr()))
print("match_batch_device mode 1", json.dumps(result["match_batch_mode1"]))
all_pairs = int((d_idx.cpu().numpy() >= 0).sum())
result["match_batch_mode1"]["n_accepted"] = all_pairs
st = stages(lambda: ctx.stereo_batch_device(d_pts.data_ptr(), d_ssum.data_ptr(), 500.0, 0.1, 35.0))
result["stereo_batch"] = st
print("stereo stages (frames 2p / 2p + 1 as pairs)", json.dumps(st))
g = result["guided"]["init"]
print(f"guided index + search + finish {g['total_ms']:.4f} ms per {B} frames; all-pairs match {result['match_batch_mode1']['match']['median_ms']:.4f} ms; "
      f"stereo_search {st['stereo_search']['median_ms']:.4f} ms per {B // 2} pairs")
if out_path:
    json.dump(result, open(out_path, "w"), indent=1)
