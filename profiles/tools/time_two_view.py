"""Per-stage HIP-event times of the two-view initialisation, one context alone on the chip: 8 problems of 2000 correspondences each
(2048 rows, 30 % gross outliers, 0.5 px noise, the synthetic scene of tests/two_view_cases.py), 200 hypotheses per problem,
ss_two_view_pairs_device.  Next to them two yardsticks on one host of the same box: the same rule on one core
(profiles/tools/two_view_host_time.cpp, the text the kernels compile, built here with g++ -O3) and sst_two_view, the bounded tracker's
own threaded form, on the same correspondences (written to a file for it).  Prints the per-call median of every stage and, with an output path, writes the rows
as JSON.
usage: python profiles/tools/time_two_view.py [problems] [reps] [out.json]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import two_view_cases as TC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
N, ROWS, ITER = 2000, 2048, 200
scenes = [TC.make_scene(900 + b, N, N * 3 // 10, ROWS, ROWS, noise=0.5, motion=TC.FORWARD) for b in range(B)]


def dev(name):
    a = np.stack([np.ascontiguousarray(sc[name]) for sc in scenes])
    return torch.from_numpy(a.view(np.uint8).reshape(B, -1) if a.dtype.fields else a).cuda()


d = {k: dev(k) for k in ("kp1", "kp2", "idx")}
d_n = torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
empty = lambda width: torch.empty((B, width), dtype=torch.uint8, device="cuda")  # noqa: E731
d_flag, d_pts, d_rows, d_np, d_res = empty(ROWS), empty(ROWS * 32), empty(ROWS * 8), empty(4), empty(192)
views = np.concatenate([np.asarray(sc["view"]).reshape(1) for sc in scenes])
torch.cuda.synchronize()
ctx = binding.OrbContext(0, n_features=500)
params = binding.two_view_params(max_iterations=ITER, seed=7)


def call():
    ctx.two_view_pairs_device(d["kp1"].data_ptr(), d_n.data_ptr(), B, d["kp2"].data_ptr(), d_n.data_ptr(), B, ROWS, d["idx"].data_ptr(), B, views, params,
                              d_flag.data_ptr(), d_pts.data_ptr(), d_rows.data_ptr(), d_np.data_ptr(), d_res.data_ptr())


for _ in range(3):
    call()
ctx.synchronize()
ctx.profile_reset()
ctx.profile(True)
for _ in range(reps):
    call()
    ctx.synchronize()
ctx.profile(False)
stages = {s["name"]: {"median_ms": round(s["median_ms"], 5), "mean_ms": round(s["total_ms"] / reps, 5), "launches_per_call": s["launches"] // reps,
                      "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("tv_")}
res = d_res.cpu().numpy().view(binding.TWO_VIEW_RESULT_DTYPE).reshape(B)
result = {"problems": B, "correspondences": N, "rows": ROWS, "iterations": ITER, "reps": reps, "device": torch.cuda.get_device_name(0), "stages": stages,
          "total_ms": round(sum(v["median_ms"] for v in stages.values()), 5), "states": [int(v) for v in res["state"]],
          "reasons": [int(v) for v in res["reason"]], "models": [int(v) for v in res["model"]], "n_inliers": [int(v) for v in res["n_inliers"]],
          "n_triangulated": [int(v) for v in res["n_triangulated"]]}
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "two_view_host_time")
    csrc = os.path.join(ROOT, "send-slam_amd", "csrc")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + csrc, "-o", exe,
                           os.path.join(ROOT, "profiles", "tools", "two_view_host_time.cpp"), os.path.join(csrc, "ss_track.cpp")])
    scene = os.path.join(tmp, "scene.bin")  # the correspondences the device was timed on, in the numbering of step 1
    with open(scene, "wb") as f:
        f.write(np.array([B, N], np.int32).tobytes())
        for sc in scenes:
            rows = sc["rows"]
            j = sc["idx"][rows]
            f.write(np.stack([sc["kp1"]["x"][rows], sc["kp1"]["y"][rows], sc["kp2"]["x"][j], sc["kp2"]["y"][j]], axis=1).astype(np.float32).tobytes())
    result["host"] = json.loads(subprocess.check_output([exe, str(B), str(N), str(ITER), "5", scene], text=True))
print(json.dumps(result))
print(f"device {result['total_ms']:.4f} ms per call of {B} x {N} x {ITER}; one host core {result['host']['median_ms']:.1f} ms; "
      f"sst_two_view {result['host']['sst_two_view_median_ms']:.1f} ms")
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
