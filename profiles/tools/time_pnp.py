"""Per-stage HIP-event times of the PnP RANSAC, one context alone on the chip: 8 relocalisation candidates of 2000 correspondences
each (2048 rows, 40 % gross outliers, 0.5 px noise, the synthetic scene of tests/pnp_cases.py), 300 hypotheses per candidate and
refine_steps 5, ss_pnp_pairs_device.  Next to them the same rule on one host core: profiles/tools/pnp_host_time.cpp, the text the
kernels compile, built here with g++ -O3 and run on a scene of the same sizes.  Prints the per-call median of every stage and, with
an output path, writes the rows as JSON.
usage: python profiles/tools/time_pnp.py [candidates] [reps] [out.json] [refine_steps]"""
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
import pnp_cases as NC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
N, ROWS, ITER = 2000, 2048, 300
REFINE = int(sys.argv[4]) if len(sys.argv) > 4 else 5
scenes = [NC.make_scene(900 + b, N, N * 2 // 5, ROWS, ROWS, noise=0.5) for b in range(B)]


def dev(name):
    a = np.stack([np.ascontiguousarray(sc[name]) for sc in scenes])
    return torch.from_numpy(a.view(np.uint8).reshape(B, -1) if a.dtype.fields else a).cuda()


d = {k: dev(k) for k in ("points", "kp", "idx")}
d_n = torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
d_inl = torch.empty((B, ROWS), dtype=torch.uint8, device="cuda")
d_res = torch.empty((B, 128), dtype=torch.uint8, device="cuda")
views = np.concatenate([np.asarray(sc["view"]).reshape(1) for sc in scenes])
torch.cuda.synchronize()
ctx = binding.OrbContext(0, n_features=500)
params = binding.pnp_params(max_iterations=ITER, refine_steps=REFINE, seed=7)


def call():
    ctx.pnp_pairs_device(d["points"].data_ptr(), d_n.data_ptr(), B, ROWS, d["kp"].data_ptr(), d_n.data_ptr(), B, ROWS, d["idx"].data_ptr(), B, views, params,
                         d_inl.data_ptr(), d_res.data_ptr())


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
                      "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("pnp_")}
res = d_res.cpu().numpy().view(binding.PNP_RESULT_DTYPE).reshape(B)
result = {"candidates": B, "correspondences": N, "rows": ROWS, "iterations": ITER, "refine_steps": REFINE, "reps": reps,
          "device": torch.cuda.get_device_name(0), "stages": stages, "total_ms": round(sum(v["median_ms"] for v in stages.values()), 5),
          "states": [int(v) for v in res["state"]], "n_inliers": [int(v) for v in res["n_inliers"]], "iteration": [int(v) for v in res["iteration"]]}
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "pnp_host_time")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "profiles", "tools", "pnp_host_time.cpp")])
    result["host_one_core"] = json.loads(subprocess.check_output([exe, str(B), str(N), str(ITER), str(REFINE), "5"], text=True))
print(json.dumps(result))
print(f"device {result['total_ms']:.4f} ms per call of {B} x {N} x {ITER}; one host core {result['host_one_core']['median_ms']:.1f} ms")
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
