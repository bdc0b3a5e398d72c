"""Per-stage HIP-event times of the Sim3 RANSAC, one context alone on the chip: 8 loop candidates of 2000 correspondences each (2048
rows, 40 % gross outliers, the synthetic scene of tests/sim3_cases.py) and 300 hypotheses per candidate, ss_sim3_pairs_device.  Next
to them the same rule on one host core: profiles/tools/sim3_host_time.cpp, the text the kernels compile, built here with g++ -O3 and
run on a scene of the same sizes.  Prints the per-call median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_sim3.py [pairs] [reps] [out.json]"""
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
import sim3_cases as SC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else None
N, ROWS, ITER = 2000, 2048, 300
pairs = [SC.make_pair(900 + b, N, N * 2 // 5, ROWS, ROWS) for b in range(B)]


def dev(name):
    a = np.stack([np.ascontiguousarray(pr[name]) for pr in pairs])
    return torch.from_numpy(a.view(np.uint8).reshape(B, -1) if a.dtype.fields else a).cuda()


d = {k: dev(k) for k in ("q_xyz", "q_kp", "t_xyz", "t_kp", "idx")}
d_n = torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
d_inl = torch.empty((B, ROWS), dtype=torch.uint8, device="cuda")
d_res = torch.empty((B, 128), dtype=torch.uint8, device="cuda")
v1 = np.concatenate([np.asarray(pr["view1"]).reshape(1) for pr in pairs])
v2 = np.concatenate([np.asarray(pr["view2"]).reshape(1) for pr in pairs])
torch.cuda.synchronize()
ctx = binding.OrbContext(0, n_features=500)
params = binding.sim3_params(min_inliers=N // 4, max_iterations=ITER, seed=7)


def call():
    ctx.sim3_pairs_device(d["q_xyz"].data_ptr(), d["q_kp"].data_ptr(), d_n.data_ptr(), d["t_xyz"].data_ptr(), d["t_kp"].data_ptr(), d_n.data_ptr(),
                          d["idx"].data_ptr(), B, ROWS, v1, v2, params, d_inl.data_ptr(), d_res.data_ptr())


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
                      "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("sim3_")}
res = d_res.cpu().numpy().view(binding.SIM3_RESULT_DTYPE).reshape(B)
result = {"pairs": B, "correspondences": N, "rows": ROWS, "iterations": ITER, "reps": reps, "device": torch.cuda.get_device_name(0), "stages": stages,
          "total_ms": round(sum(v["median_ms"] for v in stages.values()), 5), "states": [int(v) for v in res["state"]],
          "n_inliers": [int(v) for v in res["n_inliers"]], "iteration": [int(v) for v in res["iteration"]]}
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "sim3_host_time")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "profiles", "tools", "sim3_host_time.cpp")])
    result["host_one_core"] = json.loads(subprocess.check_output([exe, str(B), str(N), str(ITER), "5"], text=True))
print(json.dumps(result))
print(f"device {result['total_ms']:.4f} ms per call of {B} x {N} x {ITER}; one host core {result['host_one_core']['median_ms']:.1f} ms")
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
