"""Per-stage HIP-event times of the pose-only optimisation, one context alone on the chip: 1, 8 and 128 frames of 2000 monocular
observations each (2048 slots, 15 % gross outliers, the synthetic scene of tests/pose_cases.py, upstream's 4 rounds of 10 steps),
ss_pose_opt_pairs_device.  Next to them ss_track's host step sst_pose_only on one host core: profiles/tools/pose_host_time.cpp, built
here with g++ -O3 and run on the same observations and start poses.  Prints the per-call median of every stage and, with an output
path, writes the rows as JSON.
usage: python profiles/tools/time_pose.py [reps] [out.json]"""
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
import pose_cases as C  # noqa: E402
import pose_ref as PR  # noqa: E402
import proj_cases as PC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
N, ROWS, FRAMES = 2000, 2048, (1, 8, 128)
frames = [C.make_frame(700 + b, N, n_out=N * 15 // 100, n_points=ROWS, n_kp=ROWS) for b in range(max(FRAMES))]
ctx = binding.OrbContext(0, n_features=500)
params = binding.pose_opt_params()
rows = []
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "pose_host_time")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "profiles", "tools", "pose_host_time.cpp"), os.path.join(ROOT, "send-slam_amd", "csrc", "ss_track.cpp")])
    for B in FRAMES:
        part = frames[:B]

        def dev(name):
            a = np.stack([np.ascontiguousarray(fr[name]) for fr in part])
            return torch.from_numpy(a.view(np.uint8).reshape(B, -1) if a.dtype.fields else a).cuda()

        d = {k: dev(k) for k in ("points", "kp", "idx")}
        d_n = torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
        d_flags = torch.empty((B, ROWS), dtype=torch.uint8, device="cuda")
        d_res = torch.empty((B, 160), dtype=torch.uint8, device="cuda")
        views = np.concatenate([np.asarray(fr["view"]).reshape(1) for fr in part])
        start = np.stack([fr["start"] for fr in part])
        torch.cuda.synchronize()

        def call():
            ctx.pose_opt_pairs_device(d["points"].data_ptr(), d_n.data_ptr(), B, ROWS, d["kp"].data_ptr(), d_n.data_ptr(), B, ROWS, d["idx"].data_ptr(), views,
                                      start, params, d_flags.data_ptr(), d_res.data_ptr())

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
                              "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("pose_")}
        res = d_res.cpu().numpy().view(binding.POSE_RESULT_DTYPE).reshape(B)
        row = {"frames": B, "observations": N, "slots": ROWS, "reps": reps, "stages": stages, "total_ms": round(sum(v["median_ms"] for v in stages.values()), 5),
               "states": sorted(set(int(v) for v in res["state"])), "mean_inliers": int(res["n_inliers"].mean()), "mean_steps": float(res["steps"].sum(axis=1).mean())}
        # the same observations and start poses for the host step
        path = os.path.join(tmp, f"frames_{B}.bin")
        with open(path, "wb") as f:
            f.write(np.array([B, N], np.int32).tobytes())
            for fr in part:
                o = PR.observations(fr["points"], fr["kp"], fr["idx"], PC.scale())
                assert len(o["X"]) == N
                f.write(np.asarray(fr["start"], np.float64).tobytes())
                f.write(np.stack([o[k] for k in ("X", "Y", "Z", "u", "v", "w")], 1).astype(np.float64).tobytes())
        row["host_one_core"] = json.loads(subprocess.check_output([exe, path, "5"], text=True))
        rows.append(row)
        print(f"{B} frames x {N}: device {row['total_ms']:.4f} ms per call ({stages}); sst_pose_only on one host core {row['host_one_core']['median_ms']:.3f} ms")
result = {"device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
