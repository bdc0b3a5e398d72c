"""Per-stage HIP-event times of the Sim3 refinement, one context alone on the chip: 1, 8 and 128 pairs of 300 correspondences each in
2048 rows (15 % gross mismatches, half a pixel of noise, the synthetic scene of tests/sim3opt_cases.py, a start a few pixels off,
upstream's 5 + 10 steps), ss_sim3_opt_pairs_device; gather and solve separately, and the mutual check of SearchBySim3's bookkeeping
(ss_sim3_mutual_pairs_device: every other match as the prior ones, the matches and their inverse as the two searches' results; not in
total_ms).  Next to them the host twin on one host core:
profiles/tools/sim3opt_host_time.cpp, built here with g++ -O3 (or the executable named by the third argument) and run on the same
correspondences and start models.  Prints the per-call median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_sim3opt.py [reps] [out.json] [sim3opt_host_time executable]"""
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
import proj_cases as PC  # noqa: E402
import sim3_ref as S  # noqa: E402
import sim3opt_cases as C  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
exe = sys.argv[3] if len(sys.argv) > 3 else None
N, ROWS, PAIRS = 300, 2048, (1, 8, 128)
pairs = [C.make_pair(800 + b, N, N * 15 // 100, ROWS, ROWS) for b in range(max(PAIRS))]
ctx = binding.OrbContext(0, n_features=500)
params = binding.sim3_opt_params()
rows = []
with tempfile.TemporaryDirectory() as tmp:
    if exe is None:
        exe = os.path.join(tmp, "sim3opt_host_time")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "send-slam_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "profiles", "tools", "sim3opt_host_time.cpp")])
    for B in PAIRS:
        part = pairs[:B]

        def dev(name):
            a = np.stack([np.ascontiguousarray(pr[name]) for pr in part])
            return torch.from_numpy(a.view(np.uint8).reshape(B, -1) if a.dtype.fields else a).cuda()

        d = {k: dev(k) for k in ("q_xyz", "q_kp", "t_xyz", "t_kp", "idx")}
        starts = np.array([np.asarray(pr["start"], S.RESULT_DTYPE).reshape(()) for pr in part], S.RESULT_DTYPE)
        d_start = torch.from_numpy(starts.view(np.uint8).reshape(B, -1)).cuda()
        d_n = torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
        d_flags = torch.empty((B, ROWS), dtype=torch.uint8, device="cuda")
        d_res = torch.empty((B, 272), dtype=torch.uint8, device="cuda")
        views1 = np.concatenate([np.asarray(pr["view1"]).reshape(1) for pr in part])
        views2 = np.concatenate([np.asarray(pr["view2"]).reshape(1) for pr in part])
        idx = np.stack([pr["idx"] for pr in part])
        prior, idx21 = idx.copy(), np.full((B, ROWS), -1, np.int32)
        prior[:, ::2] = -1
        for b in range(B):
            r = np.flatnonzero(idx[b] >= 0)
            idx21[b, idx[b][r]] = r
        d_prior, d_idx21 = torch.from_numpy(prior).cuda(), torch.from_numpy(idx21).cuda()
        d_out = torch.empty((B, ROWS), dtype=torch.int32, device="cuda")
        d_summary = torch.empty((B, 8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def call():
            ctx.sim3_mutual_pairs_device(d_prior.data_ptr(), d["idx"].data_ptr(), d_idx21.data_ptr(), d_n.data_ptr(), d_n.data_ptr(), B, ROWS, d_out.data_ptr(),
                                         d_summary.data_ptr())
            ctx.sim3_opt_pairs_device(d["q_xyz"].data_ptr(), d["q_kp"].data_ptr(), d_n.data_ptr(), d["t_xyz"].data_ptr(), d["t_kp"].data_ptr(), d_n.data_ptr(),
                                      d["idx"].data_ptr(), B, ROWS, views1, views2, d_start.data_ptr(), params, d_flags.data_ptr(), d_res.data_ptr())

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
                              "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("sim3opt_")}
        res = d_res.cpu().numpy().view(binding.SIM3_OPT_RESULT_DTYPE).reshape(B)
        row = {"pairs": B, "correspondences": N, "rows": ROWS, "reps": reps, "stages": stages, "total_ms": round(sum(v["median_ms"] for k, v in stages.items() if k != "sim3opt_mutual"), 5),
               "states": sorted(set(int(v) for v in res["state"])), "mean_inliers": int(res["n_inliers"].mean()), "mean_steps": float(res["steps"].sum(axis=1).mean())}
        # the same correspondences, views and start models for the host twin
        path = os.path.join(tmp, f"pairs_{B}.bin")
        with open(path, "wb") as f:
            f.write(np.array([B, N], np.int32).tobytes())
            for pr in part:
                c = S.correspondences(pr["view1"], pr["q_xyz"], pr["q_kp"], None, pr["view2"], pr["t_xyz"], pr["t_kp"], None, pr["idx"], PC.scale(), 1.0)
                assert len(c["rows"]) == N
                sc = np.asarray(PC.scale(), np.float32)
                rec = np.concatenate([c["x1"], c["x2"], np.stack([pr["q_kp"]["x"][c["rows"]], pr["q_kp"]["y"][c["rows"]], pr["t_kp"]["x"][c["cols"]],
                                                                  pr["t_kp"]["y"][c["cols"]], sc[pr["q_kp"]["octave"][c["rows"]]],
                                                                  sc[pr["t_kp"]["octave"][c["cols"]]]], 1)], 1).astype(np.float32)
                f.write(np.asarray(pr["start"], S.RESULT_DTYPE).tobytes())
                f.write(np.asarray(pr["view1"]).tobytes() + np.asarray(pr["view2"]).tobytes())
                f.write(rec.tobytes())
        row["host_one_core"] = json.loads(subprocess.check_output([exe, path, "5"], text=True))
        assert row["host_one_core"]["mean_inliers"] == row["mean_inliers"], "the host twin and the device disagree"
        rows.append(row)
        print(f"{B} pairs x {N}: device {row['total_ms']:.4f} ms per call ({stages}); the host twin on one host core {row['host_one_core']['median_ms']:.3f} ms")
result = {"device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
