"""Per-stage HIP-event times of the local bundle adjustment, one context alone on the chip: 1, 4 and 16 problems of 8 free + 8 fixed
and of 32 free + 32 fixed keyframes with 2000 and 16384 points (the synthetic scene of tests/ba_cases.py, 5 % of the observations of
points three keyframes see gross outliers, the default schedule of 5 + 10 iterations), ss_local_ba_pairs_device.  The problems of a
call are copies of one problem over one block of points.  Next to them the host twin ss_local_ba_host on one host core, one problem,
and the same call with every match removed: its problems end in the gather, so the whole fixed schedule is empty launches.  Prints the
per-call median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_ba.py [reps] [out.json] [quick]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import ba_cases as BC  # noqa: E402
import proj_cases as PC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
quick = len(sys.argv) > 3
SHAPES = [(16, 8, 2000), (64, 32, 2000), (16, 8, 16384), (64, 32, 16384)]
PROBLEMS = (1, 4) if quick else (1, 4, 16)
ctx = binding.OrbContext(0, n_features=500)
params = binding.ba_params()
KERNELS_PER_TIMER = {"ba_gather": 3, "ba_finish": 2}  # the timers around more than one kernel
rows = []
for n_kf, n_free, n_points in SHAPES:
    pr = BC.make_problem(seed=900 + n_kf, n_kf=n_kf, n_free=n_free, n_points=n_points, p_obs=6.0 / n_kf, n_out=n_points // 20, rows=min(n_points, 8192))
    r = pr["kp"].shape[1]
    t0 = time.perf_counter()
    host = binding.local_ba_host(pr["views"], pr["start"], n_free, PC.scale(), pr["points"], pr["kp"], pr["idx"], params, pr["n_kp"])
    host_ms = (time.perf_counter() - t0) * 1e3
    for B in PROBLEMS:
        def dev(a, times):
            a = np.ascontiguousarray(np.concatenate([a] * times))
            return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).cuda()

        d_pts, d_np = dev(pr["points"][None], 1), torch.full((1,), n_points, dtype=torch.int32, device="cuda")
        d_kp, d_nk, d_idx = dev(pr["kp"], B), dev(pr["n_kp"], B), dev(pr["idx"], B)
        d_none = torch.full((B * n_kf, n_points), -1, dtype=torch.int32, device="cuda")
        table = np.array([(q * n_kf, n_kf, n_free, 0) for q in range(B)], binding.BA_PROBLEM_DTYPE)
        views, start = np.concatenate([pr["views"]] * B), np.concatenate([pr["start"]] * B)
        nf = B * n_kf
        out = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((nf, 96), (B, n_points * 24), (B, n_points), (nf, n_points), (B, 88))]
        torch.cuda.synchronize()

        def call(d_matches):
            ctx.local_ba_pairs_device(d_pts.data_ptr(), d_np.data_ptr(), 1, n_points, d_kp.data_ptr(), d_nk.data_ptr(), nf, r, d_matches.data_ptr(), table, views, start,
                                      params, *(t.data_ptr() for t in out))

        def timed(d_matches):
            for _ in range(2):
                call(d_matches)
            ctx.synchronize()
            wall = []
            for _ in range(reps):  # unprofiled: one call from enqueue to synchronize
                t0 = time.perf_counter()
                call(d_matches)
                ctx.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.profile_reset()
            ctx.profile(True)
            for _ in range(reps):
                call(d_matches)
                ctx.synchronize()
            ctx.profile(False)
            stages = {s["name"]: {"median_ms": round(s["median_ms"], 5), "total_ms_per_call": round(s["total_ms"] / reps, 5), "launches_per_call": s["launches"] // reps,
                                  "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("ba_")}
            return stages, float(np.median(wall))

        stages, wall = timed(d_idx)
        res = out[4].cpu().numpy().view(binding.BA_RESULT_DTYPE).reshape(B)
        assert res[0].tobytes() == host[4].tobytes(), "the device and the host twin differ"
        empty, empty_wall = timed(d_none)
        steps = int(res[0]["steps"].sum())
        row = {"problems": B, "n_kf": n_kf, "n_free": n_free, "points": n_points, "observations": int(res[0]["n_obs"]), "reps": reps, "stages": stages,
               "events_ms_per_call": round(sum(v["total_ms_per_call"] for v in stages.values()), 4), "wall_ms_per_call": round(wall, 4),
               "kernel_launches_per_call": sum(v["launches_per_call"] * KERNELS_PER_TIMER.get(k, 1) for k, v in stages.items()), "steps_taken_of_15": steps, "state": int(res[0]["state"]),
               "empty_schedule": {"events_ms_per_call": round(sum(v["total_ms_per_call"] for v in empty.values()), 4), "wall_ms_per_call": round(empty_wall, 4)},
               "host_twin_one_core_ms_per_problem": round(host_ms, 2)}
        rows.append(row)
        print(f"{B} x ({n_free} + {n_kf - n_free} keyframes, {n_points} points, {row['observations']} observations): events {row['events_ms_per_call']} ms, wall "
              f"{row['wall_ms_per_call']} ms per call; empty schedule {row['empty_schedule']}; host twin {host_ms:.1f} ms per problem", flush=True)
        print("   ", {k: v["total_ms_per_call"] for k, v in stages.items()}, flush=True)
        del d_kp, d_idx, d_none, out
        torch.cuda.empty_cache()
result = {"device": torch.cuda.get_device_name(0), "note": "stages: HIP events around every launch with profiling on; wall_ms_per_call: the median of one unprofiled "
          "call from enqueue to synchronize", "rows": rows}
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
