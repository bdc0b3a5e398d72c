"""Per-stage HIP-event times of the essential-graph optimisation, one context alone on the chip: 1, 4 and 16 problems of 100, 1000 and
4000 keyframes at about five edges a keyframe (a ring with chords of five lengths, tests/graph_cases.py's drifted start scaled so that
the far end of the ring is as far off as in the shared cases), the default schedule of 20 steps, ss_pose_graph_device.  The problems
of a call are copies of one problem.  Next to them the PCG iterations every step took (the totals of calls of 1, 2, ... steps), the
host twin ss_pose_graph_host on one host core, one problem, and the same call with every keyframe fixed: its problems end in the
gather, so the whole fixed schedule is empty launches.  Prints the per-call median of every stage and, with an output path, writes the
rows as JSON.
usage: python profiles/tools/time_graph.py [reps] [out.json] [quick]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import graph_cases as GC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
quick = len(sys.argv) > 3
SIZES = (100, 1000) if quick else (100, 1000, 4000)
PROBLEMS = (1, 4) if quick else (1, 4, 16)
ctx = binding.OrbContext(0, n_features=500)
KERNELS_PER_TIMER = {"graph_gather": 3}  # the timers around more than one kernel
rows = []


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).cuda()


for n_kf in SIZES:
    chords = [(v, (v + d) % n_kf) for d in (3, 7, 31, n_kf // 3, n_kf // 2) for v in range(0, n_kf, 1 if d < 32 else 2)]
    pr = GC.make_problem(900 + n_kf, n_kf, GC.ring(n_kf, chords), drift=0.02 / np.sqrt(n_kf / 40.0), scale_drift=0.01 / np.sqrt(n_kf / 40.0))
    n_e = len(pr["edges"])
    params = binding.graph_params()
    t0 = time.perf_counter()
    host = binding.pose_graph_host(pr["nc"], pr["start"], pr["fixed"], pr["edges"], params)
    host_ms = (time.perf_counter() - t0) * 1e3
    for B in PROBLEMS:
        nc, start, fixed, edges, table, _ = GC.stack([pr] * B)
        table = np.array(table, binding.GRAPH_PROBLEM_DTYPE)
        d_nc, d_start, d_fixed, d_all_fixed = dev(nc), dev(start), dev(fixed), dev(np.ones_like(fixed))
        K = len(nc)
        out = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((K, 104), (K, 96), (B, 48))]
        torch.cuda.synchronize()

        def call(d_fx, p=params):
            ctx.pose_graph_device(d_nc.data_ptr(), d_start.data_ptr(), d_fx.data_ptr(), K, table, edges, p, *(t.data_ptr() for t in out))

        def timed(d_fx):
            for _ in range(2):
                call(d_fx)
            ctx.synchronize()
            wall = []
            for _ in range(reps):  # unprofiled: one call from enqueue to synchronize
                t0 = time.perf_counter()
                call(d_fx)
                ctx.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.profile_reset()
            ctx.profile(True)
            for _ in range(reps):
                call(d_fx)
                ctx.synchronize()
            ctx.profile(False)
            stages = {s["name"]: {"median_ms": round(s["median_ms"], 5), "total_ms_per_call": round(s["total_ms"] / reps, 5), "launches_per_call": s["launches"] // reps,
                                  "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("graph_")}
            return stages, float(np.median(wall))

        stages, wall = timed(d_fixed)
        res = out[2].cpu().numpy().view(binding.GRAPH_RESULT_DTYPE).reshape(B)
        assert res[0].tobytes() == host[2].tobytes() and res[B - 1].tobytes() == host[2].tobytes(), "the device and the host twin differ"
        empty, empty_wall = timed(d_all_fixed)
        row = {"problems": B, "n_kf": n_kf, "n_edges": n_e, "reps": reps, "stages": stages,
               "events_ms_per_call": round(sum(v["total_ms_per_call"] for v in stages.values()), 4), "wall_ms_per_call": round(wall, 4),
               "kernel_launches_per_call": sum(v["launches_per_call"] * KERNELS_PER_TIMER.get(k, 1) for k, v in stages.items()),
               "steps": int(res[0]["steps"]), "accepted": int(res[0]["accepted"]), "pcg_iterations": int(res[0]["pcg_iterations"]), "state": int(res[0]["state"]),
               "cost_before": float(res[0]["cost_before"]), "cost_after": float(res[0]["cost_after"]),
               "empty_schedule": {"events_ms_per_call": round(sum(v["total_ms_per_call"] for v in empty.values()), 4), "wall_ms_per_call": round(empty_wall, 4)},
               "host_twin_one_core_ms_per_problem": round(host_ms, 2)}
        if B == 1:  # the iterations of step k: the total of a call of k steps less that of k - 1
            totals = [0]
            for k in range(1, params.iterations + 1):
                call(d_fixed, binding.graph_params(iterations=k))
                ctx.synchronize()
                totals.append(int(out[2].cpu().numpy().view(binding.GRAPH_RESULT_DTYPE)[0]["pcg_iterations"]))
            row["pcg_iterations_per_step"] = np.diff(totals).tolist()
        rows.append(row)
        print(f"{B} x ({n_kf} keyframes, {n_e} edges): events {row['events_ms_per_call']} ms, wall {row['wall_ms_per_call']} ms per call; {row['pcg_iterations']} PCG "
              f"iterations, cost {row['cost_before']:.3g} -> {row['cost_after']:.3g}; empty schedule {row['empty_schedule']}; host twin {host_ms:.1f} ms per problem", flush=True)
        print("   ", {k: v["total_ms_per_call"] for k, v in stages.items()}, row.get("pcg_iterations_per_step", ""), flush=True)
        del d_nc, d_start, d_fixed, d_all_fixed, out
        torch.cuda.empty_cache()
result = {"device": torch.cuda.get_device_name(0), "note": "stages: HIP events around every launch with profiling on; wall_ms_per_call: the median of one unprofiled "
          "call from enqueue to synchronize", "rows": rows}
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
