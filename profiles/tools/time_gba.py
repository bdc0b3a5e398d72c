"""Per-stage HIP-event times of the global bundle adjustment, one context alone on the chip: one problem of 100 .. 16 384 keyframes on
a straight track, every point seen by the four or five keyframes nearest to it (exact float32 keypoints, starts a few centimetres and
a fraction of a degree off, the first two keyframes fixed), the default schedule (one robust round of ten, pcg_tol 1e-2, 64 PCG
iterations at the most), ss_global_ba_device.  Next to them the total PCG iterations, the host twin ss_global_ba_host on one host
core (up to 4000 keyframes), and the same call with every keyframe fixed: its problem ends in the gather, so the whole fixed schedule is empty launches.
Last, a problem inside the local bundle adjustment's limits (64 keyframes, 32 free) through ss_local_ba and ss_global_ba, both
host-pointer forms under one schedule.  Prints the per-call median of every stage and, with an output path, writes the rows as JSON.
usage: python profiles/tools/time_gba.py [reps] [out.json] [quick]"""
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
import camera_cases as CC  # noqa: E402
import gba_cases as GC  # noqa: E402
import gba_ref as GR  # noqa: E402
import pose_cases as PO  # noqa: E402
import proj_cases as PC  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else None
quick = len(sys.argv) > 3
SIZES = ((100, 5000), (1000, 50000)) if quick else ((100, 5000), (1000, 50000), (4000, 250000), (16384, 800000))
HOST_TWIN_UP_TO = 1000 if quick else 4000  # the largest problem takes minutes on one core
ROWS = 16384
ctx = binding.OrbContext(0, n_features=500)
KERNELS_PER_TIMER = {"gba_gather": 3, "gba_blocks": 2, "gba_pcg": 3, "gba_update": 2, "gba_cost": 2, "gba_finish": 4}
rows = []


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.fields else a).cuda()


def track(seed, n_kf, n_points):
    """keyframe k stands at x = 0.3 k and looks along z; point i lies 4 .. 10 ahead of the track and is seen by the keyframes within
    0.6 of it along x -> (views, start, fixed, points, obs)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, _ = CC.SQUARE
    z = rng.uniform(4.0, 10.0, n_points)
    x = rng.uniform(0.0, 0.3 * (n_kf - 1), n_points)
    y = rng.uniform(-0.3, 0.3, n_points) * z
    xyz = np.stack([x, y, z], axis=1).astype(np.float32)
    near = np.rint(x / 0.3).astype(np.int64)
    kf = (near[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    pt = np.repeat(np.arange(n_points), 5)
    keep = (kf >= 0) & (kf < n_kf)
    kf, pt = kf[keep], pt[keep]
    obs = np.zeros(len(kf), GR.OBS_DTYPE)
    X = xyz.astype(np.float64)
    obs["kf"], obs["point"] = kf, pt
    obs["u"] = (fx * (X[pt, 0] - 0.3 * kf) / X[pt, 2] + cx).astype(np.float32)
    obs["v"] = (fy * X[pt, 1] / X[pt, 2] + cy).astype(np.float32)
    obs["right"], obs["octave"] = -1.0, rng.integers(0, 8, len(kf))
    start = np.zeros((n_kf, 12))
    for k in range(n_kf):
        off = k >= 2
        R = PC.rot(*(rng.normal(0, 0.003, 3) * off))
        start[k] = PO.start_of(R, R @ np.array([-0.3 * k, 0.0, 0.0]) + rng.normal(0, 0.02, 3) * off)
    fixed = (np.arange(n_kf) < 2).astype(np.uint8)
    moved = (X + rng.normal(0, 0.02, X.shape)).astype(np.float32)
    return np.array([PO.view()] * n_kf), start, fixed, PO.points_of(moved), obs[rng.permutation(len(obs))]


for n_kf, n_points in SIZES:
    views, start, fixed, points, obs = track(1700 + n_kf, n_kf, n_points)
    params = binding.gba_params()
    host_ms, host = None, None
    if n_kf <= HOST_TWIN_UP_TO:
        t0 = time.perf_counter()
        host = binding.global_ba_host(views, start, fixed, PC.scale(), points, obs, params)
        host_ms = (time.perf_counter() - t0) * 1e3
    n_blocks = -(-n_points // ROWS)
    blocks = np.zeros((n_blocks, ROWS), binding.MAP_POINT_DTYPE)
    blocks.reshape(-1)[:n_points] = points
    counts = np.array([min(ROWS, n_points - b * ROWS) for b in range(n_blocks)], np.int32)
    table = np.array([(0, n_kf, 0, n_blocks, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE)
    d_points, d_np, d_start, d_fixed, d_all_fixed = dev(blocks), dev(counts), dev(start), dev(fixed), dev(np.ones_like(fixed))
    out = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((n_kf, 96), (n_blocks, ROWS * 24), (n_blocks, ROWS), (len(obs),), (1, 104))]
    torch.cuda.synchronize()

    def call(d_fx):
        ctx.global_ba_device(d_points.data_ptr(), d_np.data_ptr(), n_blocks, ROWS, d_start.data_ptr(), d_fx.data_ptr(), n_kf, table, obs, views, params,
                             *(t.data_ptr() for t in out))

    def timed(d_fx, n):
        for _ in range(2):
            call(d_fx)
        ctx.synchronize()
        wall = []
        for _ in range(n):  # unprofiled: one call from the host's sort and enqueue to synchronize
            t0 = time.perf_counter()
            call(d_fx)
            ctx.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_reset()
        ctx.profile(True)
        for _ in range(n):
            call(d_fx)
            ctx.synchronize()
        ctx.profile(False)
        stages = {s["name"]: {"median_ms": round(s["median_ms"], 5), "total_ms_per_call": round(s["total_ms"] / n, 5), "launches_per_call": s["launches"] // n,
                              "algorithmic_bytes": s["algorithmic_bytes"]} for s in ctx.stats() if s["launches"] and s["name"].startswith("gba_")}
        return stages, float(np.median(wall))

    n = reps if n_kf <= 4000 else max(reps // 4, 3)
    stages, wall = timed(d_fixed, n)
    res = out[4].cpu().numpy().view(binding.GBA_RESULT_DTYPE).reshape(1)[0]
    if host is not None:
        assert res.tobytes() == host[4].tobytes(), "the device and the host twin differ"
        assert out[0].cpu().numpy().tobytes() == host[0].tobytes(), "the device and the host twin differ in the poses"
    empty, empty_wall = timed(d_all_fixed, n)
    t0 = time.perf_counter()
    tables_only = binding.global_ba_host(views, start, np.ones_like(fixed), PC.scale(), points, obs, params)  # state 1: the host's sort and lists alone
    sort_ms = (time.perf_counter() - t0) * 1e3
    assert tables_only[4]["state"] == 1
    row = {"n_kf": n_kf, "n_points": n_points, "n_obs": len(obs), "reps": n, "stages": stages,
           "events_ms_per_call": round(sum(v["total_ms_per_call"] for v in stages.values()), 4), "wall_ms_per_call": round(wall, 4),
           "kernel_launches_per_call": sum(v["launches_per_call"] * KERNELS_PER_TIMER.get(k, 1) for k, v in stages.items()),
           "steps": res["steps"].tolist(), "accepted": res["accepted"].tolist(), "pcg_iterations": int(res["pcg_iterations"]), "state": int(res["state"]),
           "cost_before": float(res["cost_before"]), "cost_after": float(res["cost_after"]),
           "empty_schedule": {"events_ms_per_call": round(sum(v["total_ms_per_call"] for v in empty.values()), 4), "wall_ms_per_call": round(empty_wall, 4)},
           "host_sort_and_lists_ms": round(sort_ms, 2), "host_twin_one_core_ms": None if host_ms is None else round(host_ms, 1)}
    rows.append(row)
    print(f"{n_kf} keyframes, {n_points} points, {len(obs)} records: events {row['events_ms_per_call']} ms, wall {row['wall_ms_per_call']} ms per call; "
          f"{row['kernel_launches_per_call']} launches, steps {row['steps']}, {row['pcg_iterations']} PCG iterations, cost {row['cost_before']:.3g} -> {row['cost_after']:.3g}; "
          f"empty schedule {row['empty_schedule']}; host sort {sort_ms:.1f} ms; host twin {host_ms} ms", flush=True)
    print("   ", {k: v["total_ms_per_call"] for k, v in stages.items()}, flush=True)
    del d_points, d_np, d_start, d_fixed, d_all_fixed, out
    torch.cuda.empty_cache()

# inside the local bundle adjustment's limits: one problem through both host-pointer forms, one schedule
pr = GC.make_problem(seed=1800, n_kf=64, n_free=32, n_points=2000, p_obs=0.08, n_out=0)
d = pr["dense"]
schedule = dict(n_rounds=1, iterations=(10, 0, 0, 0), robust_rounds=1)
lp, gp = binding.ba_params(**schedule), binding.gba_params(**schedule)
local_res = global_res = None
local_wall, global_wall = [], []
for it in range(reps + 2):
    t0 = time.perf_counter()
    local_res = ctx.local_ba(d["views"], d["start"], 32, d["points"], d["kp"], d["idx"], lp, d["n_kp"])
    t1 = time.perf_counter()
    global_res = ctx.global_ba(pr["views"], pr["start"], pr["fixed"], pr["points"], pr["obs"], gp)
    t2 = time.perf_counter()
    if it >= 2:
        local_wall.append((t1 - t0) * 1e3), global_wall.append((t2 - t1) * 1e3)
cross = {"n_kf": 64, "n_free": 32, "n_points": 2000, "n_obs": len(pr["obs"]), "schedule": "one robust round of ten",
         "ss_local_ba_wall_ms": round(float(np.median(local_wall)), 3), "ss_global_ba_wall_ms": round(float(np.median(global_wall)), 3),
         "local_steps": local_res[4]["steps"].tolist(), "global_steps": global_res[4]["steps"].tolist(), "global_pcg_iterations": int(global_res[4]["pcg_iterations"]),
         "local_cost_after": float(local_res[4]["cost_after"]), "global_cost_after": float(global_res[4]["cost_after"]),
         "largest_pose_difference": float(np.abs(local_res[0] - global_res[0]).max())}
print("inside the local limits:", cross, flush=True)
result = {"device": torch.cuda.get_device_name(0), "note": "stages: HIP events around every timer with profiling on (a gba_pcg timer holds the three launches of one "
          "iteration); wall_ms_per_call: the median of one unprofiled call from the host's sort and enqueue to synchronize", "rows": rows, "inside_the_local_limits": cross}
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
