"""Times of the map-point refresh, one context alone on the chip, on the track maps of time_covis.py (100 .. 16 384 keyframes on a
straight track, every point seen by the four or five keyframes nearest to it, the same record counts) with random descriptors: both
flags, geometry alone, and both flags under a select mask that leaves 10 % of the points.  For each: the `refresh` stage by HIP events,
the call to synchronize, the bytes the call must move (ss_stats: lists, rows, one descriptor per record, outputs) and the rate they
give against the HBM peak bench.py uses, and ss_refresh_host on one core on the same inputs (its table build measured apart).  The
device is held to the host twin on every workload.  A run is added under its label to the runs the output file already holds.
usage: python profiles/tools/time_refresh.py [reps] [out.json] [label] [quick]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
label = sys.argv[3] if len(sys.argv) > 3 else "default"
quick = len(sys.argv) > 4
SIZES = ((100, 5000), (1000, 50000)) if quick else ((100, 5000), (1000, 50000), (4000, 250000), (16384, 800000))
ROWS, N_LEVELS, RPF, HBM_PEAK_GBS = 16384, 8, 500, 8000.0
ctx = binding.OrbContext(0, n_features=500)
sc = [np.float32(1)]
for _ in range(1, N_LEVELS):
    sc.append(np.float32(float(sc[-1]) * float(np.float32(1.2))))
SCALE = np.array(sc, np.float32)
rows_out = []


def track(seed, n_kf, n_points):
    """time_covis.py's map: point i is seen by the keyframes within two of the one nearest to it -> the records, shuffled, and a
    keypoint row for each"""
    rng = np.random.default_rng(seed)
    near = np.rint(rng.uniform(0.0, n_kf - 1, n_points)).astype(np.int64)
    kf = (near[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    pt = np.repeat(np.arange(n_points), 5)
    keep = (kf >= 0) & (kf < n_kf)
    obs = np.zeros(int(keep.sum()), binding.GBA_OBS_DTYPE)
    obs["kf"], obs["point"], obs["right"], obs["octave"] = kf[keep], pt[keep], -1.0, rng.integers(0, 8, int(keep.sum()))
    obs = obs[rng.permutation(len(obs))]
    return obs, rng.integers(0, RPF, len(obs)).astype(np.int32)


def median_ms(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def staged(fn, n):
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(n):
        fn()
        ctx.synchronize()
    ctx.profile(False)
    return {s["name"]: {"ms_per_call": round(s["total_ms"] / n, 5), "launches_per_call": s["launches"] // n, "algorithmic_bytes": s["algorithmic_bytes"]}
            for s in ctx.stats() if s["name"] == "refresh" and s["launches"]}["refresh"]


for n_kf, n_points in SIZES:
    obs, obs_row = track(1700 + n_kf, n_kf, n_points)
    rng = np.random.default_rng(n_kf)
    n_blocks = -(-n_points // ROWS)
    table = np.array([(0, n_kf, 0, n_blocks, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE)
    pts = np.zeros((n_blocks, ROWS), binding.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = rng.normal(0, 5, (3, n_blocks, ROWS)).astype(np.float32)
    pdesc = np.zeros((n_blocks, ROWS, 32), np.uint8)
    counts = np.array([min(ROWS, n_points - b * ROWS) for b in range(n_blocks)], np.int32)
    desc = rng.integers(0, 256, (n_kf, RPF, 32), dtype=np.uint8)
    views = np.zeros(n_kf, binding.PROJ_VIEW_DTYPE)
    views["ow"] = rng.normal(0, 50, (n_kf, 3)).astype(np.float32)
    mask = (rng.random((n_blocks, ROWS)) >= 0.1).astype(np.uint8)  # 10 % of the points stay selected
    n = reps if n_kf <= 4000 else max(reps // 4, 3)
    ctx.covis_set_map(table, n_kf, n_blocks, ROWS, obs, obs_row=obs_row)
    d_pts, d_pd, d_np, d_desc, d_mask = (torch.from_numpy(a).cuda() for a in (pts.view(np.uint8).reshape(n_blocks, -1), pdesc, counts, desc, mask))
    d_info = torch.empty((n_blocks * ROWS, 32), dtype=torch.uint8, device="cuda")
    d_sum = torch.empty((n_blocks, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    build_ms = median_ms(lambda: binding.covis_kf_host(table, n_kf, n_blocks, ROWS, obs, N_LEVELS, binding.covis_params(), 4, rows=[]), 3)
    for name, g, d, sel in (("both", 1, 1, None), ("geometry", 1, 0, None), ("both_select_10", 1, 1, mask)):
        params = binding.refresh_params(g, d)

        def call():
            ctx.refresh_device(d_pts.data_ptr(), d_pd.data_ptr(), d_np.data_ptr(), d_desc.data_ptr(), RPF, views, params, d_info.data_ptr(), d_sum.data_ptr(),
                               d_select=0 if sel is None else d_mask.data_ptr())
            ctx.synchronize()

        call(), call()
        wall = median_ms(call, n)
        stage = staged(call, n)
        t0 = time.perf_counter()
        host = binding.refresh_host(table, n_kf, n_blocks, ROWS, obs, obs_row, SCALE, pts, pdesc, counts, desc, views, params, select=sel)
        host_ms = (time.perf_counter() - t0) * 1e3
        got_info = d_info.cpu().numpy().view(binding.REFRESH_INFO_DTYPE).reshape(n_blocks, ROWS)
        assert got_info.tobytes() == host[2].tobytes() and d_sum.cpu().numpy().tobytes() == host[3].tobytes(), "the device and the host twin differ"
        if sel is None:  # the blocks accumulate every workload's writes: compare what this one writes on every row
            fields = ("nx", "ny", "nz", "min_dist", "max_dist")
            dev_pts = d_pts.cpu().numpy().view(binding.MAP_POINT_DTYPE).reshape(n_blocks, ROWS)
            assert all(dev_pts[f].tobytes() == host[0][f].tobytes() for f in fields) and (not d or np.array_equal(d_pd.cpu().numpy(), host[1]))
        gbs = stage["algorithmic_bytes"] / (stage["ms_per_call"] * 1e-3) / 1e9 if stage["ms_per_call"] > 0 else 0.0
        row = {"workload": name, "n_kf": n_kf, "n_points": n_points, "n_obs": len(obs), "reps": n, "n_refreshed": int(host[3]["n_refreshed"].sum()), "stage": stage,
               "call_wall_ms": wall, "bytes_gb_per_s": round(gbs, 1), "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "host_table_build_ms": build_ms,
               "host_twin_one_core_ms": round(host_ms, 2), "host_twin_rows_only_ms": round(host_ms - build_ms, 2),
               "host_rows_over_stage": round((host_ms - build_ms) / stage["ms_per_call"], 1) if stage["ms_per_call"] > 0 else None}
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    del d_pts, d_pd, d_np, d_desc, d_mask, d_info, d_sum
    torch.cuda.empty_cache()

NOTE = ("stage: HIP events around the three launches with profiling on; call_wall_ms: the median of one unprofiled call to synchronize; host_twin_one_core_ms: "
        "ss_refresh_host, whose table build (host_table_build_ms, measured on ss_covis_kf_host with no row) the device call does not repeat; share_of_hbm_peak: "
        "the stage's bytes per second against 8000 GB/s.  One entry of runs per label: a later run with the same label replaces the earlier one")
if out_path:
    result = {"device": torch.cuda.get_device_name(0), "note": NOTE, "runs": {}}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result["runs"] = json.load(f).get("runs", {})
    result["runs"][label] = {"library": os.path.basename(os.environ.get("SENDSLAM_LIB", "the library as built")), "rows": rows_out}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
