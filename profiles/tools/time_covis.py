"""Times of the covisibility family, one context alone on the chip.  Whole-map keyframe rows on the four maps of time_gba.py (100 ..
16 384 keyframes on a straight track, every point seen by the four or five keyframes nearest to it), and 128 frame rows of 2000 hits
each against the 1000-keyframe map.  For each: the host's table build (ss_covis_kf_host with no row: the checks, the two counting
passes and the lists), ss_covis_set_map from the call to synchronize and its upload by HIP events, the query's stage by HIP events, the
query from the call to synchronize, and the host twin on one core.  SENDSLAM_LIB selects an A/B build of the kernel (lanes per item,
the touched-range scan: profiles/tools/build_variant.sh NAME -DSS_COVIS_LANES=.. -DSS_COVIS_FRAME_LANES=.. -DSS_COVIS_RANGE=..); the
label names the run, and a run is added to the runs the output file already holds.
usage: python profiles/tools/time_covis.py [reps] [out.json] [label] [quick]"""
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
ROWS, CAP, N_LEVELS = 16384, 64, 8
FRAMES, HITS = 128, 2000
ctx = binding.OrbContext(0, n_features=500)
rows = []


def track(seed, n_kf, n_points):
    """point i lies along the track and is seen by the keyframes within two of the one nearest to it -> the records, shuffled"""
    rng = np.random.default_rng(seed)
    near = np.rint(rng.uniform(0.0, n_kf - 1, n_points)).astype(np.int64)
    kf = (near[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    pt = np.repeat(np.arange(n_points), 5)
    keep = (kf >= 0) & (kf < n_kf)
    obs = np.zeros(int(keep.sum()), binding.GBA_OBS_DTYPE)
    obs["kf"], obs["point"], obs["right"], obs["octave"] = kf[keep], pt[keep], -1.0, rng.integers(0, 8, int(keep.sum()))
    return obs[rng.permutation(len(obs))]


def median_ms(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def staged(fn, n, names):
    """the per-call HIP-event time of the stages `names` over n profiled calls of fn"""
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(n):
        fn()
        ctx.synchronize()
    ctx.profile(False)
    return {s["name"]: {"ms_per_call": round(s["total_ms"] / n, 5), "launches_per_call": s["launches"] // n, "algorithmic_bytes": s["algorithmic_bytes"]}
            for s in ctx.stats() if s["name"] in names and s["launches"]}


for n_kf, n_points in SIZES:
    obs = track(1700 + n_kf, n_kf, n_points)
    n_blocks = -(-n_points // ROWS)
    table = np.array([(0, n_kf, 0, n_blocks, 0, len(obs), (0, 0))], binding.GBA_PROBLEM_DTYPE)
    params = binding.covis_params()
    n = reps if n_kf <= 4000 else max(reps // 4, 3)
    build_ms = median_ms(lambda: binding.covis_kf_host(table, n_kf, n_blocks, ROWS, obs, N_LEVELS, params, CAP, rows=[]), max(n // 4, 3))
    t0 = time.perf_counter()
    host = binding.covis_kf_host(table, n_kf, n_blocks, ROWS, obs, N_LEVELS, params, CAP)
    host_ms = (time.perf_counter() - t0) * 1e3

    def set_map():
        ctx.covis_set_map(table, n_kf, n_blocks, ROWS, obs)
        ctx.synchronize()

    d_nb = torch.empty((n_kf, CAP * 8), dtype=torch.uint8, device="cuda")
    d_row = torch.empty((n_kf, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def query():
        ctx.covis_kf_device(None, n_kf, params, CAP, d_nb.data_ptr(), d_row.data_ptr())
        ctx.synchronize()

    set_map(), query(), query()
    set_ms, call_ms = median_ms(set_map, max(n // 4, 3)), median_ms(query, n)
    stages = staged(set_map, 3, ("covis_upload",))
    stages.update(staged(query, n, ("covis_kf",)))
    assert d_nb.cpu().numpy().view(np.int32).reshape(n_kf, CAP, 2).tobytes() == host[0].tobytes() and d_row.cpu().numpy().tobytes() == host[1].tobytes(), \
        "the device and the host twin differ"
    row = {"rows": "keyframes", "n_kf": n_kf, "n_points": n_points, "n_obs": len(obs), "reps": n, "mean_listed": round(float(host[1]["n_listed"].mean()), 2),
           "host_table_build_ms": build_ms, "set_map_wall_ms": set_ms, "stages": stages, "call_wall_ms": call_ms,
           "host_twin_one_core_ms": round(host_ms, 2), "host_twin_rows_only_ms": round(host_ms - build_ms, 2)}
    rows.append(row)
    print(json.dumps(row), flush=True)

    if n_kf == 1000:  # the frame rows: FRAMES frames of HITS hits each, every frame on one block of the map
        rng = np.random.default_rng(5)
        counts = np.array([min(ROWS, n_points - b * ROWS) for b in range(n_blocks)], np.int32)
        src = rng.integers(0, n_blocks, FRAMES).astype(np.int32)
        idx = np.full((FRAMES, ROWS), -1, np.int32)
        for b in range(FRAMES):
            idx[b, rng.choice(int(counts[src[b]]), size=min(HITS, int(counts[src[b]])), replace=False)] = 1
        d_idx, d_np = torch.from_numpy(idx).cuda(), torch.from_numpy(counts).cuda()
        f_nb = torch.empty((FRAMES, CAP * 8), dtype=torch.uint8, device="cuda")
        f_row = torch.empty((FRAMES, 32), dtype=torch.uint8, device="cuda")
        fparams = binding.covis_params(min_weight=1)
        torch.cuda.synchronize()

        def frames():
            ctx.covis_frames_device(d_idx.data_ptr(), d_np.data_ptr(), src, fparams, CAP, f_nb.data_ptr(), f_row.data_ptr())
            ctx.synchronize()

        frames(), frames()
        f_call = median_ms(frames, n)
        f_stage = staged(frames, n, ("covis_frames",))
        t0 = time.perf_counter()
        fhost = binding.covis_frames_host(table, n_kf, n_blocks, ROWS, obs, N_LEVELS, idx, counts, src, fparams, CAP)
        f_host_ms = (time.perf_counter() - t0) * 1e3
        assert f_nb.cpu().numpy().view(np.int32).reshape(FRAMES, CAP, 2).tobytes() == fhost[0].tobytes() and f_row.cpu().numpy().tobytes() == fhost[1].tobytes()
        row = {"rows": "frames", "n_kf": n_kf, "n_frames": FRAMES, "hits": HITS, "mean_listed": round(float(fhost[1]["n_listed"].mean()), 2), "stages": f_stage,
               "call_wall_ms": f_call, "host_twin_one_core_ms": round(f_host_ms, 2), "host_twin_rows_only_ms": round(f_host_ms - build_ms, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_idx, d_np, f_nb, f_row
    del d_nb, d_row
    torch.cuda.empty_cache()

NOTE = ("stages: HIP events around the launch with profiling on; *_wall_ms: the median of one unprofiled call to synchronize; host_table_build_ms: "
        "ss_covis_kf_host with no row, on one core.  One entry of runs per label: a later run with the same label replaces the earlier one")
if out_path:
    # the file holds every labelled run: the library as built and its A/B builds side by side
    result = {"device": torch.cuda.get_device_name(0), "note": NOTE, "runs": {}}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result["runs"] = json.load(f).get("runs", {})
    result["runs"][label] = {"library": os.path.basename(os.environ.get("SENDSLAM_LIB", "the library as built")), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
