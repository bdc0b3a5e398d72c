"""Times of the map points from depth at the benchmark's own shape, one context alone on the chip: 128 frames of 1280 x 720, 2000
features.  Per repetition one extraction, the in-place undistortion, the depth lookup (uint16 frames), ss_unproject_batch_device in
both modes, ss_triangulate_stereo_batch_device with all-stereo rows and, as the yardstick next to them, the monocular
ss_triangulate_batch_device, both of frame b against frame b - 1 on matches idx[i] = i (arbitrary couples under a sideways baseline:
most pass the parallax test and run the DLT).  Each stage by HIP events
from ss_stats after warm-up calls, with its byte floor: the bytes it must move over the HBM peak.
usage: python profiles/tools/time_unproject.py [reps] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
B, W, H, NF = 128, 1280, 720, 2000
HBM_PEAK = 8.0e12       # bytes/s, the datasheet's; 6.29e12 was measured with a float4 copy
HBM_MEASURED = 6.29e12

cam = binding.Camera(type=b"PinHole", fx=1040.0, fy=1030.0, cx=636.0, cy=363.0, k1=-0.28, k2=0.07, p1=1e-3, p2=-5e-4, width=W, height=H, fps=30.0,
                     th_depth=40.0, baseline=0.1, depth_map_factor=5000.0)
distinct = [synth.frame(0, W, H, t) for t in range(8)]
d_frames = torch.from_numpy(np.stack([distinct[t % 8] for t in range(B)])).cuda()
rng = np.random.default_rng(7)
depth_img = rng.integers(0, 40000, (B, H, W)).astype(np.uint16)  # 0 .. 8 m: about half the rows are closer than mThDepth = 4 m
d_depth_img = torch.from_numpy(depth_img.view(np.int16)).cuda()
ctx = binding.OrbContext(0, n_features=NF, max_batch=B)
ctx.set_calibration(1, cam)
ctx.extract_batch_device(d_frames.data_ptr(), B, W, H)
ctx.synchronize()
kcap = ctx.batch_view().kp_capacity
raw = [ctx.fetch_frame(b)[:2] for b in range(B)]
counts = [len(k) for k, _ in raw]


def dev(shape, dtype=torch.uint8):
    return torch.empty(shape, dtype=dtype, device="cuda")


d_right, d_dep, d_dsum = dev((B, kcap), torch.float32), dev((B, kcap), torch.float32), dev((B, 16))
outs = {m: [dev((B, kcap * k)) for k in (4, 32, 32, 8)] + [dev((B, 4)), dev((B, 40))] for m in ("all", "close")}
tri = [dev((B, kcap * k)) for k in (16, 32, 32, 8)] + [dev((B, 4)), dev((B, 64))]
tri_st = [dev((B, kcap * k)) for k in (32, 32, 32, 8)] + [dev((B, 4)), dev((B, 80))]
d_idx = torch.arange(kcap, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous()
dp = binding.depth_params_from_camera(cam, 1)
poses = [(np.eye(3), np.array([-0.05 * b, 0.0, 0.0])) for b in range(B)]  # a sideways walk, 5 cm a frame
views = [binding.unproject_view(cam, r, t) for r, t in poses]
pairs = [binding.epi_pair(cam, *poses[b], cam, *poses[max(b - 1, 0)]) for b in range(B)]
up = {"all": binding.unproject_params(binding.SS_UNPROJECT_ALL, 0, dp.close_limit), "close": binding.unproject_params(binding.SS_UNPROJECT_CLOSE, 100, dp.close_limit)}
tp = binding.tri_params()
stp = binding.tri_stereo_params()
rigs = [binding.TriStereoRig(bf1=cam.baseline * cam.fx, b1=cam.baseline, bf2=cam.baseline * cam.fx, b2=cam.baseline)] * B
torch.cuda.synchronize()


def one():
    ctx.extract_batch_device(d_frames.data_ptr(), B, W, H)
    ctx.undistort_batch_device()
    ctx.depth_batch_device(dp, d_depth_img.data_ptr(), W, H, W * 2, W * H * 2, d_right.data_ptr(), d_dep.data_ptr(), d_dsum.data_ptr())
    ctx.synchronize()
    for m in ("all", "close"):
        ctx.unproject_batch_device(d_dep.data_ptr(), 4, views, up[m], *[t.data_ptr() for t in outs[m]])
    ctx.triangulate_batch_device(d_idx.data_ptr(), pairs, tp, *[t.data_ptr() for t in tri])
    stereo()
    ctx.synchronize()


def stereo():
    """the stereo form on the same matches; nearly every row has a depth (the depth frames hold few zeros): all-stereo rows"""
    ctx.triangulate_stereo_batch_device(d_idx.data_ptr(), pairs, rigs, d_dep.data_ptr(), 4, d_right.data_ptr(), 4, stp, *[t.data_ptr() for t in tri_st])


for _ in range(3):
    one()
# one mode per profiled pass, so that the stage named "unproject" holds one mode's launches
stats = {}
for m in ("all", "close"):
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(reps):
        ctx.unproject_batch_device(d_dep.data_ptr(), 4, views, up[m], *[t.data_ptr() for t in outs[m]])
        ctx.synchronize()
    ctx.profile(False)
    stats["unproject_" + m] = next(s for s in ctx.stats() if s["name"] == "unproject")
ctx.profile_reset()
ctx.profile(True)
for _ in range(reps):
    ctx.triangulate_batch_device(d_idx.data_ptr(), pairs, tp, *[t.data_ptr() for t in tri])
    ctx.synchronize()
ctx.profile(False)
for s in ctx.stats():
    if s["name"] in ("tri_eval", "tri_compact") and s["launches"]:
        stats[s["name"]] = s
ctx.profile_reset()
ctx.profile(True)
for _ in range(reps):
    stereo()
    ctx.synchronize()
ctx.profile(False)
for s in ctx.stats():
    if s["name"] in ("tri_stereo_eval", "tri_compact", "tri_stereo_summary") and s["launches"]:
        stats[s["name"] if s["name"] != "tri_compact" else "tri_compact_after_stereo"] = s

# the device's results once more against the host twin, so that the figures are those of a correct run
scale = np.ones(8, np.float32)  # the context's table: scale[i] = (float)(scale[i - 1] * (double)1.2f)
for k in range(1, 8):
    scale[k] = np.float32(np.float64(scale[k - 1]) * np.float64(np.float32(1.2)))
created = {}
for m in ("all", "close"):
    n_pts = outs[m][4].cpu().numpy().view(np.int32).reshape(B)
    created[m] = int(n_pts.sum())
    un = binding.undistort_host(cam, raw[5][0])
    depth5 = d_dep[5].cpu().numpy()[:counts[5]]
    want = binding.unproject_host(views[5], up[m], scale, un, raw[5][1], depth5)
    got = outs[m][1][5].cpu().numpy().view(binding.MAP_POINT_DTYPE)[:n_pts[5]]
    assert n_pts[5] == len(want[1]) and got.tobytes() == want[1].tobytes(), "the device and the host twin differ"

rows = int(np.sum(counts))
tri_points = int(tri[4].cpu().numpy().view(np.int32).sum())
st_summ = tri_st[5].cpu().numpy().view(binding.TRI_STEREO_SUMMARY_DTYPE).reshape(B)
st_info = tri_st[0][5].cpu().numpy().view(binding.TRI_STEREO_INFO_DTYPE)[:counts[5]]
un5, un4 = binding.undistort_host(cam, raw[5][0]), binding.undistort_host(cam, raw[4][0])
m5 = min(counts[5], counts[4])
want_st = binding.triangulate_stereo_host(pairs[5], rigs[5], stp, scale, un5[:m5], un4[:m5], d_dep[5].cpu().numpy()[:m5], d_right[5].cpu().numpy()[:m5],
                                          d_dep[4].cpu().numpy()[:m5], d_right[4].cpu().numpy()[:m5])[1]
assert st_info[:m5].tobytes() == want_st.tobytes(), "the stereo triangulation and its host twin differ"
# the bytes a stage must move: per live row its depth, octave and state; per created point its position, 32 bytes of point, its
# descriptor in and out, its rows; the frames' counts, views and summaries are a few KB
floor = {m: rows * 12 + created[m] * (8 + 32 + 64 + 8) for m in ("all", "close")}
out = {"device": torch.cuda.get_device_name(0), "shape": {"frames": B, "width": W, "height": H, "n_features": NF, "kp_capacity": kcap, "keypoints": rows},
       "reps": reps, "warmup": 3,
       "note": "median_ms and mean_ms: HIP events around each stage's launch, one launch per call of 128 frames; floor_us: the bytes the stage must "
               "move over the HBM peak of 8.0 TB/s (datasheet) and over the 6.29 TB/s a float4 copy reaches; tri_eval and tri_compact are the two "
               "launches of the monocular ss_triangulate_batch_device on the same batch, the yardstick; tri_stereo_eval, tri_compact_after_stereo and "
               "tri_stereo_summary are the three launches of ss_triangulate_stereo_batch_device on the same matches with the depth planes (all-stereo rows)",
       "points_created": created, "tri_points": tri_points, "tri_stereo_points": int(st_summ["n_points"].sum()),
       "tri_stereo_rows_per_mode": [int(v) for v in st_summ["n_mode"].sum(axis=0)], "stages": {}}
for name, s in stats.items():
    rec = {"median_ms": round(s["median_ms"], 5), "mean_ms": round(s["mean_ms"], 5), "launches": s["launches"], "counted_bytes": s["algorithmic_bytes"]}
    if name.startswith("unproject_"):
        fb = floor[name[len("unproject_"):]]
        rec.update(floor_bytes=fb, **{"floor_us_at_8.0TBs": round(fb / HBM_PEAK * 1e6, 3), "floor_us_at_6.29TBs": round(fb / HBM_MEASURED * 1e6, 3)})
    out["stages"][name] = rec
print(json.dumps(out))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
