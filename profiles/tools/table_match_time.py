"""Match time per 64-frame batch: the table form (ss_match_batch_sources_device: four interleaved cameras, each frame against
the previous frame of its own camera, a camera's first frame against a carry frame) against mode 1 (ss_match_batch_device:
frame b against frame b - 1).  Times are the library's stage records (HIP events on the context's stream around the
launches): "match" = matcher + finish, "expand" = the carry's expansion to operand rows (table form only).
usage: python profiles/tools/table_match_time.py [width height n_features] [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from send_slam_amd import binding, synth  # noqa: E402

w, h, nf = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (1280, 720, 2000)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
B, NCAM = 64, 4
cams = [(b * 7 + b // 3) % NCAM for b in range(B)]  # irregular interleaving
frames = np.stack([synth.frame(10 + cams[b], w, h, t=b) for b in range(B)])
table = []
for b, c in enumerate(cams):
    earlier = [j for j in range(b) if cams[j] == c]
    table.append(earlier[-1] if earlier else -2 - c)
dev = torch.device("cuda:0")
with binding.OrbContext(0, n_features=nf, max_batch=B) as ctx:
    ctx.extract_batch_device(torch.from_numpy(frames).to(dev).data_ptr(), B, w, h)
    ctx.synchronize()
    kcap = ctx.batch_view().kp_capacity
    carry = torch.from_numpy(np.ascontiguousarray(np.stack([np.pad(ctx.fetch_frame(c)[1], ((0, kcap - len(ctx.fetch_frame(c)[1])), (0, 0)))
                                                              for c in range(NCAM)]))).to(dev)
    carry_n = torch.tensor([len(ctx.fetch_frame(c)[1]) for c in range(NCAM)], dtype=torch.int32, device=dev)
    outs = [torch.empty((B, kcap), dtype=t, device=dev) for t in (torch.int32, torch.int16, torch.int16)]
    ptrs = [o.data_ptr() for o in outs]
    res = {}
    for name, run in (("mode1", lambda: ctx.match_batch_device(1, *ptrs)),
                      ("table", lambda: ctx.match_batch_sources_device(table, *ptrs, d_carry=carry.data_ptr(), d_carry_n=carry_n.data_ptr(),
                                                                       n_carry=NCAM))):
        for _ in range(10):
            run()
        ctx.synchronize()
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(reps):
            run()
        ctx.synchronize()
        st = {s["name"]: s for s in ctx.stats()}
        ctx.profile(False)
        res[name] = {k: round(st[k]["median_ms"], 4) for k in ("match", "expand") if k in st}
    print({"shape": f"{w}x{h}_n{nf}", "frames": B, "cameras": NCAM, "kp_capacity": kcap, "median_ms": res})
