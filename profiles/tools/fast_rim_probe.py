"""k_fast_score launches made almost only of interior blocks or only of rim blocks, of (nearly) equal block count, one context
alone on the chip: run under pmc.sh (SQ_INSTS_VALU) or kstats.sh (duration) and divide by the block count printed here.
usage: python profiles/tools/fast_rim_probe.py interior|corner|vrim|hrim flat|noise [reps]

  interior  one 4032 x 4032 frame, one level: 63 x 63 = 3969 blocks of two tiles: 3721 interior, 122 at the top / bottom rim
            only, 122 at the left / right rim only, 4 corners
  corner    992 frames of 128 x 128: 2 x 2 blocks each = 3968 blocks, every one at a corner (left or right AND top or bottom)
  vrim      31 frames of 4032 x 128: 63 x 2 blocks each = 3906 blocks: 3782 at the top / bottom rim only, 124 corners
  hrim      651 frames of 128 x 192 (a level may not be narrower than half its height): 2 x 3 blocks each = 3906 blocks:
            1302 at the left / right rim only, 2604 corners
Four launches, four kinds of block: the per-kind cost follows from the four totals (flat content, where a block's cost depends on
its kind alone: phase 2 stays empty, what differs is what a rim block pays around it); noise queues about every pixel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
import torch  # noqa: E402
from send_slam_amd import binding  # noqa: E402

if os.environ.get("SENDSLAM_LIB"):
    binding.LIB_PATH = os.environ["SENDSLAM_LIB"]

mode, content = sys.argv[1], sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
w, h, n = {"interior": (4032, 4032, 1), "corner": (128, 128, 992), "vrim": (4032, 128, 31), "hrim": (128, 192, 651)}[mode]
if content == "flat":
    frames = np.full((n, h, w), 90, np.uint8)
else:
    frames = np.random.default_rng(7).integers(0, 256, (n, h, w), dtype=np.uint8)
blocks = n * ((w + 63) // 64) * ((((h + 31) // 32) + 1) // 2)
d = torch.from_numpy(frames).cuda()
ctx = binding.OrbContext(0, n_features=1000, n_levels=1, max_batch=n)
for _ in range(reps + 1):
    ctx.extract_batch_device(d.data_ptr(), n, w, h)
ctx.synchronize()
print(f"{mode} {content}: {n} frames of {w}x{h}, {blocks} blocks per launch, {reps + 1} launches")
