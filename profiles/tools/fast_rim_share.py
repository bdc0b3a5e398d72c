"""Rim share of k_fast_score's blocks (two stacked 64 x 32 tiles; ss_geometry.cpp's block records) per level, from the kernel's
own conditions.  CPU only.  usage: python profiles/tools/fast_rim_share.py [width height [n_levels]]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import orb_oracle as O  # noqa: E402

w, h = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1280, 720)
p = O.default_params(n_levels=int(sys.argv[3])) if len(sys.argv) > 3 else O.default_params()
g = O.geometry(p, w, h)
tot = [0, 0, 0, 0]
print("level size blocks interior top/bottom-only left/right rim%")
for l in range(g.n_levels):
    lw, lh = g.w[l], g.h[l]
    pitch = (lw + 63) // 64 * 64
    tiles_y = (lh + 31) // 32
    n = [0, 0, 0, 0]
    for y0 in range(0, 32 * tiles_y, 64):
        hrows = 64 if y0 + 32 < 32 * tiles_y else 32
        for x0 in range(0, lw, 64):
            inner_x = x0 >= 4 and x0 + 68 <= lw
            interior = inner_x and y0 >= 4 and y0 + hrows + 4 <= lh
            wide = inner_x and x0 >= 16 and x0 - 16 + 96 <= pitch
            n[0] += 1
            n[1] += interior and wide
            n[2] += wide and not interior
            n[3] += not wide
    print(f"{l} {lw}x{lh} {n[0]} {n[1]} {n[2]} {n[3]} {100.0 * (n[0] - n[1]) / n[0]:.1f}")
    tot = [a + b for a, b in zip(tot, n)]
print(f"all - {tot[0]} {tot[1]} {tot[2]} {tot[3]} {100.0 * (tot[0] - tot[1]) / tot[0]:.1f}")
