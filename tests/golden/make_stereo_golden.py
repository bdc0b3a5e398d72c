"""Regenerates tests/golden/stereo/*.npz: what tests/stereo_ref.py (oracle extraction + the ComputeStereoMatches
restatement) returns for small 320x240 pairs.  Data only: the two eyes' pixels, the parameters, the expected points and
summary.  The files pin the restatement against drift; the GPU suite checks the HIP path against the restatement.

    python tests/golden/make_stereo_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "send-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import patterns  # noqa: E402
import stereo_ref as R  # noqa: E402
from oracle import orb_oracle as O  # noqa: E402
from send_slam_amd import synth  # noqa: E402

W, H, NF = 320, 240, 500


def pairs():
    sc = synth.scene(11, W, H)
    par = (synth.parallax_frame(11, W, H, 3, sc=sc), synth.parallax_frame(11, W, H, 0, sc=sc))
    return [  # name, left, right, fx, baseline, th_depth, scale factor, levels
        ("parallax_t3_s11_fx500", par[0], par[1], 500.0, 0.1, 35.0, 1.2, 8),
        ("parallax_t3_s11_fx12", par[0], par[1], 12.0, 0.1, 35.0, 1.2, 8),
        ("parallax_t3_s11_scale15", par[0], par[1], 500.0, 0.1, 35.0, 1.5, 4),
        ("identical_s11", par[1], par[1], 500.0, 0.1, 35.0, 1.2, 8),
        ("checker16_dx6", patterns.checker(W, H, 16, dx=6), patterns.checker(W, H, 16), 500.0, 0.1, 35.0, 1.2, 8),
        ("mixed_dx5", patterns.mixed_contrast(W, H, dx=5), patterns.mixed_contrast(W, H), 500.0, 0.25, 10.0, 1.2, 8),
    ]


def main():
    out = os.path.join(HERE, "stereo")
    os.makedirs(out, exist_ok=True)
    for name, left, right, fx, b, th, sf, nl in pairs():
        p = O.default_params(n_features=NF, lapping_x0=0, lapping_x1=0, scale_factor=sf, n_levels=nl)
        kL, dL, kR, dR, pts, summ = R.stereo_pair(left, right, p, fx, b, th)
        np.savez_compressed(os.path.join(out, name + ".npz"), left=left, right=right, n_features=NF, scale_factor=np.float32(sf), n_levels=nl,
                            fx=np.float32(fx), baseline=np.float32(b), th_depth=np.float32(th), points=pts,
                            summary=np.array([summ[k] for k in R.SUMMARY_FIELDS], np.int32))
        print(name, summ)


if __name__ == "__main__":
    main()
