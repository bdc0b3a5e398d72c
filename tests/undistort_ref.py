"""numpy restatement of Frame's keypoint post-processing (test infrastructure, plain module): with oracle/vo_oracle.py::undistort the
NORMATIVE statement of the rules in include/sendslam_orb.h ("undistorted keypoints, image bounds, RGB-D depth").

Written from the rules, not from the kernel.  The device code and the host twins must reproduce every number bit for bit.

    undistort        float32(vo.undistort(...)): the oracle's doubles, each coordinate rounded once
    bounds           Frame::ComputeImageBounds from the four corners
    min_denominator  the smallest 1 + (k2 r^2 + k1) r^2 any of the five iterations meets over a lattice of the image: while it
                     is positive, cv::undistortPoints' bail-out for icdist < 0, which the rule lacks, cannot matter
    depth            Tracking::GrabImageRGBD's scaling and Frame::ComputeStereoFromRGBD, one row at a time, float32 at every step
"""
from __future__ import annotations

import numpy as np

from oracle import vo_oracle as vo

f32 = np.float32
SUMMARY_FIELDS = ("status", "n_kp", "n_depth", "n_close")


def vo_camera(cam) -> vo.Camera:
    """anything with fx fy cx cy k1 k2 p1 p2 -> the oracle's camera"""
    return vo.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.p1, cam.p2)


def undistort(cam, xy) -> np.ndarray:
    """xy float32 [n, 2] -> mvKeysUn's positions, float32 [n, 2]"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        return vo.undistort(vo_camera(cam), xy).astype(np.float32)


def undistort_kp(cam, kp) -> np.ndarray:
    """keypoint records -> a copy with x and y undistorted, every other field as it was"""
    out = np.array(kp, copy=True).reshape(-1)
    un = undistort(cam, np.stack([out["x"], out["y"]], axis=1))
    out["x"], out["y"] = un[:, 0], un[:, 1]
    return out


def bounds(cam, width: int, height: int) -> np.ndarray:
    """-> float32 (min_x, max_x, min_y, max_y)"""
    if cam.k1 == 0 and cam.k2 == 0 and cam.p1 == 0 and cam.p2 == 0:
        return np.array([0, width, 0, height], np.float32)
    c = undistort(cam, [[0, 0], [width, 0], [0, height], [width, height]])
    return np.array([min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])], np.float32)


def min_denominator(cam, width: int, height: int, step: int = 4) -> float:
    """the smallest denominator of icdist over every iteration and every lattice position of 0 .. width x 0 .. height"""
    xs, ys = np.meshgrid(np.arange(0, width + 1, step, dtype=np.float64), np.arange(0, height + 1, step, dtype=np.float64))
    x0, y0 = (xs.ravel() - cam.cx) / cam.fx, (ys.ravel() - cam.cy) / cam.fy
    x, y, low = x0.copy(), y0.copy(), np.inf
    for _ in range(5):
        r2 = x * x + y * y
        den = 1.0 + (cam.k2 * r2 + cam.k1) * r2
        low = min(low, float(den.min()))
        dx = 2 * cam.p1 * x * y + cam.p2 * (r2 + 2 * x * x)
        dy = cam.p1 * (r2 + 2 * y * y) + 2 * cam.p2 * x * y
        x, y = (x0 - dx) / den, (y0 - dy) / den
    return low


def depth_inv(factor) -> np.float32:
    with np.errstate(all="ignore"):
        return f32(1.0) if abs(f32(factor)) < f32(1e-5) else f32(f32(1.0) / f32(factor))


def depth(bf, factor, close_limit, image: np.ndarray, width: int, xy_raw, x_un):
    """image: 2-D float32 or uint16, `width` samples of each row count.  xy_raw float32 [n, 2], x_un float32 [n] ->
    (right float32 [n], depth float32 [n], summary dict without status)"""
    xy_raw = np.asarray(xy_raw, np.float32).reshape(-1, 2)
    x_un = np.asarray(x_un, np.float32).reshape(-1)
    n, height = len(xy_raw), image.shape[0]
    inv = depth_inv(factor)
    right, out = np.full(n, -1, np.float32), np.full(n, -1, np.float32)
    with np.errstate(all="ignore"):
        scales = image.dtype == np.uint16 or abs(f32(inv - f32(1.0))) > f32(1e-5)
        for i in range(n):
            x, y = xy_raw[i]
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            col, row = int(x), int(y)  # truncation towards zero, as the C cast
            if not (0 <= col < width and 0 <= row < height):
                continue
            d = f32(image[row, col])
            if scales:
                d = f32(d * inv)
            if d > 0:
                out[i] = d
                right[i] = f32(x_un[i] - f32(f32(bf) / d))
    has = out > 0
    return right, out, {"n_kp": n, "n_depth": int(has.sum()), "n_close": int((has & (out < f32(close_limit))).sum())}
