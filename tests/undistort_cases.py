"""The cameras, keypoint rows and depth frames the undistortion tests share (test infrastructure, plain module)."""
from __future__ import annotations

import functools

import numpy as np

import undistort_ref as UR

W, H = 320, 240
FX, FY, CX, CY = 260.0, 257.5, 159.0, 121.0
# barrel, pincushion, tangential only, none
COEFFS = {"D": (-0.28, 0.07, 1e-3, -5e-4), "P": (0.12, -0.03, -8e-4, 6e-4), "T": (0.0, 0.0, 2e-3, -1e-3), "Z": (0.0, 0.0, 0.0, 0.0)}
# measured on the CPU with the numpy oracle: min_x, max_x, min_y, max_y to the second decimal
MEASURED_BOUNDS = {"D": (-39.49, 361.83, -31.63, 269.26), "P": (8.03, 311.43, 6.47, 234.03)}

F, ROWS = 3, 70            # one wave plus six lanes
COUNTS = [70, 1, 0]
FRAME_CAMERAS = ["D", "Z", "T"]
PATTERN = 0x5A

DEPTH_W, DEPTH_H = 64, 48
DEPTH_PITCH = 80           # samples per row of the pitched float32 frame


def camera(name: str, width: int = W, height: int = H, **over):
    from send_slam_amd import binding
    k1, k2, p1, p2 = COEFFS[name]
    f = dict(type=b"PinHole", fx=FX, fy=FY, cx=CX, cy=CY, k1=k1, k2=k2, p1=p1, p2=p2, width=width, height=height, fps=30.0, rgb=0, th_depth=40.0,
             baseline=0.1, depth_map_factor=5000.0)
    f.update(over)
    return binding.Camera(**f)


WIDE_F = 130.0  # camera W: D's coefficients at half the focal length


def search_camera(name: str):
    """the cameras of the search tests: D as it is, or W, under which 16 % of the extracted keypoints of the 320 x 240 test frames
    leave the image (under D 0.07 %: the extractor keeps 19 px from the border, where D's shift is below 19 px except in the
    corners), so that the batch searches meet the grid index's border cells.  W's denominator stays >= 0.72"""
    return camera("D") if name == "D" else camera("D", fx=WIDE_F, fy=WIDE_F * FY / FX)


def kp_rows(x, y, seed: int = 0) -> np.ndarray:
    """keypoint records at the given positions, the other fields filled with values no rule produces"""
    from send_slam_amd import binding
    x = np.asarray(x, np.float32)
    rng = np.random.Generator(np.random.PCG64(0xD157 + seed))
    kp = np.zeros(len(x), binding.KP_DTYPE)
    kp["x"], kp["y"] = x, np.asarray(y, np.float32)
    kp["size"], kp["angle"], kp["response"] = rng.uniform(31, 111, len(x)), rng.uniform(0, 360, len(x)), rng.uniform(7, 200, len(x))
    kp["octave"] = rng.integers(0, 8, len(x))
    return kp


def edge_positions(width: int = W, height: int = H) -> np.ndarray:
    """float32 [n, 2]: the four corners, the principal point, fractional level-scaled positions (an integer position of level l
    times 1.2^l, as the extractor writes them), the float32 neighbours of 0 and of the width"""
    f = np.float32
    pts = [(0, 0), (width, 0), (0, height), (width, height), (CX, CY)]
    for level in range(8):
        s = f(1.2) ** level
        pts += [(f(19 + 7 * level) * f(s), f(16 + 5 * level) * f(s)), (f(int((width - 20) / s)) * f(s), f(int((height - 17) / s)) * f(s))]
    inf = f(np.inf)
    for v in (np.nextafter(f(0), -inf), np.nextafter(f(0), inf), np.nextafter(f(width), -inf), np.nextafter(f(width), inf)):
        pts += [(v, f(height / 3)), (f(width / 3), v)]
    return np.array(pts, np.float32)


def nonfinite_positions() -> np.ndarray:
    f = np.float32
    return np.array([(np.nan, 10), (10, np.nan), (np.inf, 10), (10, -np.inf), (np.nan, np.nan), (f(3e38), f(3e38)), (f(-3e38), 5)], np.float32)


@functools.lru_cache(maxsize=None)
def frames_case():
    """-> kp [F][ROWS]: every row live whatever the counts say; positions over the whole image and a little beyond it, the edge
    positions first"""
    rng = np.random.Generator(np.random.PCG64(0xD15702))
    kp = []
    for b in range(F):
        e = edge_positions()
        x = np.concatenate([e[:, 0], rng.uniform(-5, W + 5, ROWS)]).astype(np.float32)[:ROWS]
        y = np.concatenate([e[:, 1], rng.uniform(-5, H + 5, ROWS)]).astype(np.float32)[:ROWS]
        if b == 0:
            x[-7:], y[-7:] = nonfinite_positions()[:, 0], nonfinite_positions()[:, 1]
        kp.append(kp_rows(x, y, seed=b))
    return np.stack(kp)


def clamp(n: int, rows: int = ROWS) -> int:
    return min(max(int(n), 0), rows)


def twin_frames(kp, counts, cams, pattern_out=None):
    """what the device forms must write: the host twin on the first clamp(count) rows of every frame, the rest as `pattern_out`
    has them (None: as kp has them, the in-place forms)"""
    from send_slam_amd import binding
    out = np.array(kp if pattern_out is None else pattern_out, copy=True)
    for b in range(len(kp)):
        n = clamp(counts[b], kp.shape[1])
        out[b, :n] = binding.undistort_host(cams[b if len(cams) > 1 else 0], kp[b, :n])
    return out


# ---- depth ----
@functools.lru_cache(maxsize=None)
def depth_frames(kind: str) -> np.ndarray:
    """[F][DEPTH_H][pitch]: "u16": uint16 millimetre-like samples, tight rows; "f32": float32 metres in rows of DEPTH_PITCH samples,
    the pad filled with a value that would be a valid depth.  Zeros, negatives (float) and NaNs (float) are sprinkled in"""
    rng = np.random.Generator(np.random.PCG64(0xDE97 + (kind == "f32")))
    if kind == "u16":
        img = rng.integers(2000, 40000, (F, DEPTH_H, DEPTH_W)).astype(np.uint16)
        img[rng.random(img.shape) < 0.1] = 0
        return img
    img = np.full((F, DEPTH_H, DEPTH_PITCH), 7.5, np.float32)
    img[:, :, :DEPTH_W] = rng.uniform(0.4, 8.0, (F, DEPTH_H, DEPTH_W)).astype(np.float32)
    hole = rng.random((F, DEPTH_H, DEPTH_W))
    img[:, :, :DEPTH_W][hole < 0.08] = 0.0
    img[:, :, :DEPTH_W][(hole >= 0.08) & (hole < 0.14)] = -1.5
    img[:, :, :DEPTH_W][(hole >= 0.14) & (hole < 0.2)] = np.nan
    return img


@functools.lru_cache(maxsize=None)
def depth_kp():
    """-> kp [F][ROWS] over the depth frame: inside it, on its edges, just outside on every side, fractional parts above one half
    (truncation and rounding then pick different pixels), non-finite"""
    rng = np.random.Generator(np.random.PCG64(0xDE9703))
    kp = []
    for b in range(F):
        x, y = rng.uniform(-2, DEPTH_W + 2, ROWS).astype(np.float32), rng.uniform(-2, DEPTH_H + 2, ROWS).astype(np.float32)
        fixed = [(0, 0), (DEPTH_W - 1, DEPTH_H - 1), (DEPTH_W - 0.01, 3), (DEPTH_W, 3), (3, DEPTH_H), (-0.5, 4), (4, -0.99), (-1, 4), (10.75, 20.5),
                 (np.nan, 3), (3, np.inf), (-np.inf, 3), (3e38, 2)]
        for i, (fx, fy) in enumerate(fixed):
            x[i], y[i] = fx, fy
        kp.append(kp_rows(x, y, seed=10 + b))
    return np.stack(kp)
