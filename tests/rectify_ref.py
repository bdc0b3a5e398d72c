"""numpy restatement of the rectification rule (test infrastructure, plain module): the normative statement.

Written from the rule's description (include/sendslam_orb.h, DESIGN.md "Rectification"), not from the kernel.  The library
must reproduce the float maps, the fixed-point maps and the remapped bytes bit for bit.

    build_map     cv::initUndistortRectifyMap(K, D = k1 k2 p1 p2 k3, R, K', size, CV_32FC1) as recalled: double precision,
                  every step one IEEE operation, the running sum along a row (np.cumsum is that sequential sum)
    to_fixed      a float32 map value -> (integer part clamped to int16, 5 fraction bits): t = v * 32.0f, s = cvRound(t)
                  (half to even; INT32_MIN when t is not finite or outside int32, as on x86-64), i = s >> 5, f = s & 31
    remap         cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit pixels in its closed form: four taps, integer weights
                  that sum to 32768, (acc + 16384) >> 15
    remap_literal the same as a per-pixel loop with remapBilinear's three branches (all taps inside, all outside, mixed)
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
INT32_MIN = -(1 << 31)
MODEL_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "R", "fx_new", "fy_new", "cx_new", "cy_new", "width", "height")


def rot_x(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_y(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_z(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def model(K, D, R, Kn, width, height) -> dict:
    """K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3), R 3 x 3, Kn = (fx', fy', cx', cy')"""
    m = dict(zip(("fx", "fy", "cx", "cy"), map(float, K)))
    m.update(zip(("k1", "k2", "p1", "p2", "k3"), map(float, D)))
    m["R"] = np.ascontiguousarray(R, np.float64).reshape(3, 3)
    m.update(zip(("fx_new", "fy_new", "cx_new", "cy_new"), map(float, Kn)))
    m["width"], m["height"] = int(width), int(height)
    return m


def model_a():
    """a raw lens: barrel distortion, a small rotation about y, a zoomed-out new camera (the corners leave the source)"""
    return model((230, 232.3, 159.7, 120.7), (-0.28, 0.07, 2e-4, 2e-5, 0), rot_y(0.02), (184, 184, 160, 120), 320, 240)


def model_e():
    """a mild lens with a roll about z: what the end-to-end cases rectify with"""
    return model((230, 230, 159.7, 120.7), (-0.12, 0.03, 2e-4, 2e-5, 0), rot_z(0.01), (218.5, 218.5, 160, 120), 320, 240)


def model_k3():
    """k3, p1, p2 all non-zero and a rotation about all three axes"""
    return model((251.5, 249.25, 163.2, 118.9), (-0.31, 0.12, 1.5e-3, -7e-4, -0.021), rot_z(0.013) @ rot_y(-0.021) @ rot_x(0.017),
                 (205.0, 207.5, 158.0, 121.5), 320, 240)


def identity(width, height, f=200.0):
    return model((f, f, width / 2, height / 2), (0, 0, 0, 0, 0), np.eye(3), (f, f, width / 2, height / 2), width, height)


def scaled(m, width, height, focal=None) -> dict:
    """the coefficients and rotation of m on another image size: principal points scale with the size, focal lengths with it
    too or, when given, by `focal` in both directions"""
    sx, sy = width / m["width"], height / m["height"]
    fx, fy = (sx, sy) if focal is None else (focal, focal)
    return model((m["fx"] * fx, m["fy"] * fy, m["cx"] * sx, m["cy"] * sy), [m[k] for k in ("k1", "k2", "p1", "p2", "k3")], m["R"],
                 (m["fx_new"] * fx, m["fy_new"] * fy, m["cx_new"] * sx, m["cy_new"] * sy), width, height)


def inverse_new_camera(m):
    """ir = (K' R)^-1 by the adjugate, row-major [9], or None when the determinant is 0 or not finite"""
    Kn = [[m["fx_new"], 0.0, m["cx_new"]], [0.0, m["fy_new"], m["cy_new"]], [0.0, 0.0, 1.0]]
    R = m["R"]
    f = np.float64
    a = [[(f(Kn[i][0]) * f(R[0][j]) + f(Kn[i][1]) * f(R[1][j])) + f(Kn[i][2]) * f(R[2][j]) for j in range(3)] for i in range(3)]
    (a00, a01, a02), (a10, a11, a12), (a20, a21, a22) = a
    with np.errstate(all="ignore"):
        det = (a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20)) + a02 * (a10 * a21 - a11 * a20)
        if det == 0 or not np.isfinite(det):
            return None
        d = f(1.0) / det
        return np.array([(a11 * a22 - a12 * a21) * d, (a02 * a21 - a01 * a22) * d, (a01 * a12 - a02 * a11) * d,
                         (a12 * a20 - a10 * a22) * d, (a00 * a22 - a02 * a20) * d, (a02 * a10 - a00 * a12) * d,
                         (a10 * a21 - a11 * a20) * d, (a01 * a20 - a00 * a21) * d, (a00 * a11 - a01 * a10) * d], np.float64)


def build_map(m):
    """-> (map_x, map_y) float32 [height][width], or None for a singular K' R"""
    ir = inverse_new_camera(m)
    if ir is None:
        return None
    w, h = m["width"], m["height"]
    i = np.arange(h, dtype=np.float64)

    def running(base, step):  # base, base + step, (base + step) + step, ... along the row
        a = np.empty((h, w), np.float64)
        a[:, 0] = base
        a[:, 1:] = step
        return np.cumsum(a, axis=1)

    _x, _y, _w = running(i * ir[1] + ir[2], ir[0]), running(i * ir[4] + ir[5], ir[3]), running(i * ir[7] + ir[8], ir[6])
    k1, k2, p1, p2, k3 = (np.float64(m[k]) for k in ("k1", "k2", "p1", "p2", "k3"))
    with np.errstate(all="ignore"):
        ww = 1.0 / _w
        x, y = _x * ww, _y * ww
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        _2xy = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy
        return (np.float64(m["fx"]) * xd + np.float64(m["cx"])).astype(np.float32), (np.float64(m["fy"]) * yd + np.float64(m["cy"])).astype(np.float32)


def to_fixed(v):
    """float32 map values -> (i int32 in [-32768, 32767], f int32 in [0, 31])"""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        t = v * f32(32.0)
        ok = np.isfinite(t) & (t >= f32(-2147483648.0)) & (t < f32(2147483648.0))
        s = np.where(ok, np.rint(np.where(ok, t, f32(0))).astype(np.int64), INT32_MIN)
    return np.clip(s >> 5, -32768, 32767).astype(np.int32), (s & 31).astype(np.int32)


def weights(a, b):
    """the four integer weights of fraction (a, b), taps (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1): they sum to 32768"""
    return (32 - a) * (32 - b) * 32, a * (32 - b) * 32, (32 - a) * b * 32, a * b * 32


def remap(src, map_x, map_y):
    """closed form.  src [h][w] or [h][w][c] uint8, maps [h][w] float32 -> uint8 of src's shape"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape[:2]
    assert map_x.shape == (h, w) and map_y.shape == (h, w)
    ix, a = to_fixed(map_x)
    iy, b = to_fixed(map_y)
    s3 = src.reshape(h, w, -1).astype(np.int64)

    def S(y, x):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside[..., None], s3[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)

    w00, w01, w10, w11 = (k[..., None] for k in weights(a.astype(np.int64), b.astype(np.int64)))
    acc = S(iy, ix) * w00 + S(iy, ix + 1) * w01 + S(iy + 1, ix) * w10 + S(iy + 1, ix + 1) * w11
    assert acc.max(initial=0) < (1 << 31)
    out = (acc + 16384) >> 15
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8).reshape(src.shape)


def tap_classes(map_x, map_y):
    """per pixel: 4 = all four taps inside the image, 0 = none, 1..3 = that many"""
    h, w = map_x.shape
    ix, _ = to_fixed(map_x)
    iy, _ = to_fixed(map_y)
    n = np.zeros((h, w), np.int32)
    for dy in (0, 1):
        for dx in (0, 1):
            n += ((ix + dx >= 0) & (ix + dx < w) & (iy + dy >= 0) & (iy + dy < h)).astype(np.int32)
    return n


WTAB = np.array([[weights(a, b) for a in range(32)] for b in range(32)], np.int64)  # [b][a][4]


def remap_literal(src, map_x, map_y):
    """remapBilinear's loop: per destination pixel one of three branches"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape[:2]
    s3 = src.reshape(h, w, -1)
    cn = s3.shape[2]
    ix, a = to_fixed(map_x)
    iy, b = to_fixed(map_y)
    out = np.zeros((h, w, cn), np.uint8)
    branches = [0, 0, 0]
    for y in range(h):
        for x in range(w):
            sx, sy = int(ix[y, x]), int(iy[y, x])
            wt = WTAB[b[y, x], a[y, x]]
            if 0 <= sx < w - 1 and 0 <= sy < h - 1:  # (unsigned)sx < width1 && (unsigned)sy < height1
                branches[0] += 1
                p = s3[sy:sy + 2, sx:sx + 2].astype(np.int64)
                acc = p[0, 0] * wt[0] + p[0, 1] * wt[1] + p[1, 0] * wt[2] + p[1, 1] * wt[3]
            elif sx >= w or sx + 1 < 0 or sy >= h or sy + 1 < 0:  # BORDER_CONSTANT: the border value, 0
                branches[1] += 1
                continue
            else:
                branches[2] += 1
                acc = np.zeros(cn, np.int64)
                for k, (yy, xx) in enumerate(((sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1))):
                    if 0 <= xx < w and 0 <= yy < h:
                        acc += s3[yy, xx].astype(np.int64) * wt[k]
            out[y, x] = (acc + 16384) >> 15
    return out.reshape(src.shape), branches


def end_to_end_pair(width=320, height=240, seed=7):
    """the raw pair of the end-to-end cases: parallax frames t = 4 (left) and t = 0 (right) of one scene"""
    from send_slam_amd import synth
    sc = synth.scene(seed, width, height)
    return synth.parallax_frame(seed, width, height, 4, sc=sc), synth.parallax_frame(seed, width, height, 0, sc=sc)


TILE_W, TILE_H = 128, 8  # the destination tile one workgroup of the kernel owns
BOX_CLASSES = ("empty", "<= 8192 B", "8193 - 10240 B", "> 10240 B")


def rotation_map(width, height, degrees):
    """-> (map_x, map_y) float32: the source position of destination pixel (x, y) is (x, y) rotated by `degrees` about the image
    centre.  An input builder, not part of the rule: any map is as good as another to remap()"""
    t = np.deg2rad(np.float64(degrees))
    c, s = np.cos(t), np.sin(t)
    cx, cy = width / 2, height / 2
    x, y = np.meshgrid(np.arange(width, dtype=np.float64) - cx, np.arange(height, dtype=np.float64) - cy)
    return (cx + c * x - s * y).astype(np.float32), (cy + s * x + c * y).astype(np.float32)


def identity_map(width, height):
    x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
    return x, y


def tile_boxes(map_x, map_y, channels):
    """-> int64 [ceil(h / 8)][ceil(w / 128)]: per 128 x 8 destination tile the bytes of the bounding box of its taps that carry
    weight (inside the image and weight > 0), as the device stages it: the byte range of the box's columns rounded outward
    to multiples of 16, times its rows; 0 for a tile without such a tap"""
    h, w = map_x.shape
    ix, a = to_fixed(map_x)
    iy, b = to_fixed(map_y)
    wts = weights(a.astype(np.int64), b.astype(np.int64))
    big = 1 << 40
    xl, xh, yl, yh = np.full((h, w), big), np.full((h, w), -1), np.full((h, w), big), np.full((h, w), -1)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        x, y = ix.astype(np.int64) + dx, iy.astype(np.int64) + dy
        on = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (wts[k] > 0)
        xl, xh = np.where(on, np.minimum(xl, x), xl), np.where(on, np.maximum(xh, x), xh)
        yl, yh = np.where(on, np.minimum(yl, y), yl), np.where(on, np.maximum(yh, y), yh)
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    out = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            t = (slice(j * TILE_H, (j + 1) * TILE_H), slice(i * TILE_W, (i + 1) * TILE_W))
            x1, y1 = int(xh[t].max()), int(yh[t].max())
            if x1 < 0:
                continue
            x0, y0 = int(xl[t].min()), int(yl[t].min())
            b0 = (x0 * channels) // 16 * 16
            out[j, i] = -(-((x1 + 1) * channels - b0) // 16) * 16 * (y1 - y0 + 1)
    return out


def box_classes(boxes):
    """tile_boxes -> how many tiles are empty, fit two 16-byte chunks per lane, need the third, do not fit the 10240-byte box"""
    return [int((boxes == 0).sum()), int(((boxes > 0) & (boxes <= 8192)).sum()), int(((boxes > 8192) & (boxes <= 10240)).sum()),
            int((boxes > 10240).sum())]
