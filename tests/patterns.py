"""Adversarial image content for the extraction and matching kernels (test infrastructure, plain module).

send_slam_amd/synth.py draws smooth noise plus shapes and always adds +-3 pixel noise: no two neighbouring FAST scores
are equal, about 0.2 % of the pixels are corners and every response is different.  The generators here produce what that
content never does: exact ties (equal scores next to each other, one response for a whole level, descriptors that
repeat), corner densities of 10 % and more, pixels pinned at 0 and 255, and contrasts exactly at the two FAST thresholds.

Integer-only numpy, seeded where random: (arguments) name the same bytes on every machine.  Every generator returns a
C-contiguous (h, w) uint8 array; periodic ones take a phase (dx, dy) so that their maxima can be put on any column / row of
a cell window or of a 64 x 32 tile.
"""
from __future__ import annotations

import numpy as np

from send_slam_amd import synth


def flat(w: int, h: int, value: int) -> np.ndarray:
    return np.full((h, w), value, np.uint8)


def dots(w: int, h: int, dx: int = 0, dy: int = 0, fg: int = 255, bg: int = 0, sx: int = 2, sy: int = 4) -> np.ndarray:
    """`fg` at the lattice (dx + sx a, dy + sy b) on `bg`.  With (sx, sy) = (2, 4) the FAST-9-16 ring of a dot holds no other
    dot (its offsets are (0, +-3), (+-1, +-3), (+-2, +-2), (+-3, +-1), (+-3, 0): odd x or y not a multiple of 4), so every dot
    is a corner whose 16 ring pixels are equal, with R = |fg - bg|; no background pixel is one; dots are never 8-adjacent."""
    img = np.full((h, w), bg, np.uint8)
    img[dy % sy::sy, dx % sx::sx] = fg
    return img


def ramp_dots(w: int, h: int, dx: int = 0, dy: int = 0) -> np.ndarray:
    """The (2, 4) lattice on 0 with dot values 40 + (7 x + 13 y) % 216: as dense, but the responses differ."""
    ys, xs = np.mgrid[0:h, 0:w]
    val = 40 + (7 * xs + 13 * ys) % 216
    on = ((xs - dx) % 2 == 0) & ((ys - dy) % 4 == 0)
    return np.ascontiguousarray(np.where(on, val, 0).astype(np.uint8))


def checker(w: int, h: int, k: int, dx: int = 0, dy: int = 0) -> np.ndarray:
    """k-px checkerboard of 0 and 255."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(((((xs + dx) // k + (ys + dy) // k) & 1) * 255).astype(np.uint8))


def blocks(w: int, h: int, k: int, seed: int, levels=(0, 255)) -> np.ndarray:
    """Random k-px blocks, each one of `levels`."""
    rng = np.random.Generator(np.random.PCG64([seed, k, len(levels), 0xB10C]))
    lv = np.asarray(levels, np.uint8)
    pick = rng.integers(0, len(lv), size=((h + k - 1) // k, (w + k - 1) // k))
    return np.ascontiguousarray(np.repeat(np.repeat(lv[pick], k, axis=0), k, axis=1)[:h, :w])


def noise(w: int, h: int, seed: int) -> np.ndarray:
    """Uniform random bytes."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x4015E]))
    return rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def noise01(w: int, h: int, seed: int) -> np.ndarray:
    """Every pixel 0 or 255."""
    rng = np.random.Generator(np.random.PCG64([seed, 0x4015E, 1]))
    return (rng.integers(0, 2, size=(h, w), dtype=np.uint8) * np.uint8(255)).astype(np.uint8)


def saturated(seed: int, w: int, h: int) -> np.ndarray:
    """synth.frame with three times the contrast around 128: large areas pinned at 0 and at 255, real corners between."""
    f = synth.frame(seed, w, h).astype(np.int64)
    return np.clip((f - 128) * 3 + 128, 0, 255).astype(np.uint8)


def mirrored(seed: int, w: int, h: int) -> np.ndarray:
    """The seed's scene without pixel noise, the right half the mirror image of the left one: moments come in pairs."""
    m = synth._MARGIN
    img = np.clip(synth.scene(seed, w, h)[m:m + h, m:m + w], 0, 255).astype(np.uint8)
    half = w // 2
    img[:, w - half:] = img[:, :half][:, ::-1]
    return np.ascontiguousarray(img)


def contrast_dots(w: int, h: int, base: int, c: int, dx: int = 0, dy: int = 0) -> np.ndarray:
    """The lattice with dots of base + c on base: R = c exactly for every dot."""
    return dots(w, h, dx, dy, fg=base + c, bg=base)


def ring_dots(w: int, h: int, c: int, dx: int = 0, dy: int = 0, v: int = 200, deep: int = 60, pitch: int = 8) -> np.ndarray:
    """Centres of value v every `pitch` px on a background of v - c, the four ring pixels at (+-3, 0), (0, +-3) of each at
    v - deep.  Every 9-arc of a centre's ring holds background pixels, so R = c exactly, while the four compass pixels
    differ from it by `deep`: a centre passes the kernel's compass pre-test whatever c is, and the arc search alone decides
    R > minThFAST.  (On the plain lattice the compass value equals R and the pre-test decides first.)"""
    img = np.full((h, w), v - c, np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    for ox, oy in ((3, 0), (-3, 0), (0, 3), (0, -3)):
        img[((xs - dx - ox) % pitch == 0) & ((ys - dy - oy) % pitch == 0)] = v - deep
    img[dy % pitch::pitch, dx % pitch::pitch] = v
    return img


def mixed_contrast(w: int, h: int, dx: int = 0, dy: int = 0, base: int = 100, region: int = 70) -> np.ndarray:
    """The lattice on `base` with dots of contrast 8 and 20 everywhere (scores 7 and 19: corners at minThFAST = 7 only) and,
    inside every other `region`-px square, some dots of contrast 21 (score 20: corners at iniThFAST = 20).  A grid cell that
    holds one of the latter keeps only those; the others fall back to all their minTh survivors."""
    ys, xs = np.mgrid[0:h, 0:w]
    a, b = (xs - dx) // 2, (ys - dy) // 4
    on = ((xs - dx) % 2 == 0) & ((ys - dy) % 4 == 0)
    c = np.where((a + b) % 2 == 0, 8, 20)
    strong = (((xs // region) + (ys // region)) % 2 == 0) & (a % 4 == 1) & (b % 2 == 1)
    c = np.where(strong, 21, c)
    return np.ascontiguousarray(np.where(on, base + c, base).astype(np.uint8))
