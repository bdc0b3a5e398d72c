"""The frames, parameters and cached reference extractions the guided-matching tests share (test infrastructure, plain module)."""
from __future__ import annotations

import functools
import itertools

import numpy as np

import guided_ref as R
import patterns
import stereo_ref
from oracle import orb_oracle as O
from send_slam_amd import synth

W, H, NF = 320, 240, 500
RADIUS, SPAN = 15.0, 1

# the two acceptance rules of upstream (SearchForInitialization, SearchByProjection) x one_to_one x orientation
RULES = [dict(th=50, ratio_num=9, ratio_den=10), dict(th=100, ratio_num=0, ratio_den=0)]
COMBOS = [dict(r, one_to_one=bool(o), orientation=k) for r, o, k in itertools.product(RULES, (0, 1), (0, 1, 2))]


def combo_name(c) -> str:
    return f"th{c['th']}_r{c['ratio_num']}_{c['ratio_den']}_u{int(c['one_to_one'])}_o{c['orientation']}"


@functools.lru_cache(maxsize=None)
def frame(name: str, w: int = W, h: int = H) -> np.ndarray:
    """the named test frames; a shifted pattern moves by (2, 4) px"""
    if name.startswith("synth_t"):
        return synth.frame(0, w, h, int(name[7:]))
    if name.startswith("parallax_t"):
        return synth.parallax_frame(11, w, h, int(name[10:]))
    img = {"dots": lambda: patterns.dots(w, h), "dots_shift": lambda: patterns.dots(w, h, dx=2, dy=4),
           "checker": lambda: patterns.checker(w, h, 16), "checker_shift": lambda: patterns.checker(w, h, 16, dx=2, dy=4),
           "noise": lambda: patterns.noise(w, h, 3), "noise_shift": lambda: np.roll(patterns.noise(w, h, 3), (4, 2), axis=(0, 1)),
           "flat": lambda: patterns.flat(w, h, 90)}[name]()
    return np.ascontiguousarray(img)


# one batch, frame b against frame b - 1: every filter has work, one frame has no keypoints (as a query, then as a train)
BATCH = ["synth_t0", "synth_t1", "synth_t2", "synth_t3", "parallax_t0", "parallax_t3", "dots", "dots_shift", "checker", "checker_shift",
         "noise", "flat", "synth_t0"]


def params(nf: int = NF):
    return O.default_params(n_features=nf)


@functools.lru_cache(maxsize=None)
def features(name: str, w: int = W, h: int = H, nf: int = NF):
    """(keypoints, descriptors) of a named frame from the CPU oracle"""
    kp, desc, _ = O.extract(frame(name, w, h), params(nf))
    return kp, desc


@functools.lru_cache(maxsize=None)
def scales(w: int = W, h: int = H, nf: int = NF):
    return tuple(stereo_ref.level_scales(params(nf), w, h))


def own_windows(kp, w: int = W, h: int = H, nf: int = NF, radius: float = RADIUS, by_octave: bool = True, span: int = SPAN):
    return R.own_windows(kp, radius, by_octave, span, scales(w, h, nf))


@functools.lru_cache(maxsize=None)
def _found(query: str, train, w: int, h: int, nf: int, exclude_self: bool):
    qk, qd = features(query, w, h, nf)
    tk, td = features(train, w, h, nf) if train is not None else (None, None)
    return R.search(qd, tk, td, own_windows(qk, w, h, nf), exclude_self)


def reference_pair(query: str, train, combo, w: int = W, h: int = H, nf: int = NF, exclude_self: bool = False):
    """guided_ref.match of two named frames (train None: no train frame) with the query's own windows; the search, which
    does not depend on the parameter set, is computed once per pair"""
    qk, _ = features(query, w, h, nf)
    tk = features(train, w, h, nf)[0] if train is not None else None
    return R.finish(_found(query, train, w, h, nf, exclude_self), qk, tk, **combo)


# ---- the full-capacity pair of frames (pairs form and host form; tests/test_guided.py, tests/test_guided_ref.py) --------------
CAP_ROWS = 16384            # SS_GUIDED_MAX_ROWS: two passes of the 8192-row conflict table of k_guided_finish
CAP_KEY_ROWS = 8192         # the rows of one pass
CAP_W, CAP_H = 3840, 2160   # a 60 x 34 grid of 64 px cells: 32 px cells would be 8160 > 4096
CAP_PLANTED = (8191, 8192, 16383)  # contested train rows on both sides of the pass boundary and at the last row
CAP_FAR = 1 << 24           # a few coordinates lie beyond it: float32 holds even integers there, bins clamp to the last cell
CAP_COMBOS = [dict(th=256, ratio_num=10, ratio_den=10, one_to_one=True, orientation=2),
              dict(th=50, ratio_num=9, ratio_den=10, one_to_one=True, orientation=0)]
# the grids the suite never forms otherwise: cells of 256 px (shift 8); extents beyond 2^24 (4096 x 1 cells of 4096 px, every
# ordinary coordinate in cell 0); a 2 x 2 grid whose last cell holds nearly everything
CAP_EXTENTS = [(16000, 12000), (1 << 25, 37), (33, 33)]


def kp_rows(x, y, octave=0, angle=0.0) -> np.ndarray:
    from send_slam_amd import binding
    x = np.asarray(x, np.float32)
    kp = np.zeros(len(x), binding.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"], kp["angle"], kp["size"] = x, y, octave, angle, 31
    return kp


def near(rng, proto, n: int) -> np.ndarray:
    """n descriptors drawn from the prototypes with one byte disturbed (the near() of test_guided._crafted_frames)"""
    d = proto[rng.integers(0, len(proto), n)].copy()
    d[np.arange(n), rng.integers(0, 32, n)] ^= rng.integers(0, 256, n).astype(np.uint8)
    return d


@functools.lru_cache(maxsize=None)
def capacity_frames():
    """-> [frame 0, frame 1], dicts q_kp q_desc t_kp t_desc windows.

    Frame 0: CAP_ROWS train rows uniform over CAP_W x CAP_H (quarter pixels, octaves 0 - 7, angles in quarter degrees), 3000
    queries in groups of three that share a window centre, radii 150 - 399, octaves 0 - 7, all descriptors near 48 prototypes.
    Planted on top: per row of CAP_PLANTED a descriptor of its own and two queries that carry exactly it, in a small window
    around the row (a contested row at a chosen index); eight train rows and six window centres beyond 2^24 px.
    Frame 1: frame 0 with the sides swapped -- CAP_ROWS queries, windows around their own positions."""
    rng = np.random.Generator(np.random.PCG64(0xCA9AC17))
    proto = rng.integers(0, 256, size=(48, 32), dtype=np.uint8)

    def angles(n):
        return rng.integers(0, 360 * 4, size=n).astype(np.float32) / np.float32(4)

    def quarter(n, hi):
        return rng.integers(0, hi * 4, size=n).astype(np.float32) / np.float32(4)

    nt, groups = CAP_ROWS, 1000
    tk = kp_rows(quarter(nt, CAP_W), quarter(nt, CAP_H), octave=rng.integers(0, 8, nt), angle=angles(nt))
    td = near(rng, proto, nt)
    cx, cy = np.repeat(quarter(groups, CAP_W), 3), np.repeat(quarter(groups, CAP_H), 3)
    nq = 3 * groups
    qk = kp_rows(cx, cy, octave=rng.integers(0, 8, nq), angle=angles(nq))
    qd = near(rng, proto, nq)
    win = R.make_windows(cx, cy, rng.integers(150, 400, nq), 0, 7)
    # coordinates beyond 2^24: four train rows in each conflict pass, two queries whose windows hold some of them (every
    # octave admitted, |dx| < 64 around 2^24 + 100 and 2^24 + 4000)
    far_rows = np.array([100, 101, 102, 103, 9000, 9001, 9002, 9003])
    tk["x"][far_rows] = np.float32(CAP_FAR) + np.array([60, 100, 140, 3960, 80, 120, 4000, 4060], np.float32)
    tk["y"][far_rows] = np.array([10, 20, 30, 10, 12, 22, 20, np.float32(CAP_FAR) + 8], np.float32)
    far_q = np.array([30, 31, 32, 1500, 1501, 1502])
    win["x"][far_q] = np.float32(CAP_FAR) + np.array([100, 100, 100, 4000, 4000, 4000], np.float32)
    win["y"][far_q] = np.array([20, 20, 20, 20, 20, np.float32(CAP_FAR)], np.float32)
    win["radius"][far_q] = np.array([64, 30, 2000, 64, 5000, 100], np.float32)
    for q, row in zip(far_q, (101, 9001, 102, 9002, 103, 9003)):  # each finds one far row at distance 1
        qd[q] = td[row]
        qd[q, 0] ^= 1
    # the planted rows: two queries each, appended
    pd = rng.integers(0, 256, size=(len(CAP_PLANTED), 32), dtype=np.uint8)
    for k, row in enumerate(CAP_PLANTED):
        td[row] = pd[k]
    px, py = tk["x"][list(CAP_PLANTED)], tk["y"][list(CAP_PLANTED)]
    pk = kp_rows(np.repeat(px, 2), np.repeat(py, 2), octave=0, angle=angles(2 * len(CAP_PLANTED)))
    pw = R.make_windows(np.repeat(px, 2) + np.float32(1), np.repeat(py, 2) - np.float32(1), 4.0, 0, 7)
    qk, qd, win = np.concatenate([qk, pk]), np.concatenate([qd, np.repeat(pd, 2, axis=0)]), np.concatenate([win, pw])
    frame0 = {"q_kp": qk, "q_desc": qd, "t_kp": tk, "t_desc": td, "windows": win}
    # frame 1: the sides swapped; 16384 windows of 60 - 199 px around the queries' own positions, octave ranges that bite
    win1 = R.make_windows(tk["x"], tk["y"], rng.integers(60, 200, nt), rng.integers(0, 4, nt), rng.integers(4, 8, nt))
    frame1 = {"q_kp": tk, "q_desc": td, "t_kp": qk, "t_desc": qd, "windows": win1}
    return [frame0, frame1]


@functools.lru_cache(maxsize=None)
def capacity_found(b: int):
    """guided_ref.search of capacity frame b: the part of the reference that does not depend on the parameter set, once"""
    f = capacity_frames()[b]
    return R.search(f["q_desc"], f["t_kp"], f["t_desc"], f["windows"])


def capacity_reference(b: int, combo):
    f = capacity_frames()[b]
    return R.finish(capacity_found(b), f["q_kp"], f["t_kp"], **combo)


def grid_shift(extent_w: int, extent_h: int, max_cells: int = 4096) -> int:
    """the documented grid rule (include/sendslam_orb.h): cells of 32 px, doubled until the grid fits max_cells; extents
    beyond 2^24 px count as 2^24"""
    w, h = min(extent_w, CAP_FAR), min(extent_h, CAP_FAR)
    s = 5
    while (((w - 1) >> s) + 1) * (((h - 1) >> s) + 1) > max_cells:
        s += 1
    return s
