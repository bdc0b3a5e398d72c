"""The frames, cameras, poses and depth planes the tests of the map points from depth share (test infrastructure, plain module)."""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import guided_cases as G
import proj_cases as PC
import undistort_cases as UC
import unproject_ref as U

F, ROWS = 3, 70                 # one wave plus six lanes
COUNTS = ([70, 1, 0], [200, -3, 69])
PATTERN = 0x5A
CLOSE_LIMIT = 3.0
MAX_POINTS = 5
# rotated and translated: no entry of rcw is 0 or 1, no entry of ow is 0
POSES = [(PC.rot(0.31, -0.22, 0.13), (0.5, -0.25, 1.0)), (PC.rot(-0.4, 0.15, -0.27), (-1.5, 0.75, 0.125)), (PC.rot(0.05, 0.6, 0.2), (0.25, 2.0, -0.5))]
# the depths of the frames: ties on both sides of the limit and on it, the largest finite float, +inf; then what is no depth
DEPTHS = (0.5, 1.0, 1.0, 1.5, 2.0, 2.5, CLOSE_LIMIT, CLOSE_LIMIT, 3.5, 4.0, 4.0, 4.0, 6.0, 3.4e38, np.inf)
NO_DEPTHS = (0.0, -0.0, -1.0, np.nan, -np.inf)


def scale():
    """the pyramid table of the default parameters (1.2, 8 levels)"""
    return np.array(PC.scale(), np.float32)


def binding_camera(cam):
    from send_slam_amd import binding
    return binding.Camera(fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], width=G.W, height=G.H)


def ref_view(cam, pose):
    return U.view_init(cam[0], cam[1], cam[2], cam[3], pose[0], pose[1])


def ref_views(cams=CC.FRAME_CAMERAS, poses=POSES):
    return [ref_view(c, p) for c, p in zip(cams, poses)]


def twin_views(cams=CC.FRAME_CAMERAS, poses=POSES):
    from send_slam_amd import binding
    return [binding.unproject_view(binding_camera(c), p[0], p[1]) for c, p in zip(cams, poses)]


def draw_depths(rng, rows: int, p_none: float = 0.2) -> np.ndarray:
    d = rng.choice(np.array(DEPTHS, np.float32), rows)
    none = rng.random(rows) < p_none
    d[none] = rng.choice(np.array(NO_DEPTHS, np.float32), int(none.sum()))
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def frames_case():
    """-> dict of [F][ROWS] arrays: kp, desc, depth, has_point, outlier.  Every row is filled whatever the counts say.  Two rows of
    every frame have an octave outside the table"""
    rng = np.random.Generator(np.random.PCG64(0x0D39))
    kp = np.stack([UC.kp_rows(rng.uniform(0, G.W, ROWS), rng.uniform(0, G.H, ROWS), seed=40 + b) for b in range(F)])
    kp["octave"][:, 11], kp["octave"][:, 40] = 8, -1
    depth = np.stack([draw_depths(rng, ROWS) for _ in range(F)])
    depth[:, 11], depth[:, 40], depth[:, 0] = 1.0, 2.0, 0.5  # the rows outside the table have a depth; row 0 too (a count of 1)
    return dict(kp=kp, desc=rng.integers(0, 256, (F, ROWS, 32), dtype=np.uint8), depth=depth,
                has_point=(rng.random((F, ROWS)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (F, ROWS)).astype(np.uint8),
                outlier=(rng.random((F, ROWS)) < 0.3).astype(np.uint8))


def stereo_points(depth: np.ndarray) -> np.ndarray:
    """the depths inside an ss_stereo_point array of the same shape, every other field a value no rule reads"""
    from send_slam_amd import binding
    pts = np.zeros(depth.shape, binding.STEREO_POINT_DTYPE)
    pts["u_right"], pts["right_idx"], pts["orb_dist"], pts["sad"] = 7777.0, 123456, 4321, 54321
    pts["depth"] = depth
    return pts


def selection_depths(rng, rows: int, n_not_far: int, n_far: int) -> np.ndarray:
    """`rows` depths in a random order: n_not_far of them in (0, CLOSE_LIMIT] with ties and the limit itself, n_far above it, every
    far value three times over so that a cut among the far rows falls between equal depths; the rest no depth"""
    assert n_not_far + n_far <= rows
    near = rng.choice(np.array([0.5, 1.0, 1.0, 2.0, CLOSE_LIMIT], np.float32), n_not_far)
    far = np.repeat(np.array([3.5, 4.0, 6.0, np.inf], np.float32), 3)[rng.integers(0, 12, n_far)] if n_far else np.zeros(0, np.float32)
    d = np.concatenate([near, far, rng.choice(np.array(NO_DEPTHS, np.float32), rows - n_not_far - n_far)]).astype(np.float32)
    return d[rng.permutation(rows)]


def selection_cases():
    """(name, max_points, depth [ROWS]): n_not_far below, at, one above and far above max_points; no far row; only far rows; fewer
    live rows than max_points; equal depths on both sides of the cut"""
    rng = np.random.Generator(np.random.PCG64(0x5E1EC7))
    out = []
    for mp in (0, 5, 100):
        for tag, nf in (("below", mp - 1), ("at", mp), ("one_above", mp + 1), ("far_above", 55)):
            if 0 <= nf <= 60:
                out.append((f"max{mp}_{tag}", mp, selection_depths(rng, ROWS, nf, 10)))
        out.append((f"max{mp}_no_far_row", mp, selection_depths(rng, ROWS, 30, 0)))
        out.append((f"max{mp}_only_far_rows", mp, selection_depths(rng, ROWS, 0, 40)))
        out.append((f"max{mp}_few_live_rows", mp, selection_depths(rng, ROWS, 2, 1)))
    ties = np.full(ROWS, 4.0, np.float32)  # every row at one far depth: the lower rows win
    out.append(("max5_all_equal", 5, ties))
    return out


SIZE_ROWS = 16384  # SS_GUIDED_MAX_ROWS
SIZE_MAX_POINTS = 100


@functools.lru_cache(maxsize=None)
def size_case():
    """two frames of SIZE_ROWS rows whose depths are drawn from 64 distinct values (0.25 .. 16.0), so ties are everywhere -> dict;
    with close_limit 8.0 half the rows are not far, with 0.125 none is and the cut falls inside the ties of the lowest value"""
    rng = np.random.Generator(np.random.PCG64(0x512E))
    kp = np.stack([UC.kp_rows(rng.uniform(0, G.W, SIZE_ROWS), rng.uniform(0, G.H, SIZE_ROWS), seed=60 + b) for b in range(2)])
    depth = (rng.integers(1, 65, (2, SIZE_ROWS)) * 0.25).astype(np.float32)
    depth[rng.random((2, SIZE_ROWS)) < 0.1] = -1.0
    return dict(kp=kp, desc=rng.integers(0, 256, (2, SIZE_ROWS, 32), dtype=np.uint8), depth=depth,
                has_point=(rng.random((2, SIZE_ROWS)) < 0.3).astype(np.uint8), limits=dict(above=8.0, below=0.125))


def twin_frame(view, mode, max_points, close_limit, kp, desc, depth, n=None, has_point=None, outlier=None):
    """ss_unproject_host in the shape of unproject_ref.frame"""
    from send_slam_amd import binding
    p = binding.unproject_params(mode, max_points, close_limit)
    info, pts, pd, pr, summary = binding.unproject_host(view, p, scale(), kp, desc, depth, n=n, has_point=has_point, outlier=outlier)
    return dict(state=info["state"].copy(), points=pts, desc=pd, rows=pr, summary={f: int(summary[f]) for f in U.SUMMARY_FIELDS})


def same_frame(tag, got, want):
    """two results in the shape of unproject_ref.frame, byte for byte"""
    assert got["summary"] == want["summary"], f"{tag}: summary {got['summary']} != {want['summary']}"
    bad = np.flatnonzero(got["state"] != want["state"])
    assert len(bad) == 0, f"{tag}: state differs at rows {bad[:8]}: {got['state'][bad[:8]]} != {want['state'][bad[:8]]}"
    assert got["rows"].tobytes() == want["rows"].tobytes(), f"{tag}: point rows differ"
    assert got["desc"].tobytes() == want["desc"].tobytes(), f"{tag}: point descriptors differ"
    g, w = np.ascontiguousarray(got["points"]), np.ascontiguousarray(want["points"])
    assert len(g) == len(w), tag
    for f in U.MAP_POINT_FIELDS:
        bad = np.flatnonzero(g[f].view(np.uint32) != w[f].view(np.uint32))
        assert len(bad) == 0, f"{tag}: {f} differs at points {bad[:6]}: {g[f][bad[:6]]} != {w[f][bad[:6]]}"
