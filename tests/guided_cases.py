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
