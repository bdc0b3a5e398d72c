"""The cameras the view kernels are tested under, and the ways a kernel could confuse them (test infrastructure, plain module).

A camera is (fx, fy, cx, cy, bf).  Every value is a multiple of a quarter, so float32 holds it exactly.  The odd cameras are
non-square (fx != fy) and off-centre (cx, cy away from the middle of the image, cx != cy), and no two of a call agree in any field:
a kernel that takes fy for fx, one frame's record for another's or one side of a pair for the other computes different bytes.

    FRAME_CAMERAS     the cameras of the three frames of a 320 x 240 call: A, B and the square camera of proj_cases
    PAIR_CAMERAS      (camera 1, camera 2) of the three pairs of a 320 x 240 call
    SIM3_PAIR_CAMERAS the same for the 640 x 480 Sim3 scenes
    FRAME_MIXUPS      name -> (the cameras of a call -> the cameras a wrong kernel would use)
    frame_mixups(row) FRAME_MIXUPS and "every problem with problem 0's camera row", for calls whose problems own `row` frames each
    PAIR_MIXUPS       the same for calls of pairs; bf is no part of a pair, so it has no mix-up there

tests/test_*_ref.py run every reference under every mix-up and assert that the bytes the GPU tests compare change.
"""
from __future__ import annotations

A = (317.25, 289.5, 171.5, 108.25, 41.0)
B = (268.5, 331.75, 149.25, 131.5, 23.5)
SQUARE = (300.0, 300.0, 160.0, 120.0, 30.0)  # proj_cases.FX FY CX CY BF
FRAME_CAMERAS = (A, B, SQUARE)
PAIR_CAMERAS = ((A, B), (B, A), (SQUARE, A))

P = (520.0, 430.0, 300.0, 255.0, 0.0)
Q = (415.0, 535.0, 335.0, 228.0, 0.0)
SIM3_SQUARE = (500.0, 500.0, 320.0, 240.0, 0.0)  # sim3_cases.F F CX CY
SIM3_PAIR_CAMERAS = ((P, Q), (Q, P), (SIM3_SQUARE, P))
SIM3_FRAME_CAMERAS = (P, Q, SIM3_SQUARE)  # the batch form: frame b is side 1 of pair b, frame train_src[b] its side 2


def intrinsics(cam):
    return tuple(cam[:4])


def swap_f(c):
    return (c[1], c[0]) + tuple(c[2:])


def swap_c(c):
    return (c[0], c[1], c[3], c[2]) + tuple(c[4:])


def with_bf(c, other):
    return tuple(c[:4]) + (other[4],)


FRAME_MIXUPS = {
    "fx and fy exchanged": lambda cams: [swap_f(c) for c in cams],
    "cx and cy exchanged": lambda cams: [swap_c(c) for c in cams],
    "every frame with frame 0's camera": lambda cams: [cams[0] for _ in cams],
    "every frame with its neighbour's camera": lambda cams: [cams[(b + 1) % len(cams)] for b in range(len(cams))],
    "bf of another frame": lambda cams: [with_bf(c, cams[(b + 1) % len(cams)]) for b, c in enumerate(cams)],
}

PROBLEM_ROW_MIXUP = "every problem with problem 0's camera row"


def frame_mixups(row: int):
    """FRAME_MIXUPS for a call whose problems each own `row` consecutive frames (the local bundle adjustment's keyframes), with one
    more: keyframe k of every problem read at views[k], not at views[first_frame + k].  It is a function of the row length, so it
    stands beside the table: the families that run one frame per problem iterate over FRAME_MIXUPS, where it would change nothing"""
    return dict(FRAME_MIXUPS, **{PROBLEM_ROW_MIXUP: lambda cams: [cams[b % row] for b in range(len(cams))]})


PAIR_MIXUPS = {
    "fx and fy exchanged": lambda pairs: [(swap_f(a), swap_f(b)) for a, b in pairs],
    "fx and fy exchanged on side 1": lambda pairs: [(swap_f(a), b) for a, b in pairs],
    "fx and fy exchanged on side 2": lambda pairs: [(a, swap_f(b)) for a, b in pairs],
    "cx and cy exchanged": lambda pairs: [(swap_c(a), swap_c(b)) for a, b in pairs],
    "every pair with pair 0's cameras": lambda pairs: [pairs[0] for _ in pairs],
    "every pair with its neighbour's cameras": lambda pairs: [pairs[(b + 1) % len(pairs)] for b in range(len(pairs))],
    "the sides exchanged": lambda pairs: [(b, a) for a, b in pairs],
    "side 1 on both sides": lambda pairs: [(a, a) for a, b in pairs],
    "side 2 on both sides": lambda pairs: [(b, b) for a, b in pairs],
}


def changed(cams, mixed, fields=(0, 1, 2, 3, 4)):
    """the frames (or pairs) of a call whose camera a mix-up changes in one of `fields`"""
    def flat(c):
        return [v for side in c for v in side] if isinstance(c[0], tuple) else list(c)

    def pick(c):
        f = flat(c)
        return [f[k + 5 * s] for s in range(len(f) // 5) for k in fields]
    return [b for b, (c, m) in enumerate(zip(cams, mixed)) if pick(c) != pick(m)]
