"""The pairs, rigs and couples the tests of the stereo form of the triangulation share (test infrastructure, plain module)."""
from __future__ import annotations

import functools

import numpy as np

import camera_cases as CC
import epi_ref as E
import guided_cases as G
import proj_cases as PC
import tri_stereo_ref as T

F, ROWS = 3, 70
B = 0.1                                   # the rigs' baseline in metres
TP = dict(T.UPSTREAM)
# keyframe 2 of a pair against keyframe 1: a wide baseline (the rays' parallax beats the rig's: mode 0), and a step of 2 cm (it does
# not: the unprojection modes)
MOVES = [((0.004, -0.003, 0.002), (-0.6, 0.02, 0.03)), ((-0.002, 0.003, 0.001), (-0.02, 0.0, 0.005)), ((0.003, 0.002, -0.002), (-0.02, 0.01, 0.0))]


def scale():
    return np.array(PC.scale(), np.float32)


def binding_camera(cam):
    from send_slam_amd import binding
    return binding.Camera(fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], width=G.W, height=G.H)


def poses(k: int):
    (ax, ay, az), t = MOVES[k]
    return (np.eye(3), np.zeros(3)), (PC.rot(ax, ay, az), np.array(t))


def rig_of(cam1, cam2):
    return dict(bf1=B * cam1[0], b1=B, bf2=B * cam2[0], b2=B)


def ref_pair(k: int, cams=CC.PAIR_CAMERAS):
    (r1, t1), (r2, t2) = poses(k)
    return E.pair_init(CC.intrinsics(cams[k][0]), r1, t1, CC.intrinsics(cams[k][1]), r2, t2)


def twin_pair(k: int, cams=CC.PAIR_CAMERAS):
    from send_slam_amd import binding
    (r1, t1), (r2, t2) = poses(k)
    return binding.epi_pair(binding_camera(cams[k][0]), r1, t1, binding_camera(cams[k][1]), r2, t2)


def twin_rig(rig):
    from send_slam_amd import binding
    return binding.TriStereoRig(**rig)


def twin_params(tp=None):
    from send_slam_amd import binding
    tp = TP if tp is None else tp
    p = binding.TriStereoParams()
    p.tri.cos_parallax_max, p.tri.chi2, p.tri.ratio_factor, p.tri.far_limit, p.chi2_stereo = (tp[k] for k in ("cos_parallax_max", "chi2", "ratio_factor",
                                                                                                           "far_limit", "chi2_stereo"))
    return p


def _project(cam, R, t, X, rng, noise):
    from send_slam_amd import binding
    Xc = X @ np.asarray(R).T + np.asarray(t)
    kp = np.zeros(len(X), binding.KP_DTYPE)
    kp["x"] = cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2] + rng.normal(0, noise, len(X))
    kp["y"] = cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3] + rng.normal(0, noise, len(X))
    kp["octave"] = rng.integers(0, 3, len(X))
    kp["size"], kp["angle"], kp["response"] = 31.0, rng.uniform(0, 360, len(X)), rng.uniform(7, 200, len(X))
    depth = Xc[:, 2].astype(np.float32)
    right = (kp["x"] - np.float32(B * cam[0]) / depth + rng.normal(0, noise, len(X))).astype(np.float32)
    return kp, depth, right


@functools.lru_cache(maxsize=None)
def pair_case(k: int, rows: int = ROWS):
    """pair k -> dict: q_kp, t_kp [rows] (row i of the query is the same world point as row idx[i] of the train), q_desc, idx, and the
    depth / right planes of both sides with a mix of mono rows (-1 in both planes), rows that are stereo on one side and on both;
    a few rows carry an octave outside the table, a NaN right coordinate, or no match"""
    rng = np.random.Generator(np.random.PCG64(0x7515 + k))
    cam1, cam2 = CC.PAIR_CAMERAS[k]
    (r1, t1), (r2, t2) = poses(k)
    X = np.stack([rng.uniform(-1.5, 1.5, rows), rng.uniform(-1.0, 1.0, rows), rng.uniform(2.0, 9.0, rows)], 1)
    q_kp, d1, u1 = _project(cam1, r1, t1, X, rng, 0.3)
    perm = rng.permutation(rows)
    t_kp, d2, u2 = _project(cam2, r2, t2, X[perm], rng, 0.3)
    idx = np.argsort(perm).astype(np.int32)  # train row of query row i
    kind1, kind2 = rng.integers(0, 2, rows), rng.integers(0, 2, rows)  # 0 mono, 1 stereo
    kind1[20] = 1
    d1[kind1 == 0], u1[kind1 == 0] = -1.0, -1.0
    d2[kind2 == 0], u2[kind2 == 0] = -1.0, -1.0
    u1[5], q_kp["octave"][9], t_kp["octave"][idx[12]] = np.nan, 8, -1
    u1[20] += 9.0   # a right coordinate three pixels and more off: the three-term error rejects where the two-term would not
    idx[3], idx[17] = -1, rows + 5
    return dict(q_kp=q_kp, t_kp=t_kp, q_desc=rng.integers(0, 256, (rows, 32), dtype=np.uint8), idx=idx, depth1=d1, right1=u1, depth2=d2, right2=u2,
                rig=rig_of(cam1, cam2))


def reference_rows(k: int, mono: bool = False, tp=None):
    """pair k from its matches by the reference -> (INFO_DTYPE [rows], MAP_POINT_DTYPE [rows]); rows without a match: state -1"""
    c, tp = pair_case(k), TP if tp is None else tp
    w, sc = E.PairD(ref_pair(k)), scale()
    info, pts = np.zeros(ROWS, T.INFO_DTYPE), np.zeros(ROWS, T.MAP_POINT_DTYPE)
    info["state"], info["mode"] = -1, -1
    for i in range(ROWS):
        j = int(c["idx"][i])
        if 0 <= j < ROWS:
            d1, u1, d2, u2 = (-1.0, -1.0, -1.0, -1.0) if mono else (c["depth1"][i], c["right1"][i], c["depth2"][j], c["right2"][j])
            info[i], pts[i] = T.triangulate(w, c["rig"], tp, sc, c["q_kp"]["x"][i], c["q_kp"]["y"][i], c["q_kp"]["octave"][i], d1, u1,
                                            c["t_kp"]["x"][j], c["t_kp"]["y"][j], c["t_kp"]["octave"][j], d2, u2)
    return info, pts


def twin_rows(k: int, mono: bool = False, tp=None):
    """the same by ss_triangulate_stereo_host on the matched couples"""
    from send_slam_amd import binding
    c = pair_case(k)
    ok = np.flatnonzero((c["idx"] >= 0) & (c["idx"] < ROWS))
    j = c["idx"][ok]
    planes = (None,) * 4 if mono else (c["depth1"][ok], c["right1"][ok], c["depth2"][j], c["right2"][j])
    pts_ok, info_ok = binding.triangulate_stereo_host(twin_pair(k), twin_rig(c["rig"]), twin_params(tp), scale(), c["q_kp"][ok], c["t_kp"][j], *planes)
    info, pts = np.zeros(ROWS, binding.TRI_STEREO_INFO_DTYPE), np.zeros(ROWS, binding.MAP_POINT_DTYPE)
    info["state"], info["mode"] = -1, -1
    info[ok], pts[ok] = info_ok, pts_ok
    return info, pts


def summary_of(info, n_train: int = ROWS):
    s = info["state"]
    return dict(status=0, n_query=len(info), n_train=n_train, n_matches=int((s != -1).sum()), n_points=int((s == 0).sum()),
                n_state=[int((s == v).sum()) for v in range(11)], n_mode=[int(((s == 0) & (info["mode"] == m)).sum()) for m in range(3)])
