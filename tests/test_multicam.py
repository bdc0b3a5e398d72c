"""Several cameras in one batch: the table form of the batch matcher (ss_match_batch_sources_device).

Every query frame is matched against the train frame a per-frame table names -- a frame of the batch (earlier, later or
itself), no frame, or a frame of a carry kept from an earlier batch -- and the result must equal the CPU oracle's match
of that pair bit for bit, on each device path: the matrix-core matcher on expanded rows (chunked, and fused with
SENDSLAM_MX_CHUNKS=1), the packed matrix-core kernel (SENDSLAM_MATCH_PACKED=1) and the VALU kernel (fewer than 128 rows
per frame)."""
import os

import numpy as np
import pytest

from send_slam_amd import binding, synth

W, H = 320, 240
# two cameras' sequences, interleaved irregularly, plus a third whose frames only the carry holds
BATCH = [("a", 0), ("b", 0), ("a", 1), ("a", 2), ("b", 1), ("b", 2), ("a", 3), ("b", 3), ("b", 4), ("a", 4), ("a", 5), ("b", 5)]
CARRY = [("c", 0), ("a", 7), ("b", 7)]
SEEDS = {"a": 31, "b": 47, "c": 63}
# train of each batch frame: -1 none, a later frame (1), earlier ones, itself (5: the self pair is excluded), and the
# carry (-2 - c): the third camera's frame (7) and the two cameras' frames from before the batch (10, 11)
TABLE = [-1, 7, 0, 2, 1, 5, 3, -2, 7, 6, -3, -4]


def _frames(spec):
    return np.stack([synth.frame(SEEDS[cam], W, H, t=t) for cam, t in spec])


def _run(monkeypatch, env, n_features, n_levels):
    import torch
    for k in ("SENDSLAM_MATCH_PACKED", "SENDSLAM_MX_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda:0")
    carry_frames, frames = _frames(CARRY), _frames(BATCH)
    B, NC = len(frames), len(carry_frames)
    with binding.OrbContext(0, n_features=n_features, n_levels=n_levels, max_batch=16) as ctx:
        # the carry: an earlier batch's frames, uploaded as [n_carry][kp_capacity][32] with random bytes past each count
        ctx.extract_batch_device(torch.from_numpy(carry_frames).to(dev).data_ptr(), NC, W, H)
        ctx.synchronize()
        kcap = ctx.batch_view().kp_capacity
        carry = [ctx.fetch_frame(c)[1] for c in range(NC)]
        host = np.random.default_rng(5).integers(0, 256, size=(NC, kcap, 32), dtype=np.uint8)
        for c, d in enumerate(carry):
            host[c, :len(d)] = d
        d_carry = torch.from_numpy(host).to(dev)
        d_carry_n = torch.tensor([len(d) for d in carry], dtype=torch.int32, device=dev)

        ctx.extract_batch_device(torch.from_numpy(frames).to(dev).data_ptr(), B, W, H)
        ctx.synchronize()
        assert ctx.batch_view().kp_capacity == kcap
        desc = [ctx.fetch_frame(b)[1] for b in range(B)]
        outs = [torch.empty((B, kcap), dtype=t, device=dev) for t in (torch.int32, torch.int16, torch.int16)]

        def fetch():
            ctx.synchronize()
            return outs[0].cpu().numpy().copy(), outs[1].cpu().numpy().view(np.uint16).copy(), outs[2].cpu().numpy().view(np.uint16).copy()

        ptrs = [o.data_ptr() for o in outs]
        ctx.match_batch_sources_device(TABLE, *ptrs, d_carry=d_carry.data_ptr(), d_carry_n=d_carry_n.data_ptr(), n_carry=NC)
        got = fetch()
        # mode 1's rule as a table gives mode 1's output
        ctx.match_batch_device(1, *ptrs)
        mode1 = fetch()
        ctx.match_batch_sources_device([0] + list(range(B - 1)), *ptrs)
        table1 = fetch()
        # a table naming a frame that does not exist is refused
        for bad, nc in (([B] + [0] * (B - 1), NC), ([-2 - NC] + [0] * (B - 1), NC), ([-2] + [0] * (B - 1), 0), ([-2] * B, 0)):
            with pytest.raises(binding.OrbError) as e:
                ctx.match_batch_sources_device(bad, *ptrs, d_carry=d_carry.data_ptr(), d_carry_n=d_carry_n.data_ptr(), n_carry=nc)
            assert e.value.code == binding.SS_ERR_INVALID_ARG
    return kcap, desc, carry, got, mode1, table1


@pytest.mark.gpu
@pytest.mark.parametrize("form,env,nf,nl", [
    ("expanded_chunked", {}, 500, 8),
    ("expanded_fused", {"SENDSLAM_MX_CHUNKS": "1"}, 500, 8),
    ("packed_mfma", {"SENDSLAM_MATCH_PACKED": "1"}, 500, 8),
    ("valu", {}, 30, 3),
])
def test_table_matcher_equals_oracle(monkeypatch, oracle, form, env, nf, nl):
    kcap, desc, carry, got, mode1, table1 = _run(monkeypatch, env, nf, nl)
    assert (kcap < 128) == (form == "valu"), "the form under test is not the one the row count selects"
    assert all(len(d) > 20 for d in desc + carry)
    for b, t in enumerate(TABLE):
        n = len(desc[b])
        if t == -1:
            want = (np.full(n, -1, np.int32), np.full(n, 0xFFFF, np.uint16), np.full(n, 0xFFFF, np.uint16))
        elif t <= -2:
            want = oracle.match(desc[b], carry[-2 - t])
        else:
            want = oracle.match(desc[b], desc[t], exclude_self=(t == b))
        for a, w, name in zip(got, want, ("idx", "d1", "d2")):
            assert np.array_equal(a[b, :n], w), f"{form}: frame {b} (train {t}) {name}"
        assert (got[0][b, n:] == -1).all()
        if t != -1 and BATCH[b][0] == (BATCH[t] if t >= 0 else CARRY[-2 - t])[0]:
            assert (got[0][b, :n] >= 0).sum() > n // 10, f"frame {b}: too few matches for a meaningful comparison"
    for a, m in zip(table1, mode1):
        assert np.array_equal(a, m), f"{form}: the table of mode 1 differs from mode 1"


# ---- one context, several cameras: per-camera tracking -------------------------------------------------------------
TW, TH, TNF = 640, 480, 1000
TSEEDS = {1: 77, 2: 91}
TFX = {1: 500.0, 2: 505.0}
N_TRACK = 10
# irregular interleaving of the two cameras' frames
ORDER = [1, 2, 2, 1, 1, 2, 1, 2, 2, 2, 1, 1, 2, 1, 1, 2, 1, 2, 1, 2]


def _tcam(cam_id):
    return binding.Camera(type=b"PinHole", fx=TFX[cam_id], fy=TFX[cam_id], cx=320, cy=240, k1=-0.05, k2=0.01, p1=1e-4, p2=-1e-4,
                          width=TW, height=TH, fps=30, rgb=1, th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)


def _sequences():
    out = {}
    for cam, seed in TSEEDS.items():
        sc = synth.scene(seed, TW, TH)
        out[cam] = [synth.parallax_frame(seed, TW, TH, t, sc=sc) for t in range(N_TRACK + 1)]
    return out


def _assert_same_poses(got, want, what):
    assert [g["state"] for g in got] == [o["state"] for o in want], what
    for g, o in zip(got, want):
        for k in ("camera_id", "n_keypoints", "n_matches", "n_inliers", "n_map_points", "timestamp"):
            assert g[k] == o[k], f"{what}: {k}"
        assert np.array_equal(g["position"], o["position"]) and np.array_equal(g["quaternion"], o["quaternion"]), what


def _single_camera_poses(seqs, skip=()):
    """each camera on a context of its own: the poses per-camera tracking must reproduce (frames in `skip` not shown)"""
    want = {}
    for cam, frames in seqs.items():
        with binding.OrbContext(0, n_features=TNF) as ctx:
            ctx.set_calibration(cam, _tcam(cam))
            want[cam] = {t: ctx.track(img, cam, t / 30.0) for t, img in enumerate(frames) if (cam, t) not in skip}
    return want


@pytest.mark.gpu
def test_interleaved_cameras_track_like_separate_contexts(oracle):
    import track_ref
    from oracle import vo_oracle as vo
    seqs = _sequences()
    assert sorted(ORDER.count(c) for c in (1, 2)) == [N_TRACK, N_TRACK]
    want = _single_camera_poses(seqs)
    for cam in (1, 2):
        assert want[cam][N_TRACK - 1]["state"] == 2, f"camera {cam} does not reach tracking on its own"
    got = {1: [], 2: []}
    with binding.OrbContext(0, n_features=TNF) as ctx:
        ctx.set_calibration(1, _tcam(1))
        ctx.set_calibration(2, _tcam(2))
        for cam in ORDER:
            t = len(got[cam])
            got[cam].append(ctx.track(seqs[cam][t], cam, t / 30.0))
        for cam in (1, 2):
            _assert_same_poses(got[cam], [want[cam][t] for t in range(N_TRACK)], f"camera {cam}")
            # and the CPU restatement of the pose step on the oracle's features, to the existing track tests' tolerance
            ref = track_ref.run(oracle, seqs[cam][:N_TRACK], vo.Camera(TFX[cam], TFX[cam], 320.0, 240.0, -0.05, 0.01, 1e-4, -1e-4), TNF)
            for a, b in zip(got[cam], ref):
                assert (a["state"], a["n_matches"], a["n_inliers"], a["n_map_points"]) == \
                       (b["state"], b["n_matches"], b["n_inliers"], b["n_map_points"]), f"camera {cam} vs vo_oracle"
                assert np.allclose(a["position"], b["position"], rtol=0, atol=1e-6)
                assert np.allclose(a["quaternion"], b["quaternion"], rtol=0, atol=1e-6)
        # a calibration resets its own camera only: camera 2 starts again, camera 1 goes on as if alone
        ctx.set_calibration(2, _tcam(2))
        assert ctx.track(seqs[2][0], 2, 0.0)["state"] == want[2][0]["state"] != 2
        _assert_same_poses([ctx.track(seqs[1][N_TRACK], 1, N_TRACK / 30.0)], [want[1][N_TRACK]], "camera 1 after camera 2's calibration")
        # ss_track_reset resets every camera
        ctx.track_reset()
        for cam in (1, 2):
            assert ctx.track(seqs[cam][0], cam, 0.0)["state"] == want[cam][0]["state"]
        # SS_MAX_CAMERAS ids per context (8); the ninth is refused
        kps = np.empty(0, binding.KP_DTYPE)
        for cam in range(3, 9):
            ctx.track_features(0, kps, camera_id=cam)
        with pytest.raises(binding.OrbError) as e:
            ctx.track_features(0, kps, camera_id=9)
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "SS_MAX_CAMERAS" in e.value.message


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [(), ((2, 5),)])
def test_batched_table_matches_and_detach_track_like_separate_contexts(skip):
    """The read-ahead front door's path for several cameras: batches of interleaved frames extracted together, each frame
    matched against the previous frame of its own camera in the batch (table form), ss_track_features_matched with those
    matches where their train is the frame the camera's tracker saw last, the batch's rows referred to
    (SS_TRACK_DESC_STAYS_VALID) and detached before the next batch overwrites them.  == one context per camera, bit for
    bit -- also when a frame is skipped (a bad frame at the end of a batch: the next batch's first frame of that camera
    has no usable matches and the tracker matches on its own)."""
    import torch
    seqs = _sequences()
    want = _single_camera_poses(seqs, skip)
    stream, t_of = [], {1: 0, 2: 0}
    for cam in ORDER:
        stream.append((cam, t_of[cam]))
        t_of[cam] += 1
    B = 5
    assert stream[9] == (2, 5)  # the skipped frame ends the second batch
    dev = torch.device("cuda:0")
    got = {1: [], 2: []}
    with binding.OrbContext(0, n_features=TNF, max_batch=B) as ext, binding.OrbContext(0, n_features=TNF) as trk:
        trk.set_calibration(1, _tcam(1))
        trk.set_calibration(2, _tcam(2))
        last = {}  # camera -> position in `stream` of the frame its tracker saw last
        for b0 in range(0, len(stream), B):
            batch = stream[b0:b0 + B]
            d = torch.from_numpy(np.stack([seqs[c][t] for c, t in batch])).to(dev)
            ext.extract_batch_device(d.data_ptr(), len(batch), TW, TH)
            table = []
            for i, (c, _) in enumerate(batch):
                earlier = [j for j in range(i) if batch[j][0] == c]
                table.append(earlier[-1] if earlier else -1)
            v = ext.batch_view()
            kcap = v.kp_capacity
            outs = [torch.empty((len(batch), kcap), dtype=t, device=dev) for t in (torch.int32, torch.int16, torch.int16)]
            ext.match_batch_sources_device(table, *[o.data_ptr() for o in outs])
            ext.synchronize()
            idx, d1 = outs[0].cpu().numpy(), outs[1].cpu().numpy().view(np.uint16)
            for i, (c, t) in enumerate(batch):
                if (c, t) in skip:
                    continue
                kps = ext.fetch_frame(i)[0]
                n = len(kps)
                given = table[i] >= 0 and last.get(c) == b0 + table[i]
                got[c].append(trk.track_features_matched(v.descriptors + i * kcap * 32, kps, idx[i, :n] if given else None,
                                                         d1[i, :n] if given else None, desc_stays_valid=True, camera_id=c,
                                                         timestamp=t / 30.0))
                last[c] = b0 + i
            trk.track_detach()  # the next extraction overwrites the batch's rows
    for cam in (1, 2):
        _assert_same_poses(got[cam], [w for t, w in sorted(want[cam].items()) if t < N_TRACK], f"camera {cam}")
        assert got[cam][-1]["state"] == 2


# ---- the pipe's match_mode 2: each frame against the previous frame of its own camera ------------------------------
# three cameras over batches of 5: camera 3 once per batch (every train of it from the carry), a NULL frame (batch 1,
# position 3), and a submission that fails half-way (batch 3)
PIPE_BATCHES = [[1, 2, 1, 3, 2], [2, 2, 1, 1, 3], [1, 3, 2, 2, 1], [3, 1, 2, 1, 2], [1, 1, 2, 3, 2], [2, 3, 1, 2, 1]]
PIPE_NULL = (1, 3)
PIPE_FAIL = 3


@pytest.mark.gpu
def test_pipe_mode2_matches_each_frame_against_its_cameras_previous_frame(oracle):
    w, h, nf, B, depth = 320, 240, 500, 5, 3
    t_of, last, seq = {}, {}, 0
    expected, got = [], []

    def drain(pipe, everything=False):
        while pipe.in_flight() and (everything or pipe.in_flight() == depth):
            r = pipe.wait()
            n = r["n_keypoints"]
            got.append({"sequence": r["sequence"], "status": r["status"].copy(), "camera_id": r["camera_id"].copy(),
                        "desc": [r["descriptors"][i, :n[i]].copy() for i in range(r["n_frames"])],
                        "match": [(r["match_idx"][i, :n[i]].copy(), r["match_d1"][i, :n[i]].copy(), r["match_d2"][i, :n[i]].copy())
                                  for i in range(r["n_frames"])],
                        "src": list(zip(r["train_sequence"].tolist(), r["train_frame"].tolist()))})
            pipe.release(r["slot"])

    with binding.Pipe(0, w, h, batch=B, depth=depth, match_mode=2, n_features=nf) as pipe:
        for k, cams in enumerate(PIPE_BATCHES):
            frames = []
            for i, c in enumerate(cams):
                t_of[c] = t_of.get(c, -1) + 1
                frames.append(None if (k, i) == PIPE_NULL else synth.frame(SEEDS["abc"[c - 1]], w, h, t=t_of[c]))
            drain(pipe)
            if k == PIPE_FAIL:
                pipe.debug_inject_failure(7)  # after the match and the carry update were enqueued
                with pytest.raises(binding.OrbError):
                    pipe.submit_frames(frames, camera_ids=cams)
                last = {}  # the carry is emptied
                continue
            assert pipe.submit_frames(frames, camera_ids=cams)
            exp = []
            for i, (c, f) in enumerate(zip(cams, frames)):
                if f is None:
                    exp.append((-1, -1))
                    continue
                exp.append(last.get(c, (-1, -1)))
                last[c] = (seq, i)
            expected.append(exp)
            seq += 1
        drain(pipe, everything=True)

    assert [g["sequence"] for g in got] == list(range(len(expected)))
    desc_of = {(g["sequence"], i): d for g in got for i, d in enumerate(g["desc"])}
    for g, exp in zip(got, expected):
        assert g["src"] == exp, f"batch {g['sequence']}: sources"
        for i, (src, (idx, d1, d2)) in enumerate(zip(exp, g["match"])):
            if g["status"][i] != binding.SS_OK:
                continue
            if src == (-1, -1):
                assert (idx == -1).all() and (d1 == 0xFFFF).all() and (d2 == 0xFFFF).all()
                continue
            want = oracle.match(g["desc"][i], desc_of[src])
            for a, b_, name in zip((idx, d1, d2), want, ("idx", "d1", "d2")):
                assert np.array_equal(a, b_), f"batch {g['sequence']} frame {i} (camera {g['camera_id'][i]}, train {src}): {name}"
            assert (idx >= 0).sum() > len(idx) // 10
    # the NULL frame is nobody's train; camera 3's trains all come from the carry; after the failure no frame of the first
    # batch has a train from before it
    assert got[PIPE_NULL[0]]["status"][PIPE_NULL[1]] != binding.SS_OK
    for g in got:
        for i, c in enumerate(g["camera_id"]):
            if c == 3 and g["src"][i] != (-1, -1):
                assert g["src"][i][0] == g["sequence"] - 1
    after = got[PIPE_FAIL]
    assert all(s[0] in (-1, after["sequence"]) for s in after["src"])
    assert sum(s == (-1, -1) for s in after["src"]) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [(), ((2, 5),)])
def test_pipe_mode2_tracking_with_detach_like_separate_contexts(skip):
    """ss_track_features_matched on a mode-2 pipe's results: matches handed in where ss_pipe_match_sources names the frame
    the camera's tracker saw last, the slot's rows referred to (SS_TRACK_DESC_STAYS_VALID) and detached before the slot
    is released.  == one context per camera, bit for bit, also with a bad frame at the end of a batch."""
    seqs = _sequences()
    want = _single_camera_poses(seqs, skip)
    stream, t_of = [], {1: 0, 2: 0}
    for cam in ORDER:
        stream.append((cam, t_of[cam]))
        t_of[cam] += 1
    B, depth = 5, 3
    got = {1: [], 2: []}
    last = {}  # camera -> (sequence, index) of the frame its tracker saw last

    def consume(pipe, trk):
        r = pipe.wait()
        for i in range(r["n_frames"]):
            if r["status"][i] != binding.SS_OK:
                continue
            c, n = int(r["camera_id"][i]), int(r["n_keypoints"][i])
            src = (int(r["train_sequence"][i]), int(r["train_frame"][i]))
            given = src != (-1, -1) and last.get(c) == src
            got[c].append(trk.track_features_matched(r["d_descriptors"] + i * r["kp_capacity"] * 32, r["keypoints"][i, :n],
                                                     r["match_idx"][i, :n] if given else None, r["match_d1"][i, :n] if given else None,
                                                     desc_stays_valid=True, camera_id=c, timestamp=float(r["timestamp"][i])))
            last[c] = (int(r["sequence"]), i)
        trk.track_detach()
        pipe.release(r["slot"])

    with binding.Pipe(0, TW, TH, batch=B, depth=depth, match_mode=2, n_features=TNF) as pipe, \
            binding.OrbContext(0, n_features=TNF) as trk:
        trk.set_calibration(1, _tcam(1))
        trk.set_calibration(2, _tcam(2))
        for b0 in range(0, len(stream), B):
            if pipe.in_flight() == depth:
                consume(pipe, trk)
            batch = stream[b0:b0 + B]
            assert pipe.submit_frames([None if ct in skip else seqs[ct[0]][ct[1]] for ct in batch], camera_ids=[c for c, _ in batch],
                                      timestamps=[t / 30.0 for _, t in batch])
        while pipe.in_flight():
            consume(pipe, trk)
    for cam in (1, 2):
        _assert_same_poses(got[cam], [w for t, w in sorted(want[cam].items()) if t < N_TRACK], f"camera {cam}")
        assert got[cam][-1]["state"] == 2


# ---- the front door: one connection, the host's fan-out of two cameras ---------------------------------------------
def _frontdoor_run(host_cls, run_backend, cams, order, seqs, env):
    """a fake host sends calibrations of `cams`, then the frames of `order` restricted to `cams`, then terminate; -> the
    messages that came back, the exit code and the log"""
    from send_slam_amd import wire
    host = host_cls()
    b = run_backend(host, dict({"SENDSLAM_EMIT_FEATURES": "1"}, **env))
    try:
        host.accept()
        dims = {"width": TW, "height": TH, "channels": 1}
        for c in cams:
            host.send(wire.build_calibration_packet([[TFX[c], 0, 320], [0, TFX[c], 240], [0, 0, 1]], [-0.05, 0.01, 1e-4, -1e-4], dims,
                                                    camera_id=c))
        t_of = {}
        for c in order:
            t_of[c] = t_of.get(c, -1) + 1
            if c in cams:
                host.send(wire.build_frame_packet(wire.encode_to_ppm(seqs[c][t_of[c]]), dims, camera_id=c, timestamp=1.0 + t_of[c] / 30))
        host.send(wire.build_terminate_packet())
        msgs = host.recv_packets(1 << 30)  # until the front door closes the connection
        rc = b.wait(timeout=120)
    finally:
        host.close()
    return msgs, rc, b.logs(400)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("readahead", ["1", "4"], ids=["frame_by_frame", "read_ahead"])
def test_frontdoor_serves_two_interleaved_cameras(readahead):
    """One fake host sends calibrations of cameras 1 and 2 and their frames interleaved: each camera's answers (pose and
    features messages) equal those of a front door that saw only that camera.  SENDSLAM_CAMERAS=2 answers camera 2 only."""
    import subprocess
    from test_wire import FakeHost, ROOT, run_backend
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "send-slam_amd", "frontdoor"), "-s"])
    seqs = _sequences()
    env = {"SENDSLAM_READAHEAD": readahead}
    both, rc, log = _frontdoor_run(FakeHost, run_backend, (1, 2), ORDER, seqs, env)
    assert rc == 0, log
    single = {}
    for c in (1, 2):
        single[c], rc, log = _frontdoor_run(FakeHost, run_backend, (c,), ORDER, seqs, env)
        assert rc == 0, log
        assert sum(m["type"] == "features" for m in single[c]) == N_TRACK
        assert any(m.get("tracking_state") == 2 and m["type"] != "features" for m in single[c]), f"camera {c} never tracks"
    for c in (1, 2):
        assert [m for m in both if m["camera_id"] == c] == single[c], f"camera {c}"
    only2, rc, log = _frontdoor_run(FakeHost, run_backend, (1, 2), ORDER, seqs, dict(env, SENDSLAM_CAMERAS="2"))
    assert rc == 0, log
    assert only2 == single[2]
    assert log.count("Skipping camera 1: not in SENDSLAM_CAMERAS.") == 1


@pytest.mark.gpu
def test_pipe_mode2_voids_matches_against_a_flagged_train(monkeypatch, oracle):
    """A train the kernels flag (frame_error -> SS_ERR_OVERFLOW) voids the matches of the frames matched against it: in the
    batch and through the carry.  The flags come from the pipe's test hook SENDSLAM_TEST_FLAG_FRAMES, which reports chosen
    frames as flagged when their batch is returned (nothing overflows on the device)."""
    w, h, nf = 320, 240, 500
    batches = [[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 2, 1]]
    # batch 0: frame 1 (camera 2) is the in-batch train of frame 3; frame 2 (camera 1) is carried to batch 1's frame 1
    monkeypatch.setenv("SENDSLAM_TEST_FLAG_FRAMES", "0:1,0:2")
    t_of, got = {}, []
    with binding.Pipe(0, w, h, batch=4, depth=2, match_mode=2, n_features=nf) as pipe:
        for cams in batches:
            frames = []
            for c in cams:
                t_of[c] = t_of.get(c, -1) + 1
                frames.append(synth.frame(SEEDS["abc"[c - 1]], w, h, t=t_of[c]))
            if pipe.in_flight() == 2:
                r = pipe.wait()
                got.append(_copy_result(r))
                pipe.release(r["slot"])
            assert pipe.submit_frames(frames, camera_ids=cams)
        while pipe.in_flight():
            r = pipe.wait()
            got.append(_copy_result(r))
            pipe.release(r["slot"])
    overflow = binding.SS_ERR_OVERFLOW
    assert list(got[0]["status"]) == [binding.SS_OK, overflow, overflow, binding.SS_OK]
    want_src = [[(-1, -1), (-1, -1), (-1, -1), (-1, -1)],   # 3: its train (frame 1) was flagged
                [(0, 3), (-1, -1), (1, 0), (1, 1)],         # 1: its carry train (0, 2) was flagged
                [(1, 3), (1, 2), (2, 1), (2, 0)]]
    desc_of = {(g["sequence"], i): d for g in got for i, d in enumerate(g["desc"])}
    for g, exp in zip(got, want_src):
        assert g["src"] == exp, f"batch {g['sequence']}"
        for i, src in enumerate(exp):
            idx, d1, d2 = g["match"][i]
            if src == (-1, -1):
                assert (idx == -1).all()
                continue
            want = oracle.match(g["desc"][i], desc_of[src])
            for a, b_ in zip((idx, d1, d2), want):
                assert np.array_equal(a, b_), f"batch {g['sequence']} frame {i}"
    assert len(got[0]["match"][3][0]) > 20 and len(got[1]["match"][1][0]) > 20  # the voided frames had keypoints to match


def _copy_result(r):
    n = r["n_keypoints"]
    return {"sequence": r["sequence"], "status": r["status"].copy(),
            "desc": [r["descriptors"][i, :n[i]].copy() for i in range(r["n_frames"])],
            "match": [(r["match_idx"][i, :n[i]].copy(), r["match_d1"][i, :n[i]].copy(), r["match_d2"][i, :n[i]].copy())
                      for i in range(r["n_frames"])],
            "src": list(zip(r["train_sequence"].tolist(), r["train_frame"].tolist()))}
