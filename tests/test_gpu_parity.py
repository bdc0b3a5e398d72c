"""GPU parity tests proper: the HIP path, called through the C ABI, against (a) the committed
golden vectors and (b) the CPU oracle on the same seeded inputs.  Bar: bit-exact for every
integer / byte / index result AND for the float keypoint fields (they are produced by
restated single IEEE operations, tests/test_float_steps.py).

Run on an MI355X:  python -m pytest tests/ -x -q -m gpu
"""
import glob
import hashlib
import os

import numpy as np
import pytest

from send_slam_amd import binding, synth

pytestmark = pytest.mark.gpu


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def triples(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def pts(a):
    return [(int(r["x"]), int(r["y"]), int(r["response"])) for r in a]


def level_dims(ctx, w, h, oracle):
    p = oracle.default_params(n_features=ctx.params.n_features)
    g = oracle.geometry(p, w, h)
    return [(g.w[l], g.h[l]) for l in range(g.n_levels)]


def check_golden_stages(ctx, z, oracle):
    """ctx.extract(z's frame), then every stage of every level, the outputs and the self-match against the golden vectors"""
    img = z["frame"]
    h, w = img.shape
    kps, desc, counts = ctx.extract(img)
    dims = level_dims(ctx, w, h, oracle)
    for l, (lw, lh) in enumerate(dims):
        lvl = ctx.debug_fetch(0, 0, l, (lh, lw))
        assert np.array_equal(sha(lvl), z["level_sha"][l]), f"pyramid level {l}"
        blr = ctx.debug_fetch(1, 0, l, (lh, lw))
        assert np.array_equal(sha(blr), z["blur_sha"][l]), f"blurred level {l}"
        sc = ctx.debug_fetch(2, 0, l, (lh, lw))
        assert np.array_equal(sha(sc), z["score7_sha"][l]), f"FAST score map level {l}"
        cand = ctx.debug_fetch(3, 0, l, (lw * lh,), np.int32)
        assert triples(cand) == pts(z[f"cand{l}"]), f"candidates level {l}"
        sel = ctx.debug_fetch(4, 0, l, (4096 * 3,), np.int32)
        want = [(x + 16, y + 16, r) for x, y, r in pts(z[f"sel{l}"])]
        assert triples(sel) == want, f"quadtree level {l}"
    assert np.array_equal(counts, z["level_counts"])
    assert kps.tobytes() == z["kps"].tobytes()
    assert np.array_equal(desc, z["desc"])
    idx, d1, d2 = ctx.match(desc, desc, exclude_self=True)
    assert np.array_equal(idx, z["self_idx"]) and np.array_equal(d1, z["self_d1"]) and np.array_equal(d2, z["self_d2"])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))))
def test_golden_vectors_stage_by_stage(path, oracle):
    z = np.load(path)
    lap = z["lapping"]
    with binding.OrbContext(0, n_features=int(z["n_features"]), lapping_x0=int(lap[0]), lapping_x1=int(lap[1])) as ctx:
        check_golden_stages(ctx, z, oracle)


def test_stages_across_a_geometry_change(oracle, golden_dir):
    """One context through 320x240 -> 400x260 -> 320x240: every buffer of the extraction is freed and allocated again from the
    buffer table at each change of size, the FAST score map included (which each size's first debug_fetch(2) allocates).
    Every stage of every level, the keypoints, descriptors and level counts are checked at each size; all of it equality."""
    from test_adversarial_content import check_stages
    z = np.load(os.path.join(golden_dir, "g0_320x240_n500.npz"))
    assert int(z["n_features"]) == 500 and list(z["lapping"]) == [0, 1000]  # the context below is the one g0 was made with
    with binding.OrbContext(0, n_features=500) as ctx:
        check_golden_stages(ctx, z, oracle)
        check_stages(oracle, binding, synth.frame(31, 400, 260), "after 320x240", n_features=500, ctx=ctx)
        check_golden_stages(ctx, z, oracle)


def test_golden_consecutive_frame_match():
    here = os.path.join(os.path.dirname(__file__), "golden")
    a, b = np.load(os.path.join(here, "g0_320x240_n500.npz")), np.load(os.path.join(here, "g0t1_320x240_n500.npz"))
    with binding.OrbContext(0) as ctx:
        idx, d1, d2 = ctx.match(a["desc"], b["desc"])
    assert np.array_equal(idx, b["prev_idx"]) and np.array_equal(d1, b["prev_d1"]) and np.array_equal(d2, b["prev_d2"])


@pytest.mark.parametrize("seed,w,h,nf,nl", [(3, 640, 480, 1250, 8), (4, 1280, 720, 2000, 8), (5, 333, 517, 700, 8),
                                            (6, 1920, 1080, 2000, 8), (7, 323, 243, 300, 8), (8, 640, 480, 6250, 8),
                                            (9, 131, 99, 200, 3), (10, 640, 480, 40, 8), (11, 800, 600, 1000, 1)])
def test_extract_bit_exact_vs_oracle(oracle, seed, w, h, nf, nl):
    # 640x480/1250 = config 1 of BASELINE.json, 1280x720/2000 = the metric config,
    # 1920x1080 = config 4; 6250 = the 5 x nFeatures extractor of monocular initialisation;
    # 243 px high is the smallest image 8 levels admit; 40 features gives per-level quotas of 4..9
    img = synth.frame(seed, w, h)
    with binding.OrbContext(0, n_features=nf, n_levels=nl) as ctx:
        kps, desc, counts = ctx.extract(img)
    okps, odesc, ocounts = oracle.extract(img, oracle.default_params(n_features=nf, n_levels=nl))
    assert np.array_equal(counts, ocounts)
    assert len(kps) == len(okps)
    for f in ("octave", "response", "x", "y", "size", "angle"):
        bad = np.nonzero(kps[f].view(np.uint32) != okps[f].view(np.uint32))[0]
        assert len(bad) == 0, f"{f}: {len(bad)} keypoints differ, first {bad[:5]}"
    assert np.array_equal(desc, odesc)


def test_low_contrast_falls_back_to_min_threshold(oracle):
    img = (synth.frame(9, 400, 300).astype(np.int32) // 6 + 90).astype(np.uint8)
    with binding.OrbContext(0, n_features=400) as ctx:
        kps, desc, counts = ctx.extract(img)
    okps, odesc, ocounts = oracle.extract(img, oracle.default_params(n_features=400))
    assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)
    assert (kps["response"] < 20).any()


def test_flat_image_yields_nothing():
    img = np.full((240, 320), 128, np.uint8)
    with binding.OrbContext(0) as ctx:
        kps, desc, counts = ctx.extract(img)
    assert len(kps) == 0 and counts.sum() == 0


def test_colour_input_uses_calibration_rgb_flag(oracle):
    col = synth.color_frame(10, 320, 240)
    for rgb in (1, 0):
        cam = binding.Camera(type=b"PinHole", fx=500, fy=500, cx=160, cy=120, width=320, height=240, fps=30, rgb=rgb,
                             th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
        with binding.OrbContext(0, n_features=400) as ctx:
            with pytest.raises(binding.OrbError) as e:
                ctx.extract(col)  # frame before calibration (shim :523-527)
            assert e.value.code == binding.SS_ERR_NOT_CALIBRATED
            ctx.set_calibration(1, cam)
            kps, desc, _ = ctx.extract(col)
            gray = ctx.debug_fetch(0, 0, 0, (240, 320)).reshape(240, 320)
        og = oracle.gray(col, rgb)
        assert np.array_equal(gray, og)
        okps, odesc, _ = oracle.extract(og, oracle.default_params(n_features=400))
        assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)


def test_four_channel_input_ignores_alpha(oracle):
    """RGBA / BGRA frames: GrabImageMonocular uses RGBA2GRAY / BGRA2GRAY, the same weights, alpha unused."""
    col = synth.color_frame(12, 320, 240)
    rgba = np.concatenate([col, np.random.default_rng(0).integers(0, 256, (240, 320, 1), dtype=np.uint8)], axis=2)
    cam = binding.Camera(type=b"PinHole", fx=500, fy=500, cx=160, cy=120, width=320, height=240, fps=30, rgb=1,
                         th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
    with binding.OrbContext(0, n_features=400) as ctx:
        ctx.set_calibration(1, cam)
        k4, d4, _ = ctx.extract(rgba)
        k3, d3, _ = ctx.extract(col)
    assert k4.tobytes() == k3.tobytes() and np.array_equal(d4, d3)
    okps, odesc, _ = oracle.extract(oracle.gray(np.ascontiguousarray(rgba), 1), oracle.default_params(n_features=400))
    assert k4.tobytes() == okps.tobytes() and np.array_equal(d4, odesc)


def test_errors_leave_the_context_usable(oracle):
    img = synth.frame(11, 320, 240)
    with binding.OrbContext(0, n_features=300) as ctx:
        with pytest.raises(binding.OrbError) as e:
            ctx.extract(np.zeros((60, 60), np.uint8))
        assert e.value.code == binding.SS_ERR_TOO_SMALL
        with pytest.raises(binding.OrbError) as e:
            ctx.extract(img, camera_id=0)  # "Frame message missing camera identifier." (shim :528)
        assert e.value.code == binding.SS_ERR_BAD_FRAME
        kps, desc, _ = ctx.extract(img)
        okps, odesc, _ = oracle.extract(img, oracle.default_params(n_features=300))
        assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)
    with pytest.raises(binding.OrbError) as e:
        binding.OrbContext(0, n_levels=0)
    assert e.value.code == binding.SS_ERR_INVALID_ARG


# from 128 query rows on, ssk_match launches a planned ssk_match_call on a matrix-core kernel (256 queries per block, 64 per wave,
# 32-row train tiles):
# sizes on both sides of each of those boundaries, empty / one-row / one-tile train sets, and the self-match of each
@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (63, 64), (64, 65), (65, 63), (2000, 2000), (257, 5000), (40, 0),
                                   (127, 127), (128, 128), (129, 31), (128, 1), (255, 33), (256, 256), (300, 0),
                                   (321, 321), (512, 95), (1000, 4097)])
def test_match_ragged_sizes_vs_oracle(oracle, nq, nt):
    rng = np.random.default_rng(nq * 7919 + nt)
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    if nt > 3:
        t[nt // 2] = q[0]
        t[nt // 2 + 1] = q[0]  # duplicate best: tie -> lowest index, d2 == d1
        t[1] = q[nq - 1]
        t[1, 3] ^= 0x10
    with binding.OrbContext(0) as ctx:
        for kw in (dict(th=50, ratio_num=9), dict(th=256, ratio_num=10), dict(th=100, ratio_num=7)):
            got = ctx.match(q, t, ratio_den=10, **kw)
            want = oracle.match(q, t, ratio_den=10, **kw)
            for a, b, name in zip(got, want, ("idx", "d1", "d2")):
                assert np.array_equal(a, b), f"{name} differs ({kw})"
        if nt == nq:
            got = ctx.match(q, q, th=256, ratio_num=10, exclude_self=True)
            want = oracle.match(q, q, th=256, ratio_num=10, exclude_self=True)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)


def test_match_random_sizes_vs_oracle(oracle):
    # seeded sweep over both matcher kernels: sizes around every tiling boundary drawn at random, low-entropy descriptors
    # (few distinct bytes) so that distance ties -- the lowest-index rule -- and d1 == d2 are everywhere, self-matches
    rng = np.random.default_rng(int(os.environ.get("SENDSLAM_SOAK_SEED", 4242)))
    with binding.OrbContext(0) as ctx:
        for case in range(int(os.environ.get("SENDSLAM_SOAK_CASES", 60))):
            nq = int(rng.choice([rng.integers(1, 128), rng.integers(128, 700), rng.choice([128, 160, 256, 384, 512])]))
            nt = int(rng.choice([rng.integers(0, 70), rng.integers(70, 3000), rng.choice([32, 64, 96, 1024, 2048])]))
            vals = rng.integers(0, 256, size=int(rng.integers(2, 6)), dtype=np.uint8)
            lowent = case % 3 == 0
            q = (vals[rng.integers(0, len(vals), size=(nq, 32))] if lowent else rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)).astype(np.uint8)
            t = (vals[rng.integers(0, len(vals), size=(nt, 32))] if lowent else rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)).astype(np.uint8)
            kw = dict(th=int(rng.choice([50, 100, 256])), ratio_num=int(rng.choice([7, 9, 10])), ratio_den=10)
            got = ctx.match(q, t, **kw)
            want = oracle.match(q, t, **kw)
            for a, b, name in zip(got, want, ("idx", "d1", "d2")):
                assert np.array_equal(a, b), f"case {case}: {name} differs (nq={nq}, nt={nt}, {kw})"
            if case % 2 == 0:
                got = ctx.match(q, q, exclude_self=True, **kw)
                want = oracle.match(q, q, exclude_self=True, **kw)
                for a, b, name in zip(got, want, ("idx", "d1", "d2")):
                    assert np.array_equal(a, b), f"case {case}: self-match {name} differs (nq={nq}, {kw})"


def test_match_self_exclusion_in_the_large_database_form():
    # the two-tiles-per-wave form of the matrix-core kernel (one frame, >= 65 536 train rows) with j == i excluded: a
    # 66 000-row self-match, checked for a sample of queries against distances computed here with numpy (the oracle's
    # exclusion is by query index, so it cannot check a subset)
    rng = np.random.default_rng(99)
    n = 66_000
    q = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    q[40_000] = q[5]            # an exact copy far away: d1 == 0 for both
    q[65_999] = q[65_536]
    q[65_998] = q[65_536]       # two copies: tie, lowest index wins
    sel = [0, 5, 31, 32, 63, 64, 127, 128, 255, 256, 40_000, 65_535, 65_536, 65_998, 65_999]
    with binding.OrbContext(0) as ctx:
        idx, d1, d2 = ctx.match(q, q, th=-1, ratio_num=10, exclude_self=True)  # raw mode: best row, no acceptance test
    popc = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
    for i in sel:
        d = popc[q ^ q[i]].sum(1)
        d[i] = 1 << 20
        j = int(np.argmin(d))  # first minimum = lowest index
        rest = np.delete(d, j)
        assert (int(idx[i]), int(d1[i]), int(d2[i])) == (j, int(d[j]), int(rest.min())), i
    assert d1[5] == 0 and idx[5] == 40_000 and idx[40_000] == 5 and idx[65_536] == 65_998 and d2[65_536] == 0


def test_match_large_database_chunked(oracle):
    # loop-closure shape (config 5 of BASELINE.json, scaled down): many train chunks, ties across chunks
    rng = np.random.default_rng(77)
    q = rng.integers(0, 256, size=(300, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(150000, 32), dtype=np.uint8)
    for k, pos in enumerate((5, 70000, 140001)):  # the same exact match in three far-apart chunks
        t[pos] = q[7]
    t[149999] = q[11]
    with binding.OrbContext(0) as ctx:
        got = ctx.match(q, t, th=256, ratio_num=10)
    want = oracle.match(q, t, th=256, ratio_num=10)
    for a, b, name in zip(got, want, ("idx", "d1", "d2")):
        assert np.array_equal(a, b), name
    assert got[1][7] == 0 and got[2][7] == 0 and got[1][11] == 0 and got[0][11] == 149999


def test_match_config5_full_database_chunks_at_the_index_limit(oracle):
    # BASELINE.json config 5 at full size: 2000 query descriptors against 20 M rows (640 MB).  The chunk planner
    # then hands the matrix-core kernel chunks at its 16-bit local-row limit (65 376 rows), the case no smaller
    # database reaches; ties are planted on both sides of chunk boundaries and at the two ends.  The oracle checks a
    # subset of the (independent) queries.
    rng = np.random.default_rng(2025)
    nq, nt = 2000, 20_000_000
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    for pos in (65375, 65376, 130751, 130752, 19_999_999):
        t[pos] = q[3]           # first of five exact copies must win, d2 == 0
    t[0] = q[1999]
    t[19_999_998] = q[1999]
    t[65535], t[65536] = q[64], q[64]
    t[65535, 0] ^= 1            # distance 1 just below a 2^16 row index, distance 0 just above it
    sel = np.array([0, 1, 2, 3, 63, 64, 65, 255, 256, 1000, 1998, 1999])
    with binding.OrbContext(0) as ctx:
        got = ctx.match(q, t, th=256, ratio_num=10)
        raw = ctx.match(q, t, th=-1, ratio_num=10)  # raw mode: the best row even where the ratio test rejects a tie
    want = oracle.match(np.ascontiguousarray(q[sel]), t, th=256, ratio_num=10)
    for a, b, name in zip(got, want, ("idx", "d1", "d2")):
        assert np.array_equal(a[sel], b), name
    assert got[0][3] == -1 and got[1][3] == 0 and got[2][3] == 0 and raw[0][3] == 65375
    assert got[0][1999] == -1 and got[2][1999] == 0 and raw[0][1999] == 0
    assert got[0][64] == 65536 and got[1][64] == 0 and got[2][64] == 1


def test_batch_device_path_matches_single_frame_path(oracle):
    import torch
    w, h, nf, B = 640, 480, 1000, 5
    frames = np.stack([synth.frame(20 + b // 2, w, h, t=b % 2) for b in range(B)])
    dev = torch.device("cuda:0")
    d = torch.from_numpy(frames).to(dev)
    with binding.OrbContext(0, n_features=nf, max_batch=8) as ctx:
        ctx.extract_batch_device(d.data_ptr(), B, w, h)
        ctx.synchronize()
        v = ctx.batch_view()
        kcap = v.kp_capacity
        idx = torch.empty((B, kcap), dtype=torch.int32, device=dev)
        d1 = torch.empty((B, kcap), dtype=torch.int16, device=dev)
        d2 = torch.empty((B, kcap), dtype=torch.int16, device=dev)
        res = {}
        for mode in (0, 1):
            ctx.match_batch_device(mode, idx.data_ptr(), d1.data_ptr(), d2.data_ptr())
            ctx.synchronize()
            res[mode] = (idx.cpu().numpy().copy(), d1.cpu().numpy().view(np.uint16).copy(),
                         d2.cpu().numpy().view(np.uint16).copy())
        fetched = [ctx.fetch_frame(b) for b in range(B)]
    p = oracle.default_params(n_features=nf)
    prev = None
    for b in range(B):
        okps, odesc, ocounts = oracle.extract(frames[b], p)
        kps_b, desc_b, counts_b = fetched[b]
        n = len(kps_b)
        assert n == len(okps) and np.array_equal(counts_b, ocounts)
        assert kps_b.tobytes() == okps.tobytes()
        assert np.array_equal(desc_b, odesc)
        want = oracle.match(odesc, odesc, exclude_self=True)
        for a, bb in zip(res[0], want):
            assert np.array_equal(a[b, :n], bb)
        assert (res[0][0][b, n:] == -1).all()
        want = oracle.match(odesc, odesc, exclude_self=True) if b == 0 else oracle.match(odesc, prev)
        for a, bb in zip(res[1], want):
            assert np.array_equal(a[b, :n], bb)
        prev = odesc


@pytest.mark.parametrize("w,stride,offset", [(330, 336, 0), (336, 336, 0), (330, 352, 16), (330, 333, 0), (320, 320, 4)])
def test_batch_device_strides_and_alignments(oracle, w, stride, offset):
    """Device batches with padded rows and odd base addresses: the 16-byte ingest path (aligned base and
    strides, including a last partial 16-px group) and the byte path give the oracle's result."""
    import torch
    h, nf, B = 250, 400, 3
    frames = np.stack([synth.frame(60 + b, w, h) for b in range(B)])
    buf = np.full((B * h * stride + 64,), 0xA5, np.uint8)
    for b in range(B):
        for y in range(h):
            o = offset + (b * h + y) * stride
            buf[o:o + w] = frames[b, y]
    d = torch.from_numpy(buf).to("cuda:0")
    assert d.data_ptr() % 256 == 0
    with binding.OrbContext(0, n_features=nf, max_batch=4) as ctx:
        ctx.extract_batch_device(d.data_ptr() + offset, B, w, h, 1, stride, h * stride)
        got = [ctx.fetch_frame(b) for b in range(B)]
    p = oracle.default_params(n_features=nf)
    for b in range(B):
        okps, odesc, _ = oracle.extract(frames[b], p)
        assert got[b][0].tobytes() == okps.tobytes() and np.array_equal(got[b][1], odesc)


def test_random_geometries_and_contents_vs_oracle(oracle):
    """Seeded sweep over image sizes, feature counts, level counts, scale factors and contents (textured,
    half flat, low contrast, noise): every tile / cell-window / bucket geometry the kernels index blindly is
    exercised against the oracle, bit for bit."""
    # SENDSLAM_SOAK_CASES / SENDSLAM_SOAK_SEED: a longer run of the same sweep with other draws (by hand, on a GPU box)
    rng = np.random.default_rng(int(os.environ.get("SENDSLAM_SOAK_SEED", 20261004)))
    checked = 0
    for case in range(int(os.environ.get("SENDSLAM_SOAK_CASES", 28))):
        w, h = int(rng.integers(200, 900)), int(rng.integers(170, 700))
        nl = int(rng.integers(2, 9))
        scale = float(rng.choice([1.1, 1.15, 1.2, 1.25, 1.5]))  # <= 1.2: the LDS resize kernel (other tap spacings), above: the direct one
        nf = int(rng.integers(80, 1500))
        img = synth.frame(100 + case, w, h).astype(np.int32)
        kind = case % 4
        if kind == 1:
            img[:, : w // 2] = 128  # half flat: empty cells next to busy ones
        elif kind == 2:
            img = 120 + (img - 120) // 6  # low contrast: the minTh retry everywhere
        elif kind == 3:
            img = img + rng.integers(-25, 26, size=img.shape)  # heavy noise: many corners per tile
        img = np.clip(img, 0, 255).astype(np.uint8)
        p = oracle.default_params(n_features=nf, n_levels=nl, scale_factor=scale)
        try:
            okps, odesc, ocounts = oracle.extract(img, p)
        except (ValueError, RuntimeError):
            # too small for this many levels: the product refuses it too, loudly
            with binding.OrbContext(0, n_features=nf, n_levels=nl, scale_factor=scale) as ctx:
                with pytest.raises(binding.OrbError) as e:
                    ctx.extract(img)
            assert e.value.code == binding.SS_ERR_TOO_SMALL, (case, w, h, nl, scale)
            continue
        with binding.OrbContext(0, n_features=nf, n_levels=nl, scale_factor=scale) as ctx:
            kps, desc, counts = ctx.extract(img)
        assert np.array_equal(counts, ocounts), (case, w, h, nf, nl, scale)
        assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc), (case, w, h, nf, nl, scale)
        checked += 1
    assert checked >= 15


def test_full_size_properties_metric_config():
    """BASELINE.json metric config (1280x720, 2000 kp): size-independent properties."""
    img = synth.frame(30, 1280, 720)
    with binding.OrbContext(0, n_features=2000) as ctx:
        k1, d1, c1 = ctx.extract(img)
        k2, d2, c2 = ctx.extract(img)  # idempotence / determinism
        assert k1.tobytes() == k2.tobytes() and np.array_equal(d1, d2)
        assert 1990 <= len(k1) <= 2000 + 3 * 8
        # every keypoint lies >= 19 px inside its level; angles in [0, 360]
        assert k1["angle"].min() >= 0 and k1["angle"].max() <= 360
        idx, m1, m2 = ctx.match(d1, d1, th=256, ratio_num=10, exclude_self=True)
        assert (m1 <= m2).all() and (idx != np.arange(len(d1))).all()
        # best distance is symmetric-consistent: d(i, idx[i]) == m1[i]
        ok = idx >= 0
        x = np.unpackbits(d1[ok] ^ d1[idx[ok]], axis=1).sum(axis=1)
        assert np.array_equal(x, m1[ok])
        # matching a set against itself WITHOUT exclusion is the identity at distance 0
        idx0, z1, _ = ctx.match(d1, d1, th=256, ratio_num=10)
        assert (z1 == 0).all()


@pytest.mark.parametrize("nq", [1, 2, 3, 5, 8])
def test_match_database_streaming_form(oracle, nq):
    """n_query <= 8 against a large database takes the lane-per-train streaming kernel (config 5 in
    its HBM-bound regime); results must equal the oracle's, ties across block chunks included."""
    rng = np.random.default_rng(500 + nq)
    nt = 200003
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    t[77] = q[0]
    t[150000] = q[0]             # same best twice, far apart: lowest row wins, d2 == d1 == 0
    t[199999] = q[nq - 1]
    t[199999, 9] ^= 0x81         # distance 2 at the very end of the last chunk
    t[5] = q[nq - 1]
    t[5, 0] ^= 0x07              # distance 3 near the start: second best
    with binding.OrbContext(0) as ctx:
        for kw in (dict(th=50, ratio_num=9), dict(th=256, ratio_num=10), dict(th=-1, ratio_num=9)):
            got = ctx.match(q, t, ratio_den=10, **kw)
            want = oracle.match(q, t, ratio_den=10, **kw)
            for a, b, name in zip(got, want, ("idx", "d1", "d2")):
                assert np.array_equal(a, b), f"{name} differs ({kw})"
        names = [s_["name"] for s_ in ctx.stats()]
    raw = oracle.match(q, t, th=-1)
    assert raw[0][0] == 77 and raw[1][0] == 0 and raw[2][0] == 0
    assert raw[0][nq - 1] == (77 if nq == 1 else 199999)


def test_device_std_sort_restatement_vs_oracle(oracle):
    """The wave-wide introsort on the device must leave equal keys exactly where libstdc++'s
    std::sort does (the oracle's restatement is pinned against the real one on the CPU).  Random
    tie-heavy inputs, sizes around the 16-element threshold, and McIlroy-style adversarial inputs
    that drive the depth limit into the heapsort fallback."""
    rng = np.random.default_rng(11)
    with binding.OrbContext(0) as ctx:
        for n in list(range(0, 40)) + [63, 64, 65, 100, 257, 433, 1000, 2048]:
            for rep in range(4):
                size = rng.integers(2, 2 + (3, 12, 200, 5)[rep], size=n)
                ulx = 35 * rng.integers(0, (4, 40, 7, 1)[rep], size=n)
                got = ctx.debug_sort(size, ulx)
                want = oracle.std_sort(size, ulx)
                assert np.array_equal(got, want), (n, rep)
        # McIlroy's killer adversary (tests/pyref.py) drives the algorithm to its depth limit, so
        # the heapsort fallback runs on the device too; quantised copies add ties on top
        import ctypes as C
        import pyref
        heap_calls = C.c_int.in_dll(oracle.lib(), "orc_std_sort_heap_calls")
        for n in (200, 433, 1500, 2048):
            k = np.array(pyref.quicksort_killer(n))
            for shift in (0, 1, 2):
                size = (k >> shift) + 2
                ulx = (k * 7) % 5
                before = heap_calls.value
                want = oracle.std_sort(size, ulx)
                if shift == 0:
                    assert heap_calls.value > before, "killer input did not reach the heapsort fallback"
                assert np.array_equal(ctx.debug_sort(size, ulx), want), (n, shift)


@pytest.mark.parametrize("w,h,nf,scale,nl", [(3840, 2160, 5000, 1.2, 8), (640, 480, 800, 1.5, 5), (800, 600, 600, 2.0, 4),
                                             (4095, 2600, 3000, 1.2, 8)])
def test_large_images_and_other_scale_factors(oracle, w, h, nf, scale, nl):
    """4K UHD, the widest image the packed records admit (4095 px), and pyramid scale factors
    that take the direct (non-LDS) resize kernel."""
    img = synth.frame(60 + nl, w, h)
    with binding.OrbContext(0, n_features=nf, scale_factor=scale, n_levels=nl) as ctx:
        kps, desc, counts = ctx.extract(img)
    okps, odesc, ocounts = oracle.extract(img, oracle.default_params(n_features=nf, scale_factor=scale, n_levels=nl))
    assert np.array_equal(counts, ocounts) and len(kps) == len(okps)
    assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)


def test_limits_are_errors_not_truncation():
    with binding.OrbContext(0, n_features=12000) as ctx:  # level-0 quota 2605 > 2032 sort items
        with pytest.raises(binding.OrbError) as e:
            ctx.extract(synth.frame(1, 640, 480))
        assert e.value.code == binding.SS_ERR_INVALID_ARG and "quota" in str(e.value)
    with binding.OrbContext(0) as ctx:
        with pytest.raises(binding.OrbError) as e:
            ctx.extract(np.zeros((100, 5000), np.uint8))
        assert e.value.code == binding.SS_ERR_INVALID_ARG  # wider than 4095


def test_batch_with_flat_and_textured_frames(oracle):
    import torch
    w, h, nf = 480, 360, 600
    frames = np.stack([synth.frame(70, w, h), np.full((h, w), 90, np.uint8), synth.frame(71, w, h),
                       (synth.frame(72, w, h) // 5 + 100).astype(np.uint8)])
    d = torch.from_numpy(frames).to("cuda:0")
    with binding.OrbContext(0, n_features=nf, max_batch=4) as ctx:
        ctx.extract_batch_device(d.data_ptr(), 4, w, h)
        ctx.synchronize()
        got = [ctx.fetch_frame(b) for b in range(4)]
        # a smaller batch on the same context afterwards must not see stale frames
        ctx.extract_batch_device(d[2:].data_ptr(), 2, w, h)
        ctx.synchronize()
        again = [ctx.fetch_frame(b) for b in range(2)]
        with pytest.raises(binding.OrbError):
            ctx.fetch_frame(2)
    p = oracle.default_params(n_features=nf)
    for b in range(4):
        okps, odesc, ocounts = oracle.extract(frames[b], p)
        assert got[b][0].tobytes() == okps.tobytes() and np.array_equal(got[b][1], odesc) and np.array_equal(got[b][2], ocounts)
    assert len(got[1][0]) == 0
    for b in range(2):
        assert again[b][0].tobytes() == got[b + 2][0].tobytes() and np.array_equal(again[b][1], got[b + 2][1])


def test_downstream_pnp_pose_from_hip_outputs(oracle):
    """North-star clause "downstream PnP pose within 1e-4 rel": the pose-only optimisation
    (ORB-SLAM3 PoseOptimization restated in the oracle) fed with the HIP path's keypoints and
    matches returns the pose it returns for the oracle's -- the inputs being bit-identical, the
    relative difference is 0 -- and that pose is the known camera motion of the synthetic pair."""
    w, h, nf = 640, 480, 1250
    f0, f1 = synth.frame(80, w, h, 0), synth.frame(80, w, h, 1)
    fx = fy = 500.0
    cx, cy, Z = w / 2.0, h / 2.0, 5.0

    def pose_from(kp0, kp1, idx):
        ok = idx >= 0
        a, b = kp0[idx[ok]], kp1[ok]
        pts = np.c_[(a["x"] - cx) * Z / fx, (a["y"] - cy) * Z / fy, np.full(ok.sum(), Z)]
        inv_s2 = 1.0 / (1.2 ** b["octave"].astype(np.float64)) ** 2
        return oracle.pnp_pose_only(pts, np.c_[b["x"], b["y"]].astype(np.float64), inv_s2, fx, fy, cx, cy)

    with binding.OrbContext(0, n_features=nf) as ctx:
        k0, d0, _ = ctx.extract(f0)
        k1, d1, _ = ctx.extract(f1)
        idx, _, _ = ctx.match(d1, d0)
    p = oracle.default_params(n_features=nf)
    ok0, od0, _ = oracle.extract(f0, p)
    ok1, od1, _ = oracle.extract(f1, p)
    oidx, _, _ = oracle.match(od1, od0)
    R_h, t_h, in_h = pose_from(k0, k1, idx)
    R_o, t_o, in_o = pose_from(ok0, ok1, oidx)
    rel = max(np.abs(R_h - R_o).max() / np.abs(R_o).max(), np.abs(t_h - t_o).max() / np.abs(t_o).max())
    assert rel <= 1e-4 and np.array_equal(in_h, in_o)  # tolerance stated by the north star; measured 0
    assert in_h.sum() > 300
    # the pair is the same scene shifted by (+3, -2) px: t = (3 Z / fx, -2 Z / fy, 0), R = I
    assert np.abs(t_h - np.array([3 * Z / fx, -2 * Z / fy, 0.0])).max() < 5e-3  # keypoints are integer pixels x scale
    assert np.abs(R_h - np.eye(3)).max() < 2e-3


def test_ss_track_poses_vs_oracle_pipeline_and_truth(oracle):
    """ss_track through the C ABI (HIP extraction + HIP match + host geometry) against the all-CPU
    statement of the same pipeline (C oracle extraction + match, oracle/vo_oracle.py tracker) on a
    parallax sequence, including a lost frame and the re-initialisation after it.  Features and matches
    are bit-identical, so poses differ by the eigen-solver only: tolerance 1e-6 absolute on a
    unit-median-depth map (north star: 1e-4 rel)."""
    from oracle import vo_oracle as vo
    w, h, seed, nf = 640, 480, 77, 1000
    sc = synth.scene(seed, w, h)
    frames = [synth.parallax_frame(seed, w, h, t, sc=sc) for t in range(9)]
    frames.insert(6, np.full((h, w), 90, np.uint8))  # a featureless frame: tracking is lost, then restarts
    cam = binding.Camera(type=b"PinHole", fx=500, fy=500, cx=320, cy=240, k1=-0.05, k2=0.01, p1=1e-4, p2=-1e-4,
                         width=w, height=h, fps=30, rgb=1, th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
    ocam = vo.Camera(500, 500, 320, 240, -0.05, 0.01, 1e-4, -1e-4)
    import track_ref
    want = track_ref.run(oracle, frames, ocam, nf)
    got = []
    with binding.OrbContext(0, n_features=nf) as ctx:
        with pytest.raises(binding.OrbError) as e:
            ctx.track(frames[0])
        assert e.value.code == binding.SS_ERR_NOT_CALIBRATED
        ctx.set_calibration(1, cam)
        for t, img in enumerate(frames):
            got.append(ctx.track(img, 1, t / 30.0))
        ctx.track_reset()
        assert ctx.track(frames[0])["state"] == 1
    states = [g["state"] for g in got]
    assert states[:2] == [1, 1] and states[6] == 4 and states[7] == 1 and states[-1] == 2 and states.count(2) >= 5
    for g, o in zip(got, want):
        assert (g["state"], g["n_keypoints"], g["n_matches"], g["n_inliers"], g["n_map_points"]) == \
               (o["state"], o["n_keypoints"], o["n_matches"], o["n_inliers"], o["n_map_points"])
        assert np.allclose(g["position"], o["position"], rtol=0, atol=1e-6)
        assert np.allclose(g["quaternion"], o["quaternion"], rtol=0, atol=1e-6)
    assert [g["timestamp"] for g in got] == [t / 30.0 for t in range(len(frames))]
    # truth for the first stretch: sliding along -x at constant speed, no rotation
    ok = [t for t in range(6) if states[t] == 2]
    pos = np.array([got[t]["position"] for t in ok])
    v = pos[:, 0] / np.array(ok)
    assert (v < 0).all() and np.abs(v / v.mean() - 1).max() < 0.08
    assert np.abs(pos[:, 1:]).max() < 0.15 * np.abs(pos[:, 0]).max()
    assert max(np.abs(got[t]["quaternion"][:3]).max() for t in ok) < 5e-3


def test_contexts_are_independent_across_host_threads(oracle):
    """"Distinct contexts are independent" (include/sendslam_orb.h): four host threads, one context each, different
    image sizes and feature counts, interleaved extract / match / track calls -- every result equals the oracle's."""
    import threading
    cases = [(70, 640, 480, 800), (71, 800, 600, 1250), (72, 333, 517, 500), (73, 1280, 720, 2000)]
    expected, got, errors = {}, {}, []
    for seed, w, h, nf in cases:
        img0, img1 = synth.frame(seed, w, h, 0), synth.frame(seed, w, h, 1)
        p = oracle.default_params(n_features=nf)
        k0, d0, _ = oracle.extract(img0, p)
        k1, d1, _ = oracle.extract(img1, p)
        expected[seed] = (k0, d0, k1, d1, oracle.match(d1, d0))

    def work(seed, w, h, nf):
        try:
            img0, img1 = synth.frame(seed, w, h, 0), synth.frame(seed, w, h, 1)
            with binding.OrbContext(0, n_features=nf) as ctx:
                out = []
                for _ in range(6):
                    k0, d0, _ = ctx.extract(img0)
                    k1, d1, _ = ctx.extract(img1)
                    out.append((k0, d0, k1, d1, ctx.match(d1, d0)))
                got[seed] = out
        except Exception as e:  # noqa: BLE001
            errors.append((seed, repr(e)))

    threads = [threading.Thread(target=work, args=c) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for seed, *_ in cases:
        ek0, ed0, ek1, ed1, em = expected[seed]
        for k0, d0, k1, d1, m in got[seed]:
            assert k0.tobytes() == ek0.tobytes() and np.array_equal(d0, ed0)
            assert k1.tobytes() == ek1.tobytes() and np.array_equal(d1, ed1)
            assert all(np.array_equal(a, b) for a, b in zip(m, em))


def test_contexts_do_not_leak_device_memory():
    import torch
    img = synth.frame(5, 640, 480)
    torch.cuda.synchronize()
    with binding.OrbContext(0) as ctx:  # warm the runtime's own pools
        ctx.extract(img)
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(25):
        with binding.OrbContext(0, max_batch=4) as ctx:
            ctx.extract(img)
            ctx.extract(synth.frame(6, 320, 240))  # geometry rebuild on a size change
            ctx.match(np.zeros((10, 32), np.uint8), np.zeros((300000, 32), np.uint8))
    free1, _ = torch.cuda.mem_get_info(0)
    assert free0 - free1 < 64 << 20, f"device memory shrank by {(free0 - free1) >> 20} MiB over 25 contexts"


def test_quadtree_first_pass_overshoot_vs_oracle(oracle):
    """Found by the soak sweep (seed 20262, case 1339): more keypoints than quota + 3 at a wide level -- upstream keeps
    them all; so do the oracle and the device (capacities sized for 4 x the root nodes)."""
    from test_oracle_units import wide_overshoot_case
    img, kw = wide_overshoot_case()
    with binding.OrbContext(0, **kw) as ctx:
        kps, desc, counts = ctx.extract(img)
    okps, odesc, ocounts = oracle.extract(img, oracle.default_params(**kw))
    assert np.array_equal(counts, ocounts) and counts.sum() > 85
    assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc)
@pytest.mark.gpu
def test_ss_track_keeps_a_long_back_and_forth_sequence():
    """ss_track over 150 frames of a camera that goes back and forth over 24 positions (the front door bench's sequence): tracked
    from the third frame to the last, the same position again every 46 frames.  Regression for the rotation that drifted from
    orthonormality through the constant-velocity prediction: every sequence used to be lost 41 frames after its
    initialisation."""
    w, h, nf = 640, 480, 1250
    sc = synth.scene(4000, w, h)
    base = [synth.parallax_frame(4000, w, h, t, sc=sc) for t in range(24)]
    order = list(range(24)) + list(range(22, 0, -1))
    cam = binding.Camera(type=b"PinHole", fx=0.8 * w, fy=0.8 * w, cx=w / 2, cy=h / 2, k1=0, k2=0, p1=0, p2=0, width=w, height=h, fps=30,
                         rgb=1, th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
    with binding.OrbContext(0, n_features=nf) as ctx:
        ctx.set_calibration(1, cam)
        outs = [ctx.track(base[order[i % len(order)]], 1, 1.0 + i / 30.0) for i in range(150)]
    states = [o["state"] for o in outs]
    first_ok = states.index(2)
    assert first_ok <= 4 and all(s_ == 2 for s_ in states[first_ok:]), "".join(map(str, states))
    for i in range(first_ok + len(order), 150):
        assert np.linalg.norm(outs[i]["position"] - outs[i - len(order)]["position"]) < 0.05, i
        assert abs(float(outs[i]["quaternion"] @ outs[i]["quaternion"]) - 1.0) < 1e-9


