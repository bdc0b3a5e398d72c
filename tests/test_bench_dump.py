"""bench.py --dump-outputs without a GPU: dump_outputs() on a stand-in context that returns the oracle's results, so the
files are checked value for value against what the context handed out (the GPU suite runs the real thing:
tests/test_bench_workloads.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from send_slam_amd import binding, synth  # noqa: E402

KCAP = 576
NAMES = ("frames", "n_keypoints", "level_counts", "keypoints", "descriptors", "match_idx", "match_d1", "match_d2")


class _Params:
    n_levels = 8


class _View:
    kp_capacity = KCAP


class OracleCtx:
    """the three calls dump_outputs makes on an OrbContext, answered from oracle results"""
    params = _Params()

    def __init__(self, results):
        self.results = results

    def batch_view(self):
        return _View()

    def fetch_frame(self, b):
        return self.results[b]


@pytest.fixture(scope="module")
def batch(oracle):
    import torch
    p = oracle.default_params(n_features=500)
    n_frames = 4
    idx = np.full((n_frames, KCAP), -7, np.int32)  # past a frame's keypoints the buffers hold stale values
    d1 = np.full((n_frames, KCAP), 999, np.int16)
    d2 = np.full((n_frames, KCAP), 999, np.int16)
    results = []
    for b in range(n_frames):
        kps, desc, levels = oracle.extract(synth.frame(b, 320, 240), p)
        i, a1, a2 = oracle.match(desc, desc, exclude_self=True)
        idx[b, :len(i)], d1[b, :len(i)], d2[b, :len(i)] = i, a1, a2
        results.append((kps, desc, levels))
    return OracleCtx(results), [torch.from_numpy(x) for x in (idx, d1, d2)], (idx, d1, d2)


def load(path):
    out = {}
    for name in NAMES:
        out[name] = np.load(os.path.join(path, name + ".npy"))
        assert out[name].dtype == np.float32, name
    return out


def test_dump_holds_every_frame_as_the_context_returned_it(batch, tmp_path):
    ctx, match_out, (idx, d1, d2) = batch
    bench.dump_outputs(str(tmp_path), ctx, match_out, len(ctx.results))
    got = load(str(tmp_path))
    assert got["frames"].tolist() == list(range(len(ctx.results)))
    ns = [len(r[0]) for r in ctx.results]
    assert got["n_keypoints"].tolist() == ns
    assert got["level_counts"].tolist() == [r[2].tolist() for r in ctx.results]
    off = 0
    for b, (kps, desc, _) in enumerate(ctx.results):
        n = ns[b]
        for j, f in enumerate(binding.KP_DTYPE.names):
            assert np.array_equal(got["keypoints"][off:off + n, j], kps[f].astype(np.float32)), f
        assert np.array_equal(got["descriptors"][off:off + n], desc)
        assert np.array_equal(got["match_idx"][off:off + n], idx[b, :n])
        assert np.array_equal(got["match_d1"][off:off + n], d1[b, :n])
        assert np.array_equal(got["match_d2"][off:off + n], d2[b, :n])
        off += n
    assert off == len(got["keypoints"]) == len(got["descriptors"]) == len(got["match_idx"])


def test_dump_samples_fixed_frames_under_the_size_limit(batch, tmp_path, monkeypatch):
    ctx, match_out, _ = batch
    per_frame = KCAP * (6 + 32 + 3) * 4 + (2 + 8) * 4
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * per_frame + 10)
    picks = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), ctx, match_out, len(ctx.results))
        got = load(str(tmp_path / run))
        picks.append(got["frames"].tolist())
        assert len(picks[-1]) == 2 and picks[-1] == sorted(picks[-1])
        assert got["n_keypoints"].tolist() == [len(ctx.results[int(b)][0]) for b in picks[-1]]
        assert sum(os.path.getsize(str(tmp_path / run / (n + ".npy"))) for n in NAMES) <= 2 * per_frame + 10 + 128 * len(NAMES)
    assert picks[0] == picks[1]
