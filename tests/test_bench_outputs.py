"""CPU: what `bench.py --dump-outputs DIR` writes -- the hit lists of one step as float64 .npy files, exact, and beyond
the size limit a fixed, seeded sample of the hits that is the same from run to run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def step_hits(n_q=64, seed=5):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(rng.integers(0, 40, n_q))]).astype(np.int64)
    cap = int(off[-1]) + 100                   # (the step's buffers are larger than its hits)
    hc = torch.from_numpy(rng.integers(0, 1 << 15, cap).astype(np.int32))
    hg = torch.from_numpy(rng.integers(0, (1 << 31) - 1, cap).astype(np.int32))
    return torch.from_numpy(off), hc, hg


def files(d):
    return sorted(os.listdir(d)), sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_the_hit_lists_are_written_whole_and_exact(tmp_path):
    off, hc, hg = step_hits()
    bench.dump_outputs(str(tmp_path), off, hc, hg, 1)
    n = int(off[-1])
    assert files(tmp_path)[0] == ["hit_counts.npy", "hit_gids.npy", "hit_offsets.npy"]
    for name, want in (("hit_offsets", off.numpy()), ("hit_counts", hc[:n].numpy()), ("hit_gids", hg[:n].numpy())):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64)), name
        assert np.array_equal(got.astype(np.int64), want), name


def test_an_overflowing_step_writes_the_hits_it_stored(tmp_path):
    off, hc, hg = step_hits()
    off[-1] = len(hc) + 1000                   # more hits than the buffers held
    bench.dump_outputs(str(tmp_path), off, hc, hg, 1)
    assert len(np.load(tmp_path / "hit_gids.npy")) == len(hc)


def test_beyond_the_limit_a_seeded_sample_within_it(tmp_path):
    off, hc, hg = step_hits()
    n = int(off[-1])
    limit = 4 * 128 + 8 * len(off) + 16 * (n // 3)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), off, hc, hg, 7, limit=limit)
    bench.dump_outputs(str(b), off, hc, hg, 7, limit=limit)
    names, size = files(a)
    assert names == ["hit_counts.npy", "hit_gids.npy", "hit_offsets.npy", "hit_sample_positions.npy"] and size <= limit
    pos = np.load(a / "hit_sample_positions.npy").astype(np.int64)
    assert len(pos) > 0 and np.all(np.diff(pos) > 0) and pos[-1] < n
    assert np.array_equal(np.load(a / "hit_gids.npy"), hg.numpy()[pos].astype(np.float64))
    assert np.array_equal(np.load(a / "hit_offsets.npy"), off.numpy().astype(np.float64))
    for f in names:
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
