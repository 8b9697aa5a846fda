"""The line-aligned sketch loop with its waves leveled by progress-relative issue priority (nq_sketch.hip
roll_records_lines, rule and scale in nq_sketch_lines.h) against the oracle: the priorities may change no bit.  Marker,
fixtures, text and references are those of test_gpu_sketch_lines.py: K = 31, S = 10, W = 12, candidate filter automatic
("1") and forced to three leading zeros ("4"); every reference is computed once, for both modes.

The records are the smallest the 1024 x 32 launch shape accepts, 2^21 bases per workgroup: sixteen line rounds per
wave, and a progress scale of 32 steps over them, so every wave changes its published progress (and with it, maybe,
its priority) in every round."""
import numpy as np
import pytest

import test_gpu_sketch_lines as sl

pytestmark = pytest.mark.gpu

LONG = sl.LONG
MODES = sl.MODES


@pytest.mark.parametrize("mode", MODES)
def test_ragged_record_off_the_line(native, po, mode, monkeypatch):
    """One record of 2^21 + 77 bases that starts 61 bytes past a line: 16 lines per lane and five more, ragged first and
    last line, several priority changes per wave."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    r = sl._text(LONG + 77, 6_000_000)
    sk = sl._dev_call(native, torch, 31, 10, [r], 61, sl._one_per_sketch(1))
    assert np.array_equal(sk[0], sl._ref(po, ("level", "ragged", 31), 31, 10, [r])), mode


@pytest.mark.parametrize("mode", MODES)
def test_progress_runs_across_records(native, po, mode, monkeypatch):
    """One entry of records of 2^21 + 5, 40, 3000, 130 and 2^21 + 1 bases: most waves have no lines in the short records
    (which they count as done at once), and the progress of the last record goes on from the first one's."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    lens = [LONG + 5, 40, 3000, 130, LONG + 1]
    recs, at = [], 10_000_000
    for n in lens:
        recs.append(sl._text(n, at))
        at += n + 17
    e = native.Engine(K=31, S=10, W=12, H=4)
    sk = e.sketch(recs, entry_rec=np.array([0, len(recs)], np.uint32))
    e.close()
    assert np.array_equal(sk[0], sl._ref(po, ("level", "records"), 31, 10, recs)), mode


@pytest.mark.parametrize("mode", MODES)
def test_extra_round_on_every_simd(native, po, mode, monkeypatch):
    """One record of 1024 * 16 + 5 lines of hash bytes (the buffer is line-aligned and the record starts it, so its hash
    bytes, positions K - 1 .. len - 2, end 50 bytes short of line 16 389's end): one wave on each of SIMDs 0-3 runs a
    seventeenth, predicated round -- two lanes of it on SIMD 0, one on the others."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    n = (1024 * 16 + 5) * 128 - 50 + 1
    assert n >= LONG and (n - 1 + 127) // 128 == 1024 * 16 + 5
    r = sl._text(n, 15_000_000)
    sk = sl._dev_call(native, torch, 31, 10, [r], 0, sl._one_per_sketch(1))
    assert np.array_equal(sk[0], sl._ref(po, ("level", "extra"), 31, 10, [r])), mode


@pytest.mark.parametrize("mode", MODES)
def test_ragged_record_other_k(native, po, mode, monkeypatch):
    """The first case's record at K = 21: the kernel instance that takes K from its arguments."""
    import torch
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    r = sl._text(LONG + 77, 6_000_000)
    sk = sl._dev_call(native, torch, 21, 10, [r], 61, sl._one_per_sketch(1))
    assert np.array_equal(sk[0], sl._ref(po, ("level", "ragged", 21), 21, 10, [r])), mode
