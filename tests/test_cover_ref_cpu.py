"""CPU: the two statements of the greedy cover the GPU and CLI tests check against (tests/cover_ref.py) agree with each
other -- the definition in numpy, and the oracle's query on the masked sketch round by round -- on the data and the
query kinds of tests/test_gpu_cover.py; the consequences include/niqki_hip.h states hold; and the values the data must
give, whatever any device does."""
import numpy as np
import pytest

from cover_ref import cover_by_oracle, cover_of, query_kinds, valid_cells
from test_gpu_cluster import S, W, data

F = 1 << S


@pytest.fixture(scope="module")
def case(po):
    sk = data(3000, 11)
    return sk, query_kinds(sk, W), po.Index(po.make_params(31, S, W, 3, 0.0), sk)


@pytest.mark.parametrize("thr", [50, 1])
def test_the_definition_and_the_oracle_rounds_agree(case, thr):
    sk, kinds, ix = case
    assert len(kinds) == 8
    for name, q in kinds.items():
        for max_picks in (0, 1, 3):
            a = cover_of(sk, q, W, thr, max_picks)
            assert a == cover_by_oracle(ix, sk, q, thr, max_picks), (name, max_picks)
            assert a == cover_of(sk, q, W, thr)[:max_picks or None], (name, max_picks)


@pytest.mark.parametrize("thr", [50, 1, 0])
def test_the_stated_consequences_hold(case, thr):
    sk, kinds, _ = case
    for name, q in kinds.items():
        picks = cover_of(sk, q, W, thr)
        counts, gids, totals = ([p[k] for p in picks] for k in range(3))
        r0 = int(valid_cells(q, W).sum())
        assert counts == sorted(counts, reverse=True), name                 # never increasing
        assert len(set(gids)) == len(gids), name                            # no genome twice
        assert sum(counts) <= r0, name
        assert len(picks) <= min(sk.shape[0], r0 // max(thr, 1)), name
        assert all(max(thr, 1) <= c <= t for c, t in zip(counts, totals)), name
    assert cover_of(sk, kinds["random"], W, 0) == cover_of(sk, kinds["random"], W, 1)


def test_what_the_data_must_give_at_threshold_50(case):
    sk, kinds, _ = case
    assert int((sk == sk[7]).all(1).sum()) == 7
    assert cover_of(sk, kinds["duplicates"], W, 50) == [(1009, 2809, 1009)]          # the LARGEST duplicate id
    assert cover_of(sk, kinds["empty"], W, 50) == []
    assert cover_of(sk, kinds["two"], W, 50) == [(522, 100, 522), (501, 2500, 504)]
    five = cover_of(sk, kinds["five"], W, 50)
    assert len(five) == 5 and sorted(p[1] for p in five) == [20, 500, 900, 1500, 2200]
    assert five[-1] == (99, 900, 214)                                                # a pick count far below its total
    assert cover_of(sk, kinds["random"], W, 50) == []
    assert len(cover_of(sk, kinds["random"], W, 1)) == 450
    assert int(valid_cells(kinds["holes"], W).sum()) == 255
    assert cover_of(sk, kinds["holes"], W, 50) == [(255, 300, 255)]
    sixteen = cover_of(sk, kinds["sixteen"], W, 1)
    assert sorted(p[1] for p in sixteen[:16]) == list(range(40, 40 + 16 * 180, 180))
    assert cover_of(sk[:0], kinds["two"], W, 50) == []
