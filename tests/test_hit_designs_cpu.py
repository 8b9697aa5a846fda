"""CPU: tests/hit_designs.py pinned on the oracle.  The designed sketches give the oracle's Index exactly the
prescribed counts, and reference_lists -- the expectation of tests/test_gpu_hits_designed.py -- equals the oracle's
Index.query (threshold of src/niqki_index.cpp:662-666, order of :685) on them at every threshold tried, 0 included."""
import numpy as np
import pytest

import hit_designs as hd


def oracle_index(po, S, W, sk):
    p = po.make_params(31, S, W, 3, 0.0)
    return po.Index(p, sk)


CASES = {
    # name: (S, W, n_hits per type, N)
    "s8": (8, 8, [0, 1, 9, 257, 2049, 3000], 3000),
    "s10_32_types": (10, 8, [0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
                     + [2, 6, 10, 100, 300, 700, 1500, 2500, 2999, 33, 65], 3000),
    "s8_wide_gids": (8, 8, [5, 257, 2049], 66000),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_design_gives_the_oracle_the_prescribed_counts(po, name):
    S, W, n_hits, N = CASES[name]
    rng = np.random.default_rng(len(name) + N)
    C = hd.hit_matrix(n_hits, N, rng, forced=(65535, 65536))
    assert [int((C[t] >= 20).sum()) for t in range(len(n_hits))] == n_hits
    sk, q = hd.design(C, S, W, rng)
    assert sk.shape == (N, 1 << S) and q.shape == (len(n_hits), 1 << S)
    assert (sk == -1).any() and sk.max() == len(n_hits) and sk.min() == -1
    ix = oracle_index(po, S, W, sk)
    for t in range(len(n_hits)):
        assert np.array_equal(ix.counts(q[t]).astype(np.int64), C[t]), t
    # the hits, ordered: thresholds at 0, below, between, on and above the levels (0, 19 | 20, 21, 25, 30)
    for ms in (0, 1, 19, 20, 21, 22, 30, 31):
        off, c, g = hd.reference_lists(C, ms)
        for t in range(len(n_hits)):
            ec, eg = ix.query(q[t], min_score=ms)
            lo, hi = int(off[t]), int(off[t + 1])
            assert np.array_equal(c[lo:hi], ec.astype(np.int64)) and np.array_equal(g[lo:hi], eg.astype(np.int64)), (ms, t)
    if N > 65536:
        # the forced pair ties: the order across the 16-bit edge is decided by the gid
        off, c, g = hd.reference_lists(C, 20)
        for t in range(len(n_hits)):
            gs = g[int(off[t]):int(off[t + 1])].tolist()
            assert gs.index(65536) + 1 == gs.index(65535), t


def test_design_refuses_what_it_cannot_build():
    rng = np.random.default_rng(1)
    with pytest.raises(AssertionError):
        hd.design(np.full((9, 4), 30), 8, 8, rng)          # 270 cells of 256
    with pytest.raises(AssertionError):
        hd.design(np.ones((16, 4), np.int64), 8, 4, rng)   # 16 values and the filler in 4 bits
    with pytest.raises(AssertionError):
        hd.design(-np.ones((2, 4), np.int64), 8, 8, rng)
    sk, q = hd.design(np.full((8, 4), 32), 8, 8, rng)      # every cell taken: no filler, no empty cell
    assert sk.min() == 0 and sk.max() == 7 and all(np.bincount(r, minlength=8).tolist() == [32] * 8 for r in sk)


def test_reference_lists_cut_offset_and_deal():
    rng = np.random.default_rng(7)
    rows = np.stack([hd.row_levels(300, rng), hd.row_zeros(300), hd.row_ramp(300), hd.row_const(300, 0xFFFF),
                     hd.row_bin_edges(300, rng), hd.row_u16(300, rng)])
    for ms in (0, 1, 16, 65535, 65536):
        full = hd.reference_lists(rows, ms)
        sizes = np.diff(full[0])
        assert sizes.tolist() == [int((r.astype(np.int64) >= ms).sum()) for r in rows]
        for i in range(rows.shape[0]):        # the definition, entry by entry
            c, g = full[1][full[0][i]:full[0][i + 1]], full[2][full[0][i]:full[0][i + 1]]
            assert np.array_equal(c, rows[i].astype(np.int64)[g]) and np.all(c >= ms)
            key = c * (1 << 32) + g
            assert np.all(key[:-1] > key[1:])
        for k in (1, 2, 7, 64, 299, 300, 301):
            cut = hd.reference_lists(rows, ms, top_k=k)
            exp = hd.cut_lists(full, k, 300)
            assert all(np.array_equal(a, b) for a, b in zip(cut, exp)), (ms, k)
            want = sizes if k >= 300 else np.minimum(sizes, k)
            assert np.diff(cut[0]).tolist() == want.tolist()
            for i in range(rows.shape[0]):
                lo, n = int(full[0][i]), int(want[i])
                assert np.array_equal(cut[2][cut[0][i]:cut[0][i + 1]], full[2][lo:lo + n])
        moved = hd.reference_lists(rows, ms, gid_begin=8)
        assert np.array_equal(moved[0], full[0]) and np.array_equal(moved[1], full[1]) and np.array_equal(moved[2], full[2] + 8)
        types = np.array([5, 0, 0, 3, 1, 2, 5, 4])
        dealt = hd.deal(full, types)
        again = hd.reference_lists(rows[types], ms)
        assert all(np.array_equal(a, b) for a, b in zip(dealt, again)), ms
    full = hd.reference_lists(rows, 16)
    assert hd.first_difference(full, full) is None
    wrong = (full[0], full[1], full[2].copy())
    wrong[2][-1] ^= 1
    assert "query" in hd.first_difference(wrong, full)


def test_placed_ties_make_the_three_block_states():
    """a row of placed ties over five compaction blocks: for a cut in the topmost, a middle and the lowest block the
    blocks above keep every tie, the block of the cut a part -- its first kept tie behind its first 256 genomes --
    and the blocks below none"""
    rng = np.random.default_rng(3)
    n, T = 4 * hd.BLK + 1500, 20
    pos = hd.edge_positions(n)
    assert {0, n - 1, 4095, 4096, 4097, 8191, 8192, 4096 + 300, n & ~7}.issubset(pos)
    row = hd.row_placed_ties(n, T, pos, [5, 4096 + 17, n - 2], rng)
    assert row[n - 2] == T and row[5] == T + 1 and set(np.unique(row).tolist()) == {0, T - 1, T, T + 1}
    cuts = hd.tie_cuts(row, T, 1)
    assert [b for b, _, _ in cuts] == [0, 1, 2, 3, 4]
    by_block = {b: st for b, _, st in cuts}
    assert by_block[4] == {"part", "none"} and by_block[2] == {"all", "part", "none"} and by_block[0] == {"all", "part"}
    full = hd.reference_lists(row[None, :], 1)
    for b, k, _ in cuts:
        g = hd.cut_lists(full, k, n)[2]
        c = row.astype(np.int64)[g]
        kept = np.sort(g[c == T])
        assert np.all(c >= T) and kept[0] // hd.BLK == b and kept[0] - b * hd.BLK >= 300
        assert (row[b * hd.BLK:b * hd.BLK + 256] == T).any()      # ties of the cut block that the cut drops
        assert set(hd.row_ks(row, 1, n)) >= {int((row >= 1).sum()), int((row > T).sum()) + 1}
