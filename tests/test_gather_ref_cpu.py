"""CPU: tests/gather_ref.py pinned on the oracle.  On both data sets of tests/test_gpu_gather_forms.py the plain counts
equal the oracle's Index.counts and the reference hit lists its Index.query, for a sample of queries that includes
the empty and the out-of-range one; the designed set holds the bucket lengths it was designed for."""
import numpy as np
import pytest

import gather_ref as gr


def check(po, S, W, sk, q, sample, thresholds):
    p = po.make_params(31, S, W, 3, 0.0)
    ix = po.Index(p, sk)
    ref = gr.reference_counts(sk, q, W)
    for i in sample:
        assert np.array_equal(ref[i], ix.counts(q[i]).astype(np.int64)), i
    for ms in thresholds:
        off, c, g = gr.reference_hits(ref, ms)
        for i in sample:
            ec, eg = ix.query(q[i], min_score=ms)
            lo, hi = int(off[i]), int(off[i + 1])
            assert np.array_equal(c[lo:hi], ec.astype(np.int64)) and np.array_equal(g[lo:hi], eg.astype(np.int64)), (ms, i)
    return ref


@pytest.mark.parametrize("n_tiles", [1, 3, 5])
def test_designed_set_on_the_oracle(po, n_tiles):
    sk, v = gr.designed(n_tiles)
    q, names = gr.designed_queries(sk, v)
    assert q.shape == (gr.NQ, gr.F) and sk.shape == (gr.n_genomes(n_tiles), gr.F)
    for g0, g1 in gr.tile_ranges(sk.shape[0]):
        assert {x for x in gr.LENGTHS if x <= g1 - g0} <= gr.bucket_lengths(sk[g0:g1], gr.W)
    sample = [0, 1, 4, names.index("empty"), names.index("out of range"), gr.NQ - 1]
    ref = check(po, gr.S, gr.W, sk, q, sample, (0, 1, int(np.median(ref_row0(sk, q))), gr.F))
    assert ref[names.index("empty")].max() == 0
    assert ref[0].min() > 0                      # every genome is in some long bucket
    oor = names.index("out of range")            # the cells out of range count nothing: the odd slots of v are left
    assert np.array_equal(ref[oor], gr.reference_counts(sk[:, 1::2], q[:1, 1::2], gr.W)[0])


def ref_row0(sk, q):
    return gr.reference_counts(sk, q[:1], gr.W)[0]


@pytest.mark.parametrize("S,W,n,seed", [(11, 8, 1500, 1820), (5, 8, 3000, 5)])   # (the first: the GPU sweep's own set)
def test_family_set_on_the_oracle(po, S, W, n, seed):
    sk, fam = gr.families(n, S, W, seed=seed)
    q, where = gr.family_queries(sk, fam, W)
    assert (sk == -1).any() and q.shape[0] == gr.NQ
    sample = [0, 7, where["empty"], where["out of range"], gr.NQ - 1]
    ref = check(po, S, W, sk, q, sample, (0, 1, (1 << S) // 3))
    assert ref[where["empty"]].max() == 0


def test_counts_of_a_slot_range(po):
    """slot shards: the counts of [slot_begin, slot_end) sum to the whole"""
    sk, fam = gr.families(300, 8, 8, seed=1)
    q, _ = gr.family_queries(sk, fam, 8, nq=12)
    whole = gr.reference_counts(sk, q, 8)
    parts = [gr.reference_counts(sk, q, 8, a, b) for a, b in ((0, 64), (64, 200), (200, 256))]
    assert np.array_equal(sum(parts), whole) and all(p.max() > 0 for p in parts)


def test_kernel_code():
    assert gr.decode_kernel(1024 | 32 << 12 | 0 << 20 | 1 << 24) == (1024, 32, -1, 1)
    assert gr.decode_kernel(128 | 16 << 12 | 5 << 20) == (128, 16, 4, 0)
