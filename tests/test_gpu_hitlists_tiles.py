"""GPU: the hit-list form (option hit_lists = 1) on indexes of several tiles.  The gather kernel picks a query's hits
from every tile's counters in LDS and orders their union by (count, global gid) after the last tile; a query with more
than hit_list_cap hits -- in one tile, or only in total -- leaves through its counter row.  Every result must equal the
counter-row form's (hit_lists = 0, oracle-pinned elsewhere) byte for byte: offsets, counts and gids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, W = 8, 8
F = 1 << S
STRIPE = 32          # the default tile_stripe: blocks of 32 genomes dealt to the tiles round-robin
COPIES = (7, 39, 71, 103, 135, 167)   # genome 7 and five exact copies, one per block of 32: equal counts in many tiles
MS_HIGH = 250        # only the copies reach it (a query's count against a copy is its number of filled slots)


def data(n, nq, seed):
    rng = np.random.default_rng(seed)
    fam = rng.integers(0, 1 << W, (40, F)).astype(np.int32)
    sk = fam[rng.integers(0, 40, n)].copy()
    noise = rng.random((n, F)) < rng.random((n, 1)) * 0.9    # members from near-identical to unrelated
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[rng.random((n, F)) < 0.01] = -1
    sk[7] = rng.integers(0, 1 << W, F)   # unrelated to every family, every slot filled: its count against itself is F
    sk[n - 5] = np.maximum(sk[n - 5], 0)
    for g in COPIES[1:]:
        sk[g] = sk[7]
    q = fam[rng.integers(0, 40, nq)].copy()
    m = rng.random((nq, F)) < 0.2
    q[m] = rng.integers(0, 1 << W, int(m.sum()))
    q[0] = sk[7]
    q[1] = -1
    q[2] = sk[n - 5]
    return sk, q


def engine(native, sk, tile):
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=100, tile_genomes=tile)
    e.set_option("tile_stripe", STRIPE)
    e.insert(sk)
    e.build()
    return e


def both(e, q):
    """(hit-list form, counter-row form) of one query call; the first must have taken the hit-list form.  The counter
    form runs first, then a call on other queries leaves their counts in the rows the hit-list form falls back on: a
    query whose list overflows must write every part of its row it reads again"""
    e.set_option("hit_lists", 0)
    b = e.query(q)
    assert e.stat("last_hits_form") == 0
    e.query(np.roll(q, 1, axis=0))
    e.set_option("hit_lists", 1)
    a = e.query(q)
    assert e.stat("last_hits_form") == (1 if e.min_score_now else 0)   # (min_score 0: every genome is a hit, rows)
    return a, b


def same(a, b, what):
    for x, y, name in zip(a, b, ("offsets", "counts", "gids")):
        assert np.array_equal(x, y), (what, name)


@pytest.mark.parametrize("tile,n_tiles", [(8192, 2), (5504, 3), (2048, 8)])
def test_lists_of_several_tiles_equal_counter_rows(native, tile, n_tiles):
    N, NQ = 16384, 24
    sk, q = data(N, NQ, 3 + n_tiles)
    e = engine(native, sk, tile)
    assert e.stat("tiles") == n_tiles
    for ms in (MS_HIGH, 100, 40, 0):
        e.set_option("min_score", ms)
        e.min_score_now = ms
        for cap in (4, 256, 2048):
            e.set_option("hit_list_cap", cap)
            for k in (0, 1, 10, cap + 1):
                e.set_option("top_k", k)
                a, b = both(e, q)
                same(a, b, (ms, cap, k))
            e.set_option("top_k", 0)
            off, hc, hg = e.query(q)
            sizes = np.diff(off.astype(np.int64))
            if ms == MS_HIGH:
                # query 0 is genome 7: its copies are its hits, spread over the tiles -- at cap 4 its list overflows
                # only in total (no tile holds more than 4 of them)
                lo, hi = int(off[0]), int(off[1])
                assert sorted(hg[lo:hi].tolist()) == sorted(COPIES) and np.all(hc[lo:hi] == F), (hg[lo:hi], hc[lo:hi])
                assert max(np.bincount((np.array(COPIES) // STRIPE) % n_tiles)) <= 4 < len(COPIES)
            if ms == 40 and cap == 256:
                assert sizes.max() > 256 and np.any((sizes > 0) & (sizes <= 256)), sizes   # both kinds of query
            if ms == 0:
                assert np.all(sizes == N)
    e.close()


def test_lists_of_a_wide_index_equal_counter_rows(native):
    """more than 65 536 genomes: global gids beyond 16 bits, in the lists and in the counter rows of the queries whose
    lists overflow"""
    N, NQ = 70000, 16
    sk, q = data(N, NQ, 11)
    e = engine(native, sk, 0)
    assert e.stat("tiles") == 2
    for ms, cap in ((MS_HIGH, 4), (100, 4), (100, 256), (60, 2048)):
        e.set_option("min_score", ms)
        e.min_score_now = ms
        e.set_option("hit_list_cap", cap)
        for k in (0, 10):
            e.set_option("top_k", k)
            a, b = both(e, q)
            same(a, b, (ms, cap, k))
    e.set_option("top_k", 0)
    e.set_option("min_score", MS_HIGH)
    off, hc, hg = e.query(q)
    lo, hi = int(off[2]), int(off[3])
    assert N - 5 in hg[lo:hi].tolist()
    e.close()


def test_query_ahead_takes_the_lists_of_several_tiles(native):
    """niqki_sketch_ahead / niqki_query_ahead on an 8-tile index: the batch sketched ahead comes back as the counter-row
    form's result for the same sketches"""
    import torch
    N, nq, L = 16384, 12, 20000
    seqs = [native.synth_genome_host(5, i % 3, 100 + i, 40 * i, L - 31 * i) for i in range(nq)]
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=60, tile_genomes=2048)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    qsk = e.sketch(seqs)
    sk, _ = data(N, 3, 17)
    sk[1000:1000 + nq] = qsk          # the queries' own genomes ...
    sk[9000:9000 + nq] = qsk          # ... twice, in other tiles
    e.insert(sk)
    e.build()
    assert e.stat("tiles") == 8
    off = np.zeros(nq + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    buf = torch.from_numpy(np.concatenate(seqs + [np.zeros(native.SEQ_PAD, np.uint8)])).cuda()
    d_off = torch.from_numpy(off).cuda()
    for cap in (4, 256):
        e.set_option("hit_list_cap", cap)
        e.set_option("hit_lists", 0)
        e.query(np.roll(qsk, 1, axis=0))   # (other queries' counts in the counter rows)
        e.set_option("hit_lists", 1)
        e.sketch_ahead_dev(buf, d_off, nq)
        got = e.query_ahead(nq, want_sketches=True)
        assert e.stat("last_hits_form") == 1
        assert np.array_equal(got[3], qsk)
        e.set_option("hit_lists", 0)
        exp = e.query(qsk)
        e.set_option("hit_lists", 1)
        same(got[:3], exp, cap)
        assert np.all(np.diff(got[0].astype(np.int64)) >= 2)   # every query finds its genome and the copy
    e.close()
