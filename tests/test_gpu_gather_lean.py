"""GPU: the padded bucket walk whose padding lanes leave the LDS atomics (PairWalk::apply, nq_gather.hip), against the
plain reference of tests/gather_ref.py.

A padded index (bucket_align_log2 6) at S = 10 in which, in every tile, slot s has ONE bucket of exactly
LENGTHS[s % 16] ids and nothing else: 0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193 and 200 -- around
every chunk length at which the mask of a line changes a lane (an odd length leaves a lane with one id and one padding
id; 64 fills the line, 65 leaves a second line with one id) and every cut count of cut_and_walk (one to three chunks
in a round, a second round from 193 on).  F = 1024 gives each of the sixteen waves of the 1024-thread shape exactly one
iteration of 64 slots, so a query that holds a slot's value or nothing decides how many chunks each wave cuts in a tile:
the designed queries leave waves with 0, 1, 63, 64, 65 and 120 chunks -- a last partial batch of 1 chunk and of 63 (all
other places are the tile's "no chunk" line, whose lanes all leave), no partial batch at all, and full batches followed
by one -- and rotate these over the waves.  Run under gather_variant 2 (the padded pair walk) and 3 (512 threads, the
walk with explicit lengths, untouched), with the look-up pre-pass on and off, one tile and two, counter rows and hit
lists (counter-row form and LDS lists)."""
import numpy as np
import pytest

import gather_ref as gr
import hit_designs as hd

pytestmark = pytest.mark.gpu

S, W = 10, 8
F = 1 << S
TILE, LAST = 256, 201            # genomes per tile / of the last tile (odd, >= the longest bucket)
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200)
NQ = 70                          # >= 64 and no multiple of 64, as in tests/gather_ref.py
WAVE_CHUNKS = (1, 63, 64, 65, 0, 120, 2, 62, 66, 119, 120, 64, 1, 63, 3, 61)   # chunks of wave w's 64 slots, rotated per query


def chunks_of(length):
    return -(-length // 64)


def n_genomes(n_tiles):
    return TILE * (n_tiles - 1) + LAST


def designed(n_tiles):
    """(sk, v): in every tile LENGTHS[s % 16] genomes -- a window whose start rotates with s -- hold v[s] in slot s,
    all others hold nothing there"""
    rng = np.random.default_rng(1100 + n_tiles)
    n = n_genomes(n_tiles)
    v = rng.integers(0, 1 << W, F).astype(np.int32)
    sk = np.full((n, F), -1, np.int32)
    L = np.asarray([LENGTHS[s % 16] for s in range(F)])
    for g0 in range(0, n, TILE):
        g1 = min(g0 + TILE, n)
        n_t = g1 - g0
        pos = (np.arange(n_t)[:, None] - (np.arange(F) * 37)[None, :]) % n_t
        m = pos < L[None, :]
        sk[g0:g1][m] = np.broadcast_to(v, (n_t, F))[m]
        assert gr.bucket_lengths(sk[g0:g1], W) == set(LENGTHS), (g0, g1)
    return sk, v


def wave_slots(wave, want):
    """slots of [64 * wave, 64 * wave + 64) whose buckets are cut into exactly `want` chunks in all"""
    slots = sorted(range(64 * wave, 64 * wave + 64), key=lambda s: -chunks_of(LENGTHS[s % 16]))
    took, total = [], 0
    for s in slots:
        c = chunks_of(LENGTHS[s % 16])
        if c and total + c <= want:
            took.append(s)
            total += c
    assert total == want, (wave, want, total)
    return took


def designed_queries(sk, v):
    rng = np.random.default_rng(11)
    n = sk.shape[0]
    rows = [v.copy()]                                     # every wave: 120 chunks, one full batch and 56 more
    assert sum(chunks_of(LENGTHS[s % 16]) for s in range(64)) == 120
    for r in range(16):                                   # the designed chunk counts, rotated over the waves
        q = np.full(F, -1, np.int32)
        for w in range(16):
            took = wave_slots(w, WAVE_CHUNKS[(w + r) % 16])
            q[took] = v[took]
        rows.append(q)
    for g in sorted({0, 1, TILE - 1, TILE, n // 2, n - 2, n - 1} & set(range(n))):
        rows.append(sk[g].copy())
    rows.append(np.full(F, -1, np.int32))                 # nothing to walk at all
    q = v.copy()
    q[::2] = 1 << W                                       # every second cell out of range
    rows.append(q)
    while len(rows) < NQ:                                 # a slot's value, or one whose bucket is empty
        q = v.copy()
        m = rng.random(F) < 0.5
        q[m] = (v[m] + rng.integers(1, 1 << W, int(m.sum()))) % (1 << W)
        rows.append(q)
    return np.stack(rows).astype(np.int32)


class Case:
    pass


_CASES = {}


def case(n_tiles):
    if n_tiles not in _CASES:
        c = Case()
        c.sk, v = designed(n_tiles)
        c.q = designed_queries(c.sk, v)
        assert c.q.shape == (NQ, F)
        c.ref = gr.reference_counts(c.sk, c.q, W)
        assert c.ref[0].min() > 0
        designed_rows = c.ref[1:17]
        c.min_score = int(np.median(designed_rows[designed_rows > 0]))     # about half of what a designed query touches
        c.lists = gr.reference_hits(c.ref, c.min_score)
        sizes = np.diff(c.lists[0])
        assert sizes.min() == 0 and sizes.max() == c.sk.shape[0] and len(set(sizes.tolist())) >= 3, sizes
        assert all(0 < k < c.sk.shape[0] for k in sizes[1:17]), sizes
        _CASES[n_tiles] = c
    return _CASES[n_tiles]


def same_counts(got, ref, what):
    got = np.asarray(got).astype(np.int64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        i, g = (int(x) for x in bad[0])
        raise AssertionError("%s: %d counters differ, first: query %d genome %d got %d expected %d" %
                             (what, len(bad), i, g, got[i, g], ref[i, g]))


@pytest.mark.parametrize("n_tiles", [1, 2])
def test_designed_chunk_lengths_and_partial_batches(native, n_tiles):
    c = case(n_tiles)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=c.min_score, tile_genomes=TILE)
    e.set_option("tile_stripe", 0)
    e.set_option("bucket_align_log2", 6)
    e.insert(c.sk)
    e.build()
    assert e.stat("tiles") == n_tiles and e.stat("bucket_align_log2") == 6
    capacity = int(c.lists[0][-1]) + 1
    for variant, shape in ((2, (1024, 32, 1)), (3, (512, 16, 0))):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            for order in (0, 2):
                e.set_option("query_order", order)
                what = (n_tiles, variant, pre, order)
                same_counts(e.query_counts(c.q), c.ref, what)
                B, U, NT, PAD = gr.decode_kernel(e.stat("last_gather_kernel"))
                assert (B, U, PAD) == shape, what + (B, U, PAD)
                assert (e.stat("last_gather_form") & 1) == pre, what
                assert NT == (-1 if pre else (n_tiles if n_tiles >= 2 else 1)), what + (NT,)
                for lists in (0, 1):
                    e.set_option("hit_lists", lists)
                    d = hd.first_difference(e.query(c.q, capacity=capacity), c.lists)
                    assert d is None, "%s: %s" % (what + (lists,), d)
                    assert gr.decode_kernel(e.stat("last_gather_kernel")) == (B, U, NT, PAD)
    e.close()
