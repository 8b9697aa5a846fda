"""GPU: every launch form of the gather kernel (option "gather_variant" 0..5: 1024 x 8, 1024 x 32, 512, 256 and 128
threads, each with the look-ups from the pre-pass, from the stash of 2, 3 and 4 tiles or one per tile, the 1024-thread
shapes also in their padded form) under every bucket alignment (option "bucket_align_log2" -1, 0..6) and in every
output mode (counter rows, hit lists, candidates, survivors, pages, a delta segment, two planes, slot shards, the class
mask), against the plain reference of tests/gather_ref.py -- for every query of every call, never against another
engine call.  The kernel a call launched is read from the stat "last_gather_kernel"; the last test checks that the
module has launched every instantiation launch_gather can produce."""
import numpy as np
import pytest

import gather_ref as gr
import hit_designs as hd

pytestmark = pytest.mark.gpu

VARIANTS = {0: (256, 16), 1: (1024, 8), 2: (1024, 32), 3: (512, 16), 4: (256, 16), 5: (128, 16)}   # tiles <= 12288 for 0
ALIGNS = (-1, 0, 1, 2, 3, 4, 5, 6)
SEEN = set()        # (BLOCK, UNROLL, NT, PAD) of every gather launch of this module
SWEPT = set()       # the cases of the main sweep and of the large-tile test that ran


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for k in ("NIQKI_TILE_STRIPE", "NIQKI_LOOKUP_PREPASS", "NIQKI_HMASK"):
        monkeypatch.delenv(k, raising=False)


def launched(e, variant, n_tiles, align, pre, usable=True, block=None):
    """asserts what the stats say about the last gather launch and notes the kernel"""
    B, U, NT, PAD = gr.decode_kernel(e.stat("last_gather_kernel"))
    took_pre = e.stat("last_gather_form") & 1
    if usable:
        assert took_pre == pre, (variant, pre)
    else:
        assert took_pre <= pre
    if block is None:
        assert (B, U) == VARIANTS[variant], (variant, B, U)
        assert PAD == (1 if align == 6 and variant in (1, 2) else 0), (variant, align, PAD)
    else:
        assert B == block and PAD == (1 if align == 6 else 0), (B, U, PAD, align)
    assert NT == (-1 if took_pre else (n_tiles if 2 <= n_tiles <= 4 else 1)), (NT, took_pre, n_tiles)
    SEEN.add((B, U, NT, PAD))
    return B, U, NT, PAD


def same_counts(got, ref, what):
    got = np.asarray(got).astype(np.int64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        i, g = (int(x) for x in bad[0])
        raise AssertionError("%s: %d counters differ, first: query %d genome %d got %d expected %d" %
                             (what, len(bad), i, g, got[i, g], ref[i, g]))


def same_hits(got, lists, what):
    d = hd.first_difference(got, lists)
    assert d is None, "%s: %s" % (what, d)


# ---- the data sets, each with its reference, made once ---------------------------------------------------------------

class Case:
    pass


_CASES = {}
_FAMILY = {}


def case(name, n_tiles):
    key = (name, n_tiles)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.n_tiles = n_tiles
    if name == "designed":
        c.stripe = 0
        c.sk, v = gr.designed(n_tiles)
        c.q, c.names = gr.designed_queries(c.sk, v)
        c.ref = gr.reference_counts(c.sk, c.q, gr.W)
        # what the case relies on, from the arrays alone
        ranges = gr.tile_ranges(c.sk.shape[0])
        assert len(ranges) == n_tiles and ranges[-1][1] - ranges[-1][0] == gr.LAST and gr.LAST % 2 == 1
        for g0, g1 in ranges:
            assert {x for x in gr.LENGTHS if x <= g1 - g0} <= gr.bucket_lengths(c.sk[g0:g1], gr.W), (g0, g1)
        assert c.ref[0].min() > 0 and c.ref[c.names.index("empty")].max() == 0
        c.min_score = int(np.median(c.ref[1]))     # half the genomes are hits of the first "third replaced" query
    else:
        c.stripe = 32 if name == "families32" else 1
        if not _FAMILY:
            sk, fam = gr.families(1500, gr.S, gr.W, seed=1500 + 320)
            q, where = gr.family_queries(sk, fam, gr.W)
            _FAMILY.update(sk=sk, q=q, where=where, ref=gr.reference_counts(sk, q, gr.W))
        n = 1500 if n_tiles == 5 else gr.n_genomes(n_tiles)
        assert -(-n // gr.TILE) == n_tiles
        c.sk, c.q = _FAMILY["sk"][:n], _FAMILY["q"]
        c.ref = _FAMILY["ref"][:, :n]
        assert c.ref[_FAMILY["where"]["empty"]].max() == 0 and (c.sk == -1).any()
        c.min_score = 600                           # between unrelated genomes (~ F / 2^W) and family members (~ 0.7 F)
    assert c.q.shape == (gr.NQ, gr.F) and gr.NQ >= 64 and gr.NQ % 64
    c.lists = gr.reference_hits(c.ref, c.min_score)
    c.sizes = np.diff(c.lists[0])
    assert len(set(c.sizes.tolist())) >= 3 and c.sizes.min() == 0 and c.sizes.max() > 1, c.sizes
    _CASES[key] = c
    return c


HL_CAP = 160


def engine(native, S, W, sk, tile, stripe, align, min_score=1, **kw):
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=min_score, tile_genomes=tile, **kw)
    e.set_option("tile_stripe", stripe)
    e.set_option("bucket_align_log2", align)
    e.insert(sk)
    return e


def built_as_asked(e, align, n_tiles):
    assert e.stat("tiles") == n_tiles
    a = e.stat("bucket_align_log2")
    assert a == align if align >= 0 else 0 <= a <= 6, (a, align)


# ---- the main sweep --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("n_tiles", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["designed", "families32", "families1"])
def test_every_launch_form_under_every_alignment(native, name, n_tiles, align):
    """counter rows and hits (counter-row form and hit lists) of 70 queries under gather_variant 0..5 x lookup_prepass
    0 / 1 x query_order 0 / 2 on one build; designed bucket lengths in range tiles, families in striped tiles (blocks of
    32: the quad stores of the write-out; single genomes: its element-wise branch)"""
    c = case(name, n_tiles)
    if name == "designed" and n_tiles == 1:
        # lists that fit the hit list (one of them long) and lists that overflow it
        fit = c.sizes[(c.sizes > 0) & (c.sizes <= HL_CAP)]
        assert len(set(fit.tolist())) >= 3 and fit.max() > 100 and c.sizes.max() > HL_CAP, c.sizes
    e = engine(native, gr.S, gr.W, c.sk, gr.TILE, c.stripe, align, c.min_score)
    e.set_option("hit_list_cap", HL_CAP)
    e.build()
    built_as_asked(e, align, n_tiles)
    a = e.stat("bucket_align_log2")
    capacity = int(c.lists[0][-1]) + 1
    for variant in range(6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            for order in (0, 2):
                e.set_option("query_order", order)
                what = (variant, pre, order)
                same_counts(e.query_counts(c.q), c.ref, what)
                shape = launched(e, variant, n_tiles, a, pre)
                assert (e.stat("last_gather_form") & 4) == (4 if order else 0)
                for lists in (0, 1):
                    e.set_option("hit_lists", lists)
                    same_hits(e.query(c.q, capacity=capacity), c.lists, what + (lists,))
                    assert e.stat("last_hits_form") == (1 if lists and n_tiles == 1 else 0)   # (N <= 12288: one tile)
                    assert launched(e, variant, n_tiles, a, pre) == shape
    e.close()
    SWEPT.add((name, n_tiles, align))


BIG_TILE = 12352      # > 12288: the default shape has 1024 threads


@pytest.mark.parametrize("align", [3, 6])
@pytest.mark.parametrize("n_tiles", [1, 2, 3, 4, 5])
def test_default_shape_of_large_tiles(native, n_tiles, align):
    """gather_variant 0 on tiles of more than 12288 genomes: the 1024-thread shapes of the default rule, the stash
    forms of 3 and 4 such tiles and more than four of them included (S = 5: 32 slots keep the index small)"""
    S, W = 5, 8
    n = BIG_TILE * (n_tiles - 1) + gr.LAST
    sk, fam = gr.families(n, S, W, seed=n, n_fam=40, run=30)
    q, where = gr.family_queries(sk, fam, W)
    ref = gr.reference_counts(sk, q, W)
    ms = 16
    lists = gr.reference_hits(ref, ms)
    sizes = np.diff(lists[0])
    assert sizes.min() == 0 and sizes.max() > 20 and ref[where["empty"]].max() == 0
    e = engine(native, S, W, sk, BIG_TILE, 32, align, ms)
    e.build()
    built_as_asked(e, align, n_tiles)
    for pre in (0, 1):
        e.set_option("lookup_prepass", pre)
        for order in (0, 2):
            e.set_option("query_order", order)
            same_counts(e.query_counts(q), ref, (pre, order))
            launched(e, 0, n_tiles, align, pre, block=1024)
            for hl in (0, 1):
                e.set_option("hit_lists", hl)
                same_hits(e.query(q, capacity=int(lists[0][-1]) + 1), lists, (pre, order, hl))
    e.close()
    SWEPT.add(("large", n_tiles, align))


# ---- output modes per block size -------------------------------------------------------------------------------------

def check_lists(cand, n_cand, ref, thr, cap, what):
    """candidate lists as sets: exact totals, -1 behind the entries, distinct ids that qualify, all of them where they fit"""
    for i in range(ref.shape[0]):
        want = np.nonzero(ref[i] >= thr)[0]
        assert n_cand[i] == len(want), what + (i, int(n_cand[i]), len(want))
        k = min(len(want), cap)
        got = cand[i, :k].tolist()
        assert (cand[i, k:] == -1).all(), what + (i,)
        assert len(set(got)) == k and set(got) <= set(want.tolist()), what + (i,)
        if len(want) <= cap:
            assert sorted(got) == want.tolist(), what + (i,)


@pytest.mark.parametrize("align", [0, 5, 6])
def test_candidates_and_survivors_per_block_size(native, align):
    """niqki_query_counts_candidates (lists picked while the counters leave LDS) and niqki_query_survivors (no counter
    row: the tile's counters are scanned in LDS, 4 x BLOCK quads a round, and handed over at zero) on the designed set
    with three tiles; thresholds and capacities at which some lists fit and some overflow"""
    import torch
    dev = torch.device("cuda")
    c = case("designed", 3)
    n, nq = c.sk.shape[0], gr.NQ
    m1, m0 = int(np.median(c.ref[1])), int(np.median(c.ref[0]))
    settings = ((m1, 128, 720), (m0, 64, 512), (12, 64, 700))      # (threshold, capacity, capacity of the survivors)
    for thr, cap, scap in settings:
        for k, room in (((c.ref >= thr).sum(axis=1), cap), ((c.ref >= max(thr // 2, 1)).sum(axis=1), scap)):
            assert np.any(k > room) and np.any((k > 0) & (k <= room)), (thr, room, sorted(set(k.tolist())))
    e = engine(native, gr.S, gr.W, c.sk, gr.TILE, 0, align)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.build()
    built_as_asked(e, align, 3)
    stride = native.row_stride(n)
    dq = torch.from_numpy(c.q).to(dev)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            for thr, cap, scap in settings:
                what = (variant, pre, thr, cap)
                rows = torch.full((nq, stride), 9, dtype=torch.int16, device=dev)
                cand = torch.full((nq, cap), 7, dtype=torch.int32, device=dev)
                n_cand = torch.full((nq,), 7, dtype=torch.int32, device=dev)
                e.query_counts_candidates_dev(dq, nq, rows, stride, thr, cap, cand, n_cand)
                e.synchronize()
                launched(e, variant, 3, align, pre)
                same_counts(rows[:, :n].cpu().numpy().view(np.uint16), c.ref, what)
                check_lists(cand.cpu().numpy(), n_cand.cpu().numpy(), c.ref, thr, cap, what)
                # survivors at half the threshold, without counter rows
                sthr = max(thr // 2, 1)
                cand = torch.full((nq, cap), 7, dtype=torch.int32, device=dev)
                n_cand = torch.full((nq,), 7, dtype=torch.int32, device=dev)
                surv = torch.full((nq, scap, 2), -3, dtype=torch.int32, device=dev)
                n_surv = torch.full((nq,), 7, dtype=torch.int32, device=dev)
                e.query_survivors_dev(dq, nq, thr, sthr, cap, scap, cand, n_cand, surv, n_surv)
                e.synchronize()
                launched(e, variant, 3, align, pre)
                check_lists(cand.cpu().numpy(), n_cand.cpu().numpy(), c.ref, thr, cap, what)
                h_surv, h_ns = surv.cpu().numpy(), n_surv.cpu().numpy()
                for i in range(nq):
                    want = np.nonzero(c.ref[i] >= sthr)[0]
                    assert h_ns[i] == len(want), what + (i,)
                    k = min(len(want), scap)
                    got = h_surv[i, :k]
                    assert len(set(got[:, 0].tolist())) == k and set(got[:, 0].tolist()) <= set(want.tolist()), what + (i,)
                    assert np.array_equal(got[:, 1].astype(np.int64), c.ref[i, got[:, 0]]), what + (i,)
    e.close()


@pytest.mark.parametrize("align", [0, 2, 6])
@pytest.mark.parametrize("tile,n_tiles", [(4160, 3), (3136, 4)])
def test_hit_lists_over_several_tiles_per_block_size(native, tile, n_tiles, align):
    """12 352 genomes (more than the one-tile bound of the hit-list form) in 3 and 4 striped tiles: lists that fit,
    lists that overflow within a tile, and the list of genome 7's copies that overflows only in total, at a tile > 0 --
    the kernel then zeroes the row and replays the list into it.  The rows hold another call's counts beforehand."""
    import test_gpu_hitlists_tiles as ht
    N, NQ = 12352, 24
    assert N > 12288 and -(-N // tile) == n_tiles
    sk, q = ht.data(N, NQ, 3 + n_tiles)
    ref = gr.reference_counts(sk, q, ht.W)
    settings = [(ms, cap) for ms in (ht.MS_HIGH, 40) for cap in (4, 256)]
    lists = {ms: gr.reference_hits(ref, ms) for ms in (ht.MS_HIGH, 40)}
    hits0 = np.nonzero(ref[0] >= ht.MS_HIGH)[0]
    assert hits0.tolist() == list(ht.COPIES)                       # query 0's hits: genome 7 and its copies ...
    per_tile = np.bincount((hits0 // ht.STRIPE) % n_tiles, minlength=n_tiles)
    assert per_tile.max() <= 4 < len(hits0) and per_tile[0] < len(hits0)   # ... more than 4 only in total, at a tile > 0
    sizes = np.diff(lists[40][0])
    assert sizes.max() > 256 and np.any((sizes > 0) & (sizes <= 256)) and np.any(sizes > 4)   # both kinds of query
    assert np.any(np.diff(lists[ht.MS_HIGH][0]) <= 4)
    e = engine(native, ht.S, ht.W, sk, tile, ht.STRIPE, align)
    e.build()
    built_as_asked(e, align, n_tiles)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            for ms, cap in settings:
                e.set_option("min_score", ms)
                e.set_option("hit_list_cap", cap)
                e.set_option("hit_lists", 0)
                e.query(np.roll(q, 1, axis=0))
                e.set_option("hit_lists", 1)
                same_hits(e.query(q, capacity=int(lists[ms][0][-1]) + 1), lists[ms], (variant, pre, ms, cap))
                assert e.stat("last_hits_form") == 1
                launched(e, variant, n_tiles, align, pre)
    e.close()


@pytest.mark.parametrize("align", [0, 1, 6])
def test_paged_handle_per_block_size(native, align):
    """a handle with less memory than its index: the gather kernel adds every page's counts to the rows"""
    c = case("designed", 3)
    e = engine(native, gr.S, gr.W, c.sk, gr.TILE, 0, align, c.min_score, resident_mib=8)
    assert e.stat("pages") >= 4 and e.stat("page_slots") % 64                 # (a last iteration of half a wave)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            same_counts(e.query_counts(c.q), c.ref, (variant, pre))
            launched(e, variant, 3, align, pre)
        same_hits(e.query(c.q, capacity=int(c.lists[0][-1]) + 1), c.lists, (variant,))
    built_as_asked(e, align, 3)
    e.close()


_DELTA = {}


@pytest.mark.parametrize("align", [0, 4, 6])
@pytest.mark.parametrize("n_main", [4097, 4096])
def test_delta_segment_per_block_size(native, n_main, align):
    """genomes inserted after a build (of at least 4096: fewer are rebuilt): a one-tile segment whose first column is
    odd once (the element-wise write of a dense row) and even once, behind a main index of five tiles (the last of one
    genome) or of four"""
    S, W, tile, n_delta, ms = 8, 8, 1024, 500, 80
    n_tiles = -(-n_main // tile)
    assert n_delta <= n_main // 8 and n_tiles == (5 if n_main & 1 else 4)
    if not _DELTA:
        sk, fam = gr.families(4097 + n_delta, S, W, seed=8)
        q, where = gr.family_queries(sk, fam, W)
        _DELTA.update(sk=sk, q=q, ref=gr.reference_counts(sk, q, W))
    n = n_main + n_delta
    sk, q, ref = _DELTA["sk"][:n], _DELTA["q"], _DELTA["ref"][:, :n]
    lists = gr.reference_hits(ref, ms)
    sizes = np.diff(lists[0])
    assert len(set(sizes.tolist())) >= 3 and sizes.min() == 0 and np.any(lists[2] >= n_main)   # hits in the delta too
    e = engine(native, S, W, sk[:n_main], tile, 0, align, ms)
    e.build()
    built_as_asked(e, align, n_tiles)
    e.insert(sk[n_main:])
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            same_counts(e.query_counts(q), ref, (variant, pre))
            assert e.stat("delta_genomes") == n_delta
            launched(e, variant, n_tiles, align, pre)             # (the main index is walked last)
            same_hits(e.query(q, capacity=int(lists[0][-1]) + 1), lists, (variant, pre))
    e.close()


def test_delta_segment_transitions(native):
    """what resets a segment while a delta exists, other than retain / unite / export: an explicit build and the
    options that ask for a full rebuild.  The stats "tiles" and "bucket_align_log2" are the main segment's."""
    S, W, tile, n_main, n_delta, ms = 8, 8, 1024, 4097, 500, 80
    if not _DELTA:
        sk, fam = gr.families(4097 + n_delta, S, W, seed=8)
        q, where = gr.family_queries(sk, fam, W)
        _DELTA.update(sk=sk, q=q, ref=gr.reference_counts(sk, q, W))
    n = n_main + n_delta
    sk, q, ref = _DELTA["sk"][:n], _DELTA["q"], _DELTA["ref"][:, :n]
    lists = gr.reference_hits(ref, ms)
    capacity = int(lists[0][-1]) + 1
    assert np.any(lists[2] >= n_main)                                # hits in the delta too
    # 1: a main segment alone
    e = engine(native, S, W, sk[:n_main], tile, 0, 0, ms)
    e.build()
    assert e.stat("tiles") == 5 and e.stat("delta_genomes") == 0
    b0 = e.stat("index_bytes")
    assert b0 > 0
    # 2: genomes after the build get a delta
    e.insert(sk[n_main:])
    same_counts(e.query_counts(q), ref, "delta")
    assert e.stat("delta_genomes") == n_delta and e.stat("tiles") == 5
    b1 = e.stat("index_bytes")
    assert b1 > b0
    # 3: an explicit build folds it into the main segment and gives its buffers back: the main table keeps its five
    # tiles, its ids grow by at most 500 x 256 x 2 B, the delta held a table of 256 x 256 x 8 B besides its ids
    e.build()
    assert e.stat("delta_genomes") == 0 and e.stat("tiles") == 5
    assert e.stat("index_bytes") < b1
    same_counts(e.query_counts(q), ref, "rebuilt")
    same_hits(e.query(q, capacity=capacity), lists, "rebuilt")
    e.close()
    # 4: a tile size set while a delta exists
    e = engine(native, S, W, sk[:n_main], tile, 0, 0, ms)
    e.build()
    e.insert(sk[n_main:])
    same_counts(e.query_counts(q), ref, "second delta")
    assert e.stat("delta_genomes") == n_delta
    e.set_option("tile_genomes", 2048)
    same_counts(e.query_counts(q), ref, "tile_genomes")
    assert e.stat("delta_genomes") == 0 and e.stat("tiles") == 3     # 4597 genomes in tiles of 2048
    same_hits(e.query(q, capacity=capacity), lists, "tile_genomes")
    # 5: an alignment set with nothing inserted
    e.set_option("bucket_align_log2", 6)
    same_counts(e.query_counts(q), ref, "bucket_align_log2")
    assert e.stat("bucket_align_log2") == 6 and e.stat("delta_genomes") == 0
    e.close()


@pytest.mark.parametrize("align", [0, 2, 6])
def test_two_planes_per_block_size(native, align):
    """S = 16, two tiles: the slots are walked in two passes into two counter planes; a stored sketch without empty
    cells counts 65 536 against itself"""
    S, W, N = 16, 6, 100
    F = 1 << S
    sk, fam = gr.families(N, S, W, seed=16, n_fam=3, run=20)
    sk[5] = np.maximum(sk[5], 0)
    q = np.concatenate([fam, sk[[5, 63, 64, N - 1]], np.full((1, F), -1, np.int32)]).astype(np.int32)
    q[2, ::2] = 1 << W
    ref = gr.reference_counts(sk, q, W)
    assert ref[3, 5] == 65536 and ref[-1].max() == 0
    ms = F // 3
    lists = gr.reference_hits(ref, ms)
    assert 65536 in lists[1].tolist() and len(set(np.diff(lists[0]).tolist())) >= 3
    e = engine(native, S, W, sk, 64, 0, align, ms)
    e.build()
    built_as_asked(e, align, 2)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            same_counts(e.query_counts32(q), ref, (variant, pre))
            launched(e, variant, 2, align, pre)
            same_hits(e.query(q, capacity=int(lists[0][-1]) + 1), lists, (variant, pre))
    e.close()


@pytest.mark.parametrize("align", [0, 1, 6])
def test_half_a_wave_of_slots_per_block_size(native, align):
    """S = 5: 32 slots, half a wave -- fifteen of a 1024-thread workgroup's waves have nothing to walk"""
    S, W = 5, 8
    n = gr.n_genomes(3)
    sk, fam = gr.families(n, S, W, seed=5, n_fam=12, run=40)
    q, where = gr.family_queries(sk, fam, W)
    ref = gr.reference_counts(sk, q, W)
    ms = 12
    lists = gr.reference_hits(ref, ms)
    assert len(set(np.diff(lists[0]).tolist())) >= 3 and ref[where["empty"]].max() == 0
    e = engine(native, S, W, sk, gr.TILE, 0, align, ms)
    e.build()
    built_as_asked(e, align, 3)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            for order in (0, 2):
                e.set_option("query_order", order)
                same_counts(e.query_counts(q), ref, (variant, pre, order))
                launched(e, variant, 3, align, pre)
                same_hits(e.query(q, capacity=int(lists[0][-1]) + 1), lists, (variant, pre, order))
    e.close()


@pytest.mark.parametrize("align", [0, 5, 6])
@pytest.mark.parametrize("slots", [(64, 256), (100, 300)])
def test_slot_shards_per_block_size(native, slots, align):
    """a handle that owns a slot range: 192 slots (whole iterations of 64) and 200 (a last iteration of 8 slots; no
    whole slot blocks, so the pre-pass cannot serve it)"""
    c = case("designed", 3)
    sb, se = slots
    ref = gr.reference_counts(c.sk, c.q, gr.W, sb, se)
    assert ref[0].min() > 0 and ref.max() <= se - sb
    e = engine(native, gr.S, gr.W, c.sk, gr.TILE, 0, align, slot_begin=sb, slot_end=se)
    e.build()
    built_as_asked(e, align, 3)
    for variant in range(1, 6):
        e.set_option("gather_variant", variant)
        for pre in (0, 1):
            e.set_option("lookup_prepass", pre)
            same_counts(e.query_counts(c.q), ref, (variant, pre))
            launched(e, variant, 3, align, pre, usable=(se - sb) % 64 == 0)
    e.close()


@pytest.mark.parametrize("align", [0, 3, 6])
def test_class_mask_form_per_block_size(native, align):
    """S = 14, one tile with its class mask: the masked loop takes 8 iterations per wave at a time -- 8192 slots at 1024
    threads, so only F = 16384 gives it a second outer step.  The genomes hold fingerprints of two classes per slot,
    the queries of all sixteen: most of a query's cells are never looked up."""
    S, W, N, NQ = 14, 8, 200, 16
    F = 1 << S
    rng = np.random.default_rng(14)
    cls = np.stack([np.arange(F) % 16, (np.arange(F) * 7 + 3) % 16])          # the two classes of a slot

    def draw(n):
        return (cls[rng.integers(0, 2, (n, F)), np.arange(F)[None, :]] * 16 + rng.integers(0, 4, (n, F))).astype(np.int32)

    sk = draw(5)[(np.arange(N) // 25) % 5]                                    # families of 50, 50, 50, 25 and 25 genomes
    noise = rng.random((N, F)) < 0.3
    sk[noise] = draw(N)[noise]
    sk[rng.random((N, F)) < 0.02] = -1
    q = sk[rng.integers(0, N, NQ)].copy()
    m = rng.random((NQ, F)) < 0.6
    q[m] = rng.integers(0, 1 << W, int(m.sum()))
    q[3] = -1
    q[4, ::2] = 1 << W
    q[5] = sk[N - 1]
    outside = ((q >= 0) & (q < 256) & (q >> 4 != cls[0][None, :]) & (q >> 4 != cls[1][None, :])).mean()
    assert outside > 0.3                                                    # cells the mask lets the kernel skip
    ref = gr.reference_counts(sk, q, W)
    ms = F // 8
    lists = gr.reference_hits(ref, ms)
    assert len(set(np.diff(lists[0]).tolist())) >= 3
    e = engine(native, S, W, sk, 0, 0, align, ms)
    e.build()
    built_as_asked(e, align, 1)
    assert e.stat("class_mask") == 1
    for variant in (0, 2, 5):
        e.set_option("gather_variant", variant)
        e.set_option("lookup_prepass", 0)
        for lists_on in (0, 1):
            e.set_option("hit_lists", lists_on)
            same_counts(e.query_counts(q), ref, (variant,))
            launched(e, variant, 1, align, 0)
            same_hits(e.query(q, capacity=int(lists[0][-1]) + 1), lists, (variant, lists_on))
    e.close()


# ---- small things ----------------------------------------------------------------------------------------------------

def test_unknown_shapes_and_alignments_are_refused(native):
    c = case("designed", 2)
    e = engine(native, gr.S, gr.W, c.sk, gr.TILE, 0, 2)
    e.set_option("gather_variant", 3)
    same_counts(e.query_counts(c.q[:8]), c.ref[:8], "before")
    before = (e.stat("last_gather_kernel"), e.stat("bucket_align_log2"), e.stat("tiles"))
    for key, value in (("gather_variant", 6), ("gather_variant", -1), ("bucket_align_log2", 7), ("bucket_align_log2", -2)):
        with pytest.raises(native.NiqkiError) as ei:
            e.set_option(key, value)
        assert ei.value.code == 1 and key in str(ei.value), (key, value)     # NIQKI_E_INVALID, with a text
        same_counts(e.query_counts(c.q[:8]), c.ref[:8], (key, value))
        assert (e.stat("last_gather_kernel"), e.stat("bucket_align_log2"), e.stat("tiles")) == before
    e.close()


ALL_KERNELS = sorted(
    # gather_variant 1 and 2: 1024 threads, 8 / 32 lines per round trip, padded or not
    [(1024, u, nt, pad) for u in (8, 32) for nt in (-1, 1, 2, 3, 4) for pad in (0, 1)] +
    # gather_variant 3, 4 (and the default of small tiles), 5
    [(b, 16, nt, 0) for b in (512, 256, 128) for nt in (-1, 1, 2, 3, 4)] +
    # the default of large tiles: 16 lines per round trip with look-ups of its own, padded or not; from the pre-pass
    # only without padding (a padded index with the pre-pass takes 32 lines: listed above)
    [(1024, 16, nt, pad) for nt in (1, 2, 3, 4) for pad in (0, 1)] + [(1024, 16, -1, 0)])


def test_every_instantiation_was_launched():
    """what the sweeps above launched, by the stat, against the full list of gather_kernel instantiations
    launch_gather can produce (44)"""
    ran = {(n, t, a) for n in ("designed", "families32", "families1") for t in range(1, 6) for a in ALIGNS} | \
          {("large", t, a) for t in range(1, 6) for a in (3, 6)}
    assert SWEPT == ran, "this test reads what the sweeps of this module launched: all of them must have run and passed"
    assert len(ALL_KERNELS) == 44 and len(set(ALL_KERNELS)) == 44
    assert sorted(SEEN) == ALL_KERNELS, (sorted(set(ALL_KERNELS) - SEEN), sorted(SEEN - set(ALL_KERNELS)))
