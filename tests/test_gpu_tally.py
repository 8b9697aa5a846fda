"""GPU: niqki_tally_begin / _add / _read / _end, the rows of the LCA calls counted per taxon and per clade on the device
(include/niqki_hip.h).  First designed rows through niqki_tally_add at the edges of tally_rows_kernel -- one table slot
hit by every lane, every lane another slot, more rows than a pass, more distinct taxa than the table, sums beyond 32
bits -- then the rows of niqki_query_lca / niqki_staged_query_lca themselves.  Expected values are tests/tally_ref.py
(pinned on a brute force by tests/test_tally_ref_cpu.py) over the designed rows or over lca_ref.lca_lists of reference
lists -- never from the calls under test."""
import ctypes as C

import numpy as np
import pytest

import hit_designs as hd
from lca_ref import NONE, depths, lca_lists
from tally_ref import concat_rows, tally
from test_gpu_lca import S as LS, W as LW, designed, same

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = 1, 5
S, W = 6, 8
F = 1 << S
PASS_ROWS, SLOTS = 1024, 2048                                  # nq_kernels.h: kTallyPassRows, kTallySlots


def check(got, exp, what=""):
    """(direct, clade, direct_best, clade_best, totals) against tally_ref's"""
    for k, name in enumerate(("direct", "clade", "direct_best", "clade_best")):
        assert got[k].dtype == np.uint64 and got[k].shape == exp[k].shape, (what, name)
        bad = np.flatnonzero(got[k] != exp[k])
        assert bad.size == 0, "%s %s, taxon %d: got %d, expected %d (%d differ)" % (what, name, bad[0], got[k][bad[0]], exp[k][bad[0]], bad.size)
    assert got[4] == exp[4], what
    t = got[4]
    assert t["queries"] == t["classified"] + t["no_hit"] + t["no_common"] and int(got[0].sum()) == t["classified"]
    assert (got[1] >= got[0]).all()


@pytest.fixture(scope="module")
def small(native):
    """a handle that only has to carry a taxonomy: four random genomes at S = 6, all of taxon 0"""
    rng = np.random.default_rng(3)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=4)
    e.insert(rng.integers(0, 1 << W, (4, F)).astype(np.int32))
    yield e
    e.close()


def with_taxonomy(e, parent):
    e.set_taxonomy(np.zeros(4, np.uint32), parent)
    assert e.stat("tally") == 0
    e.tally_begin()
    assert e.stat("tally") == 1 and e.stat("tally_queries") == 0


def test_g1_g2_one_slot_and_every_lane_its_own(small):
    _, _, _, parent = designed()
    with_taxonomy(small, parent)
    rows = (np.full(130, 100, np.uint32), np.arange(130, dtype=np.uint32), np.ones(130, np.uint32))   # two wavefronts and two lanes
    small.tally_add(*rows)
    check(small.tally_read(), tally(rows, parent), "G1")
    assert small.stat("tally_queries") == 130
    small.tally_begin()                                        # on an open tally: cleared
    assert small.stat("tally_queries") == 0
    rows = ((np.arange(64) * 2 + 5).astype(np.uint32), np.full(64, 7, np.uint32), np.ones(64, np.uint32))   # 64 distinct taxa
    small.tally_add(*rows)
    check(small.tally_read(), tally(rows, parent), "G2")


def test_g3_more_rows_than_four_passes_more_taxa_than_the_table(small):
    import torch
    parent = np.zeros(3001, np.uint32)
    taxon = np.concatenate([np.arange(3003) % 3000 + 1, np.full(2000, 7)]).astype(np.uint32)
    rng = np.random.default_rng(4)
    best = rng.integers(0, 65, taxon.size).astype(np.uint32)
    considered = np.ones(taxon.size, np.uint32)
    assert taxon.size == 5003 > 4 * PASS_ROWS and np.unique(taxon).size == 3000 > SLOTS
    exp = tally((taxon, best, considered), parent)
    assert exp[0][7] == 2001 and exp[0][3] == 2 and exp[1][0] == 5003 and exp[0][0] == 0
    with_taxonomy(small, parent)
    small.tally_add(taxon, best, considered)
    host = small.tally_read()
    check(host, exp, "G3 host")
    small.tally_begin()
    small.set_stream(torch.cuda.current_stream().cuda_stream)
    d = [torch.from_numpy(x.view(np.int32)).cuda() for x in (taxon, best, considered)]
    small.tally_add_dev(d[0], d[1], d[2], taxon.size)
    dev = small.tally_read()
    check(dev, exp, "G3 device")
    small.tally_begin()
    for lo, hi in ((0, 1), (1, 1024), (1024, 5003)):           # 1, 1023 and 3979 rows
        small.tally_add(taxon[lo:hi], best[lo:hi], considered[lo:hi])
    check(small.tally_read(), exp, "G3 three calls")
    small.tally_begin()
    small.tally_add_dev(d[0][:1], d[1][:1], d[2][:1], 1)
    small.tally_add(taxon[1:1024], best[1:1024], considered[1:1024])
    small.tally_add_dev(d[0][1024:], d[1][1024:], d[2][1024:], 3979)
    check(small.tally_read(), exp, "G3 three calls, both spaces")


def test_g4_every_kind_of_row(small):
    _, _, _, parent = designed()
    depth = depths(parent)
    assert depth[0] == 0 and depth[126] == 6 and depth[166] == 39 and depth[127] == 0
    # rows without a taxon of both kinds; classified ones at depths 0, 6 and 39, in both trees; taxon 62 (depth 5) only as
    # an ancestor of 125 and 126
    taxon = np.array([NONE, NONE, NONE, 0, 126, 126, 125, 166, 166, 166, 127, 140, 0, NONE], np.uint32)
    considered = np.array([0, 2, 0, 5, 1, 1, 3, 1, 2, 2, 9, 1, 300, 2], np.uint32)
    best = np.array([0, 40, 0, 30, 64, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint32)
    exp = tally((taxon, best, considered), parent)
    assert exp[4] == {"queries": 14, "classified": 10, "no_hit": 2, "no_common": 2}
    assert exp[0][62] == 0 and exp[1][62] == 3 and exp[3][62] == 67 and exp[1][0] == 5 and exp[1][127] == 5 and exp[1][140] == 4
    with_taxonomy(small, parent)
    small.tally_add(taxon, best, considered)
    check(small.tally_read(), exp, "G4")


def test_g5_sums_beyond_32_bits(small):
    _, _, _, parent = designed()
    with_taxonomy(small, parent)
    rows = (np.full(70000, 166, np.uint32), np.full(70000, 65536, np.uint32), np.ones(70000, np.uint32))
    exp = tally(rows, parent)
    assert int(exp[2][166]) == 70000 * 65536 > 1 << 32 and int(exp[3][127]) == 70000 * 65536
    small.tally_add(*rows)
    check(small.tally_read(), exp, "G5")


def test_g6_left_out_arrays(native, small):
    import torch
    _, _, _, parent = designed()
    T = parent.size
    taxon = np.array([NONE, 3, 3, 80, NONE, 166], np.uint32)
    best = np.array([0, 5, 6, 7, 8, 9], np.uint32)
    considered = np.array([0, 1, 1, 2, 3, 1], np.uint32)
    with_taxonomy(small, parent)
    small.tally_add(taxon)                                     # no best_count, no considered
    check(small.tally_read(), tally((taxon, None, None), parent), "G6 neither")
    small.tally_begin()
    small.tally_add(taxon, None, considered)
    small.tally_add(np.zeros(0, np.uint32))                    # n == 0
    check(small.tally_read(), tally((taxon, None, considered), parent), "G6 no best_count")
    small.tally_begin()
    small.tally_add(taxon, best)
    exp = tally((taxon, best, None), parent)
    first = small.tally_read()
    check(first, exp, "G6 no considered")
    again = small.tally_read()                                 # two reads in a row
    assert all(np.array_equal(a, b) for a, b in zip(first[:4], again[:4])) and first[4] == again[4]
    # a read with some or all of the arrays NULL
    tot = native.capi.TallyTotals()
    only = np.zeros(T, np.uint64)
    assert small.L.niqki_tally_read(small.h, None, only.ctypes.data, None, None, C.byref(tot), 0) == 0
    assert np.array_equal(only, exp[1]) and tot.as_dict() == exp[4]
    assert small.L.niqki_tally_read(small.h, None, None, None, None, None, 0) == 0
    only[:] = 0
    assert small.L.niqki_tally_read(small.h, None, None, None, only.ctypes.data, None, 0) == 0 and np.array_equal(only, exp[3])
    # into device tensors
    small.set_stream(torch.cuda.current_stream().cuda_stream)
    d = [torch.full((T,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
    totals = small.tally_read_dev(d[0], d[1], None, d[3])
    got = [x.cpu().numpy().view(np.uint64) for x in d]
    assert totals == exp[4] and np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[3], exp[3])
    assert (d[2] == -1).all().item()
    assert small.tally_read_dev() == exp[4]
    check(small.tally_read(), exp, "G6 after the device reads")


def test_g7_a_bad_row_breaks_the_tally(small):
    _, _, _, parent = designed()
    T = parent.size
    with_taxonomy(small, parent)
    good = np.array([5, 5, 9], np.uint32)
    small.tally_add(good)
    rows = np.array([1, T, 2, 0xFFFFFFFE], np.uint32)
    assert small.L.niqki_tally_add(small.h, rows.ctypes.data, None, None, rows.size, 0) == E_INVALID
    assert b"2 bad rows" in small.L.niqki_last_error(small.h)
    assert small.stat("tally") == 2
    out = np.zeros(T, np.uint64)
    assert small.L.niqki_tally_read(small.h, out.ctypes.data, None, None, None, None, 0) == E_STATE
    assert b"broken" in small.L.niqki_last_error(small.h)
    assert small.L.niqki_tally_add(small.h, good.ctypes.data, None, None, good.size, 0) == E_STATE
    small.tally_begin()
    assert small.stat("tally") == 1
    got = small.tally_read()
    assert all(not x.any() for x in got[:4]) and got[4] == {"queries": 0, "classified": 0, "no_hit": 0, "no_common": 0}
    small.tally_add(good)
    check(small.tally_read(), tally((good, None, None), parent), "G7 afresh")
    small.tally_end()
    assert small.stat("tally") == 0
    small.tally_end()                                          # fine when none is open


def test_g7_bad_rows_in_device_memory_show_at_the_next_read(small):
    """an add from device memory does not synchronise: the call returns NIQKI_OK, the read after it NIQKI_E_INVALID"""
    import torch
    _, _, _, parent = designed()
    T = parent.size
    with_taxonomy(small, parent)
    small.set_stream(torch.cuda.current_stream().cuda_stream)
    rows = torch.from_numpy(np.array([1, T, 2], np.uint32).view(np.int32)).cuda()
    assert small.L.niqki_tally_add(small.h, rows.data_ptr(), None, None, 3, 1) == 0
    assert small.stat("tally") == 1
    out = np.zeros(T, np.uint64)
    assert small.L.niqki_tally_read(small.h, out.ctypes.data, None, None, None, None, 0) == E_INVALID
    assert b"1 bad rows" in small.L.niqki_last_error(small.h)
    assert small.stat("tally") == 2
    assert small.L.niqki_tally_read(small.h, out.ctypes.data, None, None, None, None, 0) == E_STATE
    assert small.L.niqki_tally_add(small.h, rows.data_ptr(), None, None, 1, 1) == E_STATE
    small.tally_begin()
    good = np.array([1, 2], np.uint32)
    small.tally_add(good)
    check(small.tally_read(), tally((good, None, None), parent), "G7 device, afresh")
    small.tally_end()


# ---- through the LCA calls ------------------------------------------------------------------------------------------

PERMILLES = (0, 100, 1000)


@pytest.fixture(scope="module")
def lca_case(native):
    n, Cm, gt, parent = designed()
    rng = np.random.default_rng(8)
    sk, qt = hd.design(Cm, LS, LW, rng)
    types = np.concatenate([np.arange(11), rng.integers(0, 11, 60)])
    q = np.ascontiguousarray(qt[types])
    rows = {(ms, p): tuple(x[types] for x in lca_lists(hd.reference_lists(Cm, ms), gt, parent, p)) for ms in (20, 0) for p in PERMILLES}
    exp = tally(concat_rows([rows[20, p] for p in PERMILLES]), parent)
    assert exp[4]["queries"] == 3 * 71 and exp[4]["no_hit"] > 0 and exp[4]["no_common"] > 0 and exp[4]["classified"] > 0
    return sk, q, gt, parent, rows, exp


def lca_engine(native, lca_case, ms=20):
    sk, _, gt, parent, _, _ = lca_case
    e = native.Engine(K=31, S=LS, W=LW, H=3, min_score_value=ms)
    e.insert(sk)
    e.set_taxonomy(gt, parent)
    return e


def test_lca_calls_feed_the_tally_in_every_form(native, lca_case):
    import torch
    _, q, gt, parent, rows, exp = lca_case
    nq = q.shape[0]
    e = lca_engine(native, lca_case)
    e.tally_begin()
    for p in PERMILLES:
        same(e.query_lca(q, top_permille=p, details=True), rows[20, p])      # the rows the caller gets are unchanged
    check(e.tally_read(), exp, "host")
    assert e.stat("tally_queries") == 3 * nq
    e.set_option("query_batch", 7)
    e.tally_begin()
    for p in PERMILLES:
        same(e.query_lca(q, top_permille=p, details=True), rows[20, p])
    check(e.tally_read(), exp, "host, batches of 7")
    e.tally_begin()
    for p in PERMILLES:                                                       # the three detail arrays NULL
        assert np.array_equal(e.query_lca(q, top_permille=p), rows[20, p][0])
    check(e.tally_read(), exp, "host, no detail arrays")
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_q = torch.from_numpy(q).cuda()
    e.tally_begin()
    for p in PERMILLES:
        out = [torch.full((nq,), 0x7FFFFFFF, dtype=torch.int32, device="cuda") for _ in range(4)]
        e.query_lca_dev(d_q, nq, p, *out)
        torch.cuda.synchronize()
        same(tuple(x.cpu().numpy().view(np.uint32) for x in out), rows[20, p])
    check(e.tally_read(), exp, "device")
    e.tally_begin()
    for p in PERMILLES:
        out = torch.full((nq,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        e.query_lca_dev(d_q, nq, p, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), rows[20, p][0])
    check(e.tally_read(), exp, "device, no detail arrays")
    e.close()


def test_halved_batches_add_every_row_once(native, lca_case):
    import torch
    _, q, gt, parent, rows, _ = lca_case
    e = lca_engine(native, lca_case, ms=0)
    e.set_option("cluster_ws_mib", 1)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    q4 = np.ascontiguousarray(np.tile(q, (4, 1)))                             # 284 lists of 300 hits: more than 65 536
    nq = q4.shape[0]
    r4 = tuple(np.tile(x, 4) for x in rows[0, 100])
    e.tally_begin()
    out = [torch.full((nq,), 0x7FFFFFFF, dtype=torch.int32, device="cuda") for _ in range(4)]
    e.query_lca_dev(torch.from_numpy(q4).cuda(), nq, 100, *out)
    torch.cuda.synchronize()
    assert e.stat("lca_splits") > 0
    same(tuple(x.cpu().numpy().view(np.uint32) for x in out), r4)
    check(e.tally_read(), tally(concat_rows([r4]), parent), "halved")
    e.close()


def test_staged_query_lca_feeds_the_tally(native):
    K, S_, W_, H = 31, 12, 12, 4
    g = [native.synth_genome_host(31, f, m, r, 30000) for f, m, r in ((0, 0, 0), (0, 1, 300), (1, 0, 0), (2, 0, 0), (2, 1, 60), (3, 0, 0))]
    e = native.Engine(K=K, S=S_, W=W_, H=H, J=0.05)
    e.insert(e.sketch(g))
    gt = np.array([0, 1, 2, 3, 4, 5], np.uint32)
    parent = np.array([6, 6, 8, 7, 7, 9, 8, 8, 8, 9], np.uint32)
    e.set_taxonomy(gt, parent)

    def fasta(records):
        return b"".join(b">r%d\n" % i + bytes(r) + b"\n" for i, r in enumerate(records))

    files = [fasta([g[0], g[2]]), fasta([g[3]]), fasta([g[5], g[1]]), fasta([g[4][:K]]), fasta([g[2][100:20000]])]
    e.stage_raw(files, None)
    before = e.staged_query()                                                  # (plain calls are never tallied: the tally is not open yet)
    e.tally_begin()
    assert e.staged_query()[0].size == len(files) + 1                          # ... nor with one open
    parts = []
    for p in (0, 1000):
        exp_rows = lca_lists(before, gt, parent, p)
        same(e.staged_query_lca(top_permille=p, details=True), exp_rows)
        parts.append(exp_rows)
    exp = tally(concat_rows(parts), parent)
    assert exp[4]["queries"] == 2 * len(files)
    check(e.tally_read(), exp, "staged")
    e.close()


def test_lifecycle(native, lca_case):
    sk, q, gt, parent, rows, _ = lca_case
    T = parent.size
    e = native.Engine(K=31, S=LS, W=LW, H=3, min_score_value=20)
    e.insert(sk)
    one = np.array([3], np.uint32)
    out = np.zeros(T, np.uint64)

    def err():
        return e.L.niqki_last_error(e.h)

    # an index without genomes under a taxonomy of taxa alone: every query is a row without a hit, in both memory spaces
    # and with the detail arrays left out
    import torch
    empty = native.Engine(K=31, S=LS, W=LW, H=3, min_score_value=20)
    empty.set_taxonomy(np.zeros(0, np.uint32), parent)
    empty.tally_begin()
    got = empty.query_lca(q[:5], top_permille=100, details=True)
    assert got[0].tolist() == [NONE] * 5 and got[3].tolist() == [0] * 5
    assert empty.query_lca(q[:3]).tolist() == [NONE] * 3
    empty.set_stream(torch.cuda.current_stream().cuda_stream)
    d_t = torch.zeros(4, dtype=torch.int32, device="cuda")
    empty.query_lca_dev(torch.from_numpy(q[:4]).cuda(), 4, 0, d_t)
    torch.cuda.synchronize()
    assert d_t.cpu().numpy().view(np.uint32).tolist() == [NONE] * 4
    got = empty.tally_read()
    assert all(not x.any() for x in got[:4]) and got[4] == {"queries": 12, "classified": 0, "no_hit": 12, "no_common": 0}
    empty.close()
    # before begin, and begin without a taxonomy
    assert e.stat("tally") == 0 and e.stat("tally_queries") == 0
    assert e.L.niqki_tally_read(e.h, out.ctypes.data, None, None, None, None, 0) == E_STATE and b"niqki_tally_begin" in err()
    assert e.L.niqki_tally_add(e.h, one.ctypes.data, None, None, 1, 0) == E_STATE
    assert e.L.niqki_tally_begin(e.h) == E_STATE and b"niqki_set_taxonomy" in err()
    assert e.L.niqki_tally_end(e.h) == 0
    e.set_taxonomy(gt, parent)
    e.tally_begin()
    same(e.query_lca(q, top_permille=100, details=True), rows[20, 100])
    exp = tally(concat_rows([rows[20, 100]]), parent)
    check(e.tally_read(), exp, "open")
    # a call refused before its first batch adds nothing and leaves the tally usable
    taxon = np.zeros(q.shape[0], np.uint32)
    assert e.L.niqki_query_lca(e.h, q.ctypes.data, q.shape[0], 1001, taxon.ctypes.data, None, None, None, 0) == E_INVALID
    assert e.L.niqki_query_lca(e.h, None, q.shape[0], 100, taxon.ctypes.data, None, None, None, 0) == E_INVALID
    assert e.stat("tally") == 1
    check(e.tally_read(), exp, "after refused calls")
    # a refused niqki_set_taxonomy leaves the tally alone
    bad = parent.copy()
    bad[17] = T
    assert e.L.niqki_set_taxonomy(e.h, gt.ctypes.data, gt.size, bad.ctypes.data, T, 0) == E_INVALID
    assert e.stat("tally") == 1
    check(e.tally_read(), exp, "after a refused taxonomy")
    # begin on an open tally clears it
    e.tally_begin()
    got = e.tally_read()
    assert all(not x.any() for x in got[:4]) and got[4]["queries"] == 0
    # after tally_end an LCA call adds nothing
    e.tally_end()
    assert e.stat("tally") == 0
    same(e.query_lca(q, top_permille=100, details=True), rows[20, 100])
    assert e.L.niqki_tally_read(e.h, out.ctypes.data, None, None, None, None, 0) == E_STATE
    e.tally_begin()
    got = e.tally_read()
    assert all(not x.any() for x in got[:4]) and got[4]["queries"] == 0
    # a new taxonomy ends the tally, and so does its removal
    e.set_taxonomy(gt, parent)
    assert e.stat("tally") == 0 and e.L.niqki_tally_add(e.h, one.ctypes.data, None, None, 1, 0) == E_STATE
    e.tally_begin()
    e.set_taxonomy(None, None)
    assert e.stat("tally") == 0 and e.L.niqki_tally_begin(e.h) == E_STATE
    # an insert drops the taxonomy and with it the tally
    e.set_taxonomy(gt, parent)
    e.tally_begin()
    e.tally_add(one)
    e.insert(sk[:2])
    assert e.stat("tally") == 0 and e.stat("taxa") == 0
    assert e.L.niqki_tally_read(e.h, out.ctypes.data, None, None, None, None, 0) == E_STATE
    # ... and so does niqki_retain
    e.set_taxonomy(np.concatenate([gt, gt[:2]]), parent)
    e.tally_begin()
    keep = np.ones(gt.size + 2, np.uint8)
    keep[-2:] = 0
    assert e.retain(keep)[0] == gt.size
    assert e.stat("tally") == 0
    e.close()
    shard = native.Engine(K=31, S=LS, W=LW, H=3, min_score_value=20, slot_begin=0, slot_end=(1 << LS) // 2)
    shard.insert(sk[:10])
    shard.set_taxonomy(gt[:10], parent)
    assert shard.L.niqki_tally_begin(shard.h) == E_STATE and b"slot-range" in shard.L.niqki_last_error(shard.h)
    shard.close()


def test_profiling_times_the_two_kernels(small):
    _, _, _, parent = designed()
    with_taxonomy(small, parent)
    small.profile(True)
    small.tally_add(np.full(5000, 166, np.uint32), np.full(5000, 3, np.uint32))
    small.tally_read()
    add, clade = small.stat("tally_us_add"), small.stat("tally_us_clade")
    small.profile(False)
    assert 0 < add < 1_000_000 and 0 < clade < 1_000_000
