"""GPU: niqki_set_sizes / niqki_query_contained / niqki_staged_query_contained, per query the hits chosen and ordered by
their share (include/niqki_hip.h).  Expected lists are tests/contain_ref.py (pinned on fractions and on the header the
kernels compile by tests/test_contain_ref_cpu.py) over the full ordered lists of the existing, oracle-pinned Engine.query
at top_k = 0, or over hit_designs.reference_lists of a designed count matrix -- never from the calls under test."""
import numpy as np
import pytest

import contain_ref as cr
import hit_designs as hd
from collapse_ref import few_cell_query
from lists_ref import room, splits
from test_gpu_cluster import S, W, data, engine
from test_gpu_cover import mixed_batch, own_params

pytestmark = pytest.mark.gpu

F = 1 << S
N = 3000
MS = 50
E_INVALID, E_CAPACITY, E_STATE = 1, 4, 5
FILL = 0x7FFFFFFF
TOP = (1 << 40) - 1
MODES = (cr.QUERY, cr.GENOME, cr.MAX)


def size_sets(n, seed=5):
    rng = np.random.default_rng(seed)
    random = (10 ** rng.uniform(1, 7, n)).astype(np.uint64)              # six orders of magnitude
    third = random.copy()
    third[::3] = 0
    return {
        "equal": np.full(n, 4_000_000, np.uint64),
        "ascending": (1000 + 997 * np.arange(n)).astype(np.uint64),
        "descending": (1000 + 997 * np.arange(n))[::-1].astype(np.uint64),
        "random": random,
        "third_zero": third,
        "top": np.full(n, TOP, np.uint64),
    }


def query_sizes(full, sizes, seed=6):
    """per query: 1; 0; the size of its best hit's genome (7 without a hit); 2^40 - 1; random with a zero in ten"""
    off, _, gids = full
    nq = off.size - 1
    rng = np.random.default_rng(seed)
    best = np.array([int(sizes[int(gids[int(off[i])])]) if off[i + 1] > off[i] else 7 for i in range(nq)], np.uint64)
    mixed = (10 ** rng.uniform(1, 7, nq)).astype(np.uint64)
    mixed[rng.random(nq) < 0.1] = 0
    return {"one": np.ones(nq, np.uint64), "zero": np.zeros(nq, np.uint64), "best": best, "top": np.full(nq, TOP, np.uint64), "mixed": mixed}


class Case:
    """the index, the batch, its full lists, and every expected result asked for so far"""

    def __init__(self, sk, q, full):
        self.sk, self.q, self.full = sk, q, tuple(np.asarray(x).astype(np.int64) for x in full)
        self.sizes = size_sets(sk.shape[0])
        self.memo = {}

    def sub(self, nq):
        return hd.deal(self.full, np.arange(nq))

    def expect(self, sizes, qs, mode, min_share, k=0, nq=None):
        key = (sizes.tobytes(), qs.tobytes(), mode, min_share, k, nq)
        if key not in self.memo:
            self.memo[key] = cr.contain_lists(self.full if nq is None else self.sub(nq), sizes, qs, mode, min_share, k, F=F)
        return self.memo[key]


@pytest.fixture(scope="module")
def case(native):
    sk = data(N, 11)
    rng = np.random.default_rng(41)
    q = np.concatenate([mixed_batch(sk, W), np.stack([few_cell_query(sk, g, W, rng) for g in (100, 1234)])])
    e = engine(native, "lists", sk)
    full = e.query(q, capacity=1 << 20)                     # the full ordered lists: top_k = 0 at min_score 50
    e.close()
    lens = np.diff(full[0].astype(np.int64))
    assert lens.min() == 0 and (lens == 1).any() and lens.max() > 256
    assert (q == -1).all(1).any()                            # all-empty sketches
    assert int(full[0][-1]) > 65536                          # what test_budget relies on
    return Case(sk, q, full)


def same(got, exp, unsized=True):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0])
    for k in range(1, 5 if unsized else 4):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], exp[k]), k


@pytest.mark.parametrize("form", ["lists", "rows", "tiles", "batch64", "top_k3", "paged", "late"])
def test_contained_equals_the_definition(native, case, form):
    sk, q = case.sk, case.q
    if form == "late":                               # genomes inserted after the index was built and asked
        e = engine(native, "lists", sk[:2900])
        e.query(q[:2])
        e.insert(sk[2900:])
    else:
        e = engine(native, form, sk)
    k = 3 if form == "top_k3" else 0
    before = e.query(q[:40])
    sizes = case.sizes["random"]
    qs = query_sizes(case.full, sizes)["mixed"]
    e.set_sizes(sizes)
    assert e.stat("sizes") == N
    for mode in MODES:
        for min_share in (0, 1 << 31):
            same(e.query_contained(q, qs, mode, min_share, unsized=True), case.expect(sizes, qs, mode, min_share, k))
    if form == "tiles":
        assert e.stat("tiles") > 1
    if form == "paged":
        assert e.stat("pages") >= 4
    own_params(e, MS, k)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


def test_with_a_delta_segment(native):
    """a main index of >= 4096 genomes and less than an eighth more: the later genomes have an index of their own"""
    n = 4600
    sk = data(n, 23)
    rng = np.random.default_rng(3)
    q = np.stack([sk[g] for g in rng.integers(0, n, 60)] + [sk[4400].copy(), np.full(F, -1, np.int32)])
    sizes = size_sets(n)["random"]
    qs = (10 ** rng.uniform(3, 7, q.shape[0])).astype(np.uint64)
    whole = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    whole.insert(sk)
    full = whole.query(q, capacity=1 << 20)
    whole.close()
    assert (full[2] >= 4300).any() and (full[2] < 4300).any()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    e.insert(sk[:4300])
    e.query(q[:2])
    e.insert(sk[4300:])
    e.set_sizes(sizes)
    got = e.query_contained(q, qs, cr.MAX, 1 << 30, unsized=True)
    assert e.stat("delta_genomes") == 300
    same(got, cr.contain_lists(full, sizes, qs, cr.MAX, 1 << 30, F=F))
    e.close()


def test_designed_sizes(native, case):
    """the first 60 queries (the eight named kinds among them) under every designed size vector and query-size vector;
    every mode x threshold on the random sizes, every mode at 0 and a half and the two extreme thresholds elsewhere"""
    nq = 60
    q = case.q[:nq]
    sub = case.sub(nq)
    lens = np.diff(sub[0])
    assert lens.min() == 0 and lens.max() > 256
    e = engine(native, "lists", case.sk)
    for name, sizes in case.sizes.items():
        e.set_sizes(sizes)
        qsets = query_sizes(sub, sizes)
        for qname in ("one", "zero", "best", "top", "mixed") if name in ("equal", "random") else ("mixed", "best"):
            qs = qsets[qname]
            if (name, qname) == ("random", "mixed"):
                combos = [(mode, ms) for mode in MODES for ms in (0, 1, 1 << 31, cr.ONE)]
            else:
                combos = [(mode, ms) for mode in MODES for ms in (0, 1 << 31)] + [(cr.QUERY, 1), (cr.QUERY, cr.ONE)]
            for mode, min_share in combos:
                exp = case.expect(sizes, qs, mode, min_share, nq=nq)
                same(e.query_contained(q, qs, mode, min_share, unsized=True), exp)
            # a threshold that is a share of the result: the >= edge (the median share of the unthresholded lists)
            all_shares = np.sort(case.expect(sizes, qs, cr.QUERY, 0, nq=nq)[1])
            if all_shares.size:
                at = int(all_shares[all_shares.size // 2])
                exp = case.expect(sizes, qs, cr.QUERY, at, nq=nq)
                assert (exp[1] == at).any()
                same(e.query_contained(q, qs, cr.QUERY, at, unsized=True), exp)
        if name == "third_zero":
            exp = case.expect(sizes, qsets["top"], cr.QUERY, 0, nq=nq)
            assert 0 < int(exp[4].sum()) < int(sub[0][-1]) and int(exp[4].sum()) + int(exp[0][-1]) == int(sub[0][-1])
    # what the definition implies, on the expected arrays (the calls above were held to them)
    eq = case.sizes["equal"]
    qsets = query_sizes(sub, eq)
    for mode in MODES:
        h = case.expect(eq, qsets["best"], mode, 0, nq=nq)                   # equal sizes: H itself, ties and all
        assert np.array_equal(h[0], sub[0]) and np.array_equal(h[2], sub[1]) and np.array_equal(h[3], sub[2]) and not h[4].any()
        one = case.expect(eq, qsets["one"], cr.QUERY, cr.ONE, nq=nq)         # query sizes 1: every share is 1, the list one tie
        assert np.array_equal(one[0], sub[0]) and np.array_equal(one[3], sub[2]) and (one[1] == cr.ONE).all()
        zero = case.expect(eq, qsets["zero"], mode, 0, nq=nq)                # query sizes 0: nothing, all unsized
        assert not zero[0].any() and np.array_equal(zero[4], lens)
    e.close()


def edge_design():
    """One query type that lists all 3000 genomes at min_score 0 with counts spread over 0 .. 1000, sizes that make its
    shares distinct around every survivor count of the route edges, and the thresholds that leave exactly those."""
    rng = np.random.default_rng(12)
    C = rng.integers(0, 1001, (1, N))
    sizes = rng.integers(1_000_000, 10_000_000, N).astype(np.uint64)
    qsize = 10_000_000                                       # no genome is larger: every share is below 1
    full = hd.reference_lists(C, 0)
    shares = np.sort(cr.contain_lists(full, sizes, [qsize], cr.QUERY, 0, F=F)[1].astype(np.int64))[::-1]
    targets = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, N)
    thresholds = []
    for m in targets:
        thr = int(shares[0]) + 1 if m == 0 else int(shares[m - 1])
        assert thr <= cr.ONE and int((shares >= thr).sum()) == m, m          # (distinct at every edge)
        thresholds.append(thr)
    return C, sizes, qsize, full, targets, thresholds


def test_route_edges_on_a_designed_index(native):
    """survivors 0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049 and all 3000 of one list of 3000; cuts 1, 3 and
    beyond the list; the lists the radix passes order are counted"""
    C, sizes, qsize, full1, targets, thresholds = edge_design()
    rng = np.random.default_rng(13)
    sk, qt = hd.design(C, S, W, rng)
    q = np.ascontiguousarray(qt[[0, 0, 0]])
    full = hd.deal(full1, [0, 0, 0])
    qs = np.array([qsize, 0, qsize], np.uint64)                               # the middle one: unsized throughout
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=0)
    e.insert(sk)
    e.set_sizes(sizes)
    for m, thr in zip(targets, thresholds):
        for k in (0, 1, 3, N + 7):
            e.set_option("top_k", k)
            exp = cr.contain_lists(full, sizes, qs, cr.QUERY, thr, k, F=F)
            assert np.diff(exp[0].astype(np.int64)).tolist() == [min(m, k or m), 0, min(m, k or m)] and exp[4].tolist() == [0, N, 0]
            same(e.query_contained(q, qs, cr.QUERY, thr, unsized=True), exp)
            assert e.stat("contain_long_lists") == (2 if m > 2048 else 0)
    # the other modes over the whole list, and a size vector of ties only (the list stays H)
    e.set_option("top_k", 0)
    for mode in (cr.GENOME, cr.MAX):
        same(e.query_contained(q, qs, mode, 0, unsized=True), cr.contain_lists(full, sizes, qs, mode, 0, F=F))
    e.set_sizes(np.full(N, qsize, np.uint64))
    got = e.query_contained(q, qs, cr.QUERY, 0, unsized=True)
    same(got, cr.contain_lists(full, np.full(N, qsize), qs, cr.QUERY, 0, F=F))
    assert np.array_equal(got[3][:N], full1[2]) and np.array_equal(got[2][:N], full1[1])
    assert e.stat("contain_long_lists") == 2
    e.close()


def test_batch_edges(native, case):
    e = engine(native, "lists", case.sk)
    sizes = case.sizes["random"]
    e.set_sizes(sizes)
    for nq in (1, 63, 64, 65):
        sub = hd.deal(case.full, np.arange(8, 8 + nq))
        qs = np.arange(1, nq + 1, dtype=np.uint64) * 50_000
        same(e.query_contained(case.q[8:8 + nq], qs, cr.MAX, 1 << 28, unsized=True), cr.contain_lists(sub, sizes, qs, cr.MAX, 1 << 28, F=F))
    e.close()


def test_budget_splits_leave_the_result_unchanged(native, case):
    """1 MiB of hit buffers hold 65 536 hits; the batch's full lists hold more (checked on the expected arrays)"""
    assert int(case.full[0][-1]) > 65536
    n_splits = splits(np.diff(case.full[0]), 1024, room(1, N), False)
    assert n_splits > 0
    sizes = case.sizes["random"]
    qs = query_sizes(case.full, sizes)["mixed"]
    e = engine(native, "lists", case.sk)
    e.set_option("cluster_ws_mib", 1)
    e.set_sizes(sizes)
    same(e.query_contained(case.q, qs, cr.QUERY, 0, unsized=True), case.expect(sizes, qs, cr.QUERY, 0))
    assert e.stat("contain_splits") == n_splits
    e.set_option("top_k", 3)
    same(e.query_contained(case.q, qs, cr.QUERY, 0, unsized=True), case.expect(sizes, qs, cr.QUERY, 0, 3))
    assert e.stat("contain_splits") == n_splits
    e.close()


def test_s16_counts_reach_65536(native):
    s, w, n = 16, 8, 200
    f = 1 << s
    rng = np.random.default_rng(16)
    fam = rng.integers(0, 1 << w, (6, f)).astype(np.int32)
    sk = fam[rng.integers(0, 6, n)]
    noise = rng.random((n, f)) < 0.3
    sk[noise] = rng.integers(0, 1 << w, int(noise.sum()))
    sk[rng.random((n, f)) < 0.02] = -1
    sk[17] = fam[2]
    sk[5] = sk[17]                                    # an exact duplicate without an empty cell
    q = np.stack([sk[5], sk[3], sk[199], fam[0], rng.integers(0, 1 << w, f).astype(np.int32), np.full(f, -1, np.int32), sk[50], sk[51]])
    sizes = rng.integers(1, 1 << 40, n).astype(np.uint64)
    sizes[17] = TOP
    qs = rng.integers(1, 1 << 40, q.shape[0]).astype(np.uint64)
    qs[0] = TOP
    e = native.Engine(K=31, S=s, W=w, H=3, min_score_value=1000)
    e.insert(sk)
    full = e.query(q, capacity=8 * n)
    assert int(full[1][0]) == 65536
    e.set_sizes(sizes)
    for mode in MODES:
        got = e.query_contained(q, qs, mode, 0, unsized=True)
        same(got, cr.contain_lists(full, sizes, qs, mode, 0, F=f))
    assert 65536 in got[2].tolist()
    own_params(e, 1000, 0)
    e.close()


def test_device_memory_and_capacity(native, case):
    import torch
    nq = 200
    sizes = case.sizes["third_zero"]
    qs = query_sizes(case.sub(nq), sizes)["mixed"]
    mode, min_share = cr.MAX, 1 << 29
    exp = case.expect(sizes, qs, mode, min_share, nq=nq)
    total = int(exp[0][-1])
    assert total > 0 and exp[4].any()
    e = engine(native, "lists", case.sk)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.set_sizes(case.sizes["equal"])
    e.set_sizes(torch.from_numpy(sizes.view(np.int64)).cuda())          # a device array replaces the sizes
    d_q = torch.from_numpy(case.q[:nq]).cuda()
    d_qs = torch.from_numpy(qs.view(np.int64)).cuda()

    def fresh(cap):
        return (torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda"),) + tuple(
            torch.full((max(cap, 1),), FILL, dtype=torch.int32, device="cuda") for _ in range(3)) + (
            torch.full((nq,), FILL, dtype=torch.int32, device="cuda"),)

    ho, hs, hc, hg, nu = fresh(total - 1)
    assert e.query_contained_dev(d_q, d_qs, nq, mode, min_share, ho, hs, hc, hg, nu, total - 1) == E_CAPACITY
    torch.cuda.synchronize()
    assert int(ho[nq].item()) == total
    assert np.array_equal(ho.cpu().numpy().astype(np.uint64), exp[0])    # hit_off is complete
    for with_unsized in (True, False):
        ho, hs, hc, hg, nu = fresh(total)
        assert e.query_contained_dev(d_q, d_qs, nq, mode, min_share, ho, hs, hc, hg, nu if with_unsized else None, total) == 0
        torch.cuda.synchronize()
        got = (ho.cpu().numpy().astype(np.uint64),) + tuple(x.cpu().numpy().view(np.uint32) for x in (hs, hc, hg, nu))
        same(got, exp, unsized=with_unsized)
        assert with_unsized or int(nu.min().item()) == FILL
    # host memory: the same contract
    off = np.zeros(nq + 1, np.uint64)
    hs_h, hc_h, hg_h = (np.full(total, FILL, np.uint32) for _ in range(3))
    nu_h = np.full(nq, FILL, np.uint32)

    def host_call(cap):
        return e.L.niqki_query_contained(e.h, case.q[:nq].ctypes.data, qs.ctypes.data, nq, mode, min_share, off.ctypes.data, hs_h.ctypes.data,
                                         hc_h.ctypes.data, hg_h.ctypes.data, nu_h.ctypes.data, cap, 0)

    assert host_call(total - 1) == E_CAPACITY and int(off[nq]) == total and np.array_equal(off, exp[0])
    assert (hs_h == FILL).all() and (hc_h == FILL).all() and (hg_h == FILL).all()
    assert host_call(total) == 0
    same((off, hs_h, hc_h, hg_h, nu_h), exp)
    # capacity = nq x k never fails with top_k = k
    e.set_option("top_k", 2)
    same(e.query_contained(case.q[:nq], qs, mode, min_share, unsized=True, capacity=2 * nq), case.expect(sizes, qs, mode, min_share, 2, nq=nq))
    own_params(e, MS, 2)
    # a device query size that does not fit ends the call
    bad = qs.copy()
    bad[5] = 1 << 40
    ho, hs, hc, hg, nu = fresh(total)
    with pytest.raises(Exception, match="2\\^40"):
        e.query_contained_dev(d_q, torch.from_numpy(bad.view(np.int64)).cuda(), nq, mode, min_share, ho, hs, hc, hg, nu, total)
    own_params(e, MS, 2)
    e.close()


def test_state(native, case):
    sk, q = case.sk, case.q
    off = np.full(5, 7, np.uint64)
    hs, hc, hg = (np.zeros(4096, np.uint32) for _ in range(3))
    qs4 = np.full(4, 1000, np.uint64)

    def call(e, nq=2, mode=0, qs=qs4):
        return e.L.niqki_query_contained(e.h, q.ctypes.data, qs.ctypes.data, nq, mode, 0, off.ctypes.data, hs.ctypes.data, hc.ctypes.data,
                                         hg.ctypes.data, None, 4096, 0)

    def set_raw(e, sizes):
        return e.L.niqki_set_sizes(e.h, sizes.ctypes.data, sizes.size, 0)

    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, top_k=5)
    assert call(e, 4) == 0 and not off.any()                     # an empty index: empty lists
    e.insert(sk[:500])
    before = e.query(q[:40])
    assert call(e) == E_STATE and b"niqki_set_sizes" in e.L.niqki_last_error(e.h)
    assert e.stat("sizes") == 0
    sz = (np.arange(500) * 1000 + 1).astype(np.uint64)
    assert set_raw(e, sz[:499]) == E_INVALID and call(e) == E_STATE                   # wrong n
    assert set_raw(e, sz) == 0 and e.stat("sizes") == 500 and call(e) == 0
    too_big = sz.copy()
    too_big[250] = 1 << 40
    assert set_raw(e, too_big) == E_INVALID and b"2^40" in e.L.niqki_last_error(e.h)
    assert e.stat("sizes") == 500 and call(e) == 0                                    # ... and the old sizes stay
    assert set_raw(e, sz[:499]) == E_INVALID and e.stat("sizes") == 500
    assert call(e, mode=3) == E_INVALID
    big_q = qs4.copy()
    big_q[1] = 1 << 40
    assert call(e, qs=big_q) == E_INVALID
    own_params(e, MS, 5)
    off[:] = 7
    assert call(e, 0) == 0 and off[0] == 0                       # no queries
    e.set_sizes(None)
    assert call(e) == E_STATE and e.stat("sizes") == 0
    # every call that adds or drops genomes removes the sizes; labels do not touch them
    assert set_raw(e, sz) == 0 and call(e) == 0
    e.set_labels(np.arange(500, dtype=np.uint32))
    e.set_labels(None)
    assert e.stat("sizes") == 500 and call(e) == 0
    e.insert(sk[500:510])
    assert call(e) == E_STATE
    sz = (np.arange(510) * 1000 + 1).astype(np.uint64)
    assert set_raw(e, sz) == 0 and call(e) == 0
    keep = np.ones(510, np.uint8)
    keep[500:] = 0
    assert e.retain(keep)[0] == 500
    assert call(e) == E_STATE
    assert set_raw(e, sz[:500]) == 0 and call(e) == 0
    other = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    other.insert(sk[600:620])
    e.append_dump(other.export_dump())
    other.close()
    assert e.n_genomes == 520 and call(e) == E_STATE
    assert set_raw(e, np.arange(1, 521, dtype=np.uint64)) == 0 and call(e) == 0
    own_params(e, MS, 5)                                         # ... also after the failing calls
    e.retain(np.arange(520) < 500)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert set_raw(e, sz[:500]) == 0
    e.unite(np.arange(500, dtype=np.uint32) // 2)
    assert e.stat("sizes") == 0 and call(e) == E_STATE
    assert set_raw(e, sz[:e.n_genomes]) == 0                     # queries without a hit: empty lists
    got = e.query_contained(np.full((3, F), -1, np.int32), qs4[:3], unsized=True)
    assert got[0].tolist() == [0, 0, 0, 0] and all(x.size == 0 for x in got[1:4]) and got[4].tolist() == [0, 0, 0]
    e.close()
    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=0, slot_end=F // 2)
    shard.insert(sk[:100])
    assert set_raw(shard, sz[:100]) == 0
    assert call(shard) == E_STATE and b"slot-range" in shard.L.niqki_last_error(shard.h)
    own_params(shard, MS, 0)
    shard.close()


def test_staged_query_contained(native):
    K, S_, W_, H = 31, 12, 12, 4
    g = [native.synth_genome_host(31, f, m, r, 30000) for f, m, r in ((0, 0, 0), (0, 1, 300), (1, 0, 0), (2, 0, 0), (2, 1, 60), (3, 0, 0))]
    e = native.Engine(K=K, S=S_, W=W_, H=H, J=0.05)
    e.insert(e.sketch(g))
    sizes = np.array([30000, 29000, 0, 31000, 90000, 30000], np.uint64)
    e.set_sizes(sizes)

    def fasta(records):
        return b"".join(b">r%d\n" % i + bytes(r) + b"\n" for i, r in enumerate(records))

    files = [fasta([g[0], g[2]]), fasta([g[3]]), fasta([g[5], g[1]]), fasta([g[4][:K]]), fasta([g[2][100:20000]])]
    qs = np.array([60000, 30000, 0, 1, 19900], np.uint64)
    e.stage_raw(files, None)
    before = e.staged_query()
    got = e.staged_query_contained(qs, cr.GENOME, 1 << 20, unsized=True)
    qsk = e.staged_sketch()
    assert qsk.shape[0] == len(files)
    same(got, e.query_contained(qsk, qs, cr.GENOME, 1 << 20, unsized=True))
    same(got, cr.contain_lists(before, sizes, qs, cr.GENOME, 1 << 20, F=1 << S_))
    assert got[4].any() and int(got[0][-1]) > 0
    after = e.staged_query()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()
