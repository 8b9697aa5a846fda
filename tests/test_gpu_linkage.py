"""GPU: niqki_linkage, the complete single-linkage hierarchy and its maximum spanning forest in one self-join.

Expected hierarchies come FROM THE DEFINITION: labels_of_matrix (the union-find of tests/test_gpu_cluster.py) of the
oracle's matrix at every distinct count >= floor -- merge_count[g] is the largest such count at which g's label is not
g, merge_into[g] the label there -- and not from any forest.  Expected edges come from a plain Python Kruskal over the
oracle matrix in the edge order (larger count, then smaller lo, then smaller hi)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cluster import (F, S, T_CHAIN10, T_CHAIN20, W, data, labels_of_matrix, oracle_matrix, self_join_splits,
                              union_find)

pytestmark = pytest.mark.gpu

E_STATE = 5
FLOOR = 50


def hierarchy_by_definition(M, floor):
    """(merge_into, merge_count) read off labels_t at every distinct count t >= max(floor, 1), descending"""
    n = M.shape[0]
    ids = np.arange(n, dtype=np.uint32)
    into, cnt = ids.copy(), np.zeros(n, np.uint32)
    off_diag = M[~np.eye(n, dtype=bool)] if n > 1 else np.zeros(0, np.uint32)
    for t in np.unique(off_diag[off_diag >= max(floor, 1)])[::-1]:
        lab = labels_of_matrix(M, t)
        new = (lab != ids) & (into == ids)
        into[new] = lab[new]
        cnt[new] = t
    if floor == 0:
        rest = (into == ids) & (ids > 0)
        into[rest] = 0
    return into, cnt


def kruskal(M, floor):
    """the edges Kruskal keeps when it takes the pairs with count >= max(floor, 1) in the edge order; floor 0: then
    (0, r, 0) for every remaining root r > 0"""
    n = M.shape[0]
    lo, hi = np.nonzero(np.triu(M >= max(floor, 1), 1))
    c = M[lo, hi].astype(np.int64)
    order = np.lexsort((hi, lo, -c))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for a, b, k in zip(lo[order].tolist(), hi[order].tolist(), c[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append((a, b, k))
    if floor == 0:
        out += [(0, r, 0) for r in range(1, n) if find(r) == r]
    e = np.array(out, dtype=np.uint32).reshape(-1, 3)
    return e[:, 0].copy(), e[:, 1].copy(), e[:, 2].copy()


def expected(M, floor):
    into, cnt = hierarchy_by_definition(M, floor)
    lo, hi, c = kruskal(M, floor)
    return into, cnt, lo, hi, c, M.shape[0] - lo.size


def same(got, exp):
    into, cnt, edges, roots = got
    assert into.dtype == np.uint32 and cnt.dtype == np.uint32
    assert np.array_equal(into, exp[0]) and np.array_equal(cnt, exp[1])
    for a, b in zip(edges, exp[2:5]):
        assert a.dtype == np.uint32 and np.array_equal(a, b)
    assert roots == exp[5]


def contract(into, cnt):
    """what the header promises of any hierarchy"""
    ids = np.arange(into.size)
    child = into != ids
    assert np.all(into[child] < ids[child])
    assert np.all(cnt[child] > cnt[into[child]]) or not child.any()
    assert np.all(cnt[~child] == 0)


def engine(native, form, sk, ms=50, S_=S):
    e = native.Engine(K=31, S=S_, W=W, H=3, min_score_value=ms, tile_genomes=128 if form == "tiles" else 0,
                      resident_mib=1 if form == "paged" else 0, top_k=3 if form == "top_k3" else 0)
    if form == "rows":
        e.set_option("hit_lists", 0)
    if form == "batch64":
        e.set_option("query_batch", 64)
    e.insert(sk)
    return e


@pytest.fixture(scope="module")
def tiny(po):
    sk = data(600, 31)
    M = oracle_matrix(po, sk)
    exp = expected(M, FLOOR)
    # what the data must hold, whatever the device does: several trees, a singleton, levels with more than one edge
    assert 1 < exp[5] < 600 and exp[0][11] == 11
    contract(exp[0], exp[1])
    dup = np.nonzero((sk == sk[7]).all(1))[0]
    assert dup.size == 7 and np.all(exp[0][dup[1:]] == 7) and np.all(exp[1][dup[1:]] == M[7, 7]) and M[7, 7] > 900
    return sk, M, exp


FORMS = ["lists", "rows", "tiles", "paged", "batch64", "top_k3"]


@pytest.mark.parametrize("form", FORMS)
def test_linkage_equals_the_definition_and_kruskal(native, tiny, form):
    from niqki_amd import capi
    sk, M, exp = tiny
    e = engine(native, form, sk)
    if form == "paged":
        assert e.stat("pages") >= 4
    q = sk[[7, 100, 11, 500]]
    before = e.query(q)
    same(e.linkage(FLOOR), exp)
    if form == "tiles":
        assert e.stat("tiles") > 1
    assert e.stat("linkage_rounds") >= 1 and e.stat("linkage_splits") == 0
    assert e.stat("linkage_pairs") == int(np.sum(M >= FLOOR))
    # the handle's threshold and top_k are its own again, and a query answers as before
    p = capi.Params()
    assert e.L.niqki_get_params(e.h, C.byref(p)) == 0
    assert p.min_score == 50 and p.top_k == (3 if form == "top_k3" else 0)
    after = e.query(q)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


@pytest.fixture(scope="module")
def small(po):
    sk = data(3000, 11)
    return sk, oracle_matrix(po, sk)


def test_linkage_cuts_equal_cluster(native, small):
    sk, M = small
    N = sk.shape[0]
    e = engine(native, "lists", sk)
    into, cnt, (lo, hi, c), roots = e.linkage(FLOOR)
    contract(into, cnt)
    assert lo.size == N - roots and np.all(lo < hi)
    assert np.array_equal(c, M[lo, hi])                          # edge counts are the oracle's cells
    key = (c.astype(np.int64) << 46) | ((N - lo.astype(np.int64)) << 23) | (N - hi.astype(np.int64))
    assert np.all(np.diff(key) < 0)                              # strictly in edge order
    assert int(np.sum(union_find(N, lo, hi) == np.arange(N))) == roots      # a forest: every edge joins two trees
    for t in (FLOOR, T_CHAIN20, T_CHAIN10, F, F + 1):
        lab = labels_of_matrix(M, t)
        got, n = e.cluster(t)
        cut = native.cut_linkage(into, cnt, t)
        assert np.array_equal(cut, got) and np.array_equal(cut, lab), t
        assert n == int(np.sum(cut == np.arange(N)))
        keep = c >= t
        assert np.array_equal(union_find(N, lo[keep], hi[keep]), lab), t    # the forest cut at t has t's components
    e.close()


def test_linkage_splits_a_batch_whose_hits_exceed_the_room(native):
    N = 3000
    sk = data(N, 12, dense=1500)
    e = engine(native, "lists", sk)
    e.set_option("cluster_ws_mib", 1024)
    ref = e.linkage(T_CHAIN20)
    assert e.stat("linkage_splits") == 0
    assert np.max(np.bincount(native.cut_linkage(ref[0], ref[1], T_CHAIN20))) >= 1500
    n_splits = self_join_splits(native, sk, T_CHAIN20, 1)
    assert n_splits > 0
    for hit_lists in (1, 0):
        e.set_option("hit_lists", hit_lists)
        e.set_option("cluster_ws_mib", 1)
        got = e.linkage(T_CHAIN20)
        assert e.stat("linkage_splits") == n_splits
        same(got, (ref[0], ref[1]) + ref[2] + (ref[3],))
    e.close()


def test_linkage_with_a_delta_segment(native, po):
    N = 6000
    sk = data(N, 13)
    M = oracle_matrix(po, sk)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:5500])
    e.query(sk[:2])                                        # the main index is built
    e.insert(sk[5500:])
    e.query(sk[:2])                                        # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    into, cnt, _, roots = e.linkage(FLOOR, edges=False)
    assert e.stat("delta_genomes") > 0
    contract(into, cnt)
    for t in (FLOOR, T_CHAIN20, T_CHAIN10):
        lab = labels_of_matrix(M, t)
        got, _ = e.cluster(t)
        cut = native.cut_linkage(into, cnt, t)
        assert np.array_equal(cut, got) and np.array_equal(cut, lab), t
    assert roots == int(np.sum(labels_of_matrix(M, FLOOR) == np.arange(N)))
    e.close()


def test_linkage_s16_counts_of_2_to_the_16(native, po):
    S16, N = 16, 40
    F16 = 1 << S16
    rng = np.random.default_rng(5)
    base = rng.integers(0, 1 << W, F16).astype(np.int32)
    sk = np.empty((N, F16), np.int32)
    for i in range(N):
        sk[i] = base
        m = rng.random(F16) < (0.02 + 0.02 * (i % 7))
        sk[i][m] = rng.integers(0, 1 << W, int(m.sum()))
    sk[17] = sk[3]
    p = po.make_params(31, S16, W, 3, 0.0)
    ox = po.Index(p, sk)
    M = np.stack([ox.counts(sk[i]) for i in range(N)]).astype(np.uint32)
    assert M[3, 17] == 65536
    e = native.Engine(K=31, S=S16, W=W, H=3, min_score_value=1000)
    e.insert(sk)
    got = e.linkage(60000)
    into, cnt, (lo, hi, c), roots = got
    assert into[17] == 3 and cnt[17] == 65536
    assert (lo[0], hi[0], c[0]) == (3, 17, 65536)
    same(got, expected(M, 60000))
    for t in (65536, 65537, 62000, 60000):
        lab, _ = e.cluster(t)
        assert np.array_equal(native.cut_linkage(into, cnt, t), lab), t
        assert np.array_equal(lab, labels_of_matrix(M, t)), t
    e.close()


def test_linkage_ties(native, po):
    """Eight patterns of sixteen blocks of 64 cells; a genome is a pattern with some whole blocks taken from the next
    pattern, so the count of two genomes is a sum of whole blocks (plus the chance agreements of two patterns, fixed
    per block): many pairs have EQUAL counts, and the order's tie rules decide the forest.  Twenty exact duplicates."""
    N = 200
    rng = np.random.default_rng(77)
    pat = rng.integers(0, 1 << W, (8, F)).astype(np.int32)
    sk = np.empty((N, F), np.int32)
    for i in range(N):
        p = int(rng.integers(0, 8))
        sk[i] = pat[p]
        for b in np.nonzero(rng.random(16) < 0.4)[0]:
            sk[i, b * 64:(b + 1) * 64] = pat[(p + 1) % 8, b * 64:(b + 1) * 64]
    src = rng.integers(0, 100, 20)
    sk[180:] = sk[src]
    M = oracle_matrix(po, sk)
    exp = expected(M, FLOOR)
    values, mult = np.unique(exp[4], return_counts=True)
    assert int(np.sum(mult[mult > 1])) >= 50                     # kept edges that share their count with another one
    tied = np.isin(np.triu(M, 1), values[mult > 1]) & np.triu(np.ones((N, N), bool), 1)
    assert int(tied.sum()) >= 50                                 # ... and pairs of the graph tied at those counts
    for form in ("lists", "batch64"):
        e = engine(native, form, sk)
        same(e.linkage(FLOOR), exp)
        e.close()


def boruvka_rounds(M, floor):
    """rounds in which Boruvka, every component taking its first incident edge in the edge order, still joins"""
    n = M.shape[0]
    comp = np.arange(n)
    rounds = 0
    while True:
        best = {}
        for a in range(n):
            for b in range(a + 1, n):
                if M[a, b] >= floor and comp[a] != comp[b]:
                    k = (-int(M[a, b]), a, b)
                    for c in (comp[a], comp[b]):
                        if c not in best or k < best[c]:
                            best[c] = k
        if not best:
            return rounds
        rounds += 1
        for _, a, b in best.values():
            ca, cb = comp[a], comp[b]
            if ca != cb:
                comp[comp == max(ca, cb)] = min(ca, cb)


def test_linkage_rounds_of_a_nested_design(native, po):
    """64 genomes, six nested levels: cells of level l are shared by the genomes with equal id >> l, so pairs share
    most cells, pairs of pairs fewer, and so on.  One batch; every round can only join the groups of the next level."""
    N = 64
    rng = np.random.default_rng(3)
    level = np.arange(F) * 7 // F                                # seven equal ranges of cells: levels 0 .. 6
    sk = np.empty((N, F), np.int32)
    tables = [rng.integers(0, 1 << W, (N >> l if l < 7 else 1, F)).astype(np.int32) for l in range(7)]
    for i in range(N):
        for l in range(7):
            m = level == l
            sk[i, m] = tables[l][i >> l][m]
    M = oracle_matrix(po, sk)
    need = boruvka_rounds(M, FLOOR)
    assert need >= 3
    e = engine(native, "lists", sk)
    got = e.linkage(FLOOR)
    assert e.stat("linkage_rounds") >= need
    same(got, expected(M, FLOOR))
    assert got[3] == 1
    e.close()


def test_linkage_floor_0(native, po):
    N = 300
    sk = data(N, 41)
    M = oracle_matrix(po, sk)
    e = engine(native, "lists", sk)
    one = e.linkage(1)
    zero = e.linkage(0)
    same(zero, expected(M, 0))
    into, cnt, (lo, hi, c), roots = zero
    assert roots == 1 and lo.size == N - 1
    old_roots = np.nonzero(one[0] == np.arange(N))[0]
    assert old_roots[0] == 0 and old_roots.size == one[3] > 1
    k = one[2][0].size
    assert all(np.array_equal(a[:k], b) for a, b in zip((lo, hi, c), one[2]))
    assert np.all(lo[k:] == 0) and np.all(c[k:] == 0) and np.array_equal(hi[k:], old_roots[1:])
    assert np.all(into[old_roots] == 0) and np.all(cnt[old_roots] == 0)
    assert np.all(native.cut_linkage(into, cnt, 0) == 0)
    assert np.array_equal(native.cut_linkage(into, cnt, 1), e.cluster(1)[0])
    e.close()


def test_linkage_is_deterministic_and_device_memory(native, tiny):
    import torch
    sk, M, exp = tiny
    N = sk.shape[0]
    a = engine(native, "batch64", sk)
    b = engine(native, "lists", sk)
    r1, r2, rb = a.linkage(FLOOR), a.linkage(FLOOR), b.linkage(FLOOR)
    for r in (r1, r2, rb):
        same(r, exp)
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(r1[:2] + r1[2], r2[:2] + r2[2], rb[:2] + rb[2]))
    # NIQKI_MEM_DEVICE: the five arrays in device memory, the count still in host memory
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    d = [torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda") for _ in range(5)]
    n = C.c_uint32(0)
    assert b.L.niqki_linkage(b.h, FLOOR, *[x.data_ptr() for x in d], C.byref(n), 1) == 0
    torch.cuda.synchronize()
    h = [x.cpu().numpy().astype(np.uint32) for x in d]
    k = N - n.value
    assert n.value == exp[5] and np.array_equal(h[0], exp[0]) and np.array_equal(h[1], exp[1])
    assert all(np.array_equal(x[:k], y) for x, y in zip(h[2:], exp[2:5]))
    assert all(np.all(x[k:] == 0x7FFFFFFF) for x in h[2:])       # the places behind the edges are not written
    # n_roots and each array group may be NULL
    into, cnt = np.empty(N, np.uint32), np.empty(N, np.uint32)
    assert a.L.niqki_linkage(a.h, FLOOR, into.ctypes.data, cnt.ctypes.data, None, None, None, None, 0) == 0
    assert np.array_equal(into, exp[0]) and np.array_equal(cnt, exp[1])
    lo, hi, c = (np.zeros(N, np.uint32) for _ in range(3))
    assert a.L.niqki_linkage(a.h, FLOOR, None, None, lo.ctypes.data, hi.ctypes.data, c.ctypes.data, C.byref(n), 0) == 0
    assert all(np.array_equal(x[:k], y) for x, y in zip((lo, hi, c), exp[2:5])) and n.value == exp[5]
    assert a.L.niqki_linkage(a.h, FLOOR, None, None, None, None, None, C.byref(n), 0) == 0 and n.value == exp[5]
    assert a.L.niqki_linkage(a.h, FLOOR, into.ctypes.data, None, None, None, None, None, 0) != 0     # half a group
    a.close()
    b.close()


def test_linkage_refuses_a_slot_range_shard_and_takes_an_empty_index(native):
    sk = data(200, 2)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=10, slot_begin=0, slot_end=512)
    e.insert(sk)
    out = [np.zeros(200, np.uint32) for _ in range(5)]
    assert e.L.niqki_linkage(e.h, 100, *[x.ctypes.data for x in out], None, 0) == E_STATE
    assert b"slot-range" in e.L.niqki_last_error(e.h)
    e.close()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=10)
    n = C.c_uint32(7)
    assert e.L.niqki_linkage(e.h, 100, None, None, None, None, None, C.byref(n), 0) == 0 and n.value == 0
    into, cnt, edges, roots = e.linkage(0)
    assert into.size == 0 and cnt.size == 0 and all(x.size == 0 for x in edges) and roots == 0
    e.close()
