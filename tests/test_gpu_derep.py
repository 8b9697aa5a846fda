"""GPU: niqki_dereplicate, greedy representatives of the indexed genomes in index order.  t is a representative iff no
representative g < t has count(t, g) >= threshold; every other genome gets the linked representative (of any index
position) with the largest count, among equal counts the smallest.  Expected values come from that definition in
numpy over the oracle's matrix for small indexes, and over the neighbour lists of the oracle-pinned
niqki_neighbors_range for the large one -- never from the code under test.  The data and the engine forms are those of
test_gpu_cluster.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cluster import (F, FORMS, S, T_CHAIN10, T_CHAIN20, W, chain, data, engine, labels_of_matrix, oracle_matrix,
                              self_join_splits)

pytestmark = pytest.mark.gpu

E_STATE = 5


def derep_of_matrix(M, thr):
    """the definition over a dense symmetric matrix: (labels, label_counts)"""
    n = M.shape[0]
    L = M >= thr
    np.fill_diagonal(L, False)
    rep = np.zeros(n, bool)
    for t in range(n):
        rep[t] = not np.any(L[t, :t] & rep[:t])
    C_ = np.where(L & rep[None, :], M.astype(np.int64), -1)
    best = np.argmax(C_, axis=1)                          # the first maximum: the smallest representative
    cnt = C_[np.arange(n), best]
    assert np.all(cnt[~rep] >= max(thr, 0))               # rule 1: a linked representative exists
    labels = np.where(rep, np.arange(n), best).astype(np.uint32)
    return labels, np.where(rep, 0, cnt).astype(np.uint32)


def derep_of_lists(n, off, hc, hg):
    """the definition over neighbour lists (off, hc, hg as Engine.neighbors_range returns them for genomes [0, n))"""
    off = off.astype(np.int64)
    rep = np.zeros(n, bool)
    for t in range(n):
        g = hg[off[t]:off[t + 1]]
        rep[t] = not np.any(rep[g[g < t]])
    labels = np.arange(n, dtype=np.uint32)
    counts = np.zeros(n, np.uint32)
    for t in np.nonzero(~rep)[0]:
        g, c = hg[off[t]:off[t + 1]], hc[off[t]:off[t + 1]]
        m = rep[g] & (g != t)
        g, c = g[m], c[m]
        k = np.lexsort((g, -c.astype(np.int64)))[0]       # the largest count, then the smallest id
        labels[t], counts[t] = g[k], c[k]
    return labels, counts


def check(e, thr, exp):
    labels, lc, n = e.dereplicate(thr, counts=True)
    assert labels.dtype == np.uint32 and lc.dtype == np.uint32
    assert np.array_equal(labels, exp[0]), thr
    assert np.array_equal(lc, exp[1]), thr
    assert n == int(np.sum(exp[0] == np.arange(exp[0].size))), thr
    l2, n2 = e.dereplicate(thr)
    assert np.array_equal(l2, labels) and n2 == n
    return labels


@pytest.fixture(scope="module")
def small(po):
    N = 3000
    sk = data(N, 11)
    M = oracle_matrix(po, sk)
    thresholds = [0, 1, T_CHAIN20, T_CHAIN10, F + 1]
    exp = [(t, derep_of_matrix(M, t)) for t in thresholds]
    ids = np.arange(N)
    # what the data must hold, whatever the device does
    assert np.all(exp[0][1][0] == 0) and exp[0][1][1][0] == 0 and np.array_equal(exp[0][1][1][1:], M[1:, 0])
    assert np.array_equal(exp[-1][1][0], ids) and not exp[-1][1][1].any()        # every genome its own representative
    for (t, (lab, lc)), n_rep, n_cl in zip(exp[2:4], (2923, 2965), (2898, 2946)):
        assert int(np.sum(lab == ids)) == n_rep
        assert int(np.sum(labels_of_matrix(M, t) == ids)) == n_cl                 # fewer single-linkage clusters: chains
        assert int(np.sum(lab > ids)) == 5                                        # labels that come AFTER their genome
        dup = np.nonzero((sk == sk[7]).all(1))[0]
        assert dup.size == 7 and dup[0] == 7 and np.all(lab[dup] == 7)
        assert M[7, 7] == 1009 and np.all(lc[dup[1:]] == 1009) and lc[7] == 0
    for t, (lab, lc) in exp[1:]:
        assert lab[11] == 11, t                                                   # the all-empty sketch
        rep = lab == ids
        Lk = M >= t
        np.fill_diagonal(Lk, False)
        assert not Lk[np.ix_(rep, rep)].any()                                     # independent
        assert np.all(rep[lab]) and np.all(Lk[ids[~rep], lab[~rep]])              # dominating, by representatives
    return sk, exp


@pytest.mark.parametrize("form", FORMS)
def test_dereplicate_equals_the_definition_on_the_oracle_matrix(native, small, form):
    from niqki_amd import capi
    sk, exp = small
    e = engine(native, form, sk)
    if form == "paged":
        assert e.stat("pages") >= 4
    q = sk[[7, 100, 11, 2500]]
    before = e.query(q)
    for t, x in exp:
        check(e, t, x)
    if form == "tiles":
        assert e.stat("tiles") > 1
    # the handle's threshold and top_k are its own again, and a query answers as before
    p = capi.Params()
    assert e.L.niqki_get_params(e.h, C.byref(p)) == 0
    assert p.min_score == 50 and p.top_k == (3 if form == "top_k3" else 0)
    after = e.query(q)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


def test_dereplicate_device_memory_null_outputs_and_repeats(native, small):
    import torch
    sk, exp = small
    t, (lab, lc) = exp[2]
    N = sk.shape[0]
    e = engine(native, "lists", sk)
    a = e.dereplicate(t, counts=True)
    b = e.dereplicate(t, counts=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]          # two calls in a row
    assert np.array_equal(a[0], lab) and np.array_equal(a[1], lc)
    # NIQKI_MEM_DEVICE: labels and label_counts in device memory, the count still in host memory
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d = torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    dc = torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    n = C.c_uint32(0)
    assert e.L.niqki_dereplicate(e.h, t, d.data_ptr(), dc.data_ptr(), C.byref(n), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint32), lab) and np.array_equal(dc.cpu().numpy().astype(np.uint32), lc)
    assert n.value == a[2]
    d.fill_(0x7FFFFFFF)
    assert e.L.niqki_dereplicate(e.h, t, d.data_ptr(), None, None, 1) == 0                     # both may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint32), lab)
    assert e.L.niqki_dereplicate(e.h, 0, d.data_ptr(), dc.data_ptr(), C.byref(n), 1) == 0      # threshold 0
    torch.cuda.synchronize()
    assert int(d.abs().max().item()) == 0 and n.value == 1
    assert np.array_equal(dc.cpu().numpy().astype(np.uint32), exp[0][1][1])
    out = np.empty(N, np.uint32)
    assert e.L.niqki_dereplicate(e.h, t, out.ctypes.data, None, None, 0) == 0 and np.array_equal(out, lab)
    e.close()


def test_dereplicate_a_path_in_index_order(native, po):
    """The round loop's worst case: 300 sketches, each linked to the one before and the one after only, at consecutive
    index positions inside one batch.  By the round rule the k-th member is decided in round k."""
    N, L, at = 1024, 300, 400
    rng = np.random.default_rng(31)
    sk = rng.integers(0, 1 << W, (N, F)).astype(np.int32)
    sk[at:at + L] = chain(rng, rng.integers(0, 1 << W, F).astype(np.int32), L, 0.2)
    M = oracle_matrix(po, sk)
    thr = T_CHAIN20
    P = M[at:at + L, at:at + L]
    near, two = np.diagonal(P, 1), np.diagonal(P, 2)
    print("path: consecutive min %d, two apart max %d, threshold %d" % (near.min(), two.max(), thr))
    assert near.min() >= thr and two.max() < thr                                # it IS a path ...
    Lk = M >= thr
    np.fill_diagonal(Lk, False)
    assert int(Lk.sum()) == 2 * (L - 1)                                         # ... and nothing else is linked
    exp = derep_of_matrix(M, thr)
    ids = np.arange(N)
    assert int(np.sum(exp[0][at:at + L] == ids[at:at + L])) == L // 2
    assert np.array_equal(exp[0][at:at + L:2], ids[at:at + L:2])                # every second member, from the first
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.set_option("query_batch", 1024)
    e.insert(sk)
    got = check(e, thr, exp)
    rounds = e.stat("derep_rounds")
    print("derep_rounds", rounds)
    assert rounds >= 2
    e.set_option("query_batch", 64)
    assert np.array_equal(check(e, thr, exp), got)
    assert e.stat("derep_rounds") >= 2
    e.close()


def test_dereplicate_splits_a_batch_whose_hits_exceed_the_room(native, po):
    N = 3000
    sk = data(N, 12, dense=1500)
    M = oracle_matrix(po, sk)
    thr = T_CHAIN20
    assert int(np.sum(M[:1024] >= thr)) > 10 * 65536
    exp = derep_of_matrix(M, thr)
    n_splits = self_join_splits(native, sk, thr, 1)
    assert n_splits > 0
    e = engine(native, "lists", sk)
    e.set_option("cluster_ws_mib", 1)
    a = check(e, thr, exp)
    assert e.stat("derep_splits") == n_splits
    e.set_option("cluster_ws_mib", 1024)
    b = check(e, thr, exp)
    assert e.stat("derep_splits") == 0 and np.array_equal(a, b)
    e.set_option("hit_lists", 0)                           # counter rows: the same split rule
    e.set_option("cluster_ws_mib", 1)
    check(e, thr, exp)
    assert e.stat("derep_splits") == n_splits
    # niqki_cluster is not disturbed by the state the dereplication left, nor the other way round
    lab, _ = e.cluster(thr)
    assert np.array_equal(lab, labels_of_matrix(M, thr))
    check(e, thr, exp)
    e.close()


def test_dereplicate_with_a_delta_segment(native, po):
    N = 6000
    sk = data(N, 13)
    M = oracle_matrix(po, sk)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:5500])
    e.query(sk[:2])                                        # the main index is built
    e.insert(sk[5500:])
    e.query(sk[:2])                                        # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    for t in (T_CHAIN20, T_CHAIN10, 1, 0):
        check(e, t, derep_of_matrix(M, t))
    assert e.stat("delta_genomes") > 0
    e.close()


def test_dereplicate_s16_counts_of_2_to_the_16(native, po):
    """S = 16, two counter planes: genomes 3 and 17 share all 65 536 cells, which a wrapped u16 would read as 0."""
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
    assert M[3, 17] == 65536 and np.sum(M >= 65536) == N + 2
    e = native.Engine(K=31, S=S16, W=W, H=3, min_score_value=1000)
    e.insert(sk)
    for t in (65536, 65537, 60000, 62000, 1, 0):
        check(e, t, derep_of_matrix(M, t))
    labels, lc, n = e.dereplicate(65536, counts=True)
    assert labels[17] == 3 and lc[17] == 65536 and n == N - 1
    e.close()


def test_dereplicate_refuses_a_slot_range_shard_and_takes_an_empty_index(native):
    sk = data(200, 2)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=10, slot_begin=0, slot_end=512)
    e.insert(sk)
    out = np.zeros(200, np.uint32)
    assert e.L.niqki_dereplicate(e.h, 100, out.ctypes.data, None, None, 0) == E_STATE
    assert b"slot-range" in e.L.niqki_last_error(e.h)
    e.close()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=10)
    n = C.c_uint32(7)
    assert e.L.niqki_dereplicate(e.h, 100, None, None, C.byref(n), 0) == 0 and n.value == 0
    labels, lc, k = e.dereplicate(0, counts=True)
    assert labels.size == 0 and lc.size == 0 and k == 0
    e.close()


def test_dereplicate_large_index_against_its_neighbour_lists(native):
    """70 000 genomes (two tiles), S = 8, no dense matrix: the three structural properties and the definition, both
    over the lists niqki_neighbors_range gives on the same handle at the same threshold."""
    S8, N, THR = 8, 70000, 150
    F8 = 1 << S8
    rng = np.random.default_rng(21)
    n_fam = 2500
    fam = rng.integers(0, 1 << W, (n_fam, F8)).astype(np.int32)
    sk = fam[rng.integers(0, n_fam, N)].copy()
    noise = rng.random((N, F8)) < (rng.random((N, 1)) * 0.5)     # from identical to half replaced
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[12345] = -1
    e = native.Engine(K=31, S=S8, W=W, H=3, min_score_value=THR)
    e.insert(sk)
    offs, hcs, hgs, base = [np.zeros(1, np.uint64)], [], [], 0
    for t0 in range(0, N, 7000):
        off, hc, hg = e.neighbors_range(t0, t0 + 7000)
        offs.append(off[1:] + np.uint64(base))
        hcs.append(hc)
        hgs.append(hg)
        base += int(off[-1])
    assert e.stat("tiles") > 1
    off, hc, hg = np.concatenate(offs), np.concatenate(hcs), np.concatenate(hgs).astype(np.int64)
    exp = derep_of_lists(N, off, hc, hg)
    ids = np.arange(N)
    n_rep = int(np.sum(exp[0] == ids))
    assert n_fam <= n_rep < N and exp[0][12345] == 12345 and int(np.sum(exp[0] > ids)) > 0
    src = np.repeat(ids, np.diff(off.astype(np.int64)))
    for qb in (1024, 4096):
        e.set_option("query_batch", qb)
        labels, lc, n = e.dereplicate(THR, counts=True)
        rep = labels == ids
        assert n == int(rep.sum())
        link = src != hg
        assert not np.any(rep[src[link]] & rep[hg[link]])                         # independent
        assert np.all(rep[labels])                                                # labels are representatives
        assert np.all(np.isin(ids[~rep] * N + labels[~rep].astype(np.int64), src[link] * N + hg[link]))   # dominating
        assert np.array_equal(labels, exp[0]) and np.array_equal(lc, exp[1]) and n == n_rep, qb
    e.close()
