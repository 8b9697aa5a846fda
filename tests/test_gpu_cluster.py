"""GPU: niqki_cluster, single-linkage clusters of the indexed genomes on the device: a and b are linked when their
co-occurrence count is >= threshold, labels[g] = the smallest genome id of g's connected component.  Expected labels
come from a union-find in numpy (the larger root hooked under the smaller one) over the oracle's thresholded matrix
for small indexes, and over the hits of the existing, oracle-pinned Engine.query for the large one."""
import ctypes as C

import numpy as np
import pytest

from lists_ref import room, splits

pytestmark = pytest.mark.gpu

S, W = 10, 8
F = 1 << S


def union_find(n, a, b):
    """labels of n nodes under the links (a[i], b[i]): the smallest id of each connected component"""
    parent = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    while True:
        while True:                                   # full path compression
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[a], parent[b]
        m = ra != rb
        if not m.any():
            return parent.astype(np.uint32)
        hi, lo = np.maximum(ra[m], rb[m]), np.minimum(ra[m], rb[m])
        np.minimum.at(parent, hi, lo)                 # hook the larger root under the smallest root that asks


def labels_of_matrix(M, thr):
    a, b = np.nonzero(np.triu(M >= thr, 1))
    return union_find(M.shape[0], a, b)


def chain(rng, base, length, step):
    """`length` sketches, each the one before with a share `step` of its cells drawn again: consecutive members share
    about 1 - step of their cells, members two apart (1 - step)^2"""
    out = [base.copy()]
    for _ in range(length - 1):
        s = out[-1].copy()
        m = rng.random(F) < step
        s[m] = rng.integers(0, 1 << W, int(m.sum()))
        out.append(s)
    return out


# thresholds between the shares of neighbours and of members two apart (chance agreement adds about F / 256 = 4)
T_CHAIN20 = int(0.72 * F)     # 20 % chains: 0.80 F = 819 links, 0.64 F = 655 does not
T_CHAIN10 = int(0.86 * F)     # 10 % chains: 0.90 F = 922 links, 0.81 F = 829 does not


def data(n, seed, dense=0):
    """Several families with noise, chains of both step sizes (their members scattered over the index), exact
    duplicates, an all-empty sketch; dense: that many near-copies of one sketch (one large, dense cluster)."""
    rng = np.random.default_rng(seed)
    fam = rng.integers(0, 1 << W, (12, F)).astype(np.int32)
    sk = fam[rng.integers(0, 12, n)].copy()
    noise = rng.random((n, F)) < 0.35
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[rng.random((n, F)) < 0.01] = -1
    free = rng.permutation(np.arange(20, n))
    at = 0
    for step in (0.2, 0.1):
        for _ in range(6):
            for s in chain(rng, rng.integers(0, 1 << W, F).astype(np.int32), 9, step):
                sk[free[at]] = s
                at += 1
    if dense:
        base = rng.integers(0, 1 << W, F).astype(np.int32)
        for _ in range(dense):
            s = base.copy()
            m = rng.random(F) < 0.03
            s[m] = rng.integers(0, 1 << W, int(m.sum()))
            sk[free[at]] = s
            at += 1
    for i in range(6):
        sk[free[at + i]] = sk[7]                      # exact duplicates of genome 7
    sk[11] = -1                                       # all-empty: a singleton at any threshold >= 1
    return sk


def oracle_matrix(po, sk):
    p = po.make_params(31, S, W, 3, 0.0)
    return po.Index(p, sk).matrix_range(0, sk.shape[0]).astype(np.uint32)


def has_chain(M, thr, labels):
    """a cluster whose members are not all pairwise linked"""
    for r in np.unique(labels):
        g = np.nonzero(labels == r)[0]
        if g.size >= 3 and not np.all((M[np.ix_(g, g)] >= thr) | np.eye(g.size, dtype=bool)):
            return True
    return False


def check(e, exp):
    labels, n = e.cluster(exp[0])
    assert labels.dtype == np.uint32 and np.array_equal(labels, exp[1])
    assert n == int(np.sum(exp[1] == np.arange(exp[1].size)))
    return labels


@pytest.fixture(scope="module")
def small(po):
    N = 3000
    sk = data(N, 11)
    M = oracle_matrix(po, sk)
    thresholds = [0, 1, T_CHAIN20, T_CHAIN10, F + 1]
    exp = [(t, labels_of_matrix(M, t)) for t in thresholds]
    # what the data must hold, whatever the device does
    assert np.all(exp[0][1] == 0)
    assert np.array_equal(exp[-1][1], np.arange(N))                       # only singletons
    assert exp[1][1][11] == 11 and np.sum(exp[1][1] == 11) == 1
    for t, lab in exp[2:4]:
        n_cl = int(np.sum(lab == np.arange(N)))
        assert 1 < n_cl < N and has_chain(M, t, lab), t
    dup = np.nonzero((sk == sk[7]).all(1))[0]
    assert dup.size == 7 and np.all(exp[3][1][dup] == 7)
    return sk, exp


FORMS = ["lists", "rows", "tiles", "paged", "batch64", "batch4096", "top_k3"]


def engine(native, form, sk, ms=50):
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms, tile_genomes=512 if form == "tiles" else 0,
                      resident_mib=4 if form == "paged" else 0, top_k=3 if form == "top_k3" else 0)
    if form == "rows":
        e.set_option("hit_lists", 0)
    if form == "batch64":
        e.set_option("query_batch", 64)
    if form == "batch4096":
        e.set_option("query_batch", 4096)
    e.insert(sk)
    return e


def self_join_splits(native, sk, thr, mib, batch=1024):
    """the halvings a self-join call at threshold thr makes (lists_ref.py), from the full list lengths of the stored
    sketches: Engine.neighbors_range at min_score thr and top_k = 0, not the call under test"""
    e = engine(native, "lists", sk, ms=thr)
    off = e.neighbors_range(0, sk.shape[0])[0]
    e.close()
    return splits(np.diff(off.astype(np.int64)), batch, room(mib, sk.shape[0]), True)


@pytest.mark.parametrize("form", FORMS)
def test_cluster_equals_union_find_of_the_oracle_matrix(native, small, form):
    from niqki_amd import capi
    sk, exp = small
    e = engine(native, form, sk)
    if form == "paged":
        assert e.stat("pages") >= 4
    q = sk[[7, 100, 11, 2500]]
    before = e.query(q)
    for x in exp:
        check(e, x)
    if form == "tiles":
        assert e.stat("tiles") > 1
    # the handle's threshold and top_k are its own again, and a query answers as before
    p = capi.Params()
    assert e.L.niqki_get_params(e.h, C.byref(p)) == 0
    assert p.min_score == 50 and p.top_k == (3 if form == "top_k3" else 0)
    after = e.query(q)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


def test_cluster_is_deterministic_and_device_memory(native, small):
    import torch
    sk, exp = small
    t, lab = exp[2]
    a = engine(native, "batch64", sk)
    b = engine(native, "lists", sk)
    la1, n1 = a.cluster(t)
    la2, n2 = a.cluster(t)
    lb, nb = b.cluster(t)
    assert np.array_equal(la1, la2) and np.array_equal(la1, lb) and np.array_equal(la1, lab) and n1 == n2 == nb
    # NIQKI_MEM_DEVICE: labels in device memory, the count still in host memory
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    d = torch.full((sk.shape[0],), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    n = C.c_uint32(0)
    assert b.L.niqki_cluster(b.h, t, d.data_ptr(), C.byref(n), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint32), lab) and n.value == nb
    assert b.L.niqki_cluster(b.h, 0, d.data_ptr(), C.byref(n), 1) == 0        # threshold 0: everything is one cluster
    torch.cuda.synchronize()
    assert int(d.abs().max().item()) == 0 and n.value == 1
    # n_clusters may be NULL
    out = np.empty(sk.shape[0], np.uint32)
    assert a.L.niqki_cluster(a.h, t, out.ctypes.data, None, 0) == 0 and np.array_equal(out, lab)
    a.close()
    b.close()


def test_cluster_splits_a_batch_whose_hits_exceed_the_room(native, po):
    """One dense cluster of 1 500 genomes: a batch of 1 024 stored sketches has about 0.75 M hits, the smallest hit
    buffers (cluster_ws_mib = 1: 65 536 hits) hold a tenth of that."""
    N = 3000
    sk = data(N, 12, dense=1500)
    M = oracle_matrix(po, sk)
    thr = T_CHAIN20
    lab = labels_of_matrix(M, thr)
    assert np.max(np.bincount(lab)) >= 1500
    assert int(np.sum(M[:1024] >= thr)) > 10 * 65536
    n_splits = self_join_splits(native, sk, thr, 1)
    assert n_splits > 0
    e = engine(native, "lists", sk)
    e.set_option("cluster_ws_mib", 1)
    got, n = e.cluster(thr)
    assert e.stat("last_hits_form") == 1                   # the shape that takes hit lists
    assert e.stat("cluster_splits") == n_splits
    assert np.array_equal(got, lab) and n == int(np.sum(lab == np.arange(N)))
    e.set_option("cluster_ws_mib", 1024)
    got, _ = e.cluster(thr)
    assert e.stat("cluster_splits") == 0 and np.array_equal(got, lab)
    e.set_option("hit_lists", 0)                           # counter rows: the same split rule
    e.set_option("cluster_ws_mib", 1)
    got, _ = e.cluster(thr)
    assert e.stat("cluster_splits") == n_splits and np.array_equal(got, lab)
    e.close()


def test_cluster_with_a_delta_segment(native, po):
    N = 6000
    sk = data(N, 13)
    M = oracle_matrix(po, sk)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:5500])
    e.query(sk[:2])                                        # the main index is built
    e.insert(sk[5500:])
    e.query(sk[:2])                                        # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    for t in (T_CHAIN20, T_CHAIN10, 1):
        lab = labels_of_matrix(M, t)
        got, n = e.cluster(t)
        assert np.array_equal(got, lab) and n == int(np.sum(lab == np.arange(N))), t
    assert e.stat("delta_genomes") > 0
    e.close()


def test_cluster_s16_counts_of_2_to_the_16(native, po):
    """S = 16, two counter planes: the count compared with the threshold is the exact sum.  Genomes 3 and 17 share all
    65 536 cells: they link at threshold 65 536 (a wrapped u16 would read 0), nothing else does."""
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
    for t in (65536, 65537, 60000, 62000, 1):
        lab = labels_of_matrix(M, t)
        got, n = e.cluster(t)
        assert np.array_equal(got, lab) and n == int(np.sum(lab == np.arange(N))), t
    got, n = e.cluster(65536)
    assert got[17] == 3 and n == N - 1
    e.close()


def test_cluster_large_index_against_the_query_path(native):
    """70 000 genomes (more than kHitListMaxTile, two tiles), S = 8: the expectation is the union-find of the hits the
    existing query path returns for the stored sketches, fetched by the test in slices."""
    S8, N, THR = 8, 70000, 150
    F8 = 1 << S8
    rng = np.random.default_rng(21)
    n_fam = 2500
    fam = rng.integers(0, 1 << W, (n_fam, F8)).astype(np.int32)
    ids = rng.integers(0, n_fam, N)
    sk = fam[ids].copy()
    noise = rng.random((N, F8)) < (rng.random((N, 1)) * 0.5)     # from identical to half replaced
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[12345] = -1
    e = native.Engine(K=31, S=S8, W=W, H=3, min_score_value=THR)
    e.insert(sk)
    a, b = [], []
    for t0 in range(0, N, 7000):
        off, _, hg = e.query(e.get_sketches(t0, 7000))
        a.append(np.repeat(np.arange(t0, t0 + 7000), np.diff(off.astype(np.int64))))
        b.append(hg.astype(np.int64))
    assert e.stat("tiles") > 1
    a, b = np.concatenate(a), np.concatenate(b)
    lab = union_find(N, a, b)
    n_cl = int(np.sum(lab == np.arange(N)))
    assert n_fam <= n_cl < N and lab[12345] == 12345 and np.max(np.bincount(lab)) > 5
    for qb in (1024, 4096):
        e.set_option("query_batch", qb)
        got, n = e.cluster(THR)
        assert np.array_equal(got, lab) and n == n_cl, qb
    e.close()
