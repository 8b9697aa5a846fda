"""GPU: niqki_cover / niqki_staged_cover, the greedy cover of a query (include/niqki_hip.h).  Expected picks come from
tests/cover_ref.py -- the definition in numpy over the sketches niqki_get_sketches returns (tests/test_cover_ref_cpu.py
holds it to the oracle's query round by round) -- never from the code under test."""
import ctypes as C

import numpy as np
import pytest

from cover_ref import cover_arrays, cover_of, query_kinds, slot_minimum
from test_gpu_cluster import S, W, data, engine

pytestmark = pytest.mark.gpu

F = 1 << S
N = 3000
MS = 50
E_STATE, E_CAPACITY = 5, 4


def mixed_batch(sk, W_, seed=17):
    """About 700 queries of the eight kinds of cover_ref.query_kinds, shuffled: queries that end in round 1, 2, 3, 6
    and 12 lie next to each other."""
    rng = np.random.default_rng(seed)
    n, f = sk.shape
    q = list(query_kinds(sk, W_).values())
    q += [sk[g].copy() for g in rng.integers(0, n, 200)]
    q += [slot_minimum(sk[rng.choice(n, 2, replace=False)]) for _ in range(200)]
    q += [slot_minimum(sk[rng.choice(n, 5, replace=False)]) for _ in range(120)]
    q += [slot_minimum(sk[rng.choice(n, 16, replace=False)]) for _ in range(20)]
    q += [rng.integers(0, 1 << W_, f).astype(np.int32) for _ in range(50)]
    q += [np.full(f, -1, np.int32) for _ in range(50)]
    for g in rng.integers(0, n, 50):
        h = sk[g].copy()
        h[rng.random(f) < 0.5] = 1 << W_
        h[rng.random(f) < 0.25] = -2
        q.append(h)
    q = np.stack(q).astype(np.int32)
    order = np.concatenate([np.arange(8), 8 + rng.permutation(q.shape[0] - 8)])     # the eight named ones stay in front
    return np.ascontiguousarray(q[order])


@pytest.fixture(scope="module")
def case():
    sk = data(N, 11)
    q = mixed_batch(sk, W)
    stored = sk.copy()
    stored[(stored < 0) | (stored >= (1 << W))] = -1          # what niqki_get_sketches returns (checked on the device below)
    full = [cover_of(stored, x, W, MS) for x in q]
    lens = sorted({len(x) for x in full})
    assert lens[0] == 0 and 1 in lens and 2 in lens and lens[-1] >= 5, lens
    return sk, q, full


def expect(full, max_picks):
    return cover_arrays([x[:max_picks or None] for x in full])


def same(got, exp, totals=True):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0])
    for k in range(1, 4 if totals else 3):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], exp[k]), k


def own_params(e, ms, top_k):
    from niqki_amd import capi
    p = capi.Params()
    assert e.L.niqki_get_params(e.h, C.byref(p)) == 0
    assert p.min_score == ms and p.top_k == top_k


@pytest.mark.parametrize("form", ["lists", "rows", "tiles", "batch64", "top_k3", "late"])
def test_cover_equals_the_definition(native, case, form):
    sk, q, full = case
    if form == "late":                               # genomes inserted after the index was built and asked
        e = engine(native, "lists", sk[:2900])
        e.query(q[:2])
        e.insert(sk[2900:])
    else:
        e = engine(native, form, sk)
    assert np.array_equal(e.get_sketches(0, N), np.where((sk >= 0) & (sk < (1 << W)), sk, -1))
    before = e.query(q[:40])
    longest = max(len(x) for x in full)
    for max_picks in (0, 1, 3):
        same(e.cover(q, max_picks=max_picks, totals=True), expect(full, max_picks))
        assert e.stat("cover_recount_mismatches") == 0
        assert e.stat("cover_rounds") == (max_picks or longest + 1)
        assert e.stat("cover_picks") == int(expect(full, max_picks)[0][-1])
    if form == "tiles":
        assert e.stat("tiles") > 1
    own_params(e, MS, 3 if form == "top_k3" else 0)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


def test_cover_with_a_delta_segment(native):
    """a main index of >= 4096 genomes and less than an eighth more: the later genomes have an index of their own, and
    the store columns of both are read"""
    n = 4600
    sk = data(n, 23)
    rng = np.random.default_rng(3)
    q = np.stack([slot_minimum(sk[[g, 4300 + int(rng.integers(0, 300))]]) for g in rng.integers(0, 4300, 30)] +
                 [sk[4400].copy(), sk[10].copy()])
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    e.insert(sk[:4300])
    e.query(q[:2])
    e.insert(sk[4300:])
    got = e.cover(q, totals=True)
    assert e.stat("delta_genomes") == 300 and e.stat("cover_recount_mismatches") == 0
    full = [cover_of(sk, x, W, MS) for x in q]
    assert any(p[1] >= 4300 for x in full for p in x) and any(p[1] < 4300 for x in full for p in x)
    same(got, cover_arrays(full))
    e.close()


def test_wave_and_batch_edges(native, case):
    sk, q, full = case
    e = engine(native, "lists", sk)
    for nq in (1, 63, 64, 65):
        same(e.cover(q[8:8 + nq], totals=True), cover_arrays(full[8:8 + nq]))
        assert e.stat("cover_recount_mismatches") == 0
    e.set_option("query_batch", 64)                  # ... and the same slices across batch borders
    same(e.cover(q[:130], totals=True), cover_arrays(full[:130]))
    e.close()


def test_min_score_one_and_zero(native, case):
    sk, q, _ = case
    kinds = query_kinds(sk, W)
    stored = np.where((sk >= 0) & (sk < (1 << W)), sk, -1)
    res = []
    for ms in (1, 0):
        e = engine(native, "lists", sk, ms=ms)
        # the round loop at length: one random query, unbounded
        one = e.cover(kinds["random"][None, :], totals=True)
        assert e.stat("cover_rounds") == 451 and e.stat("cover_recount_mismatches") == 0
        few = e.cover(q[:64], max_picks=20, totals=True)
        assert e.stat("cover_recount_mismatches") == 0
        own_params(e, ms, 0)
        res.append((one, few))
        e.close()
    exp_one = cover_arrays([cover_of(stored, kinds["random"], W, 1)])
    assert int(exp_one[0][-1]) == 450
    for one, few in res:
        same(one, exp_one)
        same(few, cover_arrays([cover_of(stored, x, W, 1, 20) for x in q[:64]]))
    # the sixteen-genome mixture is fully covered: every valid cell is explained
    i = list(kinds).index("sixteen")
    lo, hi = int(res[0][1][0][i]), int(res[0][1][0][i + 1])
    assert int(res[0][1][1][lo:hi].sum()) == int(((q[i] >= 0) & (q[i] < (1 << W))).sum())


@pytest.mark.parametrize("s,w", [(5, 4), (1, 8), (16, 8)])
def test_small_and_odd_shapes(native, s, w):
    """S = 5: F below a wavefront, chance ties everywhere (the largest-gid rule decides most picks); S = 1: F = 2;
    S = 16: two counter planes"""
    f, n = 1 << s, 300
    rng = np.random.default_rng(s)
    sk = rng.integers(0, 1 << w, (n, f)).astype(np.int32)
    if s == 16:                                       # random sketches of 65 536 cells share 1/256: families instead
        fam = rng.integers(0, 1 << w, (6, f)).astype(np.int32)
        sk = fam[rng.integers(0, 6, n)]
        noise = rng.random((n, f)) < 0.3
        sk[noise] = rng.integers(0, 1 << w, int(noise.sum()))
    sk[rng.random((n, f)) < 0.02] = -1
    sk[5] = sk[17]
    q = np.stack([sk[5], slot_minimum(sk[[3, 200]]), slot_minimum(sk[[1, 50, 99, 250]]),
                  rng.integers(0, 1 << w, f).astype(np.int32), np.full(f, -1, np.int32), sk[299]]).astype(np.int32)
    q[2, ::3] = 1 << w
    ms = {5: 2, 1: 1, 16: 2000}[s]
    e = native.Engine(K=31, S=s, W=w, H=3, min_score_value=ms)
    e.insert(sk)
    for max_picks in (0, 2):
        full = [cover_of(sk, x, w, ms, max_picks) for x in q]
        same(e.cover(q, max_picks=max_picks, totals=True), cover_arrays(full))
        assert e.stat("cover_recount_mismatches") == 0
    if s == 5:
        assert any(len(x) > 2 for x in [cover_of(sk, x, w, ms) for x in q])
    e.close()


def test_device_memory_and_capacity(native, case):
    import torch
    sk, q, full = case
    nq = 200
    exp = cover_arrays(full[:nq])
    total = int(exp[0][-1])
    e = engine(native, "lists", sk)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_q = torch.from_numpy(q[:nq]).cuda()
    fill = 0x7FFFFFFF

    def fresh(cap):
        return (torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda"),
                torch.full((max(cap, 1),), fill, dtype=torch.int32, device="cuda"),
                torch.full((max(cap, 1),), fill, dtype=torch.int32, device="cuda"))

    # too small: the true total, nothing else written; hit_totals NULL
    ho, hc, hg = fresh(total - 1)
    assert e.cover_dev(d_q, nq, 0, ho, hc, hg, None, total - 1) == E_CAPACITY
    torch.cuda.synchronize()
    assert int(ho[nq].item()) == total and int(hc.min().item()) == fill and int(hg.min().item()) == fill
    # the same call with that capacity, twice
    for _ in range(2):
        ho, hc, hg = fresh(total)
        assert e.cover_dev(d_q, nq, 0, ho, hc, hg, None, total) == 0
        torch.cuda.synchronize()
        got = (ho.cpu().numpy().astype(np.uint64), hc.cpu().numpy().astype(np.uint32), hg.cpu().numpy().astype(np.uint32))
        same(got, exp, totals=False)
    ht = torch.full((total,), fill, dtype=torch.int32, device="cuda")
    assert e.cover_dev(d_q, nq, 0, ho, hc, hg, ht, total) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ht.cpu().numpy().astype(np.uint32), exp[3])
    assert e.stat("cover_recount_mismatches") == 0
    # host memory: the same contract
    off = np.zeros(nq + 1, np.uint64)
    hc_h, hg_h, ht_h = (np.full(total, fill, np.uint32) for _ in range(3))
    rc = e.L.niqki_cover(e.h, q[:nq].ctypes.data, nq, 0, off.ctypes.data, hc_h.ctypes.data, hg_h.ctypes.data, ht_h.ctypes.data, total - 1, 0)
    assert rc == E_CAPACITY and int(off[nq]) == total
    assert (hc_h == fill).all() and (hg_h == fill).all() and (ht_h == fill).all()
    rc = e.L.niqki_cover(e.h, q[:nq].ctypes.data, nq, 0, off.ctypes.data, hc_h.ctypes.data, hg_h.ctypes.data, ht_h.ctypes.data, total, 0)
    assert rc == 0
    same((off, hc_h, hg_h, ht_h), exp)
    # capacity = nq x max_picks never fails
    same(e.cover(q[:nq], max_picks=2, capacity=2 * nq, totals=True), expect(full[:nq], 2))
    e.close()


def test_staged_cover(native):
    K, S_, W_, H = 31, 12, 12, 4
    g = [native.synth_genome_host(31, f, m, r, 30000) for f, m, r in ((0, 0, 0), (0, 1, 300), (1, 0, 0), (2, 0, 0), (2, 1, 60), (3, 0, 0))]
    e = native.Engine(K=K, S=S_, W=W_, H=H, J=0.05)
    e.insert(e.sketch(g))

    def fasta(records):
        return b"".join(b">r%d\n" % i + bytes(r) + b"\n" for i, r in enumerate(records))

    files = [fasta([g[0], g[2]]), fasta([g[3]]), fasta([g[5], g[1]]), fasta([g[4][:K]]), fasta([g[2][100:20000]])]
    e.stage_raw(files, None)
    before = e.staged_query()
    got = e.staged_cover(totals=True)
    assert e.stat("cover_recount_mismatches") == 0
    qsk = e.staged_sketch()
    assert qsk.shape[0] == len(files)
    same(got, e.cover(qsk, totals=True))
    stored = e.get_sketches(0, len(g))
    full = [cover_of(stored, x, W_, e.min_score) for x in qsk]
    same(got, cover_arrays(full))
    assert [p[1] for p in full[0]][:2] in ([0, 2], [2, 0]) and len(full[3]) == 0 and len(before[1]) > len(got[1])
    after = e.staged_query()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    same(e.staged_cover(max_picks=1, totals=True), cover_arrays([x[:1] for x in full]))
    e.close()


def test_refusals_and_empty_inputs(native, case):
    sk, q, _ = case
    off = np.full(5, 7, np.uint64)
    hc, hg = np.zeros(64, np.uint32), np.zeros(64, np.uint32)

    def call(e, nq):
        return e.L.niqki_cover(e.h, q.ctypes.data, nq, 0, off.ctypes.data, hc.ctypes.data, hg.ctypes.data, None, 64, 0)

    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=0, slot_end=F // 2)
    shard.insert(sk[:100])
    assert call(shard, 2) == E_STATE and b"slot-range" in shard.L.niqki_last_error(shard.h)
    own_params(shard, MS, 0)
    shard.close()
    paged = engine(native, "paged", sk[:500])
    assert call(paged, 2) == E_STATE and b"paged" in paged.L.niqki_last_error(paged.h)
    own_params(paged, MS, 0)
    paged.close()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    assert call(e, 4) == 0 and not off.any()                     # an empty index
    e.insert(sk[:100])
    off[:] = 7
    assert call(e, 0) == 0 and off[0] == 0                       # no queries
    same(e.cover(np.full((3, F), -1, np.int32), totals=True), cover_arrays([[], [], []]))
    e.close()
