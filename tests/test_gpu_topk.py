"""GPU: top-k queries (niqki_params.top_k, option "top_k"): with k > 0 a query's result is the first min(k, n) entries
of the list it returns with k = 0 -- count descending, the larger gid first among equal counts -- selected on the device
(hits_select_kernel on counter rows, the hit-list scan / emit on the short-read shape).  Every expectation below is the
oracle's full list, or the same handle's k = 0 result (oracle-pinned elsewhere), cut to k."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def data(S, W, N, nq, seed, dup=8):
    """Families of sketches with noise; `dup` exact copies of genome 7 (ties that straddle any cut) and queries that
    are genome 7 itself or members of its family."""
    rng = np.random.default_rng(seed)
    F = 1 << S
    fam = rng.integers(0, 1 << W, (20, F)).astype(np.int32)
    sk = fam[rng.integers(0, 20, N)].copy()
    noise = rng.random((N, F)) < 0.35
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[rng.random((N, F)) < 0.01] = -1
    for i in range(dup):
        sk[N // 2 + 37 * i] = sk[7]
    q = fam[rng.integers(0, 20, nq)].copy()
    m = rng.random((nq, F)) < 0.2
    q[m] = rng.integers(0, 1 << W, int(m.sum()))
    q[0] = sk[7]
    q[1] = -1
    return sk, q


def lists(res):
    off, hc, hg = res
    return [(hc[int(off[i]):int(off[i + 1])], hg[int(off[i]):int(off[i + 1])]) for i in range(off.size - 1)]


def cut(full, k):
    return [(c[:k], g[:k]) if k else (c, g) for c, g in full]


def same(got, exp):
    assert len(got) == len(exp)
    for i, ((a, b), (c, d)) in enumerate(zip(got, exp)):
        assert np.array_equal(a, c) and np.array_equal(b, d), (i, a[:8], b[:8], c[:8], d[:8])


def oracle_lists(po, S, W, sk, q, ms):
    p = po.make_params(31, S, W, 3, 0.0)
    p.min_score = ms
    ix = po.Index(p, sk)
    return [ix.query(x, min_score=ms) for x in q]


def query_rc(e, q, cap):
    """niqki_query with exactly `cap` entries of room: (status, off)"""
    q = np.ascontiguousarray(q, dtype=np.int32)
    nq = q.shape[0]
    off = np.zeros(nq + 1, np.uint64)
    hc, hg = np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
    rc = e.L.niqki_query(e.h, q.ctypes.data, nq, off.ctypes.data, hc.ctypes.data, hg.ctypes.data, cap, 0)
    return rc, off


def ks(N):
    return [1, 3, 10, 64, N - 1, N, N + 5]


@pytest.mark.parametrize("ms", [0, 90, 300])
@pytest.mark.parametrize("form", ["lists", "lists_overflow", "rows", "tiles"])
def test_topk_equals_the_oracle_cut(native, po, ms, form):
    S, W, N, NQ = 10, 8, 3000, 24
    sk, q = data(S, W, N, NQ, 5)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms, tile_genomes=512 if form == "tiles" else 0)
    if form == "rows":
        e.set_option("hit_lists", 0)
    if form == "lists_overflow":
        e.set_option("hit_list_cap", 8)
    e.insert(sk)
    full = oracle_lists(po, S, W, sk, q, ms)
    assert max(len(c) for c, _ in full) > 64
    same(lists(e.query(q)), full)
    assert e.stat("last_hits_form") == (1 if form.startswith("lists") else 0)
    if form == "tiles":
        assert e.stat("tiles") > 1
    for k in ks(N):
        e.set_option("top_k", k)
        rc, off = query_rc(e, q, NQ * k)
        assert rc == 0, k                                     # capacity nq x k is always enough
        got = lists(e.query(q))
        same(got, cut(full, k))
    # the ties: genome 7 and its 8 copies have the query's top count; a cut inside them keeps the largest gids
    c0, g0 = full[0]
    assert np.sum(c0 == c0[0]) == 9
    e.set_option("top_k", 4)
    c, g = lists(e.query(q[:1]))[0]
    assert np.all(c == c0[0]) and np.array_equal(g, np.sort(g0[:9])[::-1][:4])
    e.close()


def test_topk_many_blocks_and_overflowing_lists(native, po):
    """9 000 genomes on 256 slots: several compaction blocks per row, and on the hit-list form the queries whose lists
    overflow take the counter row through the select (more hits than the emit kernel's network holds)."""
    S, W, N, NQ = 8, 8, 9000, 20
    sk, q = data(S, W, N, NQ, 8)
    for ms in (0, 40):
        full = oracle_lists(po, S, W, sk, q, ms)
        for hl in (1, 0):
            e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms)
            e.set_option("hit_lists", hl)
            e.set_option("hit_list_cap", 16)
            e.insert(sk)
            for k in (1, 5, 100, 3000, N):
                e.set_option("top_k", k)
                same(lists(e.query(q)), cut(full, k))
                assert e.stat("last_hits_form") == hl
            e.close()


def test_topk_paged_delta_and_s16(native, po):
    S, W, N, NQ, MS = 10, 8, 3000, 30, 60
    sk, q = data(S, W, N, NQ, 3)
    full = oracle_lists(po, S, W, sk, q, MS)
    pg = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, resident_mib=4, top_k=10)
    pg.insert(sk)
    assert pg.stat("pages") >= 4
    same(lists(pg.query(q)), cut(full, 10))
    pg.close()
    # the delta segment: genomes inserted after a query (a main index of >= 4096 genomes, less than an eighth more)
    sk, q = data(S, W, 6000, NQ, 13)
    full = oracle_lists(po, S, W, sk, q, MS)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, top_k=7)
    e.insert(sk[:5500])
    e.query(q[:2])
    e.insert(sk[5500:])
    got = lists(e.query(q))
    assert e.stat("delta_genomes") == 500
    same(got, cut(full, 7))
    e.close()
    # S = 16: two counter planes, counts up to 2^16
    S, W, N, NQ = 16, 8, 300, 6
    sk, q = data(S, W, N, NQ, 4, dup=4)
    for ms in (0, 20000):
        full = oracle_lists(po, S, W, sk, q, ms)
        e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms)
        e.insert(sk)
        for k in (1, 3, 10, N):
            e.set_option("top_k", k)
            same(lists(e.query(q)), cut(full, k))
        e.close()


def test_topk_entry_points(native, po):
    import torch
    K, S, W, H, J = 31, 12, 12, 4, 0.0
    fam = [f for f in range(4) for _ in range(5)]
    mem = [m for _ in range(4) for m in range(5)]
    rate = [0, 40, 200, 900, 3000] * 4
    genomes = [native.synth_genome_host(21, f, m, r, 30000) for f, m, r in zip(fam, mem, rate)]
    genomes += [genomes[2]] * 3 + [genomes[7]] * 2            # identical genomes: ties
    queries = [native.synth_genome_host(21, f, 50 + f, 300, 30000) for f in range(4)] + [genomes[2], genomes[9][500:9000]]
    e = native.Engine(K=K, S=S, W=W, H=H, J=J)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    sk = e.sketch(genomes)
    e.insert(sk)
    N, nq = len(genomes), len(queries)
    full = lists(e.query_sequences(queries))
    qsk = e.sketch(queries)
    counts = e.query_counts(qsk)
    for k in (1, 3, 10, N):
        e.set_option("top_k", k)
        exp = cut(full, k)
        same(lists(e.query_sequences(queries)), exp)
        same(lists(e.query(qsk)), exp)
        files = [b">q%d\n" % i + bytes(s) + b"\n" for i, s in enumerate(queries)]
        e.stage_raw(files, None)
        same(lists(e.staged_query()), exp)
        for i in range(nq):
            assert all(np.array_equal(a, b) for a, b in zip(e.query_shared(qsk[i]), exp[i]))
            assert all(np.array_equal(a, b) for a, b in zip(e.query_sequence_shared(queries[i]), exp[i]))
        # niqki_hits_from_counts over a gid range: the range's own list cut to k
        e.set_option("top_k", 0)
        rng_full = lists(e.hits_from_counts(counts, gid_begin=4, n_gids=N - 6))
        e.set_option("top_k", k)
        same(lists(e.hits_from_counts(counts, gid_begin=4, n_gids=N - 6)), cut(rng_full, k))
        # niqki_query_ahead (device memory) against niqki_query_sequences on the same records
        off = np.zeros(nq + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in queries])
        d_seq = torch.from_numpy(np.concatenate(queries + [np.zeros(native.SEQ_PAD, np.uint8)])).cuda()
        d_off = torch.from_numpy(off).cuda()
        e.sketch_ahead_dev(d_seq, d_off, nq)
        cap = nq * k
        ho = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        hc, hg = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.int32, device="cuda")
        assert e.query_ahead_dev(ho, hc, hg, cap) == nq
        torch.cuda.synchronize()
        o = ho.cpu().numpy().astype(np.uint64)
        tot = int(o[nq])
        same(lists((o, hc.cpu().numpy()[:tot].view(np.uint32), hg.cpu().numpy()[:tot].view(np.uint32))), exp)
    e.close()


def test_topk_option_params_and_dump(native, po):
    e = native.Engine(K=31, S=10, W=8, H=3, min_score_value=50, top_k=5)
    assert e.top_k == 5
    with pytest.raises(native.NiqkiError) as ei:
        e.set_option("top_k", -1)
    assert ei.value.code == 1
    with pytest.raises(native.NiqkiError):
        e.set_option("top_k", 1 << 32)
    e.set_option("top_k", 9)
    q = native.capi.Params()
    e.L.niqki_get_params(e.h, C.byref(q))
    assert q.top_k == 9
    sk, qq = data(10, 8, 1500, 12, 9)
    e.insert(sk)
    full = oracle_lists(po, 10, 8, sk, qq, 50)
    same(lists(e.query(qq)), cut(full, 9))
    raw = e.export_dump()
    for kw in (dict(), dict(resident_mib=2)):
        d = native.Engine.import_dump(raw, top_k=4, **kw)
        assert d.top_k == 4 and d.min_score == 50
        same(lists(d.query(qq)), cut(full, 4))
        d.close()
    d = native.Engine.import_dump(raw)
    assert d.top_k == 0
    same(lists(d.query(qq)), full)
    d.close()
    e.close()


def test_topk_local_group_equals_the_whole_index(native, po):
    import torch
    S, W, N, NQ, MS, world, per = 10, 8, 1200, 10, 64, 2, 5
    sk, q = data(S, W, N, NQ, 12)
    whole = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, top_k=6)
    whole.insert(sk)
    exp = lists(whole.query(q))
    same(exp, cut(oracle_lists(po, S, W, sk, q, MS), 6))
    engines = []
    for r in range(world):
        b, e_ = native.group_slot_range(r, world, S)
        engines.append(native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=b, slot_end=e_, top_k=6))
    grp = native.Group(engines)
    grp.set_option("exchange", 1)                 # asks for the sparse form: a top-k batch is dense all the same
    assert grp.stat("sparse") == 0
    dev = torch.device("cuda")
    for e_ in engines:
        e_.set_stream(torch.cuda.current_stream().cuda_stream)
    pad = np.full((world * 600, 1 << S), -1, np.int32)
    pad[:N] = sk
    grp.insert_dev([torch.from_numpy(pad[r * 600:(r + 1) * 600].copy()).to(dev) for r in range(world)], 600, N)
    pad = np.full((world * per, 1 << S), -1, np.int32)
    pad[:NQ] = q
    res = grp.query([torch.from_numpy(pad[r * per:(r + 1) * per].copy()).to(dev) for r in range(world)], per,
                    capacity=per * 6)
    got = []
    for r in range(world):
        got += lists(res[r])
    same(got[:NQ], exp)
    grp.close()
    # shards that disagree in top_k are refused
    (b0, e0), (b1, e1) = native.group_slot_range(0, 2, S), native.group_slot_range(1, 2, S)
    a = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=b0, slot_end=e0, top_k=6)
    b = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=b1, slot_end=e1, top_k=7)
    native.Group([a, native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=b1, slot_end=e1, top_k=6)]).close()
    with pytest.raises(native.NiqkiError):
        native.Group([a, b])
    for x in engines + [a, b, whole]:
        x.close()
