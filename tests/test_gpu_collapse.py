"""GPU: niqki_set_labels / niqki_query_collapsed / niqki_staged_query_collapsed, per query the best hit of every label
(include/niqki_hip.h).  Expected lists are tests/collapse_ref.py (pinned on the oracle by
tests/test_collapse_ref_cpu.py) over the full ordered lists of the existing, oracle-pinned Engine.query at top_k = 0,
or over hit_designs.reference_lists of a designed count matrix -- never from the calls under test."""
import numpy as np
import pytest

import hit_designs as hd
from collapse_ref import collapse_lists, few_cell_query
from lists_ref import room, splits
from test_gpu_cluster import S, T_CHAIN20, W, data, engine
from test_gpu_cover import mixed_batch, own_params

pytestmark = pytest.mark.gpu

F = 1 << S
N = 3000
MS = 50
E_INVALID, E_CAPACITY, E_STATE = 1, 4, 5
FILL = 0x7FFFFFFF


def label_sets(n, seed=3):
    rng = np.random.default_rng(seed)
    return {
        "identity": np.arange(n, dtype=np.uint32),
        "one": np.full(n, 42, np.uint32),
        "mod7": (np.arange(n) % 7).astype(np.uint32),                      # members interleave
        "sparse": rng.choice(np.array([0, 0xFFFFFFFF, 5, 1 << 31, 123456789, 77, 4096, 8192], np.uint32), n),
        "pow2": (rng.integers(0, 400, n) * 8192 + rng.integers(0, 3, n)).astype(np.uint32),   # r * 8192 + c
    }


@pytest.fixture(scope="module")
def case(native):
    sk = data(N, 11)
    rng = np.random.default_rng(41)
    q = np.concatenate([mixed_batch(sk, W), np.stack([few_cell_query(sk, g, W, rng) for g in (100, 1234)])])
    e = engine(native, "lists", sk)
    full = e.query(q, capacity=1 << 20)                     # the full ordered lists: top_k = 0 at min_score 50
    chain20 = e.cluster(T_CHAIN20)[0]
    e.close()
    lens = np.diff(full[0].astype(np.int64))
    assert lens.min() == 0 and (lens == 1).any() and lens.max() > 256
    assert (q == -1).all(1).any()                            # all-empty sketches
    assert int(full[0][-1]) > 65536                          # what test_budget relies on: more than 1 MiB of hit buffers holds
    sets = label_sets(N)
    sets["chain20"] = chain20
    assert 1 < np.unique(chain20).size < N
    return sk, q, full, sets


def same(got, exp, members=True):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0])
    for k in range(1, 4 if members else 3):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], exp[k]), k


@pytest.mark.parametrize("form", ["lists", "rows", "tiles", "batch64", "top_k3", "paged", "late"])
def test_collapsed_equals_the_definition(native, case, form):
    sk, q, full, sets = case
    if form == "late":                               # genomes inserted after the index was built and asked
        e = engine(native, "lists", sk[:2900])
        e.query(q[:2])
        e.insert(sk[2900:])
    else:
        e = engine(native, form, sk)
    k = 3 if form == "top_k3" else 0
    before = e.query(q[:40])
    for name in ("chain20", "mod7", "pow2"):
        e.set_labels(sets[name])
        assert e.stat("labels") == np.unique(sets[name]).size
        same(e.query_collapsed(q, members=True), collapse_lists(full, sets[name], k))
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
    labels = ((np.arange(n) * 7) % 13).astype(np.uint32)
    whole = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    whole.insert(sk)
    full = whole.query(q, capacity=1 << 20)
    whole.close()
    assert (full[2] >= 4300).any() and (full[2] < 4300).any()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    e.insert(sk[:4300])
    e.query(q[:2])
    e.insert(sk[4300:])
    e.set_labels(labels)
    got = e.query_collapsed(q, members=True)
    assert e.stat("delta_genomes") == 300
    same(got, collapse_lists(full, labels))
    e.close()


def test_label_sets_from_host_and_device_memory(native, case):
    import torch
    sk, q, full, sets = case
    e = engine(native, "lists", sk)
    for name, labels in sets.items():
        exp = collapse_lists(full, labels)
        e.set_labels(labels)
        assert e.stat("labels") == np.unique(labels).size
        same(e.query_collapsed(q, members=True), exp)
        same(e.query_collapsed(q), exp, members=False)
        if name == "identity":
            assert np.array_equal(exp[0], full[0]) and np.array_equal(exp[1], full[1]) and np.array_equal(exp[2], full[2])
        if name == "one":
            assert np.diff(exp[0].astype(np.int64)).max() == 1
    d = torch.from_numpy(sets["chain20"].view(np.int32)).cuda()
    e.set_labels(sets["one"])
    e.set_labels(d)
    same(e.query_collapsed(q, members=True), collapse_lists(full, sets["chain20"]))
    e.close()


def test_both_table_routes_on_a_designed_index(native):
    """queries with exactly 0, 1, 63, 64, 65 and 300 hits on 300 genomes; counts of four levels only, so equal counts
    across labels are everywhere (order by gid), and genomes 0 and 299, which tie in every list that holds both, share
    a label (the larger gid is the label's best member)"""
    n = 300
    n_hits = [0, 1, 63, 64, 65, 300]
    rng = np.random.default_rng(8)
    C = hd.hit_matrix(n_hits, n, rng)
    sk, qt = hd.design(C, S, W, rng)
    types = np.concatenate([np.arange(6), rng.integers(0, 6, 60)])
    q = np.ascontiguousarray(qt[types])
    labels = (np.arange(n) % 11).astype(np.uint32)
    labels[0] = labels[299] = 500
    for ms in (20, 0):
        full = hd.deal(hd.reference_lists(C, ms), types)
        exp = collapse_lists(full, labels)
        lens = np.diff(full[0])
        if ms == 20:
            assert sorted(set(lens.tolist())) == n_hits
            whole = full[2][int(full[0][5]):int(full[0][6])].tolist()              # the query that hits all 300
            assert C[5, 0] == C[5, 299] and whole.index(299) < whole.index(0)
            kept = exp[2][int(exp[0][5]):int(exp[0][6])].tolist()
            assert 299 in kept and 0 not in kept and len(kept) == 12
        else:
            assert (lens == n).all()
        e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms)
        e.insert(sk)
        e.set_labels(labels)
        at_default = e.query_collapsed(q, members=True)
        assert e.stat("collapse_long_lists") == 0        # 300 genomes: no list is longer than the default cap
        same(at_default, exp)
        e.set_option("collapse_lds_cap", 64)
        got = e.query_collapsed(q, members=True)
        assert e.stat("collapse_long_lists") == int((lens > 64).sum()) > 0
        same(got, exp)
        same(got, at_default)
        e.set_option("top_k", 4)
        same(e.query_collapsed(q, members=True), collapse_lists(full, labels, 4))
        e.close()


def test_long_lists_at_the_default_cap(native, case):
    """min_score 0 on 3000 genomes: every list holds them all and takes the global table"""
    sk, q, _, sets = case
    e = engine(native, "lists", sk, ms=0)
    qq = q[:12]
    full = e.query(qq, capacity=12 * N)
    assert (np.diff(full[0].astype(np.int64)) == N).all()
    for name in ("chain20", "sparse", "identity"):
        e.set_labels(sets[name])
        got = e.query_collapsed(qq, members=True)
        assert e.stat("collapse_long_lists") == 12
        same(got, collapse_lists(full, sets[name]))
        assert int(got[3].sum()) == 12 * N
    e.close()


def test_batch_edges(native, case):
    sk, q, full, sets = case
    e = engine(native, "lists", sk)
    e.set_labels(sets["chain20"])
    for nq in (1, 63, 64, 65):
        sub = hd.deal(tuple(x.astype(np.int64) for x in full), np.arange(8, 8 + nq))
        same(e.query_collapsed(q[8:8 + nq], members=True), collapse_lists(sub, sets["chain20"]))
    e.close()


def test_budget_splits_leave_the_result_unchanged(native, case):
    """1 MiB of hit buffers hold 65 536 hits; the batch's full lists hold more (checked on the expected arrays)"""
    sk, q, full, sets = case
    assert int(full[0][-1]) > 65536
    # a host call: batches of query_batch = 1024 queries, every one at that size (lists_ref.py)
    n_splits = splits(np.diff(full[0].astype(np.int64)), 1024, room(1, N), False)
    assert n_splits > 0
    e = engine(native, "lists", sk)
    e.set_option("cluster_ws_mib", 1)
    e.set_labels(sets["mod7"])
    exp = collapse_lists(full, sets["mod7"])
    same(e.query_collapsed(q, members=True), exp)
    assert e.stat("collapse_splits") == n_splits
    e.set_option("collapse_lds_cap", 64)             # ... and with the global tables inside the same small budget
    same(e.query_collapsed(q, members=True), exp)
    assert e.stat("collapse_splits") == n_splits and e.stat("collapse_long_lists") == int((np.diff(full[0].astype(np.int64)) > 64).sum())
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
    labels = (np.arange(n) % 5).astype(np.uint32)
    e = native.Engine(K=31, S=s, W=w, H=3, min_score_value=1000)
    e.insert(sk)
    full = e.query(q, capacity=8 * n)
    e.set_labels(labels)
    got = e.query_collapsed(q, members=True)
    same(got, collapse_lists(full, labels))
    assert int(got[1][0]) == 65536 and int(got[2][0]) == 17
    own_params(e, 1000, 0)
    e.close()


def test_device_memory_and_capacity(native, case):
    import torch
    sk, q, full, sets = case
    nq = 200
    labels = sets["chain20"]
    sub = hd.deal(tuple(x.astype(np.int64) for x in full), np.arange(nq))
    exp = collapse_lists(sub, labels)
    total = int(exp[0][-1])
    e = engine(native, "lists", sk)
    e.set_labels(labels)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_q = torch.from_numpy(q[:nq]).cuda()

    def fresh(cap):
        return (torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda"),
                torch.full((max(cap, 1),), FILL, dtype=torch.int32, device="cuda"),
                torch.full((max(cap, 1),), FILL, dtype=torch.int32, device="cuda"),
                torch.full((max(cap, 1),), FILL, dtype=torch.int32, device="cuda"))

    ho, hc, hg, hm = fresh(total - 1)
    assert e.query_collapsed_dev(d_q, nq, ho, hc, hg, hm, total - 1) == E_CAPACITY
    torch.cuda.synchronize()
    assert int(ho[nq].item()) == total
    assert int(hc.min().item()) == FILL and int(hg.min().item()) == FILL and int(hm.min().item()) == FILL
    for with_members in (True, False):
        ho, hc, hg, hm = fresh(total)
        assert e.query_collapsed_dev(d_q, nq, ho, hc, hg, hm if with_members else None, total) == 0
        torch.cuda.synchronize()
        got = (ho.cpu().numpy().astype(np.uint64),) + tuple(x.cpu().numpy().astype(np.uint32) for x in (hc, hg, hm))
        same(got, exp, members=with_members)
        assert with_members or int(hm.min().item()) == FILL
    # host memory: the same contract
    off = np.zeros(nq + 1, np.uint64)
    hc_h, hg_h, hm_h = (np.full(total, FILL, np.uint32) for _ in range(3))

    def host_call(cap):
        return e.L.niqki_query_collapsed(e.h, q[:nq].ctypes.data, nq, off.ctypes.data, hc_h.ctypes.data, hg_h.ctypes.data, hm_h.ctypes.data, cap, 0)

    assert host_call(total - 1) == E_CAPACITY and int(off[nq]) == total
    assert (hc_h == FILL).all() and (hg_h == FILL).all() and (hm_h == FILL).all()
    assert host_call(total) == 0
    same((off, hc_h, hg_h, hm_h), exp)
    # capacity = nq x k never fails with top_k = k
    e.set_option("top_k", 2)
    same(e.query_collapsed(q[:nq], capacity=2 * nq, members=True), collapse_lists(sub, labels, 2))
    own_params(e, MS, 2)
    e.close()


def test_state(native, case):
    sk, q, full, sets = case
    off = np.full(5, 7, np.uint64)
    hc, hg = np.zeros(4096, np.uint32), np.zeros(4096, np.uint32)

    def call(e, nq=2):
        return e.L.niqki_query_collapsed(e.h, q.ctypes.data, nq, off.ctypes.data, hc.ctypes.data, hg.ctypes.data, None, 4096, 0)

    def set_raw(e, labels):
        return e.L.niqki_set_labels(e.h, labels.ctypes.data, labels.size, 0)

    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, top_k=5)
    assert call(e, 4) == 0 and not off.any()                     # an empty index: empty lists
    e.insert(sk[:500])
    before = e.query(q[:40])
    assert call(e) == E_STATE and b"niqki_set_labels" in e.L.niqki_last_error(e.h)
    assert e.stat("labels") == 0
    lab = (np.arange(500) % 9).astype(np.uint32)
    assert set_raw(e, lab[:499]) == E_INVALID and call(e) == E_STATE
    assert set_raw(e, lab) == 0 and e.stat("labels") == 9 and call(e) == 0
    off[:] = 7
    assert call(e, 0) == 0 and off[0] == 0                       # no queries
    e.set_labels(None)
    assert call(e) == E_STATE and e.stat("labels") == 0
    # every call that adds or drops genomes removes the labelling
    assert set_raw(e, lab) == 0 and call(e) == 0
    e.insert(sk[500:510])
    assert call(e) == E_STATE
    lab = (np.arange(510) % 9).astype(np.uint32)
    assert set_raw(e, lab) == 0 and call(e) == 0
    keep = np.ones(510, np.uint8)
    keep[500:] = 0
    assert e.retain(keep)[0] == 500
    assert call(e) == E_STATE
    assert set_raw(e, lab[:500]) == 0 and call(e) == 0
    other = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    other.insert(sk[600:620])
    e.append_dump(other.export_dump())
    other.close()
    assert e.n_genomes == 520 and call(e) == E_STATE
    assert set_raw(e, np.arange(520, dtype=np.uint32)) == 0 and call(e) == 0
    own_params(e, MS, 5)                                         # ... also after the failing calls
    e.retain(np.arange(520) < 500)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert set_raw(e, lab[:500]) == 0                            # queries without a hit: empty lists
    got = e.query_collapsed(np.full((3, F), -1, np.int32), members=True)
    assert got[0].tolist() == [0, 0, 0, 0] and all(x.size == 0 for x in got[1:])
    e.close()
    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=0, slot_end=F // 2)
    shard.insert(sk[:100])
    assert set_raw(shard, lab[:100]) == 0
    assert call(shard) == E_STATE and b"slot-range" in shard.L.niqki_last_error(shard.h)
    own_params(shard, MS, 0)
    shard.close()


def test_staged_query_collapsed(native):
    K, S_, W_, H = 31, 12, 12, 4
    g = [native.synth_genome_host(31, f, m, r, 30000) for f, m, r in ((0, 0, 0), (0, 1, 300), (1, 0, 0), (2, 0, 0), (2, 1, 60), (3, 0, 0))]
    e = native.Engine(K=K, S=S_, W=W_, H=H, J=0.05)
    e.insert(e.sketch(g))
    labels = np.array([7, 7, 0xFFFFFFFF, 0, 0, 3], np.uint32)
    e.set_labels(labels)

    def fasta(records):
        return b"".join(b">r%d\n" % i + bytes(r) + b"\n" for i, r in enumerate(records))

    files = [fasta([g[0], g[2]]), fasta([g[3]]), fasta([g[5], g[1]]), fasta([g[4][:K]]), fasta([g[2][100:20000]])]
    e.stage_raw(files, None)
    before = e.staged_query()
    got = e.staged_query_collapsed(members=True)
    qsk = e.staged_sketch()
    assert qsk.shape[0] == len(files)
    same(got, e.query_collapsed(qsk, members=True))
    same(got, collapse_lists(before, labels))
    assert len(before[1]) > len(got[1]) and int(got[3].max()) == 2
    after = e.staged_query()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()
