"""GPU: niqki_set_taxonomy / niqki_query_lca / niqki_staged_query_lca, per query the lowest common ancestor of its
near-best hits (include/niqki_hip.h).  Expected rows are tests/lca_ref.py (pinned on a brute force by
tests/test_lca_ref_cpu.py) over the full ordered lists of the existing, oracle-pinned Engine.query at top_k = 0, or
over hit_designs.reference_lists of a designed count matrix -- never from the calls under test."""
import numpy as np
import pytest

import hit_designs as hd
from collapse_ref import few_cell_query
from lca_ref import NONE, depths, lca_lists
from lists_ref import room, splits
from test_gpu_cluster import S, T_CHAIN10, T_CHAIN20, W, data, engine
from test_gpu_cover import mixed_batch, own_params

pytestmark = pytest.mark.gpu

F = 1 << S
N = 3000
MS = 50
E_INVALID, E_STATE = 1, 5
FILL = 0x7FFFFFFF


def same(got, exp):
    assert len(got) == 4
    for k in range(4):
        assert got[k].dtype == np.uint32 and got[k].shape == exp[k].shape
        bad = np.flatnonzero(got[k] != exp[k])
        assert bad.size == 0, "array %d, query %d: got %d, expected %d (%d differ)" % (k, bad[0], got[k][bad[0]], exp[k][bad[0]], bad.size)


def random_forest(n_genomes, n_taxa, n_roots, seed):
    rng = np.random.default_rng(seed)
    parent = np.array([t if t < n_roots else rng.integers(0, t) for t in range(n_taxa)], np.uint32)
    return rng.integers(0, n_taxa, n_genomes).astype(np.uint32), parent


# ---- 1. the designed case -----------------------------------------------------------------------------------------

def designed():
    """300 genomes, 167 taxa: a complete binary tree on taxa 0..126 (leaves 63..126, 4-5 genomes each) and a path on
    127..166; eleven query types a..k (the module's issue table)"""
    n = 300
    parent = np.array([0] + [(t - 1) // 2 for t in range(1, 127)] + [127] + [t - 1 for t in range(128, 167)], np.uint32)
    gt = (63 + np.arange(n) * 64 // n).astype(np.uint32)
    gt[7], gt[150], gt[299] = 1, 140, 166
    rng = np.random.default_rng(5)
    C = rng.choice(np.array([0, 19]), size=(11, n))
    a, b, c, d, e, f, g, h, i, j, k = range(11)
    C[b, 200] = 30
    C[c, [33, 36]] = 30                                        # two genomes of leaf 70
    four = np.flatnonzero((gt >= 79) & (gt <= 82))
    C[d, four] = np.where(four % 2 == 0, 30, 21)
    under1 = np.setdiff1d(np.arange(150), [7])                 # the genomes of leaves 63..94
    pick = np.concatenate([[10, 100], rng.choice(np.setdiff1d(under1, [10, 100]), 61, replace=False)])
    C[e, pick] = rng.choice(np.array([20, 26, 27, 30]), size=63)
    C[e, [10, 100]] = 30                                       # the best hits lie under taxon 3 and under taxon 4
    in_a = np.setdiff1d(np.arange(n), [150, 299])
    pick = np.concatenate([[10, 250], rng.choice(np.setdiff1d(in_a, [10, 250]), 62, replace=False)])
    C[f, pick] = 30
    C[g, pick] = 30
    C[g, 299] = 30
    C[h, :] = 30
    C[i, :] = 20
    C[i, [34, 35]] = 30                                        # leaf 70 again
    C[i, 77], C[i, 88] = 27, 26                                # leaves 79 and 81
    C[j, 150], C[j, 299] = 22, 30
    C[k, [7, 20]] = 30
    assert gt[33] == gt[34] == gt[35] == gt[36] == 70 and gt[77] == 79 and gt[88] == 81 and gt[200] == 63 + 200 * 64 // 300
    return n, C, gt, parent


def test_designed_case_both_routes_every_outcome(native):
    n, C, gt, parent = designed()
    rng = np.random.default_rng(8)
    sk, qt = hd.design(C, S, W, rng)
    types = np.concatenate([np.arange(11), rng.integers(0, 11, 60)])
    q = np.ascontiguousarray(qt[types])
    depth = depths(parent)
    assert depth.max() == 39 and depth[126] == 6
    # what the reference gives, before the device is asked
    by_type = {(ms, p): lca_lists(hd.reference_lists(C, ms), gt, parent, p) for ms in (20, 0) for p in (0, 100, 134, 1000)}
    r0 = by_type[20, 0]
    assert r0[0].tolist() == [NONE, gt[200], 70, 19, 1, 0, NONE, NONE, 70, 166, 1]
    assert r0[3].tolist()[:3] == [0, 1, 2] and r0[3][7] == 300 and r0[3][8] == 2 and r0[3][5] == 64 and r0[3][6] == 65
    assert by_type[20, 100][3][8] == 3 and by_type[20, 100][0][8] == 1       # 27 * 1000 == 30 * 900
    assert by_type[20, 134][3][8] == 4 and by_type[20, 134][0][8] == 1       # 26 * 1000 >= 30 * 866
    assert by_type[20, 1000][0][8] == NONE and by_type[20, 1000][3][8] == 300
    assert by_type[20, 1000][0][9] == 140 and by_type[20, 1000][3][9] == 2   # an ancestor that itself carries a genome
    assert (by_type[0, 1000][0] == NONE).all() and (by_type[0, 1000][3] == 300).all()
    kinds = {"none" if t == NONE else ("root" if depth[t] == 0 else ("leaf" if t >= 63 and t <= 126 else "inner"))
             for t, c in zip(r0[0], r0[3]) if c >= 2 or t != NONE}
    assert kinds == {"none", "root", "leaf", "inner"}
    for ms in (20, 0):
        e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms)
        e.insert(sk)
        e.set_taxonomy(gt, parent)
        assert e.stat("taxa") == 167 and e.stat("taxonomy_depth") == 39
        for cap in (1024, 64):
            e.set_option("lca_wave_cap", cap)
            for p in (0, 100, 134, 1000):
                exp = tuple(x[types] for x in by_type[ms, p])
                got = e.query_lca(q, top_permille=p, details=True)
                same(got, exp)
                n_long = int((exp[3] > cap).sum())
                assert e.stat("lca_long_lists") == n_long
                assert e.stat("lca_no_common") == int(((exp[0] == NONE) & (exp[3] >= 2)).sum())
                assert (n_long > 0) == (cap == 64)            # 300 genomes: all short at the default, (g) (h) long at 64
                if ms == 0 and cap == 64 and p == 1000:
                    assert n_long == types.size              # every list holds all 300
                only = e.query_lca(q, top_permille=p)         # the three details arrays NULL
                assert only.dtype == np.uint32 and np.array_equal(only, exp[0])
        own_params(e, ms, 0)
        e.close()


# ---- 2. the definition on every index form ---------------------------------------------------------------------------

def nested_taxonomy(levels, n):
    """genomes 0 .. n - 1 under their cluster at the first level, every cluster under its cluster of the next level"""
    L = len(levels)
    parent = np.arange((L + 1) * n, dtype=np.uint32)
    parent[:n] = n + levels[0]
    for lv in range(L - 1):
        parent[n + lv * n + levels[lv]] = n + (lv + 1) * n + levels[lv + 1]
    return np.arange(n, dtype=np.uint32), parent


@pytest.fixture(scope="module")
def case(native):
    sk = data(N, 11)
    rng = np.random.default_rng(41)
    q = np.concatenate([mixed_batch(sk, W), np.stack([few_cell_query(sk, g, W, rng) for g in (100, 1234)])])
    e = engine(native, "lists", sk)
    full = e.query(q, capacity=1 << 20)                     # the full ordered lists: top_k = 0 at min_score 50
    levels = [e.cluster(t)[0] for t in (T_CHAIN10, T_CHAIN20, 300, 1)]
    e.close()
    e0 = engine(native, "lists", sk, ms=0)
    full0 = e0.query(q[:40], capacity=40 * N)
    e0.close()
    gt, parent = nested_taxonomy(levels, N)
    depth = depths(parent)
    assert depth[:N].min() == depth[:N].max() == 4
    exp = {p: lca_lists(full, gt, parent, p) for p in (0, 100, 1000)}
    # what the tests rely on, on the reference's output
    lens = np.diff(full[0].astype(np.int64))
    assert lens.min() == 0 and int(full[0][-1]) > 65536
    t1000, c1000 = exp[1000][0], exp[1000][3]
    assert {int(depth[t]) for t in t1000 if t != NONE} == {0, 1, 2, 3, 4}
    assert (c1000 > 64).any() and (c1000 > 1024).any() and (c1000 == 0).any()
    for p in (0, 100):
        assert len({int(depth[t]) for t in exp[p][0] if t != NONE}) >= 4
    exp0 = lca_lists(full0, gt, parent, 1000)
    assert (exp0[0] == NONE).all() and (exp0[3] == N).all()  # genome 11 is a tree of its own
    return sk, q, full, (gt, parent), exp, exp0


@pytest.mark.parametrize("form", ["lists", "rows", "tiles", "batch64", "top_k3", "paged", "late"])
def test_lca_equals_the_definition(native, case, form):
    sk, q, full, (gt, parent), exp, _ = case
    if form == "late":                               # genomes inserted after the index was built and asked
        e = engine(native, "lists", sk[:2900])
        e.query(q[:2])
        e.insert(sk[2900:])
    else:
        e = engine(native, form, sk)
    k = 3 if form == "top_k3" else 0
    before = e.query(q[:40])
    e.set_taxonomy(gt, parent)
    assert e.stat("taxa") == 5 * N and e.stat("taxonomy_depth") == 4
    for p in (0, 100, 1000):
        same(e.query_lca(q, top_permille=p, details=True), exp[p])     # (top_k is ignored: top_k3 gives the same)
        assert e.stat("lca_long_lists") == int((exp[p][3] > 1024).sum())
    if form == "tiles":
        assert e.stat("tiles") > 1
    if form == "paged":
        assert e.stat("pages") >= 4
    own_params(e, MS, k)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()


def test_every_genome_considered_at_min_score_0(native, case):
    sk, q, _, (gt, parent), _, exp0 = case
    e = engine(native, "lists", sk, ms=0)
    e.set_taxonomy(gt, parent)
    same(e.query_lca(q[:40], top_permille=1000, details=True), exp0)
    assert e.stat("lca_long_lists") == 40 and e.stat("lca_no_common") == 40
    e.close()


# ---- 3. delta segment ------------------------------------------------------------------------------------------------

def test_with_a_delta_segment(native):
    """a main index of >= 4096 genomes and less than an eighth more: the later genomes have an index of their own"""
    n = 4600
    sk = data(n, 23)
    rng = np.random.default_rng(3)
    q = np.stack([sk[g] for g in rng.integers(0, n, 60)] + [sk[4400].copy(), np.full(F, -1, np.int32)])
    gt, parent = random_forest(n, 400, 2, 6)
    whole = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    whole.insert(sk)
    full = whole.query(q, capacity=1 << 20)
    whole.close()
    assert (full[2] >= 4300).any() and (full[2] < 4300).any()
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    e.insert(sk[:4300])
    e.query(q[:2])
    e.insert(sk[4300:])
    e.set_taxonomy(gt, parent)
    for p in (0, 100, 1000):
        got = e.query_lca(q, top_permille=p, details=True)
        assert e.stat("delta_genomes") == 300
        same(got, lca_lists(full, gt, parent, p))
    e.close()


# ---- 4. budget -------------------------------------------------------------------------------------------------------

def test_budget_splits_leave_the_result_unchanged(native, case):
    """1 MiB of hit buffers hold 65 536 hits; the batch's full lists hold more (checked on the expected arrays)"""
    import torch
    sk, q, full, (gt, parent), exp, _ = case
    assert int(full[0][-1]) > 65536
    e = engine(native, "lists", sk)
    e.set_taxonomy(gt, parent)
    at_default = e.query_lca(q, top_permille=100, details=True)
    assert e.stat("lca_splits") == 0
    same(at_default, exp[100])
    e.set_option("cluster_ws_mib", 1)
    same(e.query_lca(q, top_permille=100, details=True), exp[100])
    lens = np.diff(full[0].astype(np.int64))
    n_splits = splits(lens, 1024, room(1, N), False)         # a host call: batches of query_batch = 1024 (lists_ref.py)
    assert e.stat("lca_splits") == n_splits > 0
    # device memory: the whole batch in one call, halved where it does not fit
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    nq = q.shape[0]
    d_q = torch.from_numpy(q).cuda()
    out = [torch.full((nq,), FILL, dtype=torch.int32, device="cuda") for _ in range(4)]
    e.query_lca_dev(d_q, nq, 100, *out)
    torch.cuda.synchronize()
    assert e.stat("lca_splits") == splits(lens, nq, room(1, N), False) > 0      # one batch of nq
    same(tuple(x.cpu().numpy().view(np.uint32) for x in out), exp[100])
    out = [torch.full((nq,), FILL, dtype=torch.int32, device="cuda") for _ in range(4)]
    e.query_lca_dev(d_q, nq, 1000, out[0], None, out[2], None)
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), exp[1000][0])
    assert np.array_equal(out[2].cpu().numpy().view(np.uint32), exp[1000][2])
    assert int(out[1].min().item()) == FILL and int(out[3].min().item()) == FILL
    e.close()


# ---- 5. state and errors ---------------------------------------------------------------------------------------------

def test_state(native, case):
    import torch
    sk, q, full, _, _, _ = case
    out = [np.full(8, 7, np.uint32) for _ in range(4)]

    def call(e, nq=2, p=0):
        return e.L.niqki_query_lca(e.h, q.ctypes.data, nq, p, *[x.ctypes.data for x in out], 0)

    def set_raw(e, gt, parent, n_genomes=None):
        gt, parent = np.ascontiguousarray(gt, np.uint32), np.ascontiguousarray(parent, np.uint32)
        return e.L.niqki_set_taxonomy(e.h, gt.ctypes.data, gt.size if n_genomes is None else n_genomes, parent.ctypes.data, parent.size, 0)

    def err(e):
        return e.L.niqki_last_error(e.h)

    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, top_k=5)
    assert call(e, 4) == 0                                       # an empty index: no hit, also without a taxonomy
    assert out[0][:4].tolist() == [NONE] * 4 and out[1][:4].tolist() == [0] * 4
    assert out[2][:4].tolist() == [0xFFFFFFFF] * 4 and out[3][:4].tolist() == [0] * 4 and out[0][4] == 7
    e.insert(sk[:500])
    before = e.query(q[:40])
    assert call(e) == E_STATE and b"niqki_set_taxonomy" in err(e)
    assert e.stat("taxa") == 0
    gt, parent = random_forest(500, 60, 2, 9)
    assert set_raw(e, gt[:499], parent) == E_INVALID and b"499" in err(e) and call(e) == E_STATE
    bad = gt.copy()
    bad[123] = 60
    assert set_raw(e, bad, parent) == E_INVALID and b"genome 123" in err(e) and call(e) == E_STATE
    bad = parent.copy()
    bad[17] = 60
    assert set_raw(e, gt, bad) == E_INVALID and b"taxon 17" in err(e) and call(e) == E_STATE
    assert set_raw(e, gt, parent) == 0 and e.stat("taxa") == 60 and e.stat("taxonomy_depth") == int(depths(parent).max())
    assert call(e) == 0
    assert call(e, 2, 1000) == 0 and call(e, 2, 1001) == E_INVALID and b"1001" in err(e)
    out[0][:] = 7
    assert call(e, 0) == 0 and out[0][0] == 7                    # no queries
    # a two-cycle and a long cycle: refused, and the taxonomy the handle had still answers
    answer = e.query_lca(q[:40], top_permille=100, details=True)
    two = parent.copy()
    two[40], two[41] = 41, 40
    assert set_raw(e, gt, two) == E_INVALID and b"cycle" in err(e)
    ring = parent.copy()
    ring[10:60] = np.arange(11, 61)
    ring[59] = 10
    assert set_raw(e, gt, ring) == E_INVALID and b"cycle" in err(e)
    assert e.stat("taxa") == 60
    same(e.query_lca(q[:40], top_permille=100, details=True), answer)
    e.set_taxonomy(None, None)
    assert call(e) == E_STATE and e.stat("taxa") == 0 and e.stat("taxonomy_depth") == 0
    # every call that adds or drops genomes removes the taxonomy
    assert set_raw(e, gt, parent) == 0 and call(e) == 0
    e.insert(sk[500:510])
    assert call(e) == E_STATE and e.stat("taxa") == 0
    gt10 = np.concatenate([gt, gt[:10]])
    assert set_raw(e, gt10, parent) == 0 and call(e) == 0
    keep = np.ones(510, np.uint8)
    keep[500:] = 0
    assert e.retain(keep)[0] == 500
    assert call(e) == E_STATE and e.stat("taxa") == 0
    assert set_raw(e, gt, parent) == 0 and call(e) == 0
    other = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    other.insert(sk[600:620])
    e.append_dump(other.export_dump())
    other.close()
    assert e.n_genomes == 520 and call(e) == E_STATE and e.stat("taxa") == 0
    assert set_raw(e, np.concatenate([gt, gt[:20]]), parent) == 0 and call(e) == 0
    own_params(e, MS, 5)                                         # ... also after the failing calls
    e.retain(np.arange(520) < 500)
    after = e.query(q[:40])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # labels and taxonomy do not disturb each other
    lab = (np.arange(500) % 9).astype(np.uint32)
    e.set_labels(lab)
    collapsed = e.query_collapsed(q[:40], members=True)
    e.set_taxonomy(torch.from_numpy(gt.view(np.int32)).cuda(), torch.from_numpy(parent.view(np.int32)).cuda())   # from device memory
    assert e.stat("taxa") == 60 and e.stat("labels") == 9
    again = e.query_collapsed(q[:40], members=True)
    assert all(np.array_equal(a, b) for a, b in zip(collapsed, again))
    got = e.query_lca(q[:40], top_permille=100, details=True)
    same(got, answer)
    e.set_labels(None)
    same(e.query_lca(q[:40], top_permille=100, details=True), answer)
    assert e.stat("taxa") == 60
    e.set_labels(lab)
    e.set_taxonomy(None, None)
    assert e.stat("labels") == 9 and all(np.array_equal(a, b) for a, b in zip(collapsed, e.query_collapsed(q[:40], members=True)))
    # queries without a hit
    assert set_raw(e, gt, parent) == 0
    got = e.query_lca(np.full((3, F), -1, np.int32), details=True)
    assert got[0].tolist() == [NONE] * 3 and got[1].tolist() == [0] * 3 and got[2].tolist() == [0xFFFFFFFF] * 3 and got[3].tolist() == [0] * 3
    e.close()
    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS, slot_begin=0, slot_end=F // 2)
    shard.insert(sk[:100])
    assert set_raw(shard, gt[:100], parent) == 0
    assert call(shard) == E_STATE and b"slot-range" in err(shard)
    own_params(shard, MS, 0)
    shard.close()


# ---- 6. staged -------------------------------------------------------------------------------------------------------

def test_staged_query_lca(native):
    K, S_, W_, H = 31, 12, 12, 4
    g = [native.synth_genome_host(31, f, m, r, 30000) for f, m, r in ((0, 0, 0), (0, 1, 300), (1, 0, 0), (2, 0, 0), (2, 1, 60), (3, 0, 0))]
    e = native.Engine(K=K, S=S_, W=W_, H=H, J=0.05)
    e.insert(e.sketch(g))
    gt = np.array([0, 1, 2, 3, 4, 5], np.uint32)
    parent = np.array([6, 6, 8, 7, 7, 9, 8, 8, 8, 9], np.uint32)   # (0 1) and (3 4) are pairs under 8 with 2; 5 is a tree of its own
    e.set_taxonomy(gt, parent)

    def fasta(records):
        return b"".join(b">r%d\n" % i + bytes(r) + b"\n" for i, r in enumerate(records))

    files = [fasta([g[0], g[2]]), fasta([g[3]]), fasta([g[5], g[1]]), fasta([g[4][:K]]), fasta([g[2][100:20000]])]
    e.stage_raw(files, None)
    before = e.staged_query()
    for p in (0, 1000):
        got = e.staged_query_lca(top_permille=p, details=True)
        qsk = e.staged_sketch()
        assert qsk.shape[0] == len(files)
        same(got, e.query_lca(qsk, top_permille=p, details=True))
        same(got, lca_lists(before, gt, parent, p))
    assert (got[3] >= 2).any()                                 # (the file of two genomes hits both)
    after = e.staged_query()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()
