"""GPU: niqki_retain drops genomes from a handle.  Definition: afterwards the handle is indistinguishable, through the
ABI, from a fresh handle into which the kept genomes' sketches were inserted in their old order.  Expected values are
numpy indexing of the sketches read BEFORE the call, a fresh handle fed sk[keep], and the oracle's Index(p, sk[keep])
-- never the code under test.  The designed masks are those of tests/retain_masks.py, which tests/test_retain_blocks.py
runs through the block arithmetic on the CPU; data and engine forms are those of test_gpu_cluster.py."""
import ctypes as C

import numpy as np
import pytest

from retain_masks import SIZES, designed_masks, expected_ids
from test_gpu_cluster import F, FORMS, S, T_CHAIN20, W, data, engine

pytestmark = pytest.mark.gpu

E_STATE = 5
NONE = 0xFFFFFFFF


def same_hits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. the compaction at designed masks ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def columns():
    """8 300 sketches whose every cell differs from its neighbours' (a column that lands one place off shows)"""
    rng = np.random.default_rng(77)
    sk = rng.integers(0, 1 << W, (max(SIZES), F)).astype(np.int32)
    sk[rng.random(sk.shape) < 0.01] = -1
    return sk


@pytest.mark.parametrize("n", SIZES)
def test_compaction_at_designed_masks(native, columns, n):
    sk = columns[:n]
    for name, m in designed_masks(n):
        e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
        e.insert(sk)
        before = e.get_sketches(0, n)
        if name == "all":
            assert np.array_equal(before, sk)
        n_kept, ids = e.retain(m)
        assert n_kept == int(m.sum()) == e.n_genomes, name
        assert ids.dtype == np.uint32 and np.array_equal(ids, expected_ids(m)), name
        after = e.get_sketches(0, n_kept)
        assert np.array_equal(after, before[m]), name          # every cell of every kept genome
        e.close()


# ---- 2. equivalence with a fresh handle and with the oracle -----------------------------------------------------

def queries_for(sk, keep, rng):
    kept, dropped = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    q = [sk[rng.choice(kept, 24, replace=False)], sk[rng.choice(dropped, 24, replace=False)],
         rng.integers(0, 1 << W, (16, sk.shape[1])).astype(np.int32)]
    return np.concatenate(q)


def check_equivalent(po, e, fresh, sub, q, s, ms, selfjoin_threshold):
    """e: the handle after retain; fresh: a new handle of the same form fed sub = sk[keep]"""
    n = sub.shape[0]
    assert e.n_genomes == fresh.n_genomes == n
    assert np.array_equal(e.get_sketches(0, n), fresh.get_sketches(0, n))
    p = po.make_params(31, s, W, 3, 0.0)
    p.min_score = ms
    ox = po.Index(p, sub)
    dump = e.export_dump()
    assert dump == fresh.export_dump() and dump == ox.dump_bytes()
    he, hf = e.query(q), fresh.query(q)
    assert same_hits(he, hf)
    if e.top_k == 0:
        off = he[0].astype(np.int64)
        for i in range(q.shape[0]):
            ec, eg = ox.query(q[i], min_score=ms)
            assert np.array_equal(he[1][off[i]:off[i + 1]], ec) and np.array_equal(he[2][off[i]:off[i + 1]], eg), i
    me = e.matrix_range(0, n)
    assert np.array_equal(me, fresh.matrix_range(0, n)) and np.array_equal(me, ox.matrix_range(0, n).T)
    for call in ("cluster", "dereplicate"):
        (la, na), (lb, nb) = getattr(e, call)(selfjoin_threshold), getattr(fresh, call)(selfjoin_threshold)
        assert np.array_equal(la, lb) and na == nb, call


@pytest.fixture(scope="module")
def small():
    return data(3000, 11)


@pytest.mark.parametrize("share", [0.17, 0.60])
@pytest.mark.parametrize("form", FORMS)
def test_retain_equals_a_fresh_handle_and_the_oracle(native, po, small, form, share):
    sk = small
    rng = np.random.default_rng(int(share * 100))
    keep = rng.random(sk.shape[0]) < share
    q = queries_for(sk, keep, rng)
    e = engine(native, form, sk)
    e.query(q[:2])                                             # an index exists before the call
    if form == "paged":
        assert e.stat("pages") >= 4
    bytes_before = e.stat("store_bytes")
    n_kept, ids = e.retain(keep)
    assert n_kept == int(keep.sum()) and np.array_equal(ids, expected_ids(keep))
    if form == "paged":
        assert e.stat("pages") >= 4
    else:
        assert e.stat("store_bytes") < bytes_before
    assert e.stat("delta_genomes") == 0
    fresh = engine(native, form, sk[keep])
    check_equivalent(po, e, fresh, sk[keep], q, S, 50, T_CHAIN20)
    e.close()
    fresh.close()


def test_retain_whole_range_s16(native, po):
    S16, N = 16, 300
    F16 = 1 << S16
    rng = np.random.default_rng(9)
    base = rng.integers(0, 1 << W, (5, F16)).astype(np.int32)
    sk = base[rng.integers(0, 5, N)].copy()
    noise = rng.random(sk.shape) < 0.3
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    keep = rng.random(N) < 0.4
    q = queries_for(sk, keep, rng)
    e = native.Engine(K=31, S=S16, W=W, H=3, min_score_value=1000)
    e.insert(sk)
    e.query(q[:2])
    n_kept, ids = e.retain(keep)
    assert n_kept == int(keep.sum()) and np.array_equal(ids, expected_ids(keep))
    fresh = native.Engine(K=31, S=S16, W=W, H=3, min_score_value=1000)
    fresh.insert(sk[keep])
    check_equivalent(po, e, fresh, sk[keep], q, S16, 1000, int(0.4 * F16))
    e.close()
    fresh.close()


# ---- 3. a handle with a delta segment ---------------------------------------------------------------------------

def test_retain_with_a_delta_segment(native):
    sk = data(4750, 13)
    rng = np.random.default_rng(3)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:4600])
    e.query(sk[:2])                                            # the main index is built
    e.insert(sk[4600:4700])
    e.query(sk[:2])                                            # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    keep = rng.random(4700) < 0.8
    keep[[4598, 4599, 4600, 4650]] = False                     # dropped on both sides of the segment boundary
    keep[[4597, 4601, 4699]] = True
    q = queries_for(sk[:4700], keep, rng)
    n_kept, _ = e.retain(keep)
    assert e.stat("delta_genomes") == 0 and n_kept == int(keep.sum())
    fresh = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    fresh.insert(sk[:4700][keep])
    assert same_hits(e.query(q), fresh.query(q))
    assert e.stat("delta_genomes") == 0
    # genomes inserted afterwards get ids from n_kept on
    e.insert(sk[4700:])
    fresh.insert(sk[4700:])
    assert e.n_genomes == n_kept + 50
    q2 = np.concatenate([q, sk[4700:]])
    got = e.query(q2)
    assert same_hits(got, fresh.query(q2))
    off = got[0].astype(np.int64)
    for i in range(50):                                        # each new genome finds itself under its new id
        assert n_kept + i in got[2][off[q.shape[0] + i]:off[q.shape[0] + i + 1]]
    assert np.array_equal(e.get_sketches(n_kept, 50), sk[4700:])
    e.close()
    fresh.close()


# ---- 4. edges ----------------------------------------------------------------------------------------------------

def test_all_kept_changes_nothing(native, small):
    sk = small
    e = engine(native, "lists", sk)
    q = sk[[7, 100, 11, 2500]]
    before = e.query(q)
    index_bytes, store_bytes = e.stat("index_bytes"), e.stat("store_bytes")
    assert index_bytes > 0
    n_kept, ids = e.retain(np.ones(sk.shape[0], bool))
    assert n_kept == sk.shape[0] and np.array_equal(ids, np.arange(sk.shape[0], dtype=np.uint32))
    assert e.stat("index_bytes") == index_bytes and e.stat("store_bytes") == store_bytes      # the built index stays
    assert same_hits(before, e.query(q))
    e.close()


def test_none_kept_leaves_a_usable_index(native, small):
    sk = small
    e = engine(native, "lists", sk)
    e.query(sk[:2])
    n_kept, ids = e.retain(np.zeros(sk.shape[0], bool))
    assert n_kept == 0 and e.n_genomes == 0 and np.all(ids == NONE)
    assert e.retain(np.zeros(0, bool))[0] == 0                 # no genomes: NIQKI_OK, 0 kept
    e.insert(sk[:100])
    fresh = engine(native, "lists", sk[:100])
    assert same_hits(e.query(sk[:200]), fresh.query(sk[:200]))
    assert e.export_dump() == fresh.export_dump()
    e.close()
    fresh.close()


def test_a_slot_range_shard_refuses(native, small):
    sk = small[:200]
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50, slot_begin=0, slot_end=F // 2)
    e.insert(sk)
    with pytest.raises(native.NiqkiError) as ei:
        e.retain(np.ones(200, bool))
    assert ei.value.code == E_STATE
    assert e.n_genomes == 200
    e.close()


def test_device_memory_null_outputs_and_composition(native, small):
    import torch
    sk = small
    rng = np.random.default_rng(5)
    k1 = rng.random(sk.shape[0]) < 0.7
    k2 = rng.random(int(k1.sum())) < 0.5
    composed = np.zeros(sk.shape[0], bool)
    composed[np.nonzero(k1)[0][k2]] = True
    a = engine(native, "lists", sk)
    n1, ids1 = a.retain(k1)
    # NIQKI_MEM_DEVICE: keep and new_ids as device arrays on the handle's stream, the count in host memory
    b = engine(native, "lists", sk)
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    d_keep = torch.from_numpy(k1.astype(np.uint8)).cuda()
    d_ids = torch.full((sk.shape[0],), 7, dtype=torch.int32, device="cuda")
    n = C.c_uint32(0)
    assert b.L.niqki_retain(b.h, d_keep.data_ptr(), d_ids.data_ptr(), C.byref(n), 1) == 0
    torch.cuda.synchronize()
    assert n.value == n1 and np.array_equal(d_ids.cpu().numpy().view(np.uint32), ids1)
    assert np.array_equal(b.get_sketches(0, n1), a.get_sketches(0, n1))
    # new_ids and n_kept may be NULL
    c = engine(native, "lists", sk)
    flags = k1.astype(np.uint8)
    assert c.L.niqki_retain(c.h, flags.ctypes.data, None, None, 0) == 0 and c.n_genomes == n1
    assert np.array_equal(c.get_sketches(0, n1), sk[k1])
    # two retains in a row equal one retain with the composed mask
    n2, ids2 = a.retain(k2)
    d = engine(native, "lists", sk)
    nc, idc = d.retain(composed)
    assert n2 == nc == int(composed.sum())
    two_steps = np.full(sk.shape[0], NONE, np.uint32)
    two_steps[k1] = ids2
    assert np.array_equal(two_steps, idc)
    q = sk[rng.integers(0, sk.shape[0], 32)]
    assert a.export_dump() == d.export_dump() and same_hits(a.query(q), d.query(q))
    for x in (a, b, c, d):
        x.close()
