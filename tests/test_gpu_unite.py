"""GPU: niqki_unite leaves one entry per label, its sketch the per-slot minimum of the members' valid cells.  Definition:
afterwards the handle is indistinguishable, through the ABI, from a fresh handle into which the labels' sketches were
inserted in label order.  Expected values are tests/unite_ref.py's numpy minimum over the sketches read BEFORE the
call, a fresh handle fed those, the oracle's Index of them and, for the sketch path, niqki_sketch with entry_rec --
never niqki_unite itself.  The designed labellings are those of tests/unite_ref.py, which names the launch's numbers
from niqki_amd/csrc/nq_unite_blocks.h; data and engine forms are those of test_gpu_cluster.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cluster import F, FORMS, S, T_CHAIN20, W, data, engine
from test_gpu_retain import check_equivalent, same_hits
from unite_ref import (PAN_GROUPS, PAN_H, PAN_K, PAN_S, PAN_W, designed_labelings, number_labels, one_valid_cell_in_the_last_member,
                       oracle_pan_sketches, pan_records, unite_ref)

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = 1, 5
SIZES = [1, 7, 64, 65, 2049, 8300]


# ---- 1. the minimum pass at designed labellings -------------------------------------------------------------------

@pytest.fixture(scope="module")
def columns():
    """8 300 sketches whose every cell differs from its neighbours' (a column that lands one place off shows)"""
    rng = np.random.default_rng(77)
    sk = rng.integers(0, 1 << W, (max(SIZES), F)).astype(np.int32)
    sk[rng.random(sk.shape) < 0.01] = -1
    return sk


@pytest.mark.parametrize("n", SIZES)
def test_minimum_at_designed_labelings(native, columns, n):
    for name, lab in designed_labelings(n):
        ids, n_labels = number_labels(lab)
        # the last label's only valid cell of slots 0 .. 7 sits in its last member; rows 16 .. 47 (two whole row blocks
        # of the launch) are empty in every member of label 0
        sk = one_valid_cell_in_the_last_member(columns[:n], lab, range(8))
        sk[np.ix_(ids == 0, np.arange(16, 48))] = -1
        e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
        e.insert(sk)
        before = e.get_sketches(0, n)
        assert np.array_equal(before, sk), name
        eu, eids = unite_ref(before, lab)
        got_l, got_ids = e.unite(lab)
        assert got_l == n_labels == e.n_genomes == eu.shape[0], name
        assert got_ids.dtype == np.uint32 and np.array_equal(got_ids, eids), name
        after = e.get_sketches(0, n_labels)
        assert np.array_equal(after, eu), name                 # every cell of every label
        assert (after[0, 16:48] == -1).all(), name
        e.close()


# ---- 2. equivalence with a fresh handle and with the oracle -----------------------------------------------------

@pytest.fixture(scope="module")
def small():
    return data(3000, 11)


def queries_for(sk, u, rng):
    q = [sk[rng.choice(sk.shape[0], 24, replace=False)], u[rng.choice(u.shape[0], 24, replace=False)],
         rng.integers(0, 1 << W, (16, sk.shape[1])).astype(np.int32)]
    return np.concatenate(q)


@pytest.mark.parametrize("labelling", ["div7", "mod37"])
@pytest.mark.parametrize("form", FORMS)
def test_unite_equals_a_fresh_handle_and_the_oracle(native, po, small, form, labelling):
    sk = small
    g = np.arange(sk.shape[0])
    lab = g // 7 if labelling == "div7" else g % 37
    u, ids = unite_ref(sk, lab)
    rng = np.random.default_rng(len(labelling))
    q = queries_for(sk, u, rng)
    e = engine(native, form, sk)
    e.query(q[:2])                                             # an index exists before the call
    if form == "paged":
        assert e.stat("pages") >= 4
    bytes_before = e.stat("store_bytes")
    n_labels, got_ids = e.unite(lab)
    assert n_labels == u.shape[0] and np.array_equal(got_ids, ids)
    if form == "paged":
        assert e.stat("pages") >= 4
    else:
        assert e.stat("store_bytes") < bytes_before
    assert e.stat("delta_genomes") == 0
    fresh = engine(native, form, u)
    check_equivalent(po, e, fresh, u, q, S, 50, T_CHAIN20)
    e.close()
    fresh.close()


# ---- 3. a handle with a delta segment ---------------------------------------------------------------------------

def test_unite_with_a_delta_segment(native, po):
    sk = data(4750, 13)
    rng = np.random.default_rng(3)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:4600])
    e.query(sk[:2])                                            # the main index is built
    e.insert(sk[4600:4700])
    e.query(sk[:2])                                            # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    lab = np.arange(4700) % 1567                               # the labels from 1466 on have members in both segments
    u, ids = unite_ref(sk[:4700], lab)
    n_labels, got_ids = e.unite(lab)
    assert e.stat("delta_genomes") == 0 and n_labels == 1567 and np.array_equal(got_ids, ids)
    fresh = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    fresh.insert(u)
    check_equivalent(po, e, fresh, u, queries_for(sk[:4700], u, rng), S, 50, T_CHAIN20)
    assert e.stat("delta_genomes") == 0
    # genomes inserted afterwards get ids from L on and are found
    e.insert(sk[4700:])
    assert e.n_genomes == n_labels + 50
    got = e.query(sk[4700:])
    off = got[0].astype(np.int64)
    for i in range(50):
        assert n_labels + i in got[2][off[i]:off[i + 1]]
    assert np.array_equal(e.get_sketches(n_labels, 50), sk[4700:])
    e.close()
    fresh.close()


# ---- 4. the sketch path agrees ------------------------------------------------------------------------------------

def test_unite_of_member_sketches_equals_the_sketch_of_the_pooled_records(native, po):
    records, labels = pan_records()
    members, groups = oracle_pan_sketches(po)
    assert (members >= 0).all()                                # no empty cell: densification plays no part
    e = native.Engine(K=PAN_K, S=PAN_S, W=PAN_W, H=PAN_H, min_score_value=10)
    one_each = e.sketch(records)
    assert np.array_equal(one_each, members)
    entry_rec = np.concatenate([[0], np.cumsum(PAN_GROUPS)]).astype(np.uint32)
    pooled = e.sketch(records, entry_rec)
    assert np.array_equal(pooled, groups)
    e.insert(one_each)
    n_labels, ids = e.unite(labels)
    assert n_labels == len(PAN_GROUPS) and np.array_equal(ids, labels)
    assert np.array_equal(e.get_sketches(0, n_labels), pooled)
    e.close()


# ---- 5. edges, refusals, reuse --------------------------------------------------------------------------------------

def test_identity_labelling_changes_nothing_but_drops_the_labels(native, small):
    sk = small
    e = engine(native, "lists", sk)
    q = sk[[7, 100, 11, 2500]]
    before = e.query(q)
    e.set_labels(np.arange(sk.shape[0]) // 5)
    e.query_collapsed(q)
    index_bytes, store_bytes = e.stat("index_bytes"), e.stat("store_bytes")
    assert index_bytes > 0
    n_labels, ids = e.unite(np.arange(sk.shape[0]))
    assert n_labels == sk.shape[0] and np.array_equal(ids, np.arange(sk.shape[0], dtype=np.uint32))
    assert e.stat("index_bytes") == index_bytes and e.stat("store_bytes") == store_bytes      # the built index stays
    assert same_hits(before, e.query(q))
    with pytest.raises(native.NiqkiError) as ei:               # the labelling set before is gone
        e.query_collapsed(q)
    assert ei.value.code == E_STATE
    e.close()


def test_refusals(native, small):
    sk = small[:200]
    e = engine(native, "lists", sk)
    dump = e.export_dump()
    ids = np.zeros(201, np.uint32)
    n = C.c_uint32(77)
    for count in (199, 201, 0):
        lab = np.zeros(201, np.uint32)
        assert e.L.niqki_unite(e.h, lab.ctypes.data, count, ids.ctypes.data, C.byref(n), 0) == E_INVALID
    assert e.n_genomes == 200 and e.export_dump() == dump
    e.append_begin(dump[:24])                                  # a pending append
    with pytest.raises(native.NiqkiError) as ei:
        e.unite(np.zeros(200, np.uint32))
    assert ei.value.code == E_STATE
    e.close()
    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50, slot_begin=0, slot_end=F // 2)
    shard.insert(sk)
    with pytest.raises(native.NiqkiError) as ei:
        shard.unite(np.zeros(200, np.uint32))
    assert ei.value.code == E_STATE and shard.n_genomes == 200
    shard.close()


def test_empty_handle_and_reuse(native, small):
    sk = small
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    n_labels, ids = e.unite(np.zeros(0, np.uint32))
    assert n_labels == 0 and ids.size == 0 and e.n_genomes == 0
    e.insert(sk[:300])
    lab = np.arange(300) % 10
    u, _ = unite_ref(sk[:300], lab)
    assert e.unite(lab)[0] == 10
    e.insert(sk[300:400])                                      # ids from L on
    fresh = engine(native, "lists", np.concatenate([u, sk[300:400]]))
    assert e.n_genomes == 110 and e.export_dump() == fresh.export_dump()
    got = e.query(sk[300:400])
    assert same_hits(got, fresh.query(sk[300:400]))
    off = got[0].astype(np.int64)
    for i in range(100):
        assert 10 + i in got[2][off[i]:off[i + 1]]
    # a second unite of the united handle: one label for all
    all_u, _ = unite_ref(np.concatenate([u, sk[300:400]]), np.zeros(110))
    n_labels, ids = e.unite(np.full(110, 0xFFFFFFFF, np.uint32))
    assert n_labels == 1 and not ids.any() and np.array_equal(e.get_sketches(0, 1), all_u)
    e.close()
    fresh.close()


def test_device_memory_and_null_outputs(native, small):
    import torch
    sk = small
    lab = (np.arange(sk.shape[0]) * 7919 % 411).astype(np.uint32)
    a = engine(native, "lists", sk)
    n_a, ids_a = a.unite(lab)
    b = engine(native, "lists", sk)
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    d_lab = torch.from_numpy(lab.view(np.int32)).cuda()
    n_b, d_ids = b.unite(d_lab)
    torch.cuda.synchronize()
    assert d_ids.is_cuda and n_b == n_a == 411
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), ids_a)
    assert np.array_equal(b.get_sketches(0, n_b), a.get_sketches(0, n_a))
    c = engine(native, "lists", sk)                            # new_ids and n_labels may be NULL
    assert c.L.niqki_unite(c.h, lab.ctypes.data, lab.size, None, None, 0) == 0 and c.n_genomes == n_a
    assert c.export_dump() == a.export_dump()
    for x in (a, b, c):
        x.close()


def test_stats(native, small):
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    v = C.c_uint64(0)
    for key in ("unite_us_prepare", "unite_us_min"):
        v.value = 0xDEAD
        assert e.L.niqki_get_stat(e.h, key.encode(), C.byref(v)) == 0 and v.value == 0, key
    v.value = 0xDEAD
    assert e.L.niqki_get_stat(e.h, b"unite_us", C.byref(v)) == E_INVALID and v.value == 0xDEAD
    e.insert(small[:500])
    e.profile(True)
    e.unite(np.arange(500) // 4)
    assert e.stat("unite_us_min") > 0 and e.stat("unite_us_prepare") > 0
    e.close()
