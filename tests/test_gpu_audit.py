"""GPU: niqki_audit, every indexed genome's leave-one-out neighbours read against the labelling of niqki_set_labels
(include/niqki_hip.h has the definition).  Expected rows never come from the call: audit_ref.audit_matrix over the
oracle's count matrix, and audit_ref.audit_lists over the lists Engine.neighbors_range returns for the same handle.

The designed index is made of cells whose agreements are known: a cell is empty (-1, agrees with nothing) or holds its
group's value, so two genomes of a group agree exactly on the slots both fill, and genomes of two groups never do."""
import ctypes as C

import numpy as np
import pytest

from audit_ref import ALONE, AGREES, MISPLACED, NONE, STRAY, TIED, audit_lists, audit_matrix
from lists_ref import room, splits
from test_gpu_cluster import F, FORMS, S, T_CHAIN10, T_CHAIN20, W, data, engine, labels_of_matrix, oracle_matrix
from test_gpu_cover import own_params

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = 1, 5
KS = (1, 5, 63)
REGION = 201                       # slots of a hub: five of them fit F = 1024
D_AT = (63, 64, 65, 128, 200)      # case (d): where in H(hub) the first own-label entry stands


class Design:
    """The genomes of the designed index: add() appends one and returns its id."""

    def __init__(self):
        self.rows, self.labels = [], []

    def add(self, label, value=0, spans=()):
        """a genome that holds `value` on the slots [lo, hi) of every span and nothing elsewhere"""
        s = np.full(F, -1, np.int32)
        for lo, hi in spans:
            s[lo:hi] = value
        self.rows.append(s)
        self.labels.append(label)
        return len(self.rows) - 1


def designed():
    d, ids = Design(), {}
    reg = lambda r, n=REGION: (r * REGION, r * REGION + n)                      # the first n slots of region r
    # (d) five hubs, one region each, and 200 spokes that fill the first 200 - i slots of EVERY region: hub r's list
    # is itself (201), then the spokes by count.  Its partner fills 201 - P slots and has a larger id than the spokes,
    # so it ties spoke P - 1 and stands before it: place P of the list, P - 1 foreign entries ahead of it.
    ids["d_hub"] = [d.add(100 + r, 1, [reg(r)]) for r in range(5)]
    ids["d_spoke"] = [d.add(50, 1, [reg(r, 200 - i) for r in range(5)]) for i in range(200)]
    ids["d_own"] = [d.add(100 + r, 1, [reg(r, REGION - P)]) for r, P in enumerate(D_AT)]
    # (e) three hubs with 63, 64 and 65 neighbours: lists of 64, 65 and 66 entries, 64 and 65 of them with and without
    # the hub itself.  Spoke i holds 10 + i slots; spoke 0, the last entry of each list, alone carries the hubs' label.
    ids["e_hub"] = [d.add(70, 2, [reg(r)]) for r in range(3)]
    ids["e_spoke"] = [d.add(70 if i == 0 else 60 + i % 3, 2, [reg(r, 10 + i) for r in range(3) if i < 63 + r]) for i in range(65)]
    # (f) (g) a hub of label 81 whose four neighbours carry 80, 81, 81, 80 in list order
    ids["f_hub"] = d.add(81, 3, [reg(0)])
    ids["f_spoke"] = [d.add(lab, 3, [reg(0, n)]) for lab, n in ((80, 50), (81, 40), (81, 30), (80, 20))]
    # (a) (h) three exact duplicates: the first one's own entry is the third of its list, the second one's the second
    ids["dup"] = [d.add(90, 4, [reg(0, 77)]) for _ in range(3)]
    # (b) nothing at all
    ids["empty"] = d.add(90)
    # (i) two genomes that agree on 30 slots, each the only member of its label
    ids["lone"] = [d.add(91 + j, 5, [reg(1, 30 + j)]) for j in range(2)]
    # (c) the own-label neighbour and the foreign one both at 40, the foreign one with the larger id
    ids["c_hub"] = d.add(95, 6, [reg(0)])
    ids["c_own"] = d.add(95, 6, [reg(0, 40)])
    ids["c_other"] = d.add(96, 6, [reg(0, 40)])
    return np.stack(d.rows), np.array(d.labels, np.uint32), ids


def place_in_list(M, g, h):
    """where h stands in H(g) at threshold 1: the entries before it hold a larger count, or the same and a larger id"""
    row = M[g].astype(np.int64)
    j = np.arange(row.size)
    return int(np.sum((row > row[h]) | ((row == row[h]) & (j > h))))


def row(exp, g):
    return tuple(int(a[g]) for a in exp)


@pytest.fixture(scope="module")
def design(po):
    sk, labels, ids = designed()
    N = sk.shape[0]
    assert N <= 400
    M = oracle_matrix(po, sk)
    exp = {(t, k): audit_matrix(M, labels, t, k) for t in (1, 100, F + 1) for k in (1, 4, 63)}
    e1, e4, e63 = exp[1, 1], exp[1, 4], exp[1, 63]
    # (a) (h): the duplicates' lists are 2 1 0, each without itself
    d0, d1, d2 = ids["dup"]
    assert [place_in_list(M, g, g) for g in (d0, d1, d2)] == [2, 1, 0]
    assert row(e1, d0) == (AGREES, 77, d2, 0, NONE, d2, 1) and row(e1, d1) == (AGREES, 77, d2, 0, NONE, d2, 1)
    assert row(e1, d2) == (AGREES, 77, d1, 0, NONE, d1, 1) and row(e4, d0)[5:] == (d2, 2)
    # (b)
    assert M[ids["empty"]].sum() == 0 and row(e63, ids["empty"]) == (ALONE, 0, NONE, 0, NONE, NONE, 0)
    # (c)
    assert ids["c_other"] > ids["c_own"]
    assert row(e1, ids["c_hub"]) == (TIED, 40, ids["c_own"], 40, ids["c_other"], ids["c_other"], 1)
    # (d)
    for hub, own, P in zip(ids["d_hub"], ids["d_own"], D_AT):
        assert place_in_list(M, hub, hub) == 0 and place_in_list(M, hub, own) == P
        assert row(e1, hub) == (MISPLACED, REGION - P, own, 200, ids["d_spoke"][0], ids["d_spoke"][0], 1)
        assert row(e63, hub)[5:] == (ids["d_spoke"][0], 62 if P == 63 else 63)       # (the partner is the 63rd of H')
    # (e)
    for r, hub in enumerate(ids["e_hub"]):
        assert int(np.sum(M[hub] >= 1)) == 64 + r
        last = ids["e_spoke"][0]
        assert place_in_list(M, hub, last) == 63 + r
        assert row(e1, hub)[:3] == (MISPLACED, 10, last) and row(e1, hub)[4] == ids["e_spoke"][62 + r]
    # (f) (g): 80 and 81 tie at k = 4 and 63, the label met first wins; k = 3 is not a tie
    f = ids["f_hub"]
    assert int(np.sum(M[f] >= 1)) == 5
    assert row(e4, f) == (MISPLACED, 40, ids["f_spoke"][1], 50, ids["f_spoke"][0], ids["f_spoke"][0], 2)
    assert row(e63, f) == row(e4, f) and row(audit_matrix(M, labels, 1, 3), f)[5:] == (ids["f_spoke"][1], 2)
    # (i)
    assert all(row(e1, g)[:3] == (STRAY, 0, NONE) and row(e1, g)[3] == 30 for g in ids["lone"])
    # the middle threshold cuts lists, F + 1 leaves nothing
    assert row(exp[100, 63], ids["d_hub"][3])[:3] == (STRAY, 0, NONE) and row(exp[100, 63], ids["d_hub"][0])[0] == MISPLACED
    assert all(np.all(exp[F + 1, k][0] == ALONE) and np.all(exp[F + 1, k][5] == NONE) for k in (1, 4, 63))
    return sk, labels, M, exp


def check(e, t, k, exp, what=None):
    got = e.audit(t, k)
    assert len(got) == 7
    for name, a, b in zip(("verdict", "own_count", "own_gid", "other_count", "other_gid", "vote_gid", "vote_n"), got, exp):
        assert a.dtype == np.uint32 and np.array_equal(a, b), (what, t, k, name, np.nonzero(a != b)[0][:8])


@pytest.mark.parametrize("form", ["lists", "rows", "batch64"])
def test_designed_index(native, design, form):
    sk, labels, M, exp = design
    e = engine(native, form, sk)
    e.set_labels(labels)
    for (t, k), rows in exp.items():
        check(e, t, k, rows, form)
    for k in (1, 4, 63):
        check(e, 0, k, exp[1, k], form)                  # threshold 0 is threshold 1
    own_params(e, 50, 0)
    e.close()


def test_designed_index_one_label_and_all_labels(native, design):
    sk, _, M, _ = design
    N = sk.shape[0]
    cases = []
    for labels, gid_col in ((np.full(N, 7, np.uint32), 4), (np.arange(N, dtype=np.uint32)[::-1] * 3, 2)):
        exp = audit_matrix(M, labels, 1, 5)
        assert np.all(exp[gid_col] == NONE) and np.all(exp[gid_col - 1] == 0)       # (j) no foreign entry; (k) no own one
        assert set(exp[0].tolist()) == ({ALONE, AGREES} if gid_col == 4 else {ALONE, STRAY})
        cases.append((labels, exp))
    e = engine(native, "lists", sk)
    for labels, exp in cases:
        e.set_labels(labels)
        check(e, 1, 5, exp)
    e.close()


# ---- the definition on every index form ------------------------------------------------

def noisy_labels(M, seed, tied_pair):
    """the single-linkage clusters at T_CHAIN10 (a union-find over the oracle's matrix), about 2 % of the genomes moved
    to another genome's label; tied_pair: two exact duplicates of one cluster, the second of which is moved too"""
    rng = np.random.default_rng(seed)
    N = M.shape[0]
    labels = labels_of_matrix(M, T_CHAIN10).astype(np.uint32)
    moved = rng.choice(N, N // 50, replace=False)
    labels[moved] = labels[rng.integers(0, N, moved.size)]
    labels[tied_pair[1]] = labels[0] if labels[0] != labels[tied_pair[0]] else labels[1]
    return labels


def neighbor_lists(e, t, top_k):
    """the full ordered lists of the stored sketches at min_score t, by the query path of this handle"""
    N = e.n_genomes
    e.set_option("min_score", t)
    e.set_option("top_k", 0)
    off, hc, hg = e.neighbors_range(0, N, capacity=N * N)
    e.set_option("min_score", 50)
    e.set_option("top_k", top_k)
    return off, hc, hg


THRESHOLDS = (1, T_CHAIN20, T_CHAIN10)


@pytest.fixture(scope="module")
def small(po):
    sk = data(3000, 11)
    M = oracle_matrix(po, sk)
    dup = np.nonzero((sk == sk[7]).all(1))[0]
    labels = noisy_labels(M, 3, (int(dup[2]), int(dup[3])))
    exp = {(t, k): audit_matrix(M, labels, t, k) for t in THRESHOLDS for k in KS}
    assert set(np.concatenate([exp[t, 1][0] for t in THRESHOLDS]).tolist()) == {ALONE, AGREES, TIED, MISPLACED, STRAY}
    assert any(np.any(exp[t, 63][6] > 1) for t in THRESHOLDS)
    return sk, labels, exp


@pytest.mark.parametrize("form", FORMS)
def test_audit_equals_the_definition(native, small, form):
    sk, labels, by_matrix = small
    e = engine(native, form, sk)
    e.set_labels(labels)
    top_k = 3 if form == "top_k3" else 0
    for t in THRESHOLDS:
        lists = neighbor_lists(e, t, top_k)
        for k in KS:
            exp = audit_lists(*lists, labels, k)
            if form == "lists":                          # once: the lists' route against the matrix's
                assert all(np.array_equal(a, b) for a, b in zip(exp, by_matrix[t, k])), (t, k)
            check(e, t, k, exp, form)
    if form == "tiles":
        assert e.stat("tiles") > 1
    if form == "paged":
        assert e.stat("pages") >= 4
    own_params(e, 50, top_k)
    e.close()


def test_audit_with_a_delta_segment(native):
    N, first = 4600, 4200                                # (a delta segment needs a main index of 4096 genomes)
    sk = data(N, 13)
    rng = np.random.default_rng(5)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    e.insert(sk[:first])
    e.query(sk[:2])                                      # the main index is built
    e.insert(sk[first:])
    e.query(sk[:2])                                      # ... and the delta segment
    assert e.stat("delta_genomes") > 0
    # labels from this handle's own lists: every genome takes the label of its best other neighbour at T_CHAIN10, where
    # it has one; then about 2 % are moved
    off, hc, hg = neighbor_lists(e, T_CHAIN10, 0)
    labels = np.arange(N, dtype=np.uint32)
    for g in range(N):
        h = hg[int(off[g]):int(off[g + 1])]
        h = h[h != g]
        if h.size:
            labels[g] = min(g, int(h[0]))
    moved = rng.choice(N, N // 50, replace=False)
    labels[moved] = labels[rng.integers(0, N, moved.size)]
    e.set_labels(labels)
    seen = set()
    for t in THRESHOLDS:
        lists = neighbor_lists(e, t, 0)
        for k in KS:
            exp = audit_lists(*lists, labels, k)
            seen |= set(exp[0].tolist())
            check(e, t, k, exp, "delta")
    assert {ALONE, AGREES, MISPLACED, STRAY} <= seen
    assert e.stat("delta_genomes") > 0
    e.close()


# ---- splits ---------------------------------------------------------------------------

def test_audit_rows_do_not_depend_on_splits(native):
    """One dense cluster of 1 500 genomes (test_gpu_cluster.py): the smallest hit buffers hold a tenth of a batch."""
    N, thr = 3000, T_CHAIN20
    sk = data(N, 12, dense=1500)
    labels = np.random.default_rng(9).integers(0, 5, N).astype(np.uint32)
    e = engine(native, "lists", sk)
    lists = neighbor_lists(e, thr, 0)
    n_splits = splits(np.diff(lists[0].astype(np.int64)), 1024, room(1, N), True)
    assert n_splits > 0
    exp = audit_lists(*lists, labels, 5)
    e.set_labels(labels)
    check(e, thr, 5, exp)
    assert e.stat("audit_splits") == 0 and e.stat("audit_pairs") == int(lists[0][-1])
    e.set_option("cluster_ws_mib", 1)
    check(e, thr, 5, exp)
    assert e.stat("audit_splits") == n_splits and e.stat("audit_pairs") == int(lists[0][-1])
    e.close()


# ---- state and arguments ----------------------------------------------------------------

def audit_raw(e, t, k, arrays, mem=0):
    ptr = [None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()) for a in arrays]
    return e.L.niqki_audit(e.h, t, k, *ptr, mem)


def test_audit_state_and_arguments(native, design):
    import torch
    from niqki_amd import capi
    sk, labels, M, exp = design
    N = sk.shape[0]
    e = engine(native, "top_k3", sk)
    for key in ("audit_splits", "audit_pairs", "audit_us_read", "audit_us_hits", "audit_us_scan"):
        assert e.stat(key) == 0, key
    none7 = [None] * 7
    out = [np.full(N, 0xABCD, np.uint32) for _ in range(7)]

    def refused_for_labels():
        assert audit_raw(e, 1, 1, out) == E_STATE
        text = e.L.niqki_last_error(e.h).decode()
        assert "niqki_audit" in text and "niqki_set_labels" in text and "again" in text
        assert all(np.all(a == 0xABCD) for a in out)
        own_params(e, 50, 3)

    refused_for_labels()                                 # no labelling yet
    e.set_labels(labels)
    for k in (0, 64, 1 << 20):
        assert audit_raw(e, 1, k, out) == E_INVALID and all(np.all(a == 0xABCD) for a in out)
        own_params(e, 50, 3)
    assert audit_raw(e, 1, 4, none7) == 0                # every array NULL
    assert audit_raw(e, 1, 4, out) == 0
    assert all(np.array_equal(a, b) for a, b in zip(out, exp[1, 4]))
    only = np.zeros(N, np.uint32)                        # ... or any of them
    assert audit_raw(e, 1, 4, [None, None, None, None, only, None, None]) == 0 and np.array_equal(only, exp[1, 4][4])
    own_params(e, 50, 3)
    # device outputs equal host outputs
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = [torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda") for _ in range(7)]
    e.audit_dev(100, 63, *dev)
    torch.cuda.synchronize()
    assert all(np.array_equal(d.cpu().numpy().view(np.uint32), b) for d, b in zip(dev, exp[100, 63]))
    e.audit_dev(1, 4, vote_n=dev[6])
    torch.cuda.synchronize()
    assert np.array_equal(dev[6].cpu().numpy().view(np.uint32), exp[1, 4][6])
    assert np.array_equal(dev[0].cpu().numpy().view(np.uint32), exp[100, 63][0])     # (not written by that call)
    own_params(e, 50, 3)
    assert capi.AUDIT_VERDICTS == ("alone", "agrees", "tied", "misplaced", "stray")
    assert (capi.AUDIT_ALONE, capi.AUDIT_AGREES, capi.AUDIT_TIED, capi.AUDIT_MISPLACED, capi.AUDIT_STRAY) == (ALONE, AGREES, TIED, MISPLACED, STRAY)
    # an insert removes the labelling
    e.insert(sk[:1])
    out = [np.full(N + 1, 0xABCD, np.uint32) for _ in range(7)]
    refused_for_labels()
    e.close()


def test_audit_without_genomes_and_on_a_shard(native, design):
    sk, labels, _, _ = design
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50)
    assert audit_raw(e, 1, 1, [None] * 7) == 0           # no genomes: also without a labelling
    assert audit_raw(e, 1, 0, [None] * 7) == E_INVALID
    assert tuple(a.size for a in e.audit(1)) == (0,) * 7
    e.close()
    shard = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50, slot_begin=0, slot_end=F // 2)
    shard.insert(sk)
    out = [np.zeros(sk.shape[0], np.uint32) for _ in range(7)]
    assert audit_raw(shard, 1, 1, out) == E_STATE
    assert "whole-range" in shard.L.niqki_last_error(shard.h).decode()
    shard.close()
