"""CPU: tests/collapse_ref.py, the expectation of the collapsed-query tests, pinned on the oracle.  A plain loop over the
oracle's own ordered hit list (pyoracle.Index.query) -- keep an entry when its label was not seen before, count every
label -- must give what the numpy module gives from the count rows, for a few hundred mixed queries and several label
sets; and the consequences include/niqki_hip.h states must hold."""
import numpy as np
import pytest

from collapse_ref import collapse_lists, collapse_rows, count_rows, few_cell_query
from cover_ref import query_kinds, slot_minimum
from test_gpu_cluster import S, W, data
import hit_designs as hd

N = 3000


def label_sets(n, seed=3):
    rng = np.random.default_rng(seed)
    sparse = rng.choice(np.array([0, 0xFFFFFFFF, 5, 1 << 31, 123456789, 77, 4096, 8192], np.uint32), n)
    return {
        "identity": np.arange(n, dtype=np.uint32),
        "one": np.full(n, 42, np.uint32),
        "mod7": (np.arange(n) % 7).astype(np.uint32),
        "sparse": sparse,
        "pow2": (rng.integers(0, 40, n) * 8192 + rng.integers(0, 3, n)).astype(np.uint32),
    }


@pytest.fixture(scope="module")
def case(po):
    sk = data(N, 11)
    rng = np.random.default_rng(29)
    q = list(query_kinds(sk, W).values())
    q += [sk[g].copy() for g in rng.integers(0, N, 120)]
    q += [slot_minimum(sk[rng.choice(N, 3, replace=False)]) for _ in range(100)]
    q += [rng.integers(0, 1 << W, 1 << S).astype(np.int32) for _ in range(20)]
    q += [np.full(1 << S, -1, np.int32)] * 4
    q += [few_cell_query(sk, g, W, rng) for g in (100, 1234)]
    q = np.stack(q).astype(np.int32)
    return sk, q, po.Index(po.make_params(31, S, W, 3, 0.0), sk), count_rows(sk, q, W)


def by_loop(ix, q, ms, labels, top_k):
    out = []
    for x in q:
        hc, hg = ix.query(x, min_score=ms)
        seen, members = {}, {}
        for c, g in zip(hc.tolist(), hg.tolist()):
            lab = int(labels[g])
            members[lab] = members.get(lab, 0) + 1
            if lab not in seen:
                seen[lab] = (c, g)
        lst = [(c, g, members[lab]) for lab, (c, g) in seen.items()]      # dicts keep insertion order: list order
        out.append(lst[:top_k] if top_k else lst)
    return out


@pytest.mark.parametrize("ms", [50, 1, 0])
def test_the_module_equals_a_loop_over_the_oracles_lists(case, ms):
    sk, q, ix, rows = case
    assert q.shape[0] >= 250
    use = q if ms else q[:24]                                  # (min_score 0: every list holds all 3000 genomes)
    r = rows[:use.shape[0]]
    for name, labels in label_sets(N).items():
        for top_k in (0, 1, 3):
            off, c, g, m = collapse_rows(r, ms, labels, top_k)
            assert off.dtype == np.uint64 and c.dtype == g.dtype == m.dtype == np.uint32
            exp = by_loop(ix, use, ms, labels, top_k)
            assert np.diff(off).tolist() == [len(x) for x in exp], (name, top_k)
            flat = [e for x in exp for e in x]
            assert list(zip(c.tolist(), g.tolist(), m.tolist())) == flat, (name, top_k)


def test_the_stated_consequences_hold(case):
    sk, q, ix, rows = case
    sets = label_sets(N)
    for ms in (50, 1):
        full = hd.reference_lists(rows, ms)
        lens = np.diff(full[0])
        assert lens.min() == 0 and lens.max() > 64 and ((lens == 1).any() or ms == 1)
        ident = collapse_lists(full, sets["identity"])
        assert np.array_equal(ident[0].astype(np.int64), full[0]) and np.array_equal(ident[1], full[1]) and np.array_equal(ident[2], full[2])
        assert (ident[3] == 1).all()
        one = collapse_lists(full, sets["one"])
        assert np.array_equal(np.diff(one[0].astype(np.int64)), np.minimum(lens, 1))
        assert np.array_equal(one[3], lens[lens > 0])
        first = full[0][:-1][lens > 0]
        assert np.array_equal(one[1], full[1][first]) and np.array_equal(one[2], full[2][first])
        for name in ("mod7", "sparse", "pow2"):
            a = collapse_lists(full, sets[name])
            o = a[0].astype(np.int64)
            assert np.array_equal(np.add.reduceat(np.append(a[3], 0).astype(np.int64), o[:-1])[np.diff(o) > 0], lens[lens > 0]), name
            for k in (1, 2, 5):
                b = collapse_lists(full, sets[name], k)
                ob = b[0].astype(np.int64)
                assert np.array_equal(np.diff(ob), np.minimum(np.diff(o), k))
                for i in range(0, lens.size, 7):                       # the cut is a prefix, members untouched
                    n = int(ob[i + 1] - ob[i])
                    for x, y in zip(a[1:], b[1:]):
                        assert np.array_equal(x[o[i]:o[i] + n], y[ob[i]:ob[i + 1]])


def test_what_designed_lists_must_give():
    """ties across labels are ordered by gid, a tie inside a label goes to the larger gid"""
    rows = np.array([[30, 30, 30, 20, 0, 30]])
    labels = np.array([9, 9, 4, 4, 4, 0xFFFFFFFF], np.uint32)
    off, c, g, m = collapse_rows(rows, 20, labels)
    assert off.tolist() == [0, 3] and g.tolist() == [5, 2, 1] and c.tolist() == [30, 30, 30] and m.tolist() == [1, 2, 2]
    off, c, g, m = collapse_rows(rows, 20, labels, 2)
    assert off.tolist() == [0, 2] and g.tolist() == [5, 2] and m.tolist() == [1, 2]
    off, c, g, m = collapse_rows(rows, 31, labels)
    assert off.tolist() == [0, 0] and c.size == 0
