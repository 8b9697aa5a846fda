"""CPU: tests/tally_ref.py, the numpy restatement of the taxon tally (niqki_tally_read), pinned on a brute force that
takes every taxon's descendant set by an explicit closure, over random forests of at most 60 taxa, a path and two
roots; the four identities of include/niqki_hip.h hold on every case."""
import numpy as np
import pytest

from tally_ref import NONE, concat_rows, tally


def brute(rows, parent):
    taxon, best, considered = rows
    n = len(parent)
    sub = [{t} for t in range(n)]                              # sub[t]: t and all its descendants
    changed = True
    while changed:
        changed = False
        for u in range(n):
            p = int(parent[u])
            if p != u and not sub[u] <= sub[p]:
                sub[p] |= sub[u]
                changed = True
    direct, direct_best = [0] * n, [0] * n
    totals = {"queries": 0, "classified": 0, "no_hit": 0, "no_common": 0}
    for i, t in enumerate(taxon):
        t = int(t)
        totals["queries"] += 1
        if t == NONE:
            totals["no_common" if considered is not None and int(considered[i]) >= 1 else "no_hit"] += 1
        else:
            assert t < n
            totals["classified"] += 1
            direct[t] += 1
            direct_best[t] += 0 if best is None else int(best[i])
    clade = [sum(direct[u] for u in sub[t]) for t in range(n)]
    clade_best = [sum(direct_best[u] for u in sub[t]) for t in range(n)]
    return direct, clade, direct_best, clade_best, totals


def forests():
    rng = np.random.default_rng(21)
    yield "path", np.array([0] + list(range(39)), np.int64)                      # one path of 40 taxa
    yield "two roots", np.array([0, 1, 0, 1, 2, 3, 4, 4], np.int64)
    yield "one taxon", np.array([0], np.int64)
    for k in range(12):
        n = int(rng.integers(2, 61))
        roots = int(rng.integers(1, min(n, 4) + 1))
        parent = np.array([t if t < roots else rng.integers(0, t) for t in range(n)], np.int64)
        perm = rng.permutation(n)                                                # parents need not precede children
        inv = np.argsort(perm)
        yield "random %d" % k, perm[parent[inv]]


def rows_for(n, rng, m):
    taxon = rng.integers(0, n, m).astype(np.uint32)
    taxon[rng.random(m) < 0.2] = NONE
    best = rng.integers(0, 1 << 16, m).astype(np.uint32)
    considered = np.where(taxon == NONE, rng.integers(0, 3, m), rng.integers(1, 9, m)).astype(np.uint32)
    return taxon, best, considered


def identities(parent, direct, clade, totals):
    n = len(parent)
    assert totals["queries"] == totals["classified"] + totals["no_hit"] + totals["no_common"]
    assert int(direct.sum()) == totals["classified"]
    assert sum(int(clade[t]) for t in range(n) if parent[t] == t) == totals["classified"]
    assert (clade >= direct).all()


@pytest.mark.parametrize("name,parent", list(forests()), ids=[n for n, _ in forests()])
def test_tally_equals_the_brute_force(name, parent):
    rng = np.random.default_rng(len(parent))
    for m in (0, 1, 7, 400):
        rows = rows_for(len(parent), rng, m)
        got = tally(rows, parent)
        exp = brute(rows, parent)
        for k in range(4):
            assert got[k].dtype == np.uint64 and got[k].tolist() == exp[k], (name, m, k)
        assert got[4] == exp[4]
        identities(parent, got[0], got[1], got[4])


def test_left_out_arrays_and_bad_rows():
    parent = np.array([0, 0, 1, 3], np.int64)
    taxon = np.array([2, NONE, 2, 3, NONE], np.uint32)
    considered = np.array([1, 0, 4, 1, 2], np.uint32)
    direct, clade, direct_best, clade_best, totals = tally((taxon, None, considered), parent)
    assert direct.tolist() == [0, 0, 2, 1] and clade.tolist() == [2, 2, 2, 1]       # taxa 0 and 1 are ancestors only
    assert direct_best.tolist() == [0] * 4 and clade_best.tolist() == [0] * 4
    assert totals == {"queries": 5, "classified": 3, "no_hit": 1, "no_common": 1}
    assert tally((taxon, None, None), parent)[4] == {"queries": 5, "classified": 3, "no_hit": 2, "no_common": 0}
    for bad in (4, 0xFFFFFFFE):
        with pytest.raises(ValueError):
            tally((np.array([1, bad], np.uint32), None, None), parent)
    # sums beyond 32 bits stay exact
    big = tally((np.zeros(70000, np.uint32), np.full(70000, 65536, np.uint32), None), parent)
    assert int(big[2][0]) == 70000 * 65536 > 1 << 32 and int(big[3][0]) == 70000 * 65536


def test_concat_rows_takes_taxon_best_and_considered():
    a = (np.array([1], np.uint32), np.array([5], np.uint32), np.array([9], np.uint32), np.array([2], np.uint32))
    b = (np.array([NONE], np.uint32), np.array([0], np.uint32), np.array([0xFFFFFFFF], np.uint32), np.array([0], np.uint32))
    t, bc, co = concat_rows([a, b])
    assert t.tolist() == [1, NONE] and bc.tolist() == [5, 0] and co.tolist() == [2, 0]
