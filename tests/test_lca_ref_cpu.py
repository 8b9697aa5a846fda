"""CPU: tests/lca_ref.py against a brute force that shares no code with it -- per query the ancestor sets of the
considered genomes' taxa are intersected and the element that is nobody's proper ancestor inside the intersection (the
deepest one) is the answer -- on random forests and random count rows through hit_designs.reference_lists."""
import numpy as np
import pytest

import hit_designs as hd
from lca_ref import NONE, depths, lca_lists


def random_forest(n_taxa, n_roots, rng, chain=False):
    """parent[] of a forest whose ids are in no particular order"""
    parent = np.zeros(n_taxa, np.int64)
    for t in range(n_taxa):
        parent[t] = t if t < n_roots else (t - 1 if chain and t > n_roots else rng.integers(0, t))
    perm = rng.permutation(n_taxa)                 # old id -> new id
    out = np.empty(n_taxa, np.int64)
    out[perm] = perm[parent]
    return out


def ancestors(t, parent):
    seen = [int(t)]
    while parent[seen[-1]] != seen[-1]:
        seen.append(int(parent[seen[-1]]))
        assert len(seen) <= parent.size
    return seen


def brute(rows, min_score, genome_taxon, parent, p):
    nq, n = rows.shape
    out = []
    for i in range(nq):
        hits = [(int(rows[i, g]), g) for g in range(n) if rows[i, g] >= min_score]
        if not hits:
            out.append((NONE, 0, 0xFFFFFFFF, 0))
            continue
        best, best_g = max(hits)
        cons = [g for c, g in hits if c * 1000 >= best * (1000 - p)]
        common = set(ancestors(genome_taxon[cons[0]], parent))
        for g in cons[1:]:
            common &= set(ancestors(genome_taxon[g], parent))
        if not common:
            out.append((NONE, best, best_g, len(cons)))
            continue
        deepest = [t for t in common if len(ancestors(t, parent)) == max(len(ancestors(u, parent)) for u in common)]
        assert len(deepest) == 1                   # the common ancestors of anything form a chain
        out.append((deepest[0], best, best_g, len(cons)))
    return tuple(np.array(x, np.uint32) for x in zip(*out))


def test_depths():
    assert depths([0, 0, 1, 3, 2]).tolist() == [0, 1, 2, 0, 3]
    assert depths([]).size == 0
    assert depths(np.arange(5)).tolist() == [0] * 5
    chain = np.maximum(np.arange(2000) - 1, 0)
    assert depths(chain).tolist() == list(range(2000))
    assert depths(chain[::-1].copy() * 0 + np.minimum(np.arange(2000) + 1, 1999)).tolist() == list(range(1999, -1, -1))
    for bad in ([1, 0], [0, 2, 3, 1], [1, 2, 3, 4, 0], [0, 5]):
        with pytest.raises(ValueError):
            depths(bad)


@pytest.mark.parametrize("seed", range(6))
def test_lca_lists_equal_the_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    n, nq = 60, 50
    n_taxa, n_roots = (40, 1) if seed % 3 == 0 else ((25, 3) if seed % 3 == 1 else (30, 2))
    parent = random_forest(n_taxa, n_roots, rng, chain=seed == 5)
    genome_taxon = rng.integers(0, n_taxa, n)      # interior taxa carry genomes too
    rows = rng.choice(np.array([0, 5, 18, 19, 20, 27, 30]), size=(nq, n), p=[0.5, 0.2, 0.05, 0.05, 0.08, 0.06, 0.06])
    rows[0] = 0                                    # no hit
    rows[1] = 0
    rows[1, 17] = 25                               # one hit
    rows[2] = 30                                   # all tie
    seen = set()
    for ms in (20, 1, 0):
        full = hd.reference_lists(rows, ms)
        for p in (0, 100, 134, 333, 1000):
            got = lca_lists(full, genome_taxon, parent, p)
            exp = brute(rows, ms, genome_taxon, parent, p)
            for a, b in zip(got, exp):
                assert a.dtype == np.uint32 and np.array_equal(a, b), (ms, p)
            d = depths(parent)
            seen |= {"none" if t == NONE else ("root" if d[t] == 0 else "inner") for t, c in zip(got[0], got[3]) if c >= 2}
    assert seen >= ({"none", "root", "inner"} if n_roots > 1 else {"root", "inner"})


def test_the_boundary_counts_as_considered():
    """27 * 1000 == 30 * 900: in at p = 100, out at p = 99; 26 * 1000 >= 30 * 866: in at p = 134, out at p = 133"""
    parent = np.array([0, 0, 0, 1, 1, 2, 6])
    genome_taxon = np.array([3, 4, 5, 6])
    rows = np.array([[30, 27, 26, 1]])
    exp = {0: (3, 1), 99: (3, 1), 100: (1, 2), 133: (1, 2), 134: (0, 3), 966: (0, 3), 967: (NONE, 4), 1000: (NONE, 4)}
    for ms in (1, 0):
        full = hd.reference_lists(rows, ms)
        for p, (t, c) in exp.items():
            got = lca_lists(full, genome_taxon, parent, p)
            assert (int(got[0][0]), int(got[1][0]), int(got[2][0]), int(got[3][0])) == (t, 30, 0, c), p
            assert tuple(int(x[0]) for x in brute(rows, ms, genome_taxon, parent, p)) == (t, 30, 0, c), p
    # a zero count is considered only at p = 1000 (0 >= 30 * 0)
    rows0 = np.array([[30, 0, 0, 0]])
    assert int(lca_lists(hd.reference_lists(rows0, 0), genome_taxon, parent, 999)[3][0]) == 1
    assert int(lca_lists(hd.reference_lists(rows0, 0), genome_taxon, parent, 1000)[3][0]) == 4
