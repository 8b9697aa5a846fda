"""The LCA row of include/niqki_hip.h (niqki_query_lca) in numpy: from a query's full ordered hit list the best hit, the
length of the considered prefix (count * 1000 >= best * (1000 - top_permille)) and the deepest taxon that is an
ancestor-or-self of every considered genome's taxon.  The full lists are hit_designs.reference_lists (pinned on the
oracle by tests/test_hit_designs_cpu.py) or any (off, counts, gids) of that order.  Nothing here calls the library
under test; tests/test_lca_ref_cpu.py pins this module on a brute force over ancestor sets."""
import numpy as np

NONE = 0xFFFFFFFF


def depths(parent):
    """depth of every taxon, a root (parent[t] == t) at 0; raises ValueError on a cycle or a parent out of range"""
    parent = np.asarray(parent).astype(np.int64)
    n = parent.size
    if n and (parent.min() < 0 or parent.max() >= n):
        raise ValueError("a parent outside the taxonomy")
    d = np.full(n, -1, np.int64)
    for t0 in range(n):
        trail, t = [], t0
        while d[t] < 0 and parent[t] != t:
            if len(trail) > n:
                raise ValueError("taxon %d lies on a cycle" % t)
            trail.append(t)
            t = int(parent[t])
        if d[t] < 0:
            d[t] = 0
        base = int(d[t])
        for j, u in enumerate(reversed(trail)):
            d[u] = base + 1 + j
    return d


def pair(a, b, parent, depth):
    """the deepest common ancestor-or-self of taxa a and b, NONE where they lie in two trees"""
    while depth[a] > depth[b]:
        a = int(parent[a])
    while depth[b] > depth[a]:
        b = int(parent[b])
    while a != b:
        if parent[a] == a and parent[b] == b:
            return NONE
        a, b = int(parent[a]), int(parent[b])
    return a


def lca_lists(full, genome_taxon, parent, top_permille):
    """full: (off, counts, gids) of full ordered lists (top_k = 0).
    -> (taxon, best_count, best_gid, considered), uint32[nq] each, what niqki_query_lca writes."""
    off, c, g = (np.asarray(x).astype(np.int64) for x in full)
    genome_taxon = np.asarray(genome_taxon).astype(np.int64)
    parent = np.asarray(parent).astype(np.int64)
    depth = depths(parent)
    p = int(top_permille)
    assert 0 <= p <= 1000
    nq = off.size - 1
    taxon = np.full(nq, NONE, np.uint32)
    best_count = np.zeros(nq, np.uint32)
    best_gid = np.full(nq, 0xFFFFFFFF, np.uint32)
    considered = np.zeros(nq, np.uint32)
    for i in range(nq):
        lo, hi = int(off[i]), int(off[i + 1])
        if hi == lo:
            continue
        best = int(c[lo])
        m = 0
        while lo + m < hi and int(c[lo + m]) * 1000 >= best * (1000 - p):
            m += 1
        acc = int(genome_taxon[g[lo]])
        for j in range(lo + 1, lo + m):
            acc = pair(acc, int(genome_taxon[g[j]]), parent, depth)
            if acc == NONE:
                break
        taxon[i], best_count[i], best_gid[i], considered[i] = acc, best, int(g[lo]), m
    return taxon, best_count, best_gid, considered
