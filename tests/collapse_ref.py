"""The collapsed list of include/niqki_hip.h (niqki_query_collapsed) in numpy: from a query's full ordered hit list the
entries that are the first of their label, in list order, each with the number of the list's entries that carry its
label, cut to top_k labels.  The full lists are hit_designs.reference_lists (pinned on the oracle by
tests/test_hit_designs_cpu.py) or any (off, counts, gids) of that order.  Nothing here calls the library under test;
tests/test_collapse_ref_cpu.py pins this module on the oracle's own hit lists."""
import numpy as np

import hit_designs as hd


def collapse_lists(full, labels, top_k=0):
    """full: (off, counts, gids) of full ordered lists (top_k = 0); labels: one value per genome.
    -> (off uint64[nq + 1], counts uint32, gids uint32, members uint32), the shape niqki_query_collapsed writes."""
    off, c, g = (np.asarray(x).astype(np.int64) for x in full)
    labels = np.asarray(labels).astype(np.int64)
    nq = off.size - 1
    out_off = np.zeros(nq + 1, np.uint64)
    cs, gs, ms = [], [], []
    for i in range(nq):
        lo, hi = int(off[i]), int(off[i + 1])
        lab = labels[g[lo:hi]]
        _, first, members = np.unique(lab, return_index=True, return_counts=True)
        order = np.argsort(first, kind="stable")             # the labels by their first position in the list
        if int(top_k) > 0:
            order = order[:int(top_k)]
        at = first[order]
        cs.append(c[lo:hi][at])
        gs.append(g[lo:hi][at])
        ms.append(members[order])
        out_off[i + 1] = out_off[i] + np.uint64(order.size)
    z = np.zeros(0, np.int64)
    return (out_off,) + tuple(np.concatenate(x + [z]).astype(np.uint32) for x in (cs, gs, ms))


def collapse_rows(rows, min_score, labels, top_k=0):
    """The same from count rows (nq, n_genomes): threshold, order, then the collapse."""
    return collapse_lists(hd.reference_lists(rows, min_score), labels, top_k)


def count_rows(sk, queries, W):
    """count(query, genome): the slots where the genome holds the query's valid cell (Index::query_sketch)"""
    sk = np.asarray(sk)
    rows = np.zeros((len(queries), sk.shape[0]), np.int64)
    for i, q in enumerate(queries):
        valid = (q >= 0) & (q < (1 << W))
        rows[i] = ((sk == q[None, :]) & valid[None, :]).sum(1)
    return rows


def few_cell_query(sk, g, W, rng, cells=60):
    """a random sketch that holds `cells` cells of genome g: one hit at a threshold between what genome g's relatives
    share of those cells and `cells`"""
    f = sk.shape[1]
    q = rng.integers(0, 1 << W, f).astype(np.int32)
    at = rng.choice(np.flatnonzero(sk[g] >= 0), cells, replace=False)
    q[at] = sk[g][at]
    return q
