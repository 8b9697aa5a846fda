"""The contained list of include/niqki_hip.h (niqki_query_contained) in numpy and Python integers: the share of a hit
from its count and the two sizes, and from a query's full ordered hit list the entries that have a size and whose share
reaches a threshold, ordered by share with ties in the list's order, cut to top_k.  The full lists are any
(off, counts, gids) of H's order (count descending, then gid descending).  Nothing here calls the library under test;
tests/test_contain_ref_cpu.py pins this module on fractions.Fraction and the header the kernels compile."""
import numpy as np

QUERY, GENOME, MAX = 0, 1, 2
ONE = 0xFFFFFFFF
SIZE_LIMIT = 1 << 40


def share(c, F, q, g, mode):
    """share of a hit with count c of F slots, query size q and genome size g (both sized: > 0), as the header defines
    it: 0xFFFFFFFF where Nn >= Dd, else floor(Nn 2^32 / Dd), in Python's big integers"""
    c, F, q, g = int(c), int(F), int(q), int(g)
    assert 0 <= c <= F and 0 < q < SIZE_LIMIT and 0 < g < SIZE_LIMIT and mode in (QUERY, GENOME, MAX)
    d = q if mode == QUERY else g if mode == GENOME else min(q, g)
    nn = c * (q + g)
    dd = (F + c) * d
    return ONE if nn >= dd else (nn << 32) // dd


def min_share_of(x):
    """the threshold of a containment 0 < x <= 1: ONE for 1, else ceil(x 2^32) clamped to it (x a float or a Fraction)"""
    from fractions import Fraction
    v = Fraction(x) * (1 << 32)
    n = v.numerator // v.denominator + (1 if v.numerator % v.denominator else 0)
    return ONE if x >= 1 else min(n, ONE)


def contain_lists(full, sizes, qsizes, mode, min_share, top_k=0, *, F):
    """full: (off, counts, gids) of full ordered lists (top_k = 0); sizes: one per genome; qsizes: one per query; F: the
    slots of a sketch.
    -> (off uint64[nq + 1], shares uint32, counts uint32, gids uint32, n_unsized uint32[nq]), the shape
    niqki_query_contained writes."""
    off, c, g = (np.asarray(x).astype(np.int64) for x in full)
    sizes = [int(x) for x in np.asarray(sizes).tolist()]
    qsizes = [int(x) for x in np.asarray(qsizes).tolist()]
    nq = off.size - 1
    assert len(qsizes) == nq
    out_off = np.zeros(nq + 1, np.uint64)
    n_unsized = np.zeros(nq, np.uint32)
    ss, cs, gs = [], [], []
    for i in range(nq):
        lo, hi = int(off[i]), int(off[i + 1])
        kept = []                                              # (share, position)
        for pos in range(hi - lo):
            gs_ = sizes[int(g[lo + pos])]
            if qsizes[i] == 0 or gs_ == 0:
                n_unsized[i] += 1
                continue
            s = share(c[lo + pos], F, qsizes[i], gs_, mode)
            if s >= int(min_share):
                kept.append((s, pos))
        kept.sort(key=lambda e: -e[0])                         # (stable: ties stay in the list's order)
        if int(top_k) > 0:
            kept = kept[:int(top_k)]
        at = np.array([p for _, p in kept], np.int64)
        ss.append(np.array([s for s, _ in kept], np.int64))
        cs.append(c[lo:hi][at])
        gs.append(g[lo:hi][at])
        out_off[i + 1] = out_off[i] + np.uint64(len(kept))
    z = np.zeros(0, np.int64)
    return (out_off,) + tuple(np.concatenate(x + [z]).astype(np.uint32) for x in (ss, cs, gs)) + (n_unsized,)
