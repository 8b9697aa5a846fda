"""The taxon tally of include/niqki_hip.h (niqki_tally_*) in numpy, and the text of `niqki --report`
(niqki_amd/host/report_file.h) restated.  tally: rows (taxon, best_count, considered) counted per taxon by bincount,
every taxon's counts walked up to its root for the clade sums, and the totals.  Nothing here calls the library under
test; tests/test_tally_ref_cpu.py pins tally on a brute force over explicit descendant sets."""
import numpy as np

NONE = 0xFFFFFFFF


def tally(rows, parent):
    """rows: (taxon, best_count, considered), best_count / considered may be None (zeros / every NONE row has no hit).
    -> (direct, clade, direct_best, clade_best, totals): four uint64[n_taxa] and a dict, what niqki_tally_read gives.
    Raises ValueError on a bad row (a taxon that is neither below n_taxa nor NONE)."""
    taxon, best, considered = rows
    taxon = np.asarray(taxon).astype(np.int64).reshape(-1)
    best = np.zeros(taxon.size, np.int64) if best is None else np.asarray(best).astype(np.int64).reshape(-1)
    considered = np.zeros(taxon.size, np.int64) if considered is None else np.asarray(considered).astype(np.int64).reshape(-1)
    parent = np.asarray(parent).astype(np.int64)
    n = parent.size
    none = taxon == NONE
    cls = taxon < n
    if not (none | cls).all():
        raise ValueError("%d bad rows" % int((~(none | cls)).sum()))
    direct = np.bincount(taxon[cls], minlength=n).astype(np.uint64)
    direct_best = np.zeros(n, np.uint64)
    np.add.at(direct_best, taxon[cls], best[cls].astype(np.uint64))
    clade, clade_best = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for t in np.flatnonzero(direct):
        u = int(t)
        for _ in range(n + 1):                                # (a taxonomy has no cycle: the walk ends at a root)
            clade[u] += direct[t]
            clade_best[u] += direct_best[t]
            if parent[u] == u:
                break
            u = int(parent[u])
    totals = {"queries": int(taxon.size), "classified": int(cls.sum()), "no_hit": int((none & (considered == 0)).sum()),
              "no_common": int((none & (considered >= 1)).sum())}
    return direct, clade, direct_best, clade_best, totals


def concat_rows(parts):
    """rows of several calls as one: [(taxon, best_count, best_gid, considered), ...] of the LCA calls -> tally's rows"""
    return tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in (0, 1, 3))


def fmt_g(v):
    return "%g" % v


def report_text(texts, parent, direct, clade, direct_best, clade_best, totals, F):
    """the bytes of the --report file: <pct>\\t<clade>\\t<direct>\\t<depth>\\t<mean>\\t<indent><text>\\n; first
    `unclassified` and `no_common_taxon`, always; then every taxon with clade > 0 in pre-order, roots and siblings by
    clade descending, then id ascending.  direct_best is not printed (clade_best of a leaf equals it)."""
    del direct_best
    parent = [int(p) for p in parent]
    n = len(parent)
    q = int(totals["queries"])

    def pct(c):
        return "%.2f" % (100.0 * int(c) / q) if q else "0.00"

    lines = []
    for name, c in (("unclassified", totals["no_hit"]), ("no_common_taxon", totals["no_common"])):
        lines.append("%s\t%d\t%d\t-\t-\t%s\n" % (pct(c), c, c, name))
    children = [[] for _ in range(n)]
    roots = []
    for t in range(n):
        if int(clade[t]) == 0:
            continue
        (roots if parent[t] == t else children[parent[t]]).append(t)

    def key(t):
        return (-int(clade[t]), t)

    stack = [(t, 0) for t in sorted(roots, key=key, reverse=True)]
    while stack:
        t, d = stack.pop()
        mean = fmt_g(int(clade_best[t]) / (int(clade[t]) * float(F)))
        lines.append("%s\t%d\t%d\t%d\t%s\t%s%s\n" % (pct(clade[t]), int(clade[t]), int(direct[t]), d, mean, "  " * d, texts[t]))
        stack.extend((c, d + 1) for c in sorted(children[t], key=key, reverse=True))
    return "".join(lines)
