"""niqki_audit in plain Python and numpy (include/niqki_hip.h has the definition), twice over and by two routes:

audit_lists   walks ordered hit lists, as Engine.neighbors_range returns them at top_k = 0: H(g) is given, H'(g) is
              H(g) without g's own entry, and everything is read off H'(g) front to back.
audit_matrix  never builds a list: per genome it selects maxima over a count matrix under the order "larger count,
              then larger gid", and takes the k best by one sort of a combined key.

Both return the seven arrays of the call: (verdict, own_count, own_gid, other_count, other_gid, vote_gid, vote_n)."""
import numpy as np

NONE = 0xFFFFFFFF
ALONE, AGREES, TIED, MISPLACED, STRAY = 0, 1, 2, 3, 4
NAMES = ("alone", "agrees", "tied", "misplaced", "stray")


def verdict(own, other):
    if own == 0 and other == 0:
        return ALONE
    if own > other:
        return AGREES
    if own == other:
        return TIED
    return MISPLACED if own > 0 else STRAY


def _rows(n):
    return tuple(np.zeros(n, np.uint32) for _ in range(7))


def audit_lists(off, counts, gids, labels, k, begin=0):
    """off (n + 1), counts, gids: the ordered lists of genomes begin .. begin + n; labels: one per indexed genome."""
    off = np.asarray(off, np.int64)
    labels = np.asarray(labels)
    n = off.size - 1
    out = _rows(n)
    for q in range(n):
        g = begin + q
        hc, hg = counts[off[q]:off[q + 1]], gids[off[q]:off[q + 1]]
        keep = hg != g                                   # H'(g), in H(g)'s order
        hc, hg = hc[keep], hg[keep]
        same = labels[hg] == labels[g]
        oc, og, fc, fg = 0, NONE, 0, NONE
        if same.any():
            at = int(np.argmax(same))                    # the first one
            oc, og = int(hc[at]), int(hg[at])
        if not same.all():
            at = int(np.argmin(same))
            fc, fg = int(hc[at]), int(hg[at])
        seen, first = {}, {}
        for h in hg[:k].tolist():                        # V, front to back
            lab = labels[h]
            seen[lab] = seen.get(lab, 0) + 1
            first.setdefault(lab, (len(first), h))
        vg, vn = NONE, 0
        if seen:
            win = min(seen, key=lambda lab: (-seen[lab], first[lab][0]))
            vg, vn = first[win][1], seen[win]
        for a, v in zip(out, (verdict(oc, fc), oc, og, fc, fg, vg, vn)):
            a[q] = v
    return out


def audit_matrix(M, labels, t, k):
    """M: the symmetric count matrix of the index (M[g, g] = g's own valid cells); t: the threshold; labels as above."""
    M = np.asarray(M, np.int64)
    labels = np.asarray(labels)
    N = M.shape[0]
    t = max(int(t), 1)
    out = _rows(N)
    ids = np.arange(N, dtype=np.int64)
    for g in range(N):
        key = M[g] * N + ids                       # larger count first, then the larger gid
        ok = (M[g] >= t) & (ids != g)
        same = ok & (labels == labels[g])
        diff = ok & (labels != labels[g])
        oc, og, fc, fg = 0, NONE, 0, NONE
        if same.any():
            og = int(np.argmax(np.where(same, key, -1)))
            oc = int(M[g, og])
        if diff.any():
            fg = int(np.argmax(np.where(diff, key, -1)))
            fc = int(M[g, fg])
        vg, vn = NONE, 0
        cand = ids[ok]
        if cand.size:
            top = cand[np.argsort(-key[cand], kind="stable")][:k]
            tl = labels[top]
            best = None
            for pos in range(top.size):            # a label is judged at its first entry
                if np.any(tl[:pos] == tl[pos]):
                    continue
                n_lab = int(np.sum(tl == tl[pos]))
                if best is None or n_lab > best[0]:
                    best = (n_lab, int(top[pos]))
            vn, vg = best
        if oc == 0 and fc == 0:
            v = ALONE
        elif oc > fc:
            v = AGREES
        elif oc == fc:
            v = TIED
        elif oc > 0:
            v = MISPLACED
        else:
            v = STRAY
        for a, x in zip(out, (v, oc, og, fc, fg, vg, vn)):
            a[g] = x
    return out
