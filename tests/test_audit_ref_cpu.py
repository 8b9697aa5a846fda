"""CPU: the two references of niqki_audit (audit_ref.py) agree: audit_lists over the ordered lists of a count matrix,
audit_matrix over the matrix itself.  Counts come from {0, 5, 6, 7}, the diagonal included, so ties are everywhere, a
genome's own entry is absent, first, or behind its ties, and lists are cut by every threshold."""
import numpy as np
import pytest

from audit_ref import ALONE, AGREES, MISPLACED, NONE, STRAY, TIED, audit_lists, audit_matrix, verdict


def lists_of(M, t):
    """H(g) for every g: the entries with count >= max(t, 1), count descending, then gid descending"""
    t = max(t, 1)
    off, hc, hg = [0], [], []
    for g in range(M.shape[0]):
        ids = np.nonzero(M[g] >= t)[0]
        ids = sorted(ids.tolist(), key=lambda j: (-int(M[g, j]), -j))
        hc += [int(M[g, j]) for j in ids]
        hg += ids
        off.append(len(hc))
    return np.array(off, np.uint64), np.array(hc, np.uint32), np.array(hg, np.uint32)


def random_matrix(rng, n=40, p_zero=0.25):
    """p_zero 0.25: every genome has about ten neighbours at the top count, so nearly every verdict is a tie; a sparse
    matrix gives the other verdicts their share"""
    A = rng.choice([0, 5, 6, 7], size=(n, n), p=[p_zero] + [(1 - p_zero) / 3] * 3)
    M = np.triu(A) + np.triu(A, 1).T
    return M.astype(np.uint32)


@pytest.mark.parametrize("n_labels", [1, 2, 3, 4, 5, 6])
def test_the_two_references_agree(n_labels):
    rng = np.random.default_rng(100 + n_labels)
    seen = set()
    for p_zero in (0.25, 0.25, 0.85, 0.93):
        M = random_matrix(rng, p_zero=p_zero)
        labels = rng.integers(0, n_labels, M.shape[0]).astype(np.uint32) * 7 + 3     # (any values, not dense)
        for t in (0, 1, 6, 7, 8):
            off, hc, hg = lists_of(M, t)
            for k in (1, 2, 3, 63):
                a = audit_lists(off, hc, hg, labels, k)
                b = audit_matrix(M, labels, t, k)
                for x, y in zip(a, b):
                    assert x.dtype == np.uint32 and np.array_equal(x, y), (n_labels, t, k)
                seen |= set(a[0].tolist())
                if t == 8:
                    assert np.all(a[0] == ALONE) and np.all(a[2] == NONE) and np.all(a[5] == NONE) and not a[6].any()
    assert seen == ({ALONE, AGREES} if n_labels == 1 else {ALONE, AGREES, TIED, MISPLACED, STRAY})


def test_a_slice_of_the_lists_is_a_slice_of_the_rows():
    rng = np.random.default_rng(7)
    M = random_matrix(rng)
    labels = rng.integers(0, 3, 40).astype(np.uint32)
    off, hc, hg = lists_of(M, 5)
    full = audit_lists(off, hc, hg, labels, 3)
    lo, hi = 13, 29
    part = audit_lists(off[lo:hi + 1] - off[lo], hc[int(off[lo]):int(off[hi])], hg[int(off[lo]):int(off[hi])], labels, 3, begin=lo)
    assert all(np.array_equal(p, f[lo:hi]) for p, f in zip(part, full))


def test_small_cases_by_hand():
    # genome 0: duplicate 3 (larger id) ties its own entry; label of 0 and 3 is 9, of 1 and 2 is 4
    M = np.array([[8, 6, 6, 8],
                  [6, 8, 2, 6],
                  [6, 2, 0, 6],
                  [8, 6, 6, 8]], np.uint32)
    labels = np.array([9, 4, 4, 9], np.uint32)
    v, oc, og, fc, fg, vg, vn = audit_matrix(M, labels, 1, 2)
    assert (v[0], oc[0], og[0], fc[0], fg[0]) == (AGREES, 8, 3, 6, 2)          # foreign ties go to the larger gid
    assert (vg[0], vn[0]) == (3, 1)                                            # V = {3, 2}: a tie, the first label wins
    assert (v[1], oc[1], og[1], fc[1], fg[1], vg[1], vn[1]) == (MISPLACED, 2, 2, 6, 3, 3, 2)
    assert (v[2], oc[2], og[2], fc[2], fg[2]) == (MISPLACED, 2, 1, 6, 3)       # 2's own entry is absent (0 valid cells)
    v7 = audit_matrix(M, labels, 7, 1)
    assert v7[0].tolist() == [AGREES, ALONE, ALONE, AGREES] and v7[5].tolist() == [3, NONE, NONE, 0]
    lone = audit_matrix(M, np.array([9, 4, 4, 5], np.uint32), 1, 1)
    assert lone[0][0] == STRAY and lone[0][3] == STRAY and lone[2][0] == NONE
    assert [verdict(*p) for p in ((0, 0), (3, 2), (3, 3), (2, 3), (0, 3))] == [ALONE, AGREES, TIED, MISPLACED, STRAY]
