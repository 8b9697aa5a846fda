"""The numpy reference of the register calls (niqki_registers, niqki_sketch_registers, niqki_staged_registers), of the
size estimator and the containment (niqki_amd/host/size_estimate.h), and an exact counter of distinct canonical k-mers
to hold the estimator against.  Written from the definitions in include/niqki_hip.h and DESIGN.md 4.6j, not from the
product's code."""
import math

import numpy as np

OK, BELOW, ABOVE = "ok", "below", "above"


def bins(H):
    return (1 << H) + 1


def hist_ref(cells, W, H):
    """uint32 [n][2^H + 1] of int32 cells [n][F]: column c >> (W - H) counts the valid cells (0 <= c < 2^W) with that
    register value, the last column the cells that are not valid."""
    c = np.asarray(cells, dtype=np.int64)
    c = c.reshape(-1, c.shape[-1]) if c.ndim > 1 else c.reshape(1, -1)
    n, B = c.shape[0], bins(H)
    valid = (c >= 0) & (c < (1 << W))
    b = np.where(valid, c >> (W - H), 1 << H)
    flat = (np.arange(n, dtype=np.int64)[:, None] * B + b).reshape(-1)
    return np.bincount(flat, minlength=n * B).reshape(n, B).astype(np.uint32)


def estimate(hist, S, H):
    """(estimate as float, status) of one histogram row: Z = hist[2^H] + sum_r hist[r] 2^-(2^H - r) in ascending r,
    E = alpha F^2 / Z; below when E < 8 F (or H < 2, S < 4), above when hist[0] > F / 8."""
    n_reg, F = 1 << H, 1 << S
    Z = float(int(hist[n_reg]))
    for r in range(n_reg):
        Z += math.ldexp(float(int(hist[r])), r - n_reg)
    if Z <= 0:
        return 0.0, BELOW
    alpha = {4: 0.673, 5: 0.697, 6: 0.709}.get(S, 0.673 if S < 4 else 0.7213 / (1.0 + 1.079 / F))
    E = alpha * F * F / Z
    if H < 2 or S < 4 or E < 8.0 * F:
        return E, BELOW
    if 8 * int(hist[0]) > F:
        return E, ABOVE
    return E, OK


def containment(count, S, q, g):
    """(J, cq, cg) from the common slots of a query and a genome and their (estimate, status); cq = cg = None unless
    both sizes are ok.  |A n B| = J (|A| + |B|) / (1 + J)."""
    J = float(count) / float(1 << S)
    if q[1] != OK or g[1] != OK:
        return J, None, None
    inter = J * (q[0] + g[0]) / (1.0 + J)
    return J, min(1.0, inter / q[0]), min(1.0, inter / g[0])


def sizes_text(names, hists, S, H):
    """the --sizes file"""
    return "".join("%s\t%.0f\t%s\n" % ((n,) + estimate(h, S, H)) for n, h in zip(names, hists))


def containment_entry(name, count, S, q, g):
    """one entry of a --containment list"""
    J, cq, cg = containment(count, S, q, g)
    return "%s:%g:%s" % (name, J, "-:-" if cq is None else "%g:%g" % (cq, cg))


_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def canonical_kmers(seq, K):
    """the canonical K-mers (the smaller of a K-mer and its reverse complement, 2 bits a base, A C G T = 0 1 2 3) of the
    windows of one record that hold only A, C, G, T; uint64, one per window, duplicates kept"""
    code = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq.astype(np.uint8)]
    n = code.size - K + 1
    if n <= 0:
        return np.empty(0, dtype=np.uint64)
    bad = np.concatenate(([0], np.cumsum(code > 3)))
    ok = (bad[K:] - bad[:-K]) == 0
    c = (code & 3).astype(np.uint64)
    fw = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(K):   # rolling over the window position, vectorised over the windows
        fw = (fw << np.uint64(2)) | c[j:j + n]
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fw, rc)[ok]


def distinct_kmers(records, K):
    """the sorted distinct canonical K-mers of a list of records"""
    parts = [canonical_kmers(r, K) for r in records]
    return np.unique(np.concatenate(parts)) if parts else np.empty(0, dtype=np.uint64)
