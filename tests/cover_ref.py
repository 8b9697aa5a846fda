"""The greedy cover of a query (include/niqki_hip.h, niqki_cover) in numpy, for the tests: once straight from the
definition over an (N, F) array of stored sketches, once round by round through the oracle's query on the masked
sketch.  Neither touches the code under test."""
import numpy as np


def valid_cells(q, W):
    q = np.asarray(q)
    return (q >= 0) & (q < (1 << W))


def cover_of(sk, q, W, thr, max_picks=0):
    """[(count, gid, total), ...] in pick order.  The last index among equal maxima wins."""
    sk = np.asarray(sk)
    q = np.asarray(q)
    if sk.shape[0] == 0:
        return []
    valid = valid_cells(q, W)
    match = sk == q[None, :]                          # (whole rows: a column gather costs ten times the compare)
    match &= valid[None, :]
    total = np.count_nonzero(match, axis=1).astype(np.int64)
    floor = max(int(thr), 1)
    # c_r(g) <= total(g): a genome below the floor is never picked, and dropping it moves no tie among the others
    gids = np.nonzero(total >= floor)[0]
    match, total = match[gids], total[gids]
    c = total.copy()                                  # c_r(g): matches among the slots still to explain
    left = valid.copy()                               # R_(r-1)
    picks = []
    while gids.size and (not max_picks or len(picks) < max_picks):
        g = c.size - 1 - int(np.argmax(c[::-1]))
        if c[g] < floor:
            break
        picks.append((int(c[g]), int(gids[g]), int(total[g])))
        gone = np.nonzero(match[g] & left)[0]
        left[gone] = False
        c -= np.count_nonzero(match[:, gone], axis=1)
    return picks


def cover_by_oracle(po_index, sk, q, thr, max_picks=0):
    """The same through pyoracle.Index.query on the masked sketch: the first hit of its reference-ordered list (count
    descending, the larger gid first) is the pick."""
    sk = np.asarray(sk)
    q = np.ascontiguousarray(q, dtype=np.int32)
    valid = valid_cells(q, po_index.p.W)
    m = q.copy()
    picks = []
    while not max_picks or len(picks) < max_picks:
        hc, hg = po_index.query(m, min_score=max(int(thr), 1))
        if len(hc) == 0:
            break
        g = int(hg[0])
        hit = (sk[g] == q) & valid
        picks.append((int(hc[0]), g, int(hit.sum())))
        m[hit] = -1
    return picks


def cover_arrays(lists):
    """per-query pick lists -> (off uint64, counts, gids, totals uint32), the shape niqki_cover writes"""
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = [p for x in lists for p in x]
    cols = [np.array([p[k] for p in flat], dtype=np.uint32) for k in range(3)]
    return off, cols[0], cols[1], cols[2]


def slot_minimum(rows):
    """per-slot minimum of sketches as a sample of several genomes has it: the smallest fingerprint of a slot, an empty
    cell (-1) only where every row is empty"""
    return np.minimum.reduce(np.ascontiguousarray(rows, dtype=np.int32).view(np.uint32)).view(np.int32)


def query_kinds(sk, W, seed=5):
    """The eight kinds of query the cover tests mix, over the data of test_gpu_cluster.data(3000, 11): name -> sketch."""
    rng = np.random.default_rng(seed)
    F = sk.shape[1]
    holes = sk[300].copy()
    holes[0::2] = 1 << W
    holes[1::4] = -2
    return {
        "duplicates": sk[7].copy(),
        "empty": sk[11].copy(),
        "two": slot_minimum(sk[[100, 2500]]),
        "five": slot_minimum(sk[[20, 500, 900, 1500, 2200]]),
        "random": rng.integers(0, 1 << W, F).astype(np.int32),
        "holes": holes,
        "sixteen": slot_minimum(sk[np.arange(40, 40 + 16 * 180, 180)]),
        "stored": sk[1234].copy(),
    }
