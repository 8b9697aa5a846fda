"""Designed inputs for the hit kernels (nq_hits.hip, the list tail of gather_kernel) and their plain reference.

Two ways to put a chosen count on a chosen genome:

* synthetic u16 counter rows (the `row_*` recipes), fed to niqki_hits_from_counts without an index;
* `design(C, S, W, rng)`: sketches of an index and of T query types whose count matrix is exactly C.  Query type t
  holds the value t in every cell; genome g holds t in exactly C[t, g] cells of a random choice and a filler value
  (T, which no query holds) or -1 elsewhere, so count(t, g) = C[t, g].

`reference_lists` is the expectation of every test built on them: threshold, (count, gid) descending, cut to k, in
numpy on int64.  Nothing here calls the library under test; tests/test_hit_designs_cpu.py pins this module on the
oracle."""
import numpy as np

BLK = 4096          # genomes per compaction block of the counter-row kernels (kHitsBlk)
STEP = 256          # genomes per step of hits_compact_kernel inside a block
WIDE_FROM = 7 * BLK + 1   # 28 673 genomes = 8 blocks: hits_count_kernel<true> from here on


# ---- the reference ---------------------------------------------------------------------------------------------------

def reference_lists(rows, min_score, top_k=0, gid_begin=0):
    """rows: (nq, n_gids) counts.  Per row the genomes with count >= min_score, count descending, then gid descending,
    cut to top_k when 0 < top_k < n_gids; gids offset by gid_begin.  -> (off int64[nq + 1], counts int64, gids int64)"""
    rows = np.asarray(rows)
    assert rows.ndim == 2
    nq, n_gids = rows.shape
    k = int(top_k) if 0 < int(top_k) < n_gids else 0
    gid = np.arange(n_gids, dtype=np.int64)
    cs, gs, off = [], [], np.zeros(nq + 1, np.int64)
    for i in range(nq):
        c = rows[i].astype(np.int64)
        m = c >= int(min_score)
        c, g = c[m], gid[m]
        order = np.lexsort((-g, -c))       # last key first: count descending, then gid descending
        if k:
            order = order[:k]
        cs.append(c[order])
        gs.append(g[order] + int(gid_begin))
        off[i + 1] = off[i] + order.size
    z = np.zeros(0, np.int64)
    return off, np.concatenate(cs + [z]), np.concatenate(gs + [z])


def _segments(start, keep):
    """indices start[i] .. start[i] + keep[i] of every segment i, and the offsets of the lists they make"""
    new_off = np.zeros(keep.size + 1, np.int64)
    np.cumsum(keep, out=new_off[1:])
    idx = np.arange(int(new_off[-1]), dtype=np.int64) - np.repeat(new_off[:-1] - start, keep)
    return new_off, idx


def cut_lists(ref, k, n_gids):
    """The lists of reference_lists(.., top_k=0) cut to k, as reference_lists(.., top_k=k) returns them."""
    off, c, g = ref
    if not 0 < int(k) < n_gids:
        return ref
    new_off, idx = _segments(off[:-1], np.minimum(np.diff(off), int(k)))
    return new_off, c[idx], g[idx]


def deal(ref, types):
    """Lists of len(types) queries, query i being a copy of row types[i] of `ref`."""
    off, c, g = ref
    types = np.asarray(types, dtype=np.int64)
    lens = np.diff(off)[types]
    new_off, idx = _segments(off[types], lens)
    return new_off, c[idx], g[idx]


def first_difference(got, exp):
    """None when (off, counts, gids) agree entry for entry; else a short text naming the first query that differs."""
    go, gc, gg = (np.asarray(x).astype(np.int64) for x in got)
    eo, ec, eg = exp
    if go.shape != eo.shape:
        return "offsets: %d entries, expected %d" % (go.size, eo.size)
    if not np.array_equal(go, eo):
        i = int(np.flatnonzero(go != eo)[0])
        return "offset %d is %d, expected %d (query %d has %d hits)" % (i, go[i], eo[i], i - 1, eo[i] - eo[i - 1])
    tot = int(eo[-1])
    if gc.size < tot or gg.size < tot:
        return "%d / %d entries returned, expected %d" % (gc.size, gg.size, tot)
    bad = (gc[:tot] != ec) | (gg[:tot] != eg)
    if not bad.any():
        return None
    p = int(np.flatnonzero(bad)[0])
    q = int(np.searchsorted(eo, p, side="right") - 1)
    lo, hi = int(eo[q]), int(eo[q + 1])
    a, b = max(lo, p - 2), min(hi, p + 4)
    return ("query %d (%d hits), entry %d of its list: (count, gid) got %s expected %s" %
            (q, hi - lo, p - lo, list(zip(gc[a:b].tolist(), gg[a:b].tolist())), list(zip(ec[a:b].tolist(), eg[a:b].tolist()))))


# ---- an index with a prescribed count matrix -------------------------------------------------------------------------

def design(C, S, W, rng, empty_every=3):
    """(index_sketches int32[N, 2^S], query_sketches int32[T, 2^S]) with count(query t, genome g) = C[t, g].
    Every empty_every-th unused cell of a genome is -1 (no fingerprint), the others hold the filler T."""
    C = np.asarray(C, dtype=np.int64)
    assert C.ndim == 2
    T, N = C.shape
    F = 1 << S
    assert C.min() >= 0, "counts are cell numbers"
    assert T + 1 <= (1 << W), "T query values and the filler must fit W bits"
    cum = np.cumsum(C, axis=0)                              # cum[t, g]: cells of genome g that hold a value <= t
    assert cum[-1].max() <= F, "a genome has 2^S cells: sum_t C[t, g] <= 2^S"
    cell = np.arange(F, dtype=np.int64)
    val = np.zeros((N, F), dtype=np.int32)                  # by rank: C[0, g] cells of 0, C[1, g] of 1, ..., then T
    for t in range(T):
        val += cell[None, :] >= cum[t][:, None]
    if empty_every:
        unused = cell[None, :] - cum[-1][:, None]           # 0, 1, 2 .. over a genome's filler cells
        val[(unused >= 0) & (unused % empty_every == empty_every - 1)] = -1
    # the random choice of cells: rank r of genome g goes to cell order[g, r]
    order = np.argsort(rng.random((N, F), dtype=np.float32), axis=1)
    sk = np.empty((N, F), dtype=np.int32)
    np.put_along_axis(sk, order, val, axis=1)
    q = np.repeat(np.arange(T, dtype=np.int32)[:, None], F, axis=1)
    return sk, q


def hit_matrix(n_hits, N, rng, min_score=20, levels=(20, 21, 25, 30), below=(0, 19), forced=()):
    """C for design(): type t has exactly n_hits[t] genomes at or above min_score, at random ids that include 0 and N - 1
    (and `forced`) where n_hits[t] allows, with counts drawn from `levels`; every other genome holds one of `below`."""
    T = len(n_hits)
    C = rng.choice(np.asarray(below, dtype=np.int64), size=(T, N))
    assert max(below) < min_score <= min(levels)
    for t, n in enumerate(n_hits):
        must = [g for g in dict.fromkeys(list(forced) + [N - 1, 0]) if g < N][:n]
        rest = np.setdiff1d(np.arange(N), must)
        ids = np.concatenate([np.asarray(must, dtype=np.int64), rng.choice(rest, n - len(must), replace=False)])
        C[t, ids] = rng.choice(np.asarray(levels, dtype=np.int64), size=n)
        if len(must) >= 2:
            C[t, must] = levels[0]          # the forced ids tie with each other: their order is decided by the gid
    return C


# ---- counter-row recipes: u16[n] ---------------------------------------------------------------------------------------

def row_zeros(n, rng=None):
    return np.zeros(n, np.uint16)


def row_const(n, value):
    return np.full(n, value, np.uint16)


def row_ramp(n, rng=None):
    """all distinct while n <= 65 536, the largest count on genome 0"""
    return ((n - 1 - np.arange(n, dtype=np.int64)) % 65536).astype(np.uint16)


def row_levels(n, rng, levels=(0, 3, 5, 9, 40)):
    """random over a handful of levels: heavy ties"""
    return rng.choice(np.asarray(levels, dtype=np.uint16), size=n)


def row_u16(n, rng):
    return rng.integers(0, 65536, n).astype(np.uint16)


def row_bin_edges(n, rng):
    """levels 15 / 16 / 17 / 31 / 32: a top-k boundary on the lowest (16) and the highest (31) count of a bin of
    sel_boundary's first histogram (count >> 4), and on its neighbours in the bins beside it"""
    return row_levels(n, rng, (15, 16, 17, 31, 32))


def row_placed_ties(n, T, tie_pos, above_pos, rng):
    """count T at tie_pos, T + 1 at above_pos (positions >= n are dropped), T - 1 or 0 elsewhere"""
    row = rng.choice(np.asarray([T - 1, 0], dtype=np.uint16), size=n)
    tie_pos = np.asarray([p for p in tie_pos if 0 <= p < n], dtype=np.int64)
    above_pos = np.asarray([p for p in above_pos if 0 <= p < n and p not in set(tie_pos.tolist())], dtype=np.int64)
    row[tie_pos] = T
    row[above_pos] = T + 1
    return row


def edge_positions(n):
    """where placed ties go: gid 0 and n - 1, either side of every multiple of 4096, the row's last incomplete group of
    eight, and a run from position 300 of every block on (behind the block's first 256-genome step)"""
    pos = {0, n - 1}
    for b in range(0, n, BLK):
        pos.update((b - 1, b, b + 1, b + STEP - 1, b + STEP))
        pos.update(range(b + 300, b + 306))
        pos.update((b + 2047, b + 2048, b + 4000))
    pos.update(range(n & ~7, n))
    return sorted(p for p in pos if 0 <= p < n)


def tie_cuts(row, T, min_score):
    """For a row of placed ties at count T: per compaction block that holds ties, the k that puts the top-k cut inside
    that block's ties so that the kept ones start behind the block's first 256 genomes where it has ties there.
    -> list of (block, k, states) with states the set of blk_skip states the cut makes over the row's blocks:
    'all' (every tie of a block kept), 'part', 'none'."""
    c = np.asarray(row).astype(np.int64)
    n = c.size
    assert T >= min_score
    above = int((c > T).sum())
    tie = np.flatnonzero(c == T)
    blk = tie // BLK
    out = []
    for b in sorted(set(blk.tolist())):
        mine = tie[blk == b]
        late = mine[mine - b * BLK >= 300]
        kept = late.size if 0 < late.size < mine.size else (1 if mine.size > 1 else 0)
        if not kept:
            continue
        k = above + int((blk > b).sum()) + kept
        if not 0 < k < n:
            continue
        states = set()
        for bb in sorted(set(blk.tolist())):
            states.add("all" if bb > b else ("part" if bb == b else "none"))
        out.append((b, k, states))
    return out


def row_ks(row, min_score, n_gids):
    """the top-k values that matter for one row: around its hit count h, and for a boundary count L -- every level of a
    row of few levels, else the most frequent hit count -- a + 1, a + eq - 1, a + eq with a the hits above L and eq the
    ties at it"""
    c = np.asarray(row).astype(np.int64)
    hit = c[c >= min_score]
    h = hit.size
    ks = {h - 1, h, h + 1}
    if h:
        vals, cnt = np.unique(hit, return_counts=True)
        for L in (vals if vals.size <= 6 else vals[[int(np.argmax(cnt))]]):
            a, eq = int((hit > L).sum()), int((hit == L).sum())
            ks.update((a + 1, a + eq - 1, a + eq))
    return {k for k in ks if k > 0}


GENERIC_KS = (1, 2, 7, 64)


def call_ks(rows, min_score):
    """every k of the issue's list for one call: the fixed ones, around n_gids, and row_ks of every row"""
    n = rows.shape[1]
    ks = set(GENERIC_KS) | {n - 1, n, n + 1}
    for r in rows:
        ks |= row_ks(r, min_score, n)
    return sorted(k for k in ks if k > 0)
