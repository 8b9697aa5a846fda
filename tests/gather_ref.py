"""Plain reference of the gather kernel and the two small data sets of tests/test_gpu_gather_forms.py.

counts[q][g] = #{ s in [slot_begin, slot_end) : 0 <= Q[q][s] < 2^W and SK[g][s] == Q[q][s] }  (src/niqki_index.cpp:652-661)
in int64 numpy; the hits are hit_designs.reference_lists of these counts.  Nothing here calls the library under test;
tests/test_gather_ref_cpu.py pins this module on the oracle."""
import numpy as np

import hit_designs as hd

S, W = 11, 8            # F = 2048: a 1024-thread workgroup's waves take two iterations of 64 slots, a 128-thread one's sixteen
F = 1 << S
TILE = 320              # genomes per tile
LAST = 257              # genomes of the last tile: odd
NQ = 70                 # >= 64 (query_order = 2 orders them), no multiple of 64 (the ordered grid has padding blocks)
# bucket lengths around every alignment unit 2^a (a = 1..5), around one, two and three chunks of 64 ids -- 192 / 193 is
# where the cutting of a bucket needs a second round -- and two long ones
LENGTHS = sorted({0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 257} |
                 {(1 << a) + d for a in range(1, 6) for d in (-1, 0, 1)})


def reference_counts(sk, q, W, slot_begin=0, slot_end=None):
    """(nq, N) int64"""
    sk = np.asarray(sk)[:, slot_begin:slot_end]
    q = np.asarray(q)[:, slot_begin:slot_end]
    out = np.zeros((q.shape[0], sk.shape[0]), np.int64)
    for i in range(q.shape[0]):
        ok = (q[i] >= 0) & (q[i] < (1 << W))
        out[i] = ((sk == q[i][None, :]) & ok[None, :]).sum(axis=1, dtype=np.int64)
    return out


def reference_hits(counts, min_score):
    return hd.reference_lists(counts, min_score)


def n_genomes(n_tiles):
    return TILE * (n_tiles - 1) + LAST


def tile_ranges(n):
    """the id ranges of the tiles of an index of n genomes with tile_stripe 0"""
    return [(g0, min(g0 + TILE, n)) for g0 in range(0, n, TILE)]


def bucket_lengths(sk, W):
    """the set of bucket lengths (slot, value) over the genomes `sk` of one tile; 0 where some value is absent from a slot"""
    n, f = sk.shape
    key = np.arange(f, dtype=np.int64)[None, :] * ((1 << W) + 1) + (sk.astype(np.int64) + 1)   # -1 -> its own column
    c = np.bincount(key.ravel(), minlength=f * ((1 << W) + 1)).reshape(f, (1 << W) + 1)[:, 1:]
    return set(np.unique(c).tolist())


def designed(n_tiles, seed=5):
    """(sk, v): n_genomes(n_tiles) sketches in which, in every tile, LENGTHS[s % len(LENGTHS)] genomes (as many as the
    tile has) hold v[s] in slot s -- a window of the tile's genomes whose start rotates with s -- and the others a
    value other than v[s], or nothing"""
    rng = np.random.default_rng(seed + n_tiles)
    n = n_genomes(n_tiles)
    v = rng.integers(0, 1 << W, F).astype(np.int32)
    other = rng.integers(1, 1 << W, (n, F)).astype(np.int32)
    sk = (v[None, :] + other) % (1 << W)                      # never v[s]
    sk[rng.random((n, F)) < 0.02] = -1
    L = np.asarray([LENGTHS[s % len(LENGTHS)] for s in range(F)])
    for g0, g1 in tile_ranges(n):
        n_t = g1 - g0
        pos = (np.arange(n_t)[:, None] - (np.arange(F) * 37)[None, :]) % n_t   # place of the genome in slot s's window
        sk[g0:g1][pos < L[None, :]] = np.broadcast_to(v, (n_t, F))[pos < L[None, :]]
    return sk.astype(np.int32), v


def designed_queries(sk, v, seed=9):
    """NQ queries: v, v with a third of its cells replaced, stored sketches, an empty one, one with every second cell
    out of range, random ones.  -> (q, names)"""
    rng = np.random.default_rng(seed)
    n = sk.shape[0]
    rows, names = [v.copy()], ["v"]
    for _ in range(3):
        r = v.copy()
        m = rng.random(F) < 1 / 3
        r[m] = rng.integers(0, 1 << W, int(m.sum()))
        rows.append(r)
        names.append("v third replaced")
    for g in sorted({0, 1, TILE - 1, TILE, n // 2, n - 2, n - 1} & set(range(n))):
        rows.append(sk[g].copy())
        names.append("stored %d" % g)
    rows.append(np.full(F, -1, np.int32))
    names.append("empty")
    r = v.copy()
    r[::2] = 1 << W
    rows.append(r)
    names.append("out of range")
    while len(rows) < NQ:
        rows.append(rng.integers(0, 1 << W, F).astype(np.int32))
        names.append("random")
    return np.stack(rows).astype(np.int32), names


def families(n, S, W, seed, n_fam=8, run=50, empty=0.02):
    """families + noise + empty cells: runs of `run` genomes share a family sketch, 30 % of the cells are redrawn"""
    rng = np.random.default_rng(seed)
    f = 1 << S
    fam = rng.integers(0, 1 << W, (n_fam, f)).astype(np.int32)
    sk = fam[(np.arange(n) // run) % n_fam].copy()
    noise = rng.random((n, f)) < 0.3
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[rng.random((n, f)) < empty] = -1
    return sk, fam


def family_queries(sk, fam, W, nq=NQ, seed=3):
    """nq queries: the families, stored sketches with a tenth of the cells redrawn, an empty one, one with every
    second cell out of range, random ones"""
    rng = np.random.default_rng(seed)
    n, f = sk.shape
    q = sk[rng.integers(0, n, nq)].copy()
    m = rng.random((nq, f)) < 0.1
    q[m] = rng.integers(0, 1 << W, int(m.sum()))
    k = min(len(fam), nq - 8)
    q[:k] = fam[:k]
    q[k] = sk[0]
    q[k + 1] = sk[n - 1]
    q[k + 2] = -1
    q[k + 3, ::2] = 1 << W
    q[k + 4:k + 7] = rng.integers(0, 1 << W, (3, f))
    return q.astype(np.int32), {"empty": k + 2, "out of range": k + 3}


def decode_kernel(code):
    """stat "last_gather_kernel" -> (BLOCK, UNROLL, NT, PAD)"""
    code = int(code)
    return code & 0xFFF, (code >> 12) & 0xFF, ((code >> 20) & 0xF) - 1, (code >> 24) & 1
