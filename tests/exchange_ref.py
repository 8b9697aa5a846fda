"""The slot-shard exchange (niqki_group_*, niqki_amd/csrc/nq_group.hip) from its definition, in plain numpy, and designed
sketches whose per-rank partial counts are a chosen matrix.

Rank r of `world` owns the slots [F*r//world, F*(r+1)//world) of every genome.  The partial count of genome g for query i
on rank r is the number of its slots s with 0 <= q[i][s] < 2^W and sk[g][s] == q[i][s]; the hit count is the sum over
the ranks.  With thr = ceil(min_score / world) and sthr = max(1, thr // 2) a rank's CANDIDATES of a query are the genomes
with partial >= thr, its SURVIVORS those with partial >= sthr; the hits of a query are the genomes whose sum reaches
min_score, ordered by descending (count, gid).

Nothing here calls the library under test, and nothing is taken from tests/torch_exchange.py (the older protocol with
counter rows).  `designed` checks its own construction: the partials of the arrays it returns equal the matrix it was
asked for, or it raises."""
import numpy as np

from hit_designs import reference_lists

T_DESIGN = 5          # the candidate threshold of the two designed min_scores of a world


def cuts(F, world):
    """first slot of rank 0 .. world (the last entry is F)"""
    return np.array([F * r // world for r in range(world + 1)], dtype=np.int64)


def thresholds(min_score, world):
    """(thr, sthr) from the definition"""
    thr = -(-int(min_score) // int(world))
    return thr, max(1, thr // 2)


def designed_min_scores(world, t=T_DESIGN):
    """the two thresholds of a world: thr = t with world*(t-1) = min_score - 1, and min_score = world*t"""
    return world * (t - 1) + 1, world * t


def range_counts(sk, q, W, bounds):
    """[len(bounds) - 1][nq][N] int64: matches of query i and genome g over the slots [bounds[k], bounds[k+1])"""
    sk, q = np.asarray(sk), np.asarray(q)
    bounds = np.asarray(bounds, dtype=np.int64)
    nq, N = q.shape[0], sk.shape[0]
    out = np.zeros((bounds.size - 1, nq, N), dtype=np.int64)
    for i in range(nq):
        valid = (q[i] >= 0) & (q[i] < (1 << W))
        eq = (sk == q[i][None, :]) & valid[None, :]
        cs = np.zeros((N, eq.shape[1] + 1), dtype=np.int64)
        np.cumsum(eq, axis=1, out=cs[:, 1:])
        out[:, i, :] = (cs[:, bounds[1:]] - cs[:, bounds[:-1]]).T
    return out


def partials(sk, q, W, world):
    """[world][nq][N]: entry (r, i, g) = slots s of rank r's range with 0 <= q[i][s] < 2^W and sk[g][s] == q[i][s]"""
    return range_counts(sk, q, W, cuts(np.asarray(sk).shape[1], world))


def pad_queries(q, world):
    """(rows [world * per, F] with empty sketches behind the queries, per): the batch as the ranks hold it"""
    q = np.asarray(q)
    per = -(-q.shape[0] // world)
    pad = np.full((world * per, q.shape[1]), -1, np.int32)
    pad[:q.shape[0]] = q
    return pad, per


class Exchange:
    """What every rank must see and answer for one batch.  q: the batch as the ranks hold it, padding rows included."""

    def __init__(self, sk, q, W, world, min_score):
        self.world, self.min_score = int(world), int(min_score)
        self.thr, self.sthr = thresholds(min_score, world)
        self.p = partials(sk, q, W, world)                     # [world][nq][N]
        self.total = self.p.sum(axis=0)                        # [nq][N]
        self.n_cand = (self.p >= self.thr).sum(axis=2)         # [world][nq]
        self.n_surv = (self.p >= self.sthr).sum(axis=2)

    def candidates(self, r, i):
        return np.flatnonzero(self.p[r, i] >= self.thr)

    def survivors(self, r, i):
        return np.flatnonzero(self.p[r, i] >= self.sthr)

    def expected_overflow(self, cand_cap, surv_cap):
        """some list of some row of the batch (padding rows included) holds more than its cap"""
        return bool((self.n_cand > cand_cap).any() or (self.n_surv > surv_cap).any())

    def lists(self):
        """(off, counts, gids) of all rows: total >= min_score, descending (count, gid)"""
        return reference_lists(self.total, self.min_score)

    def query_list(self, i):
        off, c, g = self.lists()
        return c[off[i]:off[i + 1]], g[off[i]:off[i + 1]]


# ---- designed sketches ------------------------------------------------------------------------------------------------

def query_values(j, F, W):
    """query j holds (s + 37 j) mod (2^W - 1) at slot s: never the filler 2^W - 1, and equal to another query's value at
    no slot while their numbers differ by less than 2^W - 1 (gcd(37, 2^W - 1) = 1 for W = 8)"""
    return ((np.arange(F, dtype=np.int64) + 37 * j) % ((1 << W) - 1)).astype(np.int32)


def fill(G, fixed, first, base, target, caps, order=None):
    """A vector of G partial counts with sum `target`: `fixed` ranks as given, rank `first` (may be None) at its given
    start, every other rank at min(base, cap); then free ranks are raised (in `order`, up to their caps) or lowered
    (from the end of `order`) until the sum is right."""
    v = np.minimum(np.full(G, base, dtype=np.int64), caps)
    free = [r for r in range(G) if r not in fixed]
    for r, x in fixed.items():
        v[r] = x
    if first is not None:
        v[first[0]] = first[1]
    order = [r for r in (order if order is not None else free) if r in free]
    assert (v <= caps).all() and (v >= 0).all(), (v, caps)
    d = int(target) - int(v.sum())
    for r in order:
        if d <= 0:
            break
        step = min(d, int(caps[r] - v[r]))
        v[r] += step
        d -= step
    for r in reversed(order):
        if d >= 0:
            break
        if first is not None and r == first[0]:
            continue
        step = min(-d, int(v[r]))
        v[r] -= step
        d += step
    assert d == 0, "no split of %d over these ranks" % target
    return v


def row_vectors(G, min_score, caps, rot):
    """The designed rows of one query as (class, tag, partial vector).  Roles (the candidate rank A, the weak rank B, the
    empty rank C) are dealt to ranks (rot, rot + 1, rot + 2) mod G, so that queries differ in where they fall; rows h
    and i are tied to the slot ranges themselves."""
    thr, sthr = thresholds(min_score, G)
    A, B, C_ = rot % G, (rot + 1) % G, (rot + 2) % G
    lo = max(thr - 1, 0)
    ring = [(A + k) % G for k in range(G)]
    rows = []
    v = np.full(G, lo, dtype=np.int64)
    v[A] = thr
    rows.append(("a", "one rank at thr, the others at thr - 1", v))
    rows.append(("b", "every rank at thr - 1", np.full(G, lo, dtype=np.int64)))
    rows.append(("c", "a candidate rank, sum min_score - 1", fill(G, {A: thr}, None, lo, min_score - 1, caps, ring)))
    for tag, (a_, b_, c_) in (("d", (A, B, C_)), ("d2", (B, C_ if G >= 3 else A, A))):
        fixed = {b_: min(1, caps[b_])}
        if G >= 3:
            fixed[c_] = 0
        rows.append(("d", tag + ": sum min_score, a rank below sthr decides", fill(G, fixed, (a_, thr), lo, min_score, caps,
                                                                               [(a_ + k) % G for k in range(G)])))
    rows.append(("e", "e1: a non-candidate rank at sthr", fill(G, {B: sthr}, (A, thr), lo, min_score, caps, ring)))
    rows.append(("e", "e2: a non-candidate rank at sthr - 1", fill(G, {B: sthr - 1}, (A, thr), lo, min_score, caps, ring)))
    if G >= 3:
        rows.append(("e", "e3: ranks at sthr and sthr - 1", fill(G, {B: sthr, C_: sthr - 1}, (A, thr), lo, min_score, caps, ring)))
    rows.append(("f", "every rank at thr", np.full(G, thr, dtype=np.int64)))
    tie = min(min_score + 3, int(caps.sum()))
    back = [(A - k) % G for k in range(G)]
    mid = [(A + G // 2 + k) % G for k in range(G)]
    rows.append(("g", "g1: tie, the surplus on the first ranks", fill(G, {}, None, lo, tie, caps, ring)))
    rows.append(("g", "g2: tie, the surplus on the last ranks", fill(G, {}, None, lo, tie, caps, back[1:] + back[:1])))
    rows.append(("g", "g3: tie, all of it on few ranks", fill(G, {}, None, 0, tie, caps, mid)))
    v = np.zeros(G, dtype=np.int64)
    v[G - 1] = caps[G - 1]
    rows.append(("h", "all slots of the last rank, nothing else", v))
    if caps[G - 1] < min_score:      # (wide worlds: the last rank alone cannot reach min_score -- topped up to exactly it)
        rows.append(("h", "h2: all slots of the last rank, sum min_score",
                     fill(G, {G - 1: caps[G - 1]}, None, lo, min_score, caps, list(range(G - 1)))))
    rows.append(("i", "equal to the query in every slot", caps.copy()))
    return rows


N_QUERIES = 11                  # a multiple of none of the worlds 2, 3, 5, 8, 16, 17, 64
EMPTY_QUERY, NO_HIT_QUERY = 7, 8
BAD_CELL_QUERIES = (3, 5)       # queries with cells that are never queried: -1 and values >= 2^W


def _bad_cells(F):
    return np.array([3, 100, F // 2 + 1, F - 1]), np.array([7, 200, 300, F - 7])


class Design:
    """sk [N, F], q [nq, F], want [world][nq][N] (the partial counts asked for), rows: (query, class, tag, gid)"""

    def __init__(self, sk, q, want, rows, world, min_score, W):
        self.sk, self.q, self.want, self.rows = sk, q, want, rows
        self.world, self.min_score, self.W = world, min_score, W

    def gids(self, query, cls):
        return [g for (j, c, _, g) in self.rows if j == query and c == cls]


def _build(world, W, q, per_query, n_genomes, rng, border=None, border_query=0):
    """q: the query sketches; per_query: {query number: [(class, tag, vector)]}; the rest of n_genomes are genomes that
    match nothing.  Genome ids are a random permutation, except that with `border` the rows of `border_query` lie
    on consecutive ids around it."""
    nq, F = q.shape
    filler = (1 << W) - 1
    cut = cuts(F, world)
    n_rows = sum(len(v) for v in per_query.values())
    assert n_rows <= n_genomes
    ids = rng.permutation(n_genomes)
    if border is not None:
        k = len(per_query[border_query])
        block = np.arange(border - k // 2, border - k // 2 + k)
        assert block[0] >= 0 and block[-1] < n_genomes
        rest = np.setdiff1d(np.arange(n_genomes), block)
        ids = np.concatenate([block, rng.permutation(rest)])
        order = [border_query] + [j for j in sorted(per_query) if j != border_query]
    else:
        order = sorted(per_query)
    sk = np.full((n_genomes, F), filler, dtype=np.int32)
    sk[rng.random((n_genomes, F)) < 0.03] = -1                    # cells without a fingerprint, among the fillers
    want = np.zeros((world, nq, n_genomes), dtype=np.int64)
    rows, k = [], 0
    for j in order:
        ok = (q[j] >= 0) & (q[j] < (1 << W))
        for cls, tag, v in per_query[j]:
            g = int(ids[k])
            k += 1
            for r in range(world):
                slots = np.flatnonzero(ok[cut[r]:cut[r + 1]]) + cut[r]
                pick = rng.choice(slots, size=int(v[r]), replace=False)
                sk[g, pick] = q[j, pick]
            want[:, j, g] = v
            rows.append((j, cls, tag, g))
    return sk, want, rows


def _spoil(q, W, which):
    """cells that are never queried: -1 and values >= 2^W"""
    F = q.shape[1]
    neg, big = _bad_cells(F)
    for j in which:
        q[j, neg] = -1
        q[j, big] = [1 << W, (1 << W) + 44, 70000, 1 << W]


def _valid_widths(q_row, W, cut):
    ok = ((q_row >= 0) & (q_row < (1 << W))).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(ok)])
    return cs[cut[1:]] - cs[cut[:-1]]


def designed(world, S, W, t, min_score=None, n_genomes=300, seed=0, border=None):
    """The rows a-j for one world and min_score (default world*(t-1) + 1; t must be its candidate threshold):
    N_QUERIES queries -- nine with the full set of rows, each with the roles on other ranks, the empty query and one
    whose genomes all stay below min_score -- over n_genomes genomes.  -> Design"""
    if min_score is None:
        min_score = world * (t - 1) + 1
    assert thresholds(min_score, world)[0] == t, "t is ceil(min_score / world)"
    F = 1 << S
    assert F // world >= t, "the narrowest shard must hold a candidate"
    rng = np.random.default_rng(1000 * world + min_score + seed)
    cut = cuts(F, world)
    qv = np.stack([query_values(j, F, W) for j in range(N_QUERIES)])
    _spoil(qv, W, BAD_CELL_QUERIES)
    per_query = {}
    for j in range(N_QUERIES):
        if j == EMPTY_QUERY:
            per_query[j] = []
            continue
        caps = _valid_widths(qv[j], W, cut)
        rows = row_vectors(world, min_score, caps, rot=j)
        if j == NO_HIT_QUERY:
            rows = [r for r in rows if r[0] in ("b", "c")]
        per_query[j] = rows
    qv[EMPTY_QUERY] = -1
    sk, want, rows = _build(world, W, qv, per_query, n_genomes, rng, border=border)
    d = Design(sk, qv, want, rows, world, min_score, W)
    check(d)
    return d


CAND_CAP, SURV_CAP = 8, 16
CAP_QUERIES = ("at cap", "cand + 1", "surv + 1")


def designed_capacity(world, S, W, min_score, n_genomes=200, seed=0):
    """Three queries for cand_cap 8 and surv_cap 16 over one index (world >= 3):
      0 "at cap"    exactly 8 candidates on rank 0 and exactly 16 survivors on rank 1
      1 "cand + 1"  9 candidates on the last rank
      2 "surv + 1"  17 survivors on rank 1, 4 candidates on rank 0
    The candidates' sums are exactly min_score, so each query has hits.  -> Design"""
    assert world >= 3
    F = 1 << S
    thr, sthr = thresholds(min_score, world)
    assert sthr < thr
    cut = cuts(F, world)
    caps = np.diff(cut)
    rng = np.random.default_rng(7000 + 10 * world + seed)

    def vec(**at):
        v = np.zeros(world, dtype=np.int64)
        for r, x in at.items():
            v[int(r[1:])] = x
        assert (v <= caps).all()
        return v
    last = "r%d" % (world - 1)
    per_query = {
        0: [("cap", "candidate on rank 0, survivor on rank 1", vec(r0=min_score - sthr, r1=sthr)) for _ in range(8)] +
           [("cap", "survivor on rank 1 only", vec(r1=sthr)) for _ in range(8)],
        1: [("cap", "candidate on the last rank", vec(**{last: min_score - 1, "r0": 1})) for _ in range(9)],
        2: [("cap", "candidate on rank 0, survivor on rank 1", vec(r0=min_score - sthr, r1=sthr)) for _ in range(4)] +
           [("cap", "survivor on rank 1 only", vec(r1=sthr + 1)) for _ in range(13)],
    }
    q = np.stack([query_values(j, F, W) for j in range(len(per_query))])
    sk, want, rows = _build(world, W, q, per_query, n_genomes, rng)
    d = Design(sk, q, want, rows, world, min_score, W)
    check(d)
    return d


def check(d):
    """the arrays alone give the matrix that was asked for"""
    got = partials(d.sk, d.q, d.W, d.world)
    if not np.array_equal(got, d.want):
        r, i, g = (int(x[0]) for x in np.nonzero(got != d.want))
        raise AssertionError("design: rank %d, query %d, genome %d holds %d, wanted %d" % (r, i, g, got[r, i, g], d.want[r, i, g]))


# ---- the group configurations the GPU module runs (tests/test_exchange_ref_cpu.py pins the plan function on each) -----

def group_cases(t=T_DESIGN):
    """(world, min_score, exchange option, cand_cap) of every designed group run"""
    out = []
    for world in (2, 3, 5, 8, 16, 17):
        out += [(world, ms, 1, 256) for ms in designed_min_scores(world, t)]
    out += [(64, designed_min_scores(64, t)[0], 1, 64)]
    for world in (3, 8):
        out += [(world, ms, 2, 256) for ms in designed_min_scores(world, t)]
        out += [(world, 4 * world - 1, 0, 256), (world, 4 * world, 0, 256)]
        out += [(world, designed_min_scores(world, t)[0], 1, CAND_CAP)]
    out += [(8, 7, 1, 256)]
    return out
