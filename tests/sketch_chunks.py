"""Designs for the chunked sketch loop (niqki_amd/csrc/nq_sketch.hip roll_records): record lengths at the edges of the
chunk rule, the launch shape a batch takes, and the batches that tests/test_gpu_sketch_chunks.py runs and
tests/test_sketch_chunks_cpu.py checks.  Designs only: nothing here calls the library under test.

Three restatements, each of code read in the product:
  * plan_of / shape_of: sketch_dev's cut into parts (nq_api_build.hip) and the rule of nq_sketch_plan.h;
  * strength: the filter strength sketch_kernel picks per sketch (T = 2 / 3 / 4 at 55 / 115 / 240 k-mers per slot,
    a forced strength from mode n >= 2, off where T > 2^H - 1);
  * chunk_geometry: the four lines at the head of roll_records' record loop.
The CPU test holds plan_of against the compiled header for every batch below, so the restatement cannot drift.

A record of `len` bases has n = len - K k-mers (the last one is skipped).  The tables are in k-mers; K is added where
a batch is built.  Every row carries the property it was chosen for and the module asserts it at import."""
import numpy as np

# ---- the thresholds of nq_sketch_plan.h (average input bytes per sketch and workgroup) ----
LEN_WAVE, LEN_LONG, LEN_GROUPS8, LEN_NO_LATE, LEN_LINES = 415, 16384, 1 << 18, 1 << 19, 1 << 21
LDS_LIMIT = 160 * 1024
STACK_BYTES = 192 * 8                     # one wave's candidate stack
LEVEL_BYTES = 4 * 16 + 16 * 4 * 8         # the line form's words behind 16 stacks
NONE, WAVE, PLAIN, DISTINCT, LATE, GLOBAL = range(6)   # stat "last_densify_form"
SHAPE_NAMES = {(64, 0): 1, (256, 1): 2, (1024, 2): 3, (1024, 8): 4, (1024, 32): 5}   # SketchShape of (BLOCK, GROUPS)

_cache = {}


def text(n, at=0):
    """n bases of one seeded random ACGT text, from position `at`."""
    if "text" not in _cache:
        rng = np.random.default_rng(20261021)
        _cache["text"] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (1 << 25) + (1 << 23), dtype=np.uint8)]
    assert at + n <= _cache["text"].size
    return _cache["text"][at:at + n]


def reference(po, b):
    """(oracle parameters, the oracle's sketches of batch b, one row per sketch), computed once whatever the filter mode."""
    key = ("ref", b.name)
    if key not in _cache:
        p = po.make_params(b.K, b.S, b.W, b.H, 0.0, genome_size=b.G or 0.0)
        rows = []
        for recs in b.entry_records():
            if len(recs) == 1:
                rows.append(po.compute_sketch(p, recs[0]))
            else:
                acc = np.full(1 << b.S, -1, np.int32)
                for r in recs:
                    po.sketch_accumulate(p, r, acc)
                rows.append(po.densify(p, acc)[0])
        ref = np.stack(rows)
        ref.flags.writeable = False
        _cache[key] = (p, ref)
    return _cache[key]


# ---- launch shape ------------------------------------------------------------------------------------------------

def _lds(F, R, distinct, stacks, halves):
    return F // halves * 4 + 16 + 256 + 2048 + (12 * R if distinct else 0) + stacks * STACK_BYTES + (LEVEL_BYTES if stacks == 16 else 0)


def plan_of(K, S, W, H, total, n_entry, entry_rec, filter_mode, H_after=None):
    """What sketch_dev launches for n_entry sketches of `total` input bytes: the split count, and the plan of
    nq_sketch_plan.h for record bytes, own cells, the one-wavefront kernel allowed.  H_after: the handle's H once
    niqki_select_best_H has run (mask and saturation constants stay the constructor's: the parameters are irregular)."""
    F, R = 1 << S, 1 << W
    avg = total // n_entry
    splits = 1
    if avg >= 16384 and not entry_rec and n_entry < 128 and avg >= (1 << 20):
        splits = min(32, 512 // n_entry)
    halves = 2 if _lds(F, R, False, 16, 1) > LDS_LIMIT else 1
    merged = splits > 1 or halves > 1          # partial sketches merged in global memory, a densify launch behind
    densify = not merged
    avg_len = avg // splits
    p = dict(splits=splits, halves=halves, avg_len=avg_len, densify=densify, distinct=0, filter=0, late=False, K=K)
    if avg_len <= LEN_WAVE and splits == 1 and halves == 1:
        p.update(block=64, groups=0, form=WAVE)
        return p
    short = avg_len < LEN_LONG
    regular = H_after is None or H_after == H
    p["distinct"] = int(regular and short and halves == 1 and 4 * R <= F and S <= 13 and _lds(F, R, True, 0, 1) <= 150 * 1024)
    p["filter"] = filter_mode if regular and not short else 0
    p["late"] = bool(densify and not p["distinct"] and regular and avg_len < LEN_NO_LATE and 4 * R <= F and R <= 4096 and
                     F * 4 + R * 4 + 64 <= LDS_LIMIT)
    own = LATE if p["late"] else NONE if not densify else DISTINCT if p["distinct"] else PLAIN
    # the form the stat reports: the merging launch's where there is one
    p["form"] = (GLOBAL if halves > 1 else PLAIN) if merged else own
    p["lds"] = _lds(F, R, p["distinct"], (4 if short else 16) if p["filter"] else 0, halves)
    assert p["lds"] <= LDS_LIMIT
    p["block"], p["groups"] = ((256, 1) if short else (1024, 2) if avg_len < LEN_GROUPS8
                               else (1024, 8) if avg_len < LEN_LINES or F < 4 else (1024, 32))
    return p


def shape_of(K, S, W, H, total, n_entry, entry_rec, filter_mode, H_after=None):
    """(BLOCK, GROUPS, KFIX, splits, filtered, line_loop).  filtered: the plan hands the kernel a filter mode (the kernel
    may still find strength 0 for a sketch: strength()); line_loop: a sketch with a strength takes roll_records_lines."""
    p = plan_of(K, S, W, H, total, n_entry, entry_rec, filter_mode, H_after)
    filtered = p["filter"] != 0
    return (p["block"], p["groups"], 31 if K == 31 else 0, p["splits"], filtered,
            filtered and p["groups"] == 32 and p["halves"] == 1 and 17 <= K <= 31)


def strength(S, H, n_kmers, splits, filter_mode):
    """Leading zeros T the filter of a planned-filtered launch asks of a sketch with n_kmers k-mers; 0 = unfiltered."""
    if not filter_mode:
        return 0
    per_slot = (n_kmers // splits) >> S
    T = 4 if per_slot >= 240 else 3 if per_slot >= 115 else 2 if per_slot >= 55 else 0
    if filter_mode >= 2:
        T = filter_mode - 1
    return 0 if T > (1 << H) - 1 or T > 16 else T


# ---- chunk rule --------------------------------------------------------------------------------------------------

def chunk_geometry(BLOCK, GROUPS, n_kmers, splits=1):
    """(groups, CHUNK, n_chunks, k-mers in the last chunk) of a record with n_kmers > 0 k-mers."""
    groups = 1
    if GROUPS > 1:
        share = n_kmers // splits + 1
        rounds = -(-share // (BLOCK * 16 * GROUPS))
        groups = min(max(-(-share // (rounds * BLOCK * 16)), 1), GROUPS)
    CHUNK = 16 * groups
    n_chunks = -(-n_kmers // CHUNK)
    return groups, CHUNK, n_chunks, n_kmers - (n_chunks - 1) * CHUNK


def design(BLOCK, GROUPS, groups, mod, residue, last, lo):
    """The search: the fewest chunks, at least `lo`, with n_chunks % mod == residue for which the rule gives `groups`
    groups and a last chunk of `last` k-mers ("full", "short" = one fewer, or "one").  Returns n_kmers."""
    CHUNK = 16 * groups
    cnt = {"full": CHUNK, "short": CHUNK - 1, "one": 1}[last]
    for n_chunks in range(lo, lo + 64 * mod):
        n = (n_chunks - 1) * CHUNK + cnt
        if n_chunks % mod == residue and chunk_geometry(BLOCK, GROUPS, n) == (groups, CHUNK, n_chunks, cnt):
            return n
    raise AssertionError("no such record")


def _row(BLOCK, GROUPS, n, why, groups, lanes=None, last=None, rows=None, chunks_mod=None):
    """A table row; asserts the property it is there for.  lanes: live lanes of the last row of 64 chunks;
    rows: n_chunks modulo the workgroup's lanes (0: every lane the same rounds, 1: one lane one round more)."""
    g, CHUNK, n_chunks, cnt = chunk_geometry(BLOCK, GROUPS, n)
    assert g == groups, (n, why, g)
    if lanes is not None:
        assert (n_chunks - 1) % 64 + 1 == lanes, (n, why, n_chunks)
    if last is not None:
        assert cnt == {"full": CHUNK, "short": CHUNK - 1, "one": 1}[last], (n, why, cnt)
    if rows is not None:
        assert n_chunks % BLOCK == rows, (n, why, n_chunks)
    if chunks_mod is not None:
        assert n_chunks % chunks_mod[0] == chunks_mod[1], (n, why, n_chunks)
    return (n, why)


def _edge(BLOCK, GROUPS, n, below, above):
    """n k-mers take `below` groups and n + 1 take `above`."""
    assert chunk_geometry(BLOCK, GROUPS, n)[0] == below and chunk_geometry(BLOCK, GROUPS, n + 1)[0] == above, (n, below, above)
    return [(n, "groups %d, the last length before %d" % (below, above)), (n + 1, "groups %d, the first length after %d" % (above, below))]


def _first_change(BLOCK, GROUPS, lo, below, above):
    """The search: the first n >= lo whose successor takes another number of groups."""
    n = lo
    while chunk_geometry(BLOCK, GROUPS, n + 1)[0] == chunk_geometry(BLOCK, GROUPS, n)[0]:
        n += 1
    return _edge(BLOCK, GROUPS, n, below, above)


# 1024 x 2: groups 1 up to 16383 k-mers, 2 beyond; chunks of 16 or 32 k-mers
T2 = (
    [_row(1024, 2, design(1024, 2, 1, 64, 63, "one", 1000), "groups 1, 63 live lanes in the last row, a last chunk of one", 1, 63, "one")]
    + _first_change(1024, 2, 16000, 1, 2)
    + [_row(1024, 2, design(1024, 2, 2, 1024, 0, "full", 1000), "every chunk full, whole rows of 1024", 2, 64, "full", rows=0)]
    + [_row(1024, 2, design(1024, 2, 2, 1024, 1, "one", 1000), "one chunk more, holding one k-mer: one lane one round more", 2, 1, "one", rows=1)]
    + [_row(1024, 2, design(1024, 2, 2, 1024, 0, "short", 1000), "64 live lanes, the last chunk one short", 2, 64, "short", rows=0)]
    + [_row(1024, 2, design(1024, 2, 2, 64, 63, last, 513), "63 live lanes, last chunk " + last, 2, 63, last) for last in ("full", "short", "one")]
    + [_row(1024, 2, design(1024, 2, 2, 64, 1, last, 513), "one live lane, last chunk " + last, 2, 1, last) for last in ("full", "one")]
)
# 1024 x 8: chunks of up to 128 k-mers, rounds of 131072
T8 = (
    _first_change(1024, 8, 262000, 8, 6)
    + _first_change(1024, 8, 290000, 6, 7)
    + [_row(1024, 8, design(1024, 8, 8, 64, 0, "full", 2600), "groups 8, all chunks full, whole rows of 64", 8, 64, "full")]
    + [_row(1024, 8, design(1024, 8, 8, 64, 1, "one", 2600), "one k-mer more", 8, 1, "one")]
    + [_row(1024, 8, design(1024, 8, 8, 1024, 0, "full", 7000), "a whole number of rounds", 8, 64, "full", rows=0)]
    + [_row(1024, 8, design(1024, 8, 8, 1024, 1, "one", 7000), "one lane one round more", 8, 1, "one", rows=1)]
    + [_row(1024, 8, design(1024, 8, 8, 64, 63, last, 2600), "63 live lanes, last chunk " + last, 8, 63, last) for last in ("full", "short", "one")]
    + [_row(1024, 8, design(1024, 8, 8, 64, 1, "full", 2600), "one live lane, last chunk full", 8, 1, "full")]
    + [_row(1024, 8, design(1024, 8, 8, 64, 0, "short", 2600), "64 live lanes, the last chunk one short", 8, 64, "short")]
)
# the lengths the rule was read to give at K = 31: derived above, not copied
assert [n + 31 for n, _ in T2[:10]] == [16384, 16414, 16415, 32799, 32800, 32798, 18431, 18430, 18400, 16447], T2
assert [n + 31 for n, _ in T8[:8]] == [262174, 262175, 294942, 294943, 344095, 344096, 917535, 917536], T8

# a record gets groups = g inside a 1024 x 8 launch when n + 1 lies in ((g - 1) * 16384, g * 16384]: both ends of each
# interval, the lower end of the first being a record of one k-mer
T8_GROUPS = []
for _g in range(1, 9):
    T8_GROUPS += [_row(1024, 8, max((_g - 1) * 16384, 1), "groups %d, lower end" % _g, _g), _row(1024, 8, _g * 16384 - 1, "groups %d, upper end" % _g, _g)]
assert chunk_geometry(1024, 8, 8 * 16384)[0] == 5      # (beyond: two rounds)

# 256 x 1: one group per chunk whatever the length
T1 = [
    _row(256, 1, 64 * 16, "n_chunks = 0 mod 64, full", 1, 64, "full", chunks_mod=(64, 0)),
    _row(256, 1, 64 * 16 + 1, "n_chunks = 1 mod 64, a last chunk of one", 1, 1, "one", chunks_mod=(64, 1)),
    _row(256, 1, 63 * 16 - 1, "n_chunks = 63 mod 64, one short", 1, 63, "short", chunks_mod=(64, 63)),
    _row(256, 1, 256 * 16, "n_chunks = 0 mod 256: every lane one chunk", 1, 64, "full", rows=0),
    _row(256, 1, 256 * 16 + 1, "n_chunks = 1 mod 256: one lane a second round", 1, 1, "one", rows=1),
    _row(256, 1, 3 * 256 * 16 - 16, "n_chunks = 255 mod 256 in the third round", 1, 63, "full", chunks_mod=(256, 255)),
    (0, "K bases: no k-mer"), (1, "K + 1 bases: one k-mer"), (2, "K + 2 bases"),
]


# ---- batches -----------------------------------------------------------------------------------------------------

class Batch:
    """One call of niqki_sketch: records (a function, so that nothing is built at import), how they fall into sketches
    (entries: None = one record per sketch WITHOUT entry_rec, so that sketch_dev may cut; else a list of record counts),
    the parameters, the filter modes to run and the shape the design means to run."""

    def __init__(self, name, K, S, W, H, build, entries, modes, block, groups, splits=1, G=None, H_after=None, form=PLAIN, line=False):
        self.name, self.K, self.S, self.W, self.H = name, K, S, W, H
        self._build, self.entries, self.modes = build, entries, modes
        self.block, self.groups, self.splits, self.G, self.H_after, self.form, self.line = block, groups, splits, G, H_after, form, line

    def records(self):
        key = ("records", self.name)
        if key not in _cache:
            recs = [np.ascontiguousarray(r, dtype=np.uint8) for r in self._build()]
            for r in recs:
                r.flags.writeable = False
            _cache[key] = recs
        return _cache[key]

    def entry_rec(self):
        if self.entries is None:
            return None
        return np.concatenate([[0], np.cumsum(self.entries)]).astype(np.uint32)

    def entry_records(self):
        """The records of every sketch, in order."""
        recs = self.records()
        if self.entries is None:
            return [[r] for r in recs]
        er = self.entry_rec()
        return [recs[er[i]:er[i + 1]] for i in range(er.size - 1)]

    def n_entry(self):
        return len(self.records()) if self.entries is None else len(self.entries)

    def total(self):
        return sum(r.size for r in self.records())

    def shape(self, mode):
        return shape_of(self.K, self.S, self.W, self.H, self.total(), self.n_entry(), self.entries is not None, int(mode), self.H_after)

    def plan(self, mode):
        return plan_of(self.K, self.S, self.W, self.H, self.total(), self.n_entry(), self.entries is not None, int(mode), self.H_after)

    def check_shape(self, mode):
        """The batch runs the shape it was designed for; returns the plan."""
        s = self.shape(mode)
        assert s[:4] == (self.block, self.groups, 31 if self.K == 31 else 0, self.splits), (self.name, mode, s)
        p = self.plan(mode)
        assert p["form"] == self.form, (self.name, mode, p)
        assert s[5] == (self.line and int(mode) != 0), (self.name, mode, s)
        return p

    def entry_kmers(self):
        return [sum(max(int(r.size) - self.K, 0) for r in recs) for recs in self.entry_records()]


def _one(n):
    return [1] * n


def _slices(lengths, at=1000):
    """Records of these lengths, cut from the text one behind the other."""
    out = []
    for n in lengths:
        out.append(text(n, at))
        at += n + 7
    return out


def _padded(lengths, lo, hi, pad_len):
    """The lengths, and plain records behind them until the batch's average lies in [lo, hi)."""
    ls = list(lengths)
    while not lo <= sum(ls) // len(ls) < hi:
        ls.append(pad_len)
        assert len(ls) < 200
    return ls


ALL = []


def _add(b):
    ALL.append(b)
    return b


# -- 1. length edges, S = 10, W = 12, H = 4 --
LENGTH_EDGES = []
for _K in (31, 21):
    _l2 = _padded([n + _K for n, _ in T2], LEN_LONG, LEN_GROUPS8, 40000 + _K)
    LENGTH_EDGES.append(_add(Batch("edges-1024x2-K%d" % _K, _K, 10, 12, 4, lambda l=_l2: _slices(l), _one(len(_l2)), ("1", "4"), 1024, 2)))
    _l8 = _padded([n + _K for n, _ in T8], LEN_GROUPS8, LEN_LINES, 500000 + _K)
    LENGTH_EDGES.append(_add(Batch("edges-1024x8-K%d" % _K, _K, 10, 12, 4, lambda l=_l8: _slices(l), _one(len(_l8)), ("1", "4"), 1024, 8)))
    # the eight values of `groups` inside one 1024 x 8 launch: long companions choose the launch
    _lg = _padded([n + _K for n, _ in T8_GROUPS], LEN_GROUPS8, LEN_LINES, 1500000 + _K)
    LENGTH_EDGES.append(_add(Batch("groups-1024x8-K%d" % _K, _K, 10, 12, 4, lambda l=_lg: _slices(l), _one(len(_lg)), ("1", "4"), 1024, 8)))
    _l1 = [n + _K for n, _ in T1]
    assert LEN_WAVE < sum(_l1) // len(_l1) < LEN_LONG
    LENGTH_EDGES.append(_add(Batch("edges-256x1-K%d" % _K, _K, 10, 12, 4, lambda l=_l1: _slices(l), _one(len(_l1)), ("1", "4"), 256, 1)))
# filter off: roll_records<1024, 32> on the line loop's lengths -- a record of 2^21 + 77 bases (five rounds of 26 groups),
# one that takes all 32 groups in one round, and a companion that keeps the average
_lu = [(1 << 21) + 77, 32 * 16384 - 1 + 31, 3700000]
assert chunk_geometry(1024, 32, _lu[0] - 31)[0] == 26 and chunk_geometry(1024, 32, _lu[1] - 31) == (32, 512, 1024, 511)
UNFILTERED_32 = _add(Batch("unfiltered-1024x32", 31, 10, 12, 4, lambda: _slices(_lu), _one(3), ("0",), 1024, 32))

# -- 2. address phases: records back to back in a device buffer; the last one has every chunk full --
_PH2 = [20005, 17013, 30005, 16421, T2[3][0] + 31]
_PH8 = [300005, 270005, 400005, 262149, T8[4][0] + 31]
for _ls in (_PH2, _PH8):
    _starts = np.concatenate([[0], np.cumsum(_ls)[:-1]])
    assert {int(s) % 4 for s in _starts} == {0, 1, 2, 3} and len({int(s) % 16 for s in _starts}) >= 4, _starts
assert chunk_geometry(1024, 2, _PH2[-1] - 31)[3] == 32 and chunk_geometry(1024, 8, _PH8[-1] - 31)[3] == 128
PHASES = [_add(Batch("phases-1024x2", 31, 10, 12, 4, lambda: _slices(_PH2, 5000), _one(5), ("1", "4"), 1024, 2)),
          _add(Batch("phases-1024x8", 31, 10, 12, 4, lambda: _slices(_PH8, 9000), _one(5), ("1", "4"), 1024, 8))]


# -- 3. dirty bytes at chunk edges --
def _dirty(K, BLOCK, GROUPS, length, at):
    """Two records of `length` bases.  The first: 'N' and lower case on the last hash byte of a chunk and the first of
    the next (k-mer i is hashed when base i + K - 1 arrives: chunk c ends at base (c + 1) * CHUNK + K - 2), at a lane in
    the middle of a wave, at a wave's last lane, at the workgroup's last lane and at the record's last whole chunk; a run
    of N; an illegal byte inside the K - 1 prefix, which zeroes all its digits.  The second: a legal lower-case prefix
    byte, which is kept, and dirty bytes in the first K - 1 + (31 - K) bases and just behind, where the first wave takes
    the generic warm-up and a lane of the fast form would reach back into the prefix."""
    _, CHUNK, n_chunks, _ = chunk_geometry(BLOCK, GROUPS, length - K)
    assert n_chunks > BLOCK + 2
    a = text(length, at).copy()
    for c, tail, head in ((3, b"N", b"a"), (63, b"c", b"N"), (BLOCK - 1, b"g", b"t"), (n_chunks - 2, b"N", b"N")):
        a[(c + 1) * CHUNK + K - 2] = tail[0]
        a[(c + 1) * CHUNK + K - 1] = head[0]
    a[length // 2:length // 2 + 40] = ord("N")
    a[min(7, K - 2)] = ord("n")
    b = text(length, at).copy()
    b[3] = ord("g")
    if K < 31:
        b[K - 1] = ord("N")
        b[29] = ord("c")
    b[30:34] = np.frombuffer(b"aNtn", np.uint8)
    b[K - 1 + CHUNK:K + 9 + CHUNK] = np.frombuffer(b"acgtNacgtn", np.uint8)
    return [a, b]


DIRTY = []
for _K in (31, 30, 17, 16, 9):
    DIRTY.append(_add(Batch("dirty-1024x2-K%d" % _K, _K, 10, 12, 4, lambda K=_K: _dirty(K, 1024, 2, 70000 + K, 11000), _one(2), ("1", "4"), 1024, 2)))
    DIRTY.append(_add(Batch("dirty-1024x8-K%d" % _K, _K, 10, 12, 4, lambda K=_K: _dirty(K, 1024, 8, 300000 + K, 12000), _one(2), ("1", "4"), 1024, 8)))


# -- 4. the candidate stack under full pressure --
def _runs(K, BLOCK, GROUPS, length, at, run=None):
    """Four records of random text: a run of N, of A and of T, each of at least 3 * 64 * CHUNK + K bases (two whole
    wave-rows and more of steps at which all 64 lanes push: every k-mer inside is all A or all T, canonical word 0),
    and a run of A that starts and ends in the middle of a chunk."""
    _, CHUNK, n_chunks, _ = chunk_geometry(BLOCK, GROUPS, length - K)
    run = run or 3 * 64 * CHUNK + K
    assert CHUNK == 16 * GROUPS and run >= 3 * 64 * CHUNK + K and n_chunks * CHUNK > 2 * run
    out = []
    for i, ch in enumerate(b"NAT"):
        r = text(length, at + 1000 * i).copy()
        start = 5 * CHUNK + K - 1 + 1000 * i      # (i = 0: a chunk's first hash byte)
        r[start:start + run] = ch
        out.append(r)
    r = text(length, at + 5000).copy()
    start = 70 * CHUNK + K - 1 + CHUNK // 2
    r[start:start + run + CHUNK + 5] = ord("A")
    assert (start - (K - 1)) % CHUNK == CHUNK // 2 and 1 < (start + run + CHUNK + 5 - (K - 1)) % CHUNK < CHUNK - 1
    out.append(r)
    return out


STACK = [
    _add(Batch("stack-1024x2-K31", 31, 10, 12, 4, lambda: _runs(31, 1024, 2, 70031, 20000), _one(4), ("1", "4"), 1024, 2)),
    _add(Batch("stack-1024x8-K31", 31, 10, 12, 4, lambda: _runs(31, 1024, 8, 350031, 21000), _one(4), ("1", "4"), 1024, 8)),
    _add(Batch("stack-1024x8-K21", 21, 10, 12, 4, lambda: _runs(21, 1024, 8, 350021, 22000), _one(4), ("1", "4"), 1024, 8)),
    _add(Batch("stack-generic-K16", 16, 10, 12, 4, lambda: _runs(16, 1024, 2, 70016, 23000), _one(4), ("1", "4"), 1024, 2)),
    # S = 16: every workgroup keeps half the slots, which takes the generic filtered form with `hsel`
    _add(Batch("stack-halves-S16", 31, 16, 12, 4, lambda: _runs(31, 1024, 2, 70031, 24000), _one(4), ("4",), 1024, 2, form=GLOBAL)),
]


def _line_runs(K, at):
    out = []
    for i, ch in enumerate(b"NAT"):
        r = text((1 << 21) + 77, at + 3000 * i).copy()
        r[400_000 + 37 * i:700_000 + 37 * i] = ch
        out.append(r)
    return out


for _K in (31, 21):
    STACK.append(_add(Batch("stack-lines-K%d" % _K, _K, 10, 12, 4, lambda K=_K: _line_runs(K, 30000), _one(3), ("1", "4"), 1024, 32, line=True)))

# -- 5. filter strength, S = 9, automatic: both sides of 55, 115 and 240 k-mers per slot --
STRENGTH_KMERS = [55 * 512 - 1, 55 * 512, 115 * 512 - 1, 115 * 512, 240 * 512 - 1, 240 * 512]
assert [strength(9, 4, n, 1, 1) for n in STRENGTH_KMERS] == [0, 2, 2, 3, 3, 4]
assert [strength(9, 2, n, 1, 1) for n in STRENGTH_KMERS] == [0, 2, 2, 3, 3, 0]       # 4 > 2^2 - 1: the guard
assert [strength(9, 1, n, 1, 1) for n in STRENGTH_KMERS] == [0, 0, 0, 0, 0, 0]
assert [strength(9, 0, n, 1, 1) for n in STRENGTH_KMERS] == [0, 0, 0, 0, 0, 0]
assert [strength(9, 7, n, 1, 1) for n in STRENGTH_KMERS] == [0, 2, 2, 3, 3, 4]
assert strength(9, 1, STRENGTH_KMERS[0], 1, 2) == 1 and strength(9, 2, STRENGTH_KMERS[0], 1, 5) == 0 and strength(9, 4, STRENGTH_KMERS[0], 1, 7) == 6
STRENGTH = []
for _W, _H in ((12, 4), (6, 2), (10, 1), (8, 0), (15, 7)):
    _modes = ("1",) + {(10, 1): ("2",), (6, 2): ("5",), (12, 4): ("7",)}.get((_W, _H), ())
    STRENGTH.append(_add(Batch("strength-W%d-H%d" % (_W, _H), 31, 9, _W, _H, lambda: _slices([n + 31 for n in STRENGTH_KMERS], 40000),
                               _one(6), _modes, 1024, 2, form=LATE if 4 << _W <= 512 else PLAIN)))

# -- 6. after niqki_select_best_H: K = 31, S = 12, W = 12, H = 4, G = 150 --
SELECT_G = 150.0
SELECTED = [
    _add(Batch("selected-20000", 31, 12, 12, 4, lambda: _slices([20000], 50000), _one(1), ("1",), 1024, 2, G=SELECT_G, H_after=2)),
    _add(Batch("selected-300000", 31, 12, 12, 4, lambda: _slices([300000], 51000), _one(1), ("1",), 1024, 8, G=SELECT_G, H_after=2)),
    _add(Batch("selected-2M", 31, 12, 12, 4, lambda: _slices([(1 << 21) + 77], 52000), _one(1), ("1",), 1024, 32, G=SELECT_G, H_after=2)),
    _add(Batch("selected-entry", 31, 12, 12, 4, lambda: _slices([300000, 40, 20000], 53000), [3], ("1",), 1024, 8, G=SELECT_G, H_after=2)),
]

# -- 7. splits other than 32: no entry_rec, so sketch_dev cuts with min(32, 512 / n_entry) --
_S17 = [(1 << 20) + x for x in (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 77)]
_S37 = [(1 << 20) + 2 * i + 1 for i in range(37)]
assert sum(_S37) < 40 << 20
SPLITS = [
    _add(Batch("splits-30", 31, 10, 12, 4, lambda: _slices(_S17, 0), None, ("1", "4", "7"), 1024, 2, splits=30)),
    _add(Batch("splits-13", 31, 10, 12, 4, lambda: _slices(_S37, 100), None, ("1", "4", "7"), 1024, 2, splits=13)),
    _add(Batch("splits-30-S16", 31, 16, 12, 4, lambda: _slices(_S17, 0), None, ("1",), 1024, 2, splits=30, form=GLOBAL)),
]
# the part boundaries n_chunks * part / splits are uneven: not every part holds the same number of chunks
for _b, _n in ((30, _S17[0] - 31), (13, _S37[0] - 31)):
    _nc = chunk_geometry(1024, 2, _n, _b)[2]
    assert len({_nc * (p + 1) // _b - _nc * p // _b for p in range(_b)}) > 1


# -- 8. whole-file entries in the chunked shapes --
def _file(long1, long2, at):
    """Two sketches of the same six records: [long, K bases, K + 1, empty, 40 bases, long], and with the second long one
    2 K + 1 bases behind the first one's end."""
    a, k0, k1, e, s, b = (text(long1, at), text(31, at + 3_000_000), text(32, at + 3_100_000), text(0, 0), text(40, at + 3_200_000),
                          text(long2, at + 1_500_000))
    return [a, k0, k1, e, s, b, a, k0, k1, b, e, s]


FILES = [_add(Batch("file-1024x2", 31, 10, 12, 4, lambda: _file(60011, 50130, 60000), [6, 6], ("1", "4"), 1024, 2)),
         _add(Batch("file-1024x8", 31, 10, 12, 4, lambda: _file(400011, 300130, 61000), [6, 6], ("1", "4"), 1024, 8))]

assert len({b.name for b in ALL}) == len(ALL)
