"""GPU: the hit kernels on designed counts (tests/hit_designs.py, pinned on the oracle by test_hit_designs_cpu.py).

Every expectation is hit_designs.reference_lists -- threshold, (count, gid) descending, cut to k, in numpy -- and every
query of every call is compared: offsets, counts and gids.

A. synthetic u16 counter rows through niqki_hits_from_counts (hits_count / hits_select + sel_boundary / hits_scan /
   hits_compact / hits_sort): range shapes at the block, alignment and launch-shape edges, thresholds 0 .. 65 536, top-k
   cuts placed inside runs of ties across compaction blocks, batches of several scan rounds, capacities below the total.
B. designed indexes through niqki_query, both forms (hitlist_scan / hitlist_emit with network_sort and compact_desc, the
   list tail of gather_kernel; counter rows): exact list sizes around hit_list_cap and the network's sizes, several
   tiles, gids beyond 16 bits, batches beyond one scan workgroup.

Which case reaches which path:
  hitlist_scan_kernel, workgroup >= 5, k = 0 and k > 0 .. test_batches_beyond_one_scan_block[20489] (6 workgroups)
  hits_scan_kernel, >= 3 rounds ......................... test_rows_batches[8193 | 12289], ..beyond_one_scan_block (rows)
  hits_count_kernel<false> / <true> on the same rows .... test_rows_shapes[28672-* | 28673-*]
  sel_walk, scalar and 16-byte path ..................... test_rows_shapes: odd strides (test_the_shapes_cover_..)
  hitlist_emit_kernel, networks 256 / 512 / 1024 / 2048 and the path above, 4-byte keys
      ................................................... test_exact_list_sizes[cap4]: 5 .. 256 / 257 .. 512 / 513 ..
                                                          1024 / 1025 .. 2048 / 2049 and N hits
      the same with 8-byte keys ......................... test_beyond_16_bit_gids: 5, 257, 1000, 2048, 2049 hits
  blk_skip 0 / partial / kSkipAllTies in one row ........ test_rows_shapes, every shape of >= 3 blocks (asserted there)
"""
import functools

import numpy as np
import pytest

import hit_designs as hd

pytestmark = pytest.mark.gpu

E_CAPACITY = 4
T_TIE = 20           # the count of the placed ties: above min_score 16, T - 1 = 19 still a hit there


def small_engine(native, min_score=1):
    return native.Engine(K=31, S=10, W=8, H=3, min_score_value=min_score)


def check(got, exp, *what):
    d = hd.first_difference(got, exp)
    assert d is None, "%s: %s" % (what, d)


# ---- A. synthetic rows -------------------------------------------------------------------------------------------------

RECIPES = ("placed_ties", "levels", "bin_edges", "u16", "ramp", "zeros", "const1", "const16", "const65535", "placed_ties_b")


def make_rows(n, nq, seed):
    """nq rows of n counters, row i by recipe i % len(RECIPES) -> (rows u16[nq, n], names)"""
    rng = np.random.default_rng(seed)
    pos = hd.edge_positions(n)
    rows, names = [], []
    for i in range(nq):
        name = RECIPES[i % len(RECIPES)]
        if name == "placed_ties":
            r = hd.row_placed_ties(n, T_TIE, pos, [5, n // 2, n - 2, hd.BLK + 17], rng)
        elif name == "placed_ties_b":   # ties only late in every block, a few genomes above in every block
            r = hd.row_placed_ties(n, T_TIE, [b + o for b in range(0, n, hd.BLK) for o in (0, 700, 701, 3000)],
                                   [b + 1000 for b in range(0, n, hd.BLK)], rng)
        elif name == "levels":
            r = hd.row_levels(n, rng)
        elif name == "bin_edges":
            r = hd.row_bin_edges(n, rng)
        elif name == "u16":
            r = hd.row_u16(n, rng)
        elif name == "ramp":
            r = hd.row_ramp(n)
        elif name == "zeros":
            r = hd.row_zeros(n)
        else:
            r = hd.row_const(n, int(name[5:]))
        rows.append(r)
        names.append(name)
    return np.stack(rows), names


def framed(rows, gid_begin, pad):
    """the rows inside a (nq, stride) array, stride = gid_begin + n_gids + pad; the cells outside the range hold 65 535
    (a hit at every threshold but the last, were one of them read)"""
    nq, n = rows.shape
    buf = np.full((nq, gid_begin + n + pad), 0xFFFF, np.uint16)
    buf[:, gid_begin:gid_begin + n] = rows
    return buf


def on_16_bytes(nq, stride, gid_begin):
    """per row: does it start on a 16-byte boundary of a 16-byte-aligned buffer (the 8-counter loads of hits_count_kernel,
    sel_walk) or not (their scalar loops)"""
    return (np.arange(nq) * stride + gid_begin) % 8 == 0


# (n_gids, gid_begin, pad, nq, rows made at this size and cut to n_gids)
SHAPES = [
    (1, 0, 0, 1, 1), (7, 1, 1, 15, 7), (8, 0, 0, 16, 8), (9, 4, 63, 17, 9), (255, 8, 1, 33, 255), (257, 1, 0, 16, 257),
    (4095, 0, 1, 17, 4095), (4096, 4, 1, 15, 4096), (4097, 8, 0, 16, 4097), (8200, 0, 63, 17, 8200), (8200, 4, 0, 33, 8200),
    (28672, 0, 0, 17, 28673), (28673, 0, 0, 17, 28673), (28672, 1, 0, 17, 28673), (28673, 1, 1, 17, 28673),
    (40000, 8, 1, 16, 40000), (70001, 4, 63, 15, 70001),
]
MIN_SCORES = (0, 1, 16, 65535, 65536)


def test_the_shapes_cover_what_they_claim():
    ns = {s[0] for s in SHAPES}
    assert ns == {1, 7, 8, 9, 255, 257, 4095, 4096, 4097, 8200, 28672, 28673, 40000, 70001}
    assert {s[1] for s in SHAPES} == {0, 1, 4, 8} and {s[2] for s in SHAPES} == {0, 1, 63}
    assert {s[3] for s in SHAPES} == {1, 15, 16, 17, 33}
    for narrow, wide in (((28672, 0, 0), (28673, 0, 0)), ((28672, 1, 0), (28673, 1, 1))):
        a = [s for s in SHAPES if s[:3] == narrow][0]
        b = [s for s in SHAPES if s[:3] == wide][0]
        assert a[3:] == b[3:] and a[0] < hd.WIDE_FROM <= b[0]     # the same rows, one genome apart
    # rows on and off the 16-byte path in one call, on both sides of the switch of hits_count_kernel
    for lo, hi in ((2, hd.WIDE_FROM), (hd.WIDE_FROM, 1 << 20)):
        mixed = [s for s in SHAPES if lo <= s[0] < hi and len(set(on_16_bytes(s[3], s[0] + s[1] + s[2], s[1]).tolist())) == 2]
        assert mixed, (lo, hi)
    assert any((s[0] + s[1] + s[2]) % 2 for s in SHAPES)


@pytest.mark.parametrize("n_gids,gid_begin,pad,nq,made_at", SHAPES, ids=["%d-%d-%d-%d" % s[:4] for s in SHAPES])
def test_rows_shapes(native, n_gids, gid_begin, pad, nq, made_at):
    rows, names = make_rows(made_at, nq, 1000 + made_at)
    rows = np.ascontiguousarray(rows[:, :n_gids])
    buf = framed(rows, gid_begin, pad)
    e = small_engine(native)
    n_blk = -(-n_gids // hd.BLK)
    seen_states, cut_blocks = [], set()
    for ms in MIN_SCORES:
        e.set_option("min_score", ms)
        full = hd.reference_lists(rows, ms, gid_begin=gid_begin)
        assert np.diff(full[0]).tolist() == [int((r.astype(np.int64) >= ms).sum()) for r in rows]
        ks = set(hd.call_ks(rows, ms))
        if ms <= T_TIE:
            for i, name in enumerate(names):
                if name.startswith("placed_ties"):
                    for b, k, states in hd.tie_cuts(rows[i], T_TIE, ms):
                        ks.add(k)
                        seen_states.append(states)
                        cut_blocks.add(b)
        for k in [0] + sorted(ks):
            e.set_option("top_k", k)
            exp = hd.cut_lists(full, k, n_gids)
            got = e.hits_from_counts(buf, gid_begin=gid_begin, n_gids=n_gids, capacity=int(exp[0][-1]))
            d = hd.first_difference(got, exp)
            if d is not None:
                q = int(d.split()[1]) if d.startswith("query") else -1
                pytest.fail("n_gids %d gid_begin %d stride %d nq %d min_score %d top_k %d, recipe %s: %s" %
                            (n_gids, gid_begin, buf.shape[1], nq, ms, k, names[q] if q >= 0 else "?", d))
    if n_blk >= 3:
        # one row, one cut: blocks that keep every tie, the block of the cut, blocks that keep none; and the cut block
        # is once the topmost block, once a middle one, once block 0
        assert {"all", "part", "none"} in seen_states
        # (a last block of a single genome holds one tie: nothing to cut inside it)
        top = n_blk - 1 if n_gids - (n_blk - 1) * hd.BLK >= 2 else n_blk - 2
        assert {0, top} <= cut_blocks and any(0 < b < top for b in cut_blocks)
    e.close()


@pytest.mark.parametrize("nq", [4095, 4096, 4097, 8193, 12289])
def test_rows_batches(native, nq):
    """the rounds of hits_scan_kernel (4096 queries each): 40 genomes, heavy ties, empty rows among them"""
    rng = np.random.default_rng(nq)
    n_gids, gid_begin = 40, 1
    rows = rng.choice(np.asarray([0, 0, 3, 5, 9], np.uint16), size=(nq, n_gids))
    rows[rng.random(nq) < 0.2] = 0
    rows[-1] = 9
    buf = framed(rows, gid_begin, 0)     # stride 41: one row in eight on the 16-byte path
    e = small_engine(native, 3)
    full = hd.reference_lists(rows, 3, gid_begin=gid_begin)
    assert (np.diff(full[0]) == 0).any() and full[0][-1] > 10 * nq
    for k in (0, 3):
        e.set_option("top_k", k)
        exp = hd.cut_lists(full, k, n_gids)
        check(e.hits_from_counts(buf, gid_begin=gid_begin, n_gids=n_gids, capacity=int(exp[0][-1])), exp, nq, k)
    e.close()


def capacity_rows():
    rows, _ = make_rows(8200, 17, 77)
    return rows


def test_rows_capacity_host(native):
    """one entry short: NIQKI_E_CAPACITY, every offset exact, nothing written; exactly enough: the words behind the
    capacity untouched"""
    rows = capacity_rows()
    gid_begin, n = 4, rows.shape[1]
    buf = framed(rows, gid_begin, 1)
    nq, stride = buf.shape
    e = small_engine(native, 16)
    GUARD = 0xDEADBEEF
    for k in (0, 7):
        e.set_option("top_k", k)
        exp = hd.reference_lists(rows, 16, top_k=k, gid_begin=gid_begin)
        total = int(exp[0][-1])
        for capacity in (total - 1, total):
            off = np.zeros(nq + 1, np.uint64)
            hc, hg = np.full(total + 64, GUARD, np.uint32), np.full(total + 64, GUARD, np.uint32)
            rc = e.L.niqki_hits_from_counts(e.h, buf.ctypes.data, nq, stride, gid_begin, n, off.ctypes.data, hc.ctypes.data,
                                            hg.ctypes.data, capacity, native.capi.MEM_HOST)
            assert rc == (E_CAPACITY if capacity < total else 0), (k, capacity, rc)
            assert np.array_equal(off.astype(np.int64), exp[0]), (k, capacity)
            assert np.all(hc[capacity:] == GUARD) and np.all(hg[capacity:] == GUARD), (k, capacity)
            if rc:
                assert np.all(hc == GUARD) and np.all(hg == GUARD), (k, capacity)
            else:
                check((off, hc[:total], hg[:total]), exp, k, capacity)
    e.close()


def test_rows_capacity_device(native):
    """device outputs 64 entries longer than the capacity passed: offsets exact, every query that ends within the
    capacity complete, no entry at or behind the capacity written"""
    import torch
    rows = capacity_rows()
    gid_begin, n = 4, rows.shape[1]
    buf = framed(rows, gid_begin, 1)
    nq, stride = buf.shape
    dev = torch.device("cuda")
    e = small_engine(native, 16)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_counts = torch.from_numpy(buf.view(np.int16)).to(dev)
    SENT = -7
    for k in (0, 7):
        e.set_option("top_k", k)
        exp = hd.reference_lists(rows, 16, top_k=k, gid_begin=gid_begin)
        total = int(exp[0][-1])
        for capacity in (total + 5, total, int(exp[0][nq // 2]) + 3, 1):
            d_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            d_hc = torch.full((capacity + 64,), SENT, dtype=torch.int32, device=dev)
            d_hg = torch.full((capacity + 64,), SENT, dtype=torch.int32, device=dev)
            e.hits_from_counts_dev(d_counts, nq, stride, gid_begin, n, d_off, d_hc, d_hg, capacity)
            e.synchronize()
            hc, hg = d_hc.cpu().numpy(), d_hg.cpu().numpy()
            assert np.array_equal(d_off.cpu().numpy(), exp[0]), (k, capacity)
            assert np.all(hc[capacity:] == SENT) and np.all(hg[capacity:] == SENT), (k, capacity)
            whole = int(exp[0][np.searchsorted(exp[0], capacity, side="right") - 1])
            assert whole == total or whole <= capacity < total
            assert np.array_equal(hc[:whole].astype(np.int64), exp[1][:whole]), (k, capacity)
            assert np.array_equal(hg[:whole].astype(np.int64), exp[2][:whole]), (k, capacity)
    e.close()


# ---- B. designed indexes -----------------------------------------------------------------------------------------------

MS = 20              # min_score of the designed indexes: hits at 20 / 21 / 25 / 30, the others at 0 / 19
B1_SIZES = [0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3000]


@functools.lru_cache(maxsize=None)
def b1_design():
    N, S = 3000, 10
    rng = np.random.default_rng(101)
    n_hits = B1_SIZES + [2, 6, 10, 16, 17, 100, 300, 700, 1500, 2500, 2999]     # 32 query types
    C = hd.hit_matrix(n_hits, N, rng, MS)
    sk, q = hd.design(C, S, 8, rng)
    return N, S, n_hits, sk, q, hd.reference_lists(C, MS)


def query_exact(e, q, exp, *what):
    """niqki_query with exactly the expected total of room, compared with exp"""
    check(e.query(q, capacity=int(exp[0][-1])), exp, *what)


@pytest.mark.parametrize("form", ["cap4", "cap5", "cap256", "cap2048", "rows"])
def test_exact_list_sizes(native, form):
    """32 query types with exactly 0 .. N hits each, ties everywhere: the list capacity (5 rounds up to 8: 8 / 9 hits
    straddle it), the emit kernel's networks of 256 / 512 / 1024 / 2048 keys, the path above 2048, and the top-k cut at
    every list's size and one below it"""
    N, S, n_hits, sk, q, full = b1_design()
    assert np.diff(full[0]).tolist() == n_hits
    e = native.Engine(K=31, S=S, W=8, H=3, min_score_value=MS)
    e.insert(sk)
    e.build()
    assert e.stat("tiles") == 1
    cap = 0
    if form == "rows":
        e.set_option("hit_lists", 0)
    else:
        cap = int(form[3:])
        e.set_option("hit_list_cap", cap)
    ks = {0, 1, cap + 1} | {n - 1 for n in B1_SIZES} | set(B1_SIZES)
    for k in sorted(k for k in ks if k >= 0):
        e.set_option("top_k", k)
        query_exact(e, q, hd.cut_lists(full, k, N), form, "top_k", k)
        assert e.stat("last_hits_form") == (0 if form == "rows" else 1)
    e.close()


@functools.lru_cache(maxsize=None)
def b2_design(n_tiles):
    """N = 16 384 in n_tiles tiles (blocks of 32 genomes dealt round-robin: tile = gid // 32 % n_tiles)"""
    N, S = 16384, 8
    rng = np.random.default_rng(200 + n_tiles)
    tile_of = (np.arange(N) // 32) % n_tiles
    last = n_tiles - 1

    def pick(tile_mask, n):
        return rng.choice(np.flatnonzero(tile_mask), n, replace=False)

    ids = [
        np.concatenate([pick(tile_of == t, 2) for t in range(n_tiles)]),                 # 0: equal counts in every tile
        np.concatenate([pick(tile_of == 0, 2), pick(tile_of == 1, 2), pick(tile_of == last, 1)]),   # 1: 4, the 5th in the last
        np.concatenate([pick(tile_of != last, 256), pick(tile_of == last, 1)]),          # 2: 256, the 257th in the last
        pick(tile_of == 0, 300),                                                         # 3: beyond both caps at tile 0
        pick(tile_of >= 0, 3),                                                           # 4: fits everywhere
        np.zeros(0, np.int64),                                                           # 5: no hit
        pick(tile_of >= 0, 2049),                                                        # 6: beyond the network
        np.concatenate([[0, N - 1], pick((tile_of >= 0) & (np.arange(N) % (N - 1) != 0), 698)]),   # 7
    ]
    C = rng.choice(np.asarray([0, 19], np.int64), size=(len(ids), N))
    for t, g in enumerate(ids):
        C[t, g] = MS if t in (0, 1) else rng.choice(np.asarray([20, 21, 25, 30]), size=len(g))
    sk, q = hd.design(C, S, 8, rng)
    return N, S, sk, q, hd.reference_lists(C, MS)


def both_forms(e, q, full, N, caps, ks, what):
    """the counter-row form, then -- behind a call on other queries, whose counts stay in the rows the list form falls
    back on -- the list form at every cap, each against the reference"""
    for k in ks:
        e.set_option("top_k", k)
        exp = hd.cut_lists(full, k, N)
        e.set_option("hit_lists", 0)
        query_exact(e, q, exp, what, "rows", k)
        assert e.stat("last_hits_form") == 0
        e.query(np.roll(q, 1, axis=0))
        e.set_option("hit_lists", 1)
        for cap in caps:
            e.set_option("hit_list_cap", cap)
            query_exact(e, q, exp, what, "lists", cap, k)
            assert e.stat("last_hits_form") == 1


@pytest.mark.parametrize("tile,n_tiles", [(2048, 8), (5504, 3)])
def test_several_tiles(native, tile, n_tiles):
    N, S, sk, q, full = b2_design(n_tiles)
    assert np.diff(full[0]).tolist() == [2 * n_tiles, 5, 257, 300, 3, 0, 2049, 700]
    e = native.Engine(K=31, S=S, W=8, H=3, min_score_value=MS, tile_genomes=tile)
    e.insert(sk)
    e.build()
    assert e.stat("tiles") == n_tiles
    both_forms(e, q, full, N, (4, 256), (0, 10), tile)
    e.close()


@functools.lru_cache(maxsize=None)
def b3_design():
    N, S = 66000, 8
    rng = np.random.default_rng(303)
    n_hits = [5, 257, 1000, 2048, 2049, 0, 1]
    C = hd.hit_matrix(n_hits, N, rng, MS, forced=(65535, 65536))
    sk, q = hd.design(C, S, 8, rng)
    return N, S, n_hits, sk, q, hd.reference_lists(C, MS)


def test_beyond_16_bit_gids(native):
    """66 000 genomes: 8-byte keys in network_sort at each of its sizes, compact_desc above them; gids 65 535 and 65 536
    hold the same count in every list, so their order is the gid's"""
    N, S, n_hits, sk, q, full = b3_design()
    assert np.diff(full[0]).tolist() == n_hits
    for t in range(5):
        g = full[2][int(full[0][t]):int(full[0][t + 1])].tolist()
        assert g.index(65536) + 1 == g.index(65535)
    e = native.Engine(K=31, S=S, W=8, H=3, min_score_value=MS)
    e.insert(sk)
    e.build()
    assert e.stat("tiles") >= 2
    both_forms(e, q, full, N, (4, 256), (0, 10), "wide")
    e.close()


@functools.lru_cache(maxsize=None)
def b4_design():
    N, S = 3000, 8
    rng = np.random.default_rng(404)
    n_hits = [0, 1, 8, 9, 100, 257, 2049, N]
    C = hd.hit_matrix(n_hits, N, rng, MS)
    sk, q = hd.design(C, S, 8, rng)
    return N, S, n_hits, sk, q, hd.reference_lists(C, MS)


def dealt_types(nq):
    """query i's type: a multiplicative hash of i, the two long lists (2049 and N hits) a sixteenth of the batch each"""
    table = np.array([0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 2, 3, 6, 7])
    i = np.arange(nq, dtype=np.uint64)
    return table[((i * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)]


@pytest.mark.parametrize("nq", [4097, 20489])
def test_batches_beyond_one_scan_block(native, nq):
    """more queries than one workgroup of hitlist_scan_kernel takes (4096): workgroup b > 0 first sums what lies before
    it -- min(n, k) with top-k; at 20 489 queries the sixth workgroup's sum runs the unrolled loop and its remainder"""
    N, S, n_hits, sk, qt, per_type = b4_design()
    types = dealt_types(nq)
    assert len(set(types.tolist())) == 8
    q = np.ascontiguousarray(qt[types])
    full = hd.deal(per_type, types)
    assert np.array_equal(np.diff(full[0]), np.asarray(n_hits)[types])
    e = native.Engine(K=31, S=S, W=8, H=3, min_score_value=MS)
    e.insert(sk)
    e.build()
    for k in (0, 2):
        e.set_option("top_k", k)
        exp = hd.cut_lists(full, k, N)
        e.set_option("hit_lists", 1)
        for cap in (8, 256):
            e.set_option("hit_list_cap", cap)
            query_exact(e, q, exp, nq, "lists", cap, k)
            assert e.stat("last_hits_form") == 1
        e.set_option("hit_lists", 0)
        e.set_option("query_batch", 32768)          # one hit step sees the whole batch
        query_exact(e, q, exp, nq, "rows", k)
        assert e.stat("last_hits_form") == 0
        e.set_option("query_batch", 1024)
    # host call with room up to the middle of the batch: NIQKI_E_CAPACITY, every offset exact
    e.set_option("hit_lists", 1)
    e.set_option("hit_list_cap", 8)
    for k in (0, 2):
        e.set_option("top_k", k)
        exp = hd.cut_lists(full, k, N)
        capacity = int(exp[0][nq // 2]) + 1
        off = np.zeros(nq + 1, np.uint64)
        hc, hg = np.empty(capacity, np.uint32), np.empty(capacity, np.uint32)
        rc = e.L.niqki_query(e.h, q.ctypes.data, nq, off.ctypes.data, hc.ctypes.data, hg.ctypes.data, capacity, native.capi.MEM_HOST)
        assert rc == E_CAPACITY, (k, rc)
        assert np.array_equal(off.astype(np.int64), exp[0]), k
    e.close()
