"""GPU: niqki_neighbors_range, the sparse self-join: the hits of the STORED sketches of genomes [begin, end).  Its
definition is niqki_query on the output of niqki_get_sketches, so every shape is compared byte for byte with exactly
that (offsets, counts, gids); one shape is also compared with the oracle directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY, E_STATE = 1, 4, 5


def data(S, W, N, seed, dup=8):
    """Families of sketches with noise, `dup` exact copies of genome 7 (ties) and an all-empty genome."""
    rng = np.random.default_rng(seed)
    F = 1 << S
    fam = rng.integers(0, 1 << W, (20, F)).astype(np.int32)
    sk = fam[rng.integers(0, 20, N)].copy()
    noise = rng.random((N, F)) < 0.35
    sk[noise] = rng.integers(0, 1 << W, int(noise.sum()))
    sk[rng.random((N, F)) < 0.01] = -1
    for i in range(dup):
        sk[N // 2 + 37 * i] = sk[7]
    sk[11] = -1
    return sk


def same(got, exp):
    for name, a, b in zip(("offsets", "counts", "gids"), got, exp):
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def raw(e, begin, end, cap):
    """niqki_neighbors_range with exactly `cap` entries of room: (status, off, hc, hg)"""
    off = np.zeros(max(end - begin, 0) + 1, np.uint64)
    hc, hg = np.empty(max(cap, 1), np.uint32), np.empty(max(cap, 1), np.uint32)
    rc = e.L.niqki_neighbors_range(e.h, begin, end, off.ctypes.data, hc.ctypes.data, hg.ctypes.data, cap, 0)
    return rc, off, hc, hg


FORMS = ["lists", "rows", "lists_cap8", "tiles", "paged"]


def engine(native, form, S, W, ms, top_k=0):
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=ms, top_k=top_k,
                      tile_genomes=512 if form == "tiles" else 0, resident_mib=4 if form == "paged" else 0)
    if form == "rows":
        e.set_option("hit_lists", 0)
    if form == "lists_cap8":
        e.set_option("hit_list_cap", 8)
    return e


@pytest.mark.parametrize("ms", [0, 90, 300])
@pytest.mark.parametrize("form", FORMS)
def test_neighbors_equal_query_of_the_stored_sketches(native, form, ms):
    S, W, N = 10, 8, 3000
    sk = data(S, W, N, 5)
    e = engine(native, form, S, W, ms)
    e.set_option("query_batch", 256)
    e.insert(sk)
    if form == "paged":
        assert e.stat("pages") >= 4
    # ranges that start and end inside a batch, whole batches, one genome, the empty range
    for k in (0, 1, 10, N + 5):
        e.set_option("top_k", k)
        for b, t in ((0, 300), (100, 700), (255, 257), (2990, N), (7, 8), (40, 40), (N, N)):
            same(e.neighbors_range(b, t), e.query(e.get_sketches(b, t - b)))
        rc, off, _, _ = raw(e, 100, 700, 600 * k)
        assert k == 0 or rc == 0, k                        # capacity n x k is always enough under top_k = k
    e.set_option("top_k", 0)
    if form == "tiles":
        assert e.stat("tiles") > 1
    if form in ("lists", "lists_cap8"):
        assert e.stat("last_hits_form") == 1
    # the stored sketch of a genome finds the genome itself, with the number of its valid cells
    off, hc, hg = e.neighbors_range(0, 20)
    for t in range(20):
        valid = int(np.sum(sk[t] >= 0))
        g = hg[int(off[t]):int(off[t + 1])]
        c = hc[int(off[t]):int(off[t + 1])]
        assert (valid >= ms) == bool(np.any(g == t))
        if valid >= ms:
            assert int(c[g == t][0]) == valid
    for b, t in ((5, 4), (0, N + 1), (N + 1, N + 1)):
        rc, _, _, _ = raw(e, b, t, 16)
        assert rc == E_INVALID, (b, t)
    e.close()


def test_neighbors_equal_the_oracle(native, po):
    S, W, N, MS = 10, 8, 3000, 90
    sk = data(S, W, N, 9)
    p = po.make_params(31, S, W, 3, 0.0)
    p.min_score = MS
    ox = po.Index(p, sk)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=MS)
    e.insert(sk)
    b, t = 1480, 1560                                       # holds copies of genome 7: ties
    off, hc, hg = e.neighbors_range(b, t)
    assert int(off[-1]) > (t - b)
    for i in range(t - b):
        ehc, ehg = ox.query(sk[b + i], min_score=MS)
        lo, hi = int(off[i]), int(off[i + 1])
        assert np.array_equal(hc[lo:hi], ehc) and np.array_equal(hg[lo:hi], ehg), i
    e.close()


@pytest.mark.parametrize("form", ["lists", "rows"])
def test_neighbors_capacity_protocol(native, form):
    S, W, N, MS = 10, 8, 3000, 90
    sk = data(S, W, N, 6)
    e = engine(native, form, S, W, MS)
    e.set_option("query_batch", 128)                       # several batches: the total is reported over all of them
    e.insert(sk)
    exp = e.query(e.get_sketches(50, 450))
    total = int(exp[0][-1])
    assert total > 4000
    for cap in (0, 1, total // 3, total - 1):
        rc, off, _, _ = raw(e, 50, 500, cap)
        assert rc == E_CAPACITY and np.array_equal(off, exp[0]), cap
    rc, off, hc, hg = raw(e, 50, 500, total)
    assert rc == 0
    same((off, hc[:total], hg[:total]), exp)
    e.close()


def test_neighbors_refuse_a_slot_range_shard(native):
    S, W = 10, 8
    sk = data(S, W, 200, 2, dup=2)
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=10, slot_begin=0, slot_end=512)
    e.insert(sk)
    rc, _, _, _ = raw(e, 0, 10, 1 << 16)
    assert rc == E_STATE
    assert b"slot-range" in e.L.niqki_last_error(e.h)
    out = np.zeros(200, np.uint32)
    assert e.L.niqki_cluster(e.h, 100, out.ctypes.data, None, 0) == E_STATE
    e.close()
