"""GPU: niqki_append_* put the genomes of a dump behind those of a live handle.  Definition: a committed append leaves
the handle indistinguishable, through the ABI, from the handle after niqki_insert of the dump's sketches -- so every
expectation here is a FRESH handle into which A's then B's sketches were inserted, never the code under test.  Before
the commit, and after a cancelled or failed append, the handle is the old one: same count, same dump bytes.
K=21, S=8, W=8, small synthetic genomes and tile_genomes=64, so that several tiles and stripes exist."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, S, W, H, MS = 21, 8, 8, 4, 40
F = 1 << S
NA, NB = 70, 130
E_INVALID, E_STATE = 1, 5


def make(native, **kw):
    kw.setdefault("tile_genomes", 64)
    return native.Engine(K=K, S=S, W=W, H=H, min_score_value=MS, **kw)


def filled(native, sk, **kw):
    e = make(native, **kw)
    if sk.shape[0]:
        e.insert(sk)
    return e


@pytest.fixture(scope="module")
def world(native):
    """sketches of 70 + 130 small synthetic genomes (families of mutated members, so that hits and links exist; B holds
    one family of 70 identical genomes: one bucket with more than 64 ids), 32 mixed queries, and the expectation: the
    fresh handle C with A's then B's sketches, read once"""
    e = make(native)
    recs = [native.synth_genome_host(5, i // 6, i % 6, 300 * (i % 6), 3000) for i in range(NA + NB - 69)]
    sk = e.sketch(recs)
    e.close()
    a, b = sk[:NA], np.concatenate([sk[NA:NA + 30], np.repeat(sk[NA + 30:NA + 31], 70, axis=0), sk[NA + 31:]])
    assert b.shape[0] == NB
    rng = np.random.default_rng(2)
    both = np.concatenate([a, b])
    q = np.concatenate([both[rng.choice(NA + NB, 24, replace=False)], rng.integers(0, 1 << W, (8, F)).astype(np.int32)])
    c = filled(native, both)
    exp = dict(n=NA + NB, sk=c.get_sketches(0, NA + NB), dump=c.export_dump(), hits=c.query(q), matrix=c.matrix_range(0, NA + NB))
    c.close()
    hb = filled(native, b)
    dump_b = hb.export_dump()
    hb.close()
    ha = filled(native, a)
    dump_a = ha.export_dump()
    ha.close()
    assert max(struct.unpack_from("<I", dump_b, p)[0] for p in bucket_positions(dump_b)) > 64      # the big bucket
    assert exp["hits"][1].size > 32 and int(exp["matrix"][0, 1]) > 0
    return dict(a=a, b=b, q=q, exp=exp, dump_a=dump_a, dump_b=dump_b)


def bucket_positions(dump):
    """byte position of every bucket's size word"""
    s, w = struct.unpack_from("<I", dump, 0)[0], struct.unpack_from("<I", dump, 12)[0]
    pos, p = [], 24
    for _ in range((1 << s) << w):
        pos.append(p)
        p += 4 + 4 * struct.unpack_from("<I", dump, p)[0]
    assert p == len(dump)
    return pos


def slot_positions(dump):
    s, w = struct.unpack_from("<I", dump, 0)[0], struct.unpack_from("<I", dump, 12)[0]
    return bucket_positions(dump)[::1 << w] + [len(dump)]


def check_parity(e, world):
    exp = world["exp"]
    assert e.n_genomes == exp["n"]
    assert np.array_equal(e.get_sketches(0, exp["n"]), exp["sk"])
    assert e.export_dump() == exp["dump"]
    assert all(np.array_equal(x, y) for x, y in zip(e.query(world["q"]), exp["hits"]))
    assert np.array_equal(e.matrix_range(0, exp["n"]), exp["matrix"])


def stream(e, dump, group):
    pos = slot_positions(dump)
    e.append_begin(dump[:24])
    for s0 in range(0, F, group):
        s1 = min(F, s0 + group)
        assert e.append_slots(s0, s1, dump[pos[s0]:pos[s1]]) == pos[s1] - pos[s0]


# ---- parity ------------------------------------------------------------------------------------------------------

def test_one_shot_append_equals_inserting_the_sketches(native, world):
    e = filled(native, world["a"])
    assert e.append_dump(world["dump_b"] + b"name\n") == len(world["dump_b"])        # consumed: the first name byte
    check_parity(e, world)
    assert e.stat("tiles") > 1
    e.close()


@pytest.mark.parametrize("incremental", [1, 0])
def test_append_to_a_built_and_queried_handle(native, world, incremental):
    e = make(native)
    e.set_option("incremental_build", incremental)
    e.insert(world["a"])
    e.build()
    before = e.query(world["q"])
    assert before[0][-1] > 0
    e.append_dump(world["dump_b"])
    check_parity(e, world)
    e.close()


@pytest.mark.parametrize("group", [1, 37])
def test_streamed_slots_equal_one_shot(native, world, group):
    e = filled(native, world["a"])
    stream(e, world["dump_b"], group)
    check_parity(e, world)
    e.close()


def test_before_the_commit_the_index_is_the_old_one(native, world):
    e = filled(native, world["a"])
    old_dump, old_hits = e.export_dump(), e.query(world["q"])
    dump, pos = world["dump_b"], slot_positions(world["dump_b"])
    e.append_begin(dump[:24])
    e.append_slots(0, 100, dump[pos[0]:pos[100]])
    assert e.n_genomes == NA and e.export_dump() == old_dump
    assert all(np.array_equal(x, y) for x, y in zip(e.query(world["q"]), old_hits))
    for call in (lambda: e.insert(world["b"][:3]), lambda: e.retain(np.ones(NA, bool)), lambda: e.append_begin(dump[:24])):
        with pytest.raises(native.NiqkiError) as ei:
            call()
        assert ei.value.code == E_STATE
    assert e.n_genomes == NA and e.export_dump() == old_dump
    e.append_slots(100, F, dump[pos[100]:pos[F]])                                     # ... and the append goes on
    check_parity(e, world)
    e.close()


def test_append_to_a_paged_handle(native, world):
    e = filled(native, world["a"], resident_mib=1)
    e.query(world["q"][:2])
    assert e.stat("pages") >= 1
    stream(e, world["dump_b"], 37)
    check_parity(e, world)
    e.close()


def test_empty_handles_and_empty_dumps(native, world):
    both = np.concatenate([world["a"], world["b"]])
    c = filled(native, both)
    whole = c.export_dump()
    c.close()
    e = make(native)
    e.append_dump(whole)                                                              # into an empty handle: an import
    imp = native.Engine.import_dump(whole, tile_genomes=64)
    assert e.n_genomes == imp.n_genomes == NA + NB and e.export_dump() == imp.export_dump() == whole
    assert np.array_equal(e.get_sketches(0, NA + NB), imp.get_sketches(0, NA + NB))
    imp.close()
    e.close()
    empty = make(native)
    nothing = empty.export_dump()
    empty.close()
    assert struct.unpack_from("<6I", nothing, 0)[5] == 0
    e = filled(native, world["a"])
    old = e.export_dump()
    assert e.append_dump(nothing) == len(nothing)                                     # N_B = 0 commits at once
    assert e.n_genomes == NA and e.export_dump() == old
    e.append_begin(nothing[:24])
    e.insert(world["b"])                                                              # nothing is pending
    check_parity(e, world)
    e.close()


# ---- failures ----------------------------------------------------------------------------------------------------

def patched(dump, word, value):
    return dump[:4 * word] + struct.pack("<I", value) + dump[4 * word + 4:]


def failing_appends(dump):
    """(name, the call on an engine, expected status, a word of the error text)"""
    pos, bpos = slot_positions(dump), bucket_positions(dump)
    hdr = struct.unpack_from("<6I", dump, 0)
    cases = [(name, (lambda e, d=patched(dump, word, hdr[word] + 1): e.append_dump(d)), E_INVALID, "dump's %s " % name)
             for name, word in (("lF", 0), ("K", 1), ("H", 2), ("W", 3))]
    cut = (pos[150] + pos[151]) // 2 // 4 * 4                                         # inside slot 150
    assert pos[150] < cut < pos[151]
    cases.append(("cut", lambda e: e.append_dump(dump[:cut]), E_INVALID, "truncated"))

    def cut_streamed(e):
        e.append_begin(dump[:24])
        e.append_slots(0, 150, dump[pos[0]:pos[150]])
        e.append_slots(150, 151, dump[pos[150]:cut])
    cases.append(("cut-streamed", cut_streamed, E_INVALID, "ends inside"))
    at = next(p for p in bpos if p >= pos[200] and struct.unpack_from("<I", dump, p)[0] > 0)
    bad_id = patched(dump, at // 4 + 1, hdr[5])                                       # an id == N_B, late in the payload
    cases.append(("id", lambda e: e.append_dump(bad_id), E_INVALID, "genome ids"))

    def out_of_order(e):
        e.append_begin(dump[:24])
        e.append_slots(0, 10, dump[pos[0]:pos[10]])
        e.append_slots(20, 30, dump[pos[20]:pos[30]])
    cases.append(("order", out_of_order, E_INVALID, "order"))
    return cases


CASES = ["lF", "K", "H", "W", "cut", "cut-streamed", "id", "order", "cancel"]


@pytest.mark.parametrize("case", CASES)
def test_a_failed_or_cancelled_append_changes_nothing(native, world, case):
    dump, pos = world["dump_b"], slot_positions(world["dump_b"])
    e = filled(native, world["a"])
    hits_a = e.query(world["q"])                                                      # the index is built
    index_bytes = e.stat("index_bytes")
    assert index_bytes > 0
    if case == "cancel":
        e.append_begin(dump[:24])
        e.append_slots(0, 128, dump[pos[0]:pos[128]])
        e.append_cancel()
    else:
        name, call, code, word = next(c for c in failing_appends(dump) if c[0] == case)
        with pytest.raises(native.NiqkiError) as ei:
            call(e)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
    assert e.n_genomes == NA and e.stat("index_bytes") == index_bytes                 # same count, still built
    assert all(np.array_equal(x, y) for x, y in zip(e.query(world["q"]), hits_a))
    assert e.export_dump() == world["dump_a"]
    with pytest.raises(native.NiqkiError) as ei:                                      # nothing is pending any more
        e.append_slots(0, 1, dump[pos[0]:pos[1]])
    assert ei.value.code == E_STATE
    e.append_cancel()                                                                 # (fine with nothing pending)
    e.append_dump(dump)                                                               # usable afterwards
    check_parity(e, world)
    e.close()


def test_a_slot_range_shard_refuses(native, world):
    e = make(native, slot_begin=0, slot_end=F // 2)
    e.insert(world["a"])
    with pytest.raises(native.NiqkiError) as ei:
        e.append_dump(world["dump_b"])
    assert ei.value.code == E_STATE and e.n_genomes == NA
    e.close()


def test_append_at_s16(native):
    s16, w4, na, nb = 16, 4, 20, 30
    rng = np.random.default_rng(16)
    base = rng.integers(0, 1 << w4, (3, 1 << s16)).astype(np.int32)
    sk = base[rng.integers(0, 3, na + nb)].copy()
    noise = rng.random(sk.shape) < 0.3
    sk[noise] = rng.integers(0, 1 << w4, int(noise.sum()))
    sk[rng.random(sk.shape) < 0.01] = -1

    def mk():
        return native.Engine(K=K, S=s16, W=w4, H=2, min_score_value=30000)
    b = mk()
    b.insert(sk[na:])
    dump_b = b.export_dump()
    b.close()
    c = mk()
    c.insert(sk)
    e = mk()
    e.insert(sk[:na])
    e.query(sk[:2])
    e.append_dump(dump_b)
    assert e.n_genomes == na + nb and np.array_equal(e.get_sketches(0, na + nb), sk)
    assert e.export_dump() == c.export_dump()
    assert all(np.array_equal(x, y) for x, y in zip(e.query(sk[::7]), c.query(sk[::7])))
    c.close()
    e.close()
