"""GPU: niqki_registers, niqki_sketch_registers and niqki_staged_registers count the HyperLogLog registers in the top H
bits of sketch cells.  Sketches are inserted as designed cells, not sketched from sequences, and the expected histograms
are tests/registers_ref.py's over what niqki_get_sketches returns (over the cells given, for the query-side calls) --
equal word for word: nothing on the device is floating point.  Shapes: one genome, one short of / exactly / one more
than a wavefront's 64 columns, several wavefronts; ranges that start and end inside a column group; S = 16 with all
65 536 cells of a genome in one bin (a 16-bit counter would wrap) and, there, rows and sketches cut into chunks."""
import ctypes as C

import numpy as np
import pytest

import registers_ref as rr

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = 1, 5
K, S, W = 31, 8, 10
F = 1 << S
RANGES = [(0, 0), (5, 70), (64, 65)]


def designed(n, f, w, seed):
    """cells over the whole fingerprint range, some empty; genome 0 holds only the largest and the smallest valid cell"""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 1 << w, (n, f)).astype(np.int32)
    sk[rng.random(sk.shape) < 0.05] = -1
    sk[0, ::2], sk[0, 1::2] = (1 << w) - 1, 0
    return sk


def make(native, sk, H, s=S, w=W, **kw):
    e = native.Engine(K=K, S=s, W=w, H=H, min_score_value=20, **kw)
    e.insert(sk)
    return e


def ranges(n):
    return [(0, n), (n, n)] + [(b, e) for b, e in RANGES if e <= n]


def check_all_ranges(e, H, w=W):
    """both memory spaces over every range against the reference over niqki_get_sketches"""
    import torch
    n, B = e.n_genomes, rr.bins(H)
    want = rr.hist_ref(e.get_sketches(0, n), w, H) if n else np.zeros((0, B), np.uint32)
    assert (want.sum(axis=1) == e.F).all()
    for b, en in ranges(n):
        got = e.registers(b, en)
        assert got.dtype == np.uint32 and got.shape == (en - b, B)
        assert np.array_equal(got, want[b:en]), (b, en)
        d = torch.full(((en - b) * B + 1,), -7, dtype=torch.int32, device="cuda")      # (not preset, one word of margin)
        torch.cuda.synchronize()                  # (the engine writes on a stream of its own)
        e.registers_dev(d, b, en)
        torch.cuda.synchronize()
        h = d.cpu().numpy()
        assert h[-1] == -7 and np.array_equal(h[:-1].view(np.uint32).reshape(en - b, B), want[b:en]), (b, en)
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("H", [0, 1, 4, 6])
def test_store_pass_on_designed_cells(native, H, n):
    e = make(native, designed(n, F, W, 10 * H + n), H)
    want = check_all_ranges(e, H)
    assert want[0, (1 << H) - 1] + want[0, 0] == F or H == 0
    e.close()


def test_sixteen_bit_counters_would_wrap(native):
    s, w, H, n = 16, 12, 4, 65
    sk = designed(n, 1 << s, w, 16)
    sk[3, :] = (5 << (w - H)) + 17                # all 65 536 cells of genome 3 in bin 5
    sk[64, :] = -1                                # genome 64: all empty
    e = make(native, sk, H, s=s, w=w)
    want = check_all_ranges(e, H, w)
    assert want[3, 5] == 1 << s and want[64, 1 << H] == 1 << s
    # the row pass at the same shape: every sketch is cut into chunks, and cells that are not valid stay what they are
    q = sk[[3, 64, 0, 7]].copy()
    q[3, ::7] = 1 << w
    q[3, 1::7] = np.iinfo(np.int32).min
    assert np.array_equal(e.sketch_registers(q), rr.hist_ref(q, w, H))
    e.close()


@pytest.mark.parametrize("form", ["paged", "two_tiles", "delta"])
def test_the_index_form_does_not_matter(native, form):
    H = 4
    n = 4196 if form == "delta" else 200
    sk = designed(n, F, W, 5)
    plain = make(native, sk, H)
    want = plain.registers()
    plain.close()
    assert np.array_equal(want, rr.hist_ref(sk, W, H))
    if form == "delta":
        e = make(native, sk[:4096], H)
        e.query(sk[:2])
        e.insert(sk[4096:])
        e.query(sk[:2])
        assert e.stat("delta_genomes") == 100
    else:
        e = make(native, sk, H, **({"resident_mib": 1} if form == "paged" else {"tile_genomes": 64}))
        e.query(sk[:2])                           # the index is built (paged: a page is resident)
        if form == "two_tiles":
            assert e.stat("tiles") >= 2
    assert np.array_equal(check_all_ranges(e, H), want)
    e.close()


@pytest.mark.parametrize("paged", [False, True])
def test_after_retain_and_unite(native, paged):
    H, n = 4, 200
    sk = designed(n, F, W, 6)
    e = make(native, sk, H, **({"resident_mib": 1} if paged else {}))
    keep = (np.arange(n) % 3 != 1).astype(np.uint8)
    e.retain(keep)
    assert np.array_equal(check_all_ranges(e, H), rr.hist_ref(sk[keep != 0], W, H))
    e.unite(np.arange(e.n_genomes) // 4)
    assert e.n_genomes == 34
    check_all_ranges(e, H)
    e.insert(sk[:70])                             # ... and genomes behind the united ones
    check_all_ranges(e, H)
    e.close()


def test_empty_index(native):
    e = native.Engine(K=K, S=S, W=W, H=4, min_score_value=20)
    assert e.registers().shape == (0, 17)
    d = np.full(4, 9, np.uint32)
    assert e.L.niqki_registers(e.h, 0, 0, d.ctypes.data, 0) == 0 and (d == 9).all()
    assert e.L.niqki_registers(e.h, 0, 0, None, 0) == 0
    e.close()


@pytest.mark.parametrize("n", [0, 1, 257])
def test_sketch_registers(native, n):
    import torch
    H = 4
    e = native.Engine(K=K, S=S, W=W, H=H, min_score_value=20)
    q = designed(max(n, 1), F, W, n)[:n]
    if n:
        q[-1, :9] = [-1, -2, np.iinfo(np.int32).min, 1 << W, (1 << W) + 1, np.iinfo(np.int32).max, (1 << W) - 1, 0, 1 << 16]
    want = rr.hist_ref(q, W, H) if n else np.zeros((0, 17), np.uint32)
    got = e.sketch_registers(q)
    assert got.shape == (n, 17) and np.array_equal(got, want)
    d = torch.full((n * 17 + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if n:
        dq = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        e.registers_dev(d, sketches=dq, n=n)
    else:
        assert e.L.niqki_sketch_registers(e.h, None, 0, d.data_ptr(), 1) == 0
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert h[-1] == -7 and np.array_equal(h[:-1].view(np.uint32).reshape(n, 17), want)
    e.close()


def test_staged_registers(native):
    import torch
    H = 4
    rng = np.random.default_rng(8)
    sk = designed(100, F, W, 8)
    e = make(native, sk, H)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)] for ln in (3000, 40, 500, 31, 12000, 3000)]
    files = [b">q%d\n" % i + bytes(s) + b"\n" for i, s in enumerate(seqs)]
    e.stage_raw(files, None)
    before = e.staged_query()
    staged = e.staged_sketch()
    got = e.staged_registers()
    assert got.shape == (len(files), 17)
    assert np.array_equal(got, e.sketch_registers(staged)) and np.array_equal(got, rr.hist_ref(staged, W, H))
    d = torch.full((len(files) * 17,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.registers_dev(d, staged=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32).reshape(-1, 17), got)
    after = e.staged_query()                      # the batch is still usable and answers as before
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(e.staged_sketch(), staged)
    e.close()


def refused(native, e, code, call=None):
    d = np.full(8 * 129, 9, np.uint32)
    rc = (call or (lambda: e.L.niqki_registers(e.h, 0, min(e.n_genomes, 8), d.ctypes.data, 0)))()
    assert rc == code and e.L.niqki_last_error(e.h).decode() != "" and (d == 9).all()
    return e.L.niqki_last_error(e.h).decode()


def test_refusals(native):
    sk = designed(8, F, W, 1)
    shard = native.Engine(K=K, S=S, W=W, H=4, min_score_value=20, slot_begin=0, slot_end=F // 2)
    shard.insert(sk)
    assert "shard" in refused(native, shard, E_STATE)
    q = np.ascontiguousarray(sk[:2])
    d = np.full(64, 9, np.uint32)
    assert shard.L.niqki_sketch_registers(shard.h, q.ctypes.data, 2, d.ctypes.data, 0) == E_STATE and (d == 9).all()
    shard.close()

    seven = make(native, sk, 7)
    assert "H = 7" in refused(native, seven, E_INVALID)
    assert seven.L.niqki_sketch_registers(seven.h, q.ctypes.data, 2, d.ctypes.data, 0) == E_INVALID
    seven.close()

    for h0 in (2, 6):                             # (one of the two is not what select_best_H picks)
        moved = make(native, sk, h0)
        if moved.select_best_H(1e7) != h0:
            break
        moved.close()
    assert moved.H != h0
    assert "niqki_select_best_H" in refused(native, moved, E_STATE)
    assert moved.L.niqki_sketch_registers(moved.h, q.ctypes.data, 2, d.ctypes.data, 0) == E_STATE and (d == 9).all()
    moved.close()

    e = make(native, sk, 4)
    refused(native, e, E_INVALID, lambda: e.L.niqki_registers(e.h, 5, 4, d.ctypes.data, 0))
    refused(native, e, E_INVALID, lambda: e.L.niqki_registers(e.h, 0, 9, d.ctypes.data, 0))
    assert e.L.niqki_registers(e.h, 0, 8, None, 0) == E_INVALID
    assert e.L.niqki_staged_registers(e.h, d.ctypes.data, 0) == E_STATE      # nothing is staged
    assert e.L.niqki_registers(None, 0, 0, d.ctypes.data, 0) == E_INVALID
    assert (d == 9).all()
    e.close()


def test_stats(native):
    e = native.Engine(K=K, S=S, W=W, H=4, min_score_value=20)
    v = C.c_uint64(0)
    for key in ("registers_us_store", "registers_us_rows"):
        v.value = 0xDEAD
        assert e.L.niqki_get_stat(e.h, key.encode(), C.byref(v)) == 0 and v.value == 0, key
    sk = designed(4196, F, W, 2)
    e.insert(sk)
    e.registers()
    e.sketch_registers(sk)
    assert e.stat("registers_us_store") == 0 and e.stat("registers_us_rows") == 0      # profiling is off
    e.profile(True)
    e.registers()
    assert e.stat("registers_us_store") > 0 and e.stat("registers_us_rows") == 0
    e.sketch_registers(sk)
    assert e.stat("registers_us_rows") > 0
    e.close()
