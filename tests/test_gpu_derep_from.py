"""GPU: niqki_dereplicate_from, the dereplication that takes the genomes below `first` as given.
  0. every genome g < first is a representative, whatever it is linked to;
  1. a genome t >= first is a representative iff no representative g < t, given or new, is linked to t;
  2. for t >= first: labels[t] = t, or the linked representative with the largest count, ties to the smallest id (later
     ones count too); for g < first: labels[g] = g, label_counts[g] = 0.
The expectation is that text restated in plain Python over the matrix_range counts (exact at S = 8), never the call
under test; the data is designed so that each rule decides something, and the expectation is checked for that first.
S=8, 200 genomes, tiles of 64 genomes and query_batch=64: first = 70 lies mid-tile, the batches start there."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, S, W, H, MS, TOP = 21, 8, 8, 4, 40, 2
F = 1 << S
N, FIRST, THR = 200, 70, 110
E_INVALID = 1


def different(rng, *others):
    """a sketch that differs from each of `others` in every cell"""
    s = rng.integers(0, 1 << W, F).astype(np.int32)
    for _ in range(64):
        clash = np.zeros(F, bool)
        for o in others:
            clash |= s == o
        if not clash.any():
            return s
        s[clash] = rng.integers(0, 1 << W, int(clash.sum()))
    raise AssertionError("no such sketch")


def mix(rng, parts):
    """cells [a, b) of `src` for each (src, a, b) of parts, every other cell different from all the sources"""
    s = different(rng, *[p[0] for p in parts])
    for src, a, b in parts:
        s[a:b] = src[a:b]
    return s


def designed():
    rng = np.random.default_rng(70)
    sk = rng.integers(0, 1 << W, (N, F)).astype(np.int32)                  # unrelated genomes: about one cell in common
    # given genomes linked among themselves: all of them stay
    for g in (10, 40):
        sk[g] = mix(rng, [(sk[3], 0, 200)])
    # a new genome linked to a given one
    sk[80] = mix(rng, [(sk[10], 0, 130)])
    # a given representative (20) against a later new one (150) with the larger count
    sk[150] = different(rng, sk[20])
    sk[90] = mix(rng, [(sk[20], 0, 115), (sk[150], 115, 250)])
    # ... and with the same count: the smaller id
    sk[151] = different(rng, sk[21], sk[150], sk[20])
    sk[91] = mix(rng, [(sk[21], 0, 120), (sk[151], 120, 240)])
    # a chain of new genomes in index order across the batch boundary at 70 + 64: neighbours share 154 cells, genomes
    # two apart 92
    for t in range(130, 140):
        m = rng.choice(F, 102, replace=False)
        sk[t] = sk[t - 1]
        sk[t, m] = different(rng, sk[t - 1])[m]
    # two new duplicates of each other, and a new genome linked to a covered one only (80's own cells)
    sk[160] = sk[100]
    sk[170] = mix(rng, [(sk[80], 130, 256)])
    sk[11] = -1                                                            # an all-empty given sketch
    return sk


def derep_from(M, first, thr):
    """rules 0-2, word for word: (labels, label_counts)"""
    n = M.shape[0]
    first = min(first, n)
    linked = lambda a, b: a != b and M[a, b] >= thr
    rep = [g < first for g in range(n)]
    for t in range(first, n):
        rep[t] = not any(rep[g] and linked(t, g) for g in range(t))
    labels, counts = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)
    for t in range(first, n):
        if rep[t]:
            continue
        offers = [(-int(M[t, r]), r) for r in range(n) if rep[r] and linked(t, r)]
        assert offers                                                      # rule 1: one exists
        c, r = min(offers)
        labels[t], counts[t] = r, -c
    return labels, counts


def engine(native, sk):
    e = native.Engine(K=K, S=S, W=W, H=H, min_score_value=MS, tile_genomes=64, top_k=TOP)
    e.set_option("query_batch", 64)
    e.insert(sk)
    return e


@pytest.fixture(scope="module")
def world(native):
    sk = designed()
    e = engine(native, sk)
    M = e.matrix_range(0, N).astype(np.int64)
    assert np.array_equal(M, M.T) and e.stat("tiles") > 1
    e.close()
    exp = derep_from(M, FIRST, THR)
    lab, cnt = exp
    ids = np.arange(N)
    # what the design must show in the EXPECTATION, whatever the device does
    assert M[3, 10] >= THR and M[3, 40] >= THR and np.array_equal(lab[:FIRST], ids[:FIRST]) and not cnt[:FIRST].any()
    assert lab[80] in (3, 10, 40) and cnt[80] == M[80, lab[80]] >= 130
    assert THR <= M[90, 20] < M[90, 150] and lab[150] == 150 and lab[90] == 150 and cnt[90] == M[90, 150]
    assert M[91, 21] == M[91, 151] >= THR and lab[151] == 151 and lab[91] == 21
    chain = lab[129:140]
    assert [int(x) for x in chain] == [129, 129, 131, 131, 133, 133, 135, 135, 137, 137, 139]    # across 134, a batch's first
    assert lab[160] == 100 and cnt[160] == F
    assert M[170, 80] >= THR and lab[80] != 80 and lab[170] == 170        # 80 is covered: it covers nothing
    assert lab[11] == 11
    plain = derep_from(M, 0, THR)
    assert lab[40] == 40 and plain[0][40] == 3 and plain[0][10] == 3      # rule 0 is what keeps them
    return sk, M, exp


def check(e, first, thr, exp):
    labels, lc, n = e.dereplicate_from(first, thr, counts=True)
    assert labels.dtype == np.uint32 and lc.dtype == np.uint32
    assert np.array_equal(labels, exp[0]) and np.array_equal(lc, exp[1]), (first, thr)
    assert n == int(np.sum(exp[0] == np.arange(exp[0].size)))
    l2, n2 = e.dereplicate_from(first, thr)
    assert np.array_equal(l2, labels) and n2 == n


def test_given_genomes_at_a_first_that_is_mid_tile(native, world):
    sk, M, exp = world
    e = engine(native, sk)
    check(e, FIRST, THR, exp)
    assert e.stat("derep_rounds") >= 1
    e.close()


@pytest.mark.parametrize("thr", [0, 1, THR, F + 1])
def test_first_0_is_dereplicate(native, world, thr):
    sk, M, _ = world
    e = engine(native, sk)
    a = e.dereplicate(thr, counts=True)
    b = e.dereplicate_from(0, thr, counts=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    exp = derep_from(M, 0, thr)
    assert np.array_equal(b[0], exp[0]) and np.array_equal(b[1], exp[1])
    e.close()


@pytest.mark.parametrize("first", [N, N + 1, 0xFFFFFFFF])
def test_first_at_or_past_the_genome_count(native, world, first):
    sk, M, _ = world
    e = engine(native, sk)
    labels, lc, n = e.dereplicate_from(first, 1, counts=True)
    assert np.array_equal(labels, np.arange(N)) and not lc.any() and n == N
    e.close()


@pytest.mark.parametrize("first,thr", [(1, THR), (64, THR), (128, THR), (134, THR), (199, THR), (FIRST, 0), (FIRST, 1), (FIRST, 150),
                                       (FIRST, F + 1)])
def test_other_firsts_and_thresholds(native, world, first, thr):
    sk, M, _ = world
    e = engine(native, sk)
    check(e, first, thr, derep_from(M, first, thr))
    e.close()


def test_device_memory_and_the_handles_own_threshold(native, world):
    import torch
    from niqki_amd import capi
    sk, M, exp = world
    e = engine(native, sk)
    q = sk[[3, 80, 90, 150]]
    before = e.query(q)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d = torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    dc = torch.full((N,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    n = C.c_uint32(0)
    assert e.L.niqki_dereplicate_from(e.h, FIRST, THR, d.data_ptr(), dc.data_ptr(), C.byref(n), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint32), exp[0]) and np.array_equal(dc.cpu().numpy().astype(np.uint32), exp[1])
    assert n.value == int(np.sum(exp[0] == np.arange(N)))
    d.fill_(0x7FFFFFFF)
    assert e.L.niqki_dereplicate_from(e.h, FIRST, THR, d.data_ptr(), None, None, 1) == 0      # both may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint32), exp[0])
    d.fill_(0x7FFFFFFF)
    assert e.L.niqki_dereplicate_from(e.h, N, THR, d.data_ptr(), dc.data_ptr(), C.byref(n), 1) == 0   # nothing launched
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), np.arange(N)) and int(dc.abs().max().item()) == 0 and n.value == N

    def params():
        p = capi.Params()
        assert e.L.niqki_get_params(e.h, C.byref(p)) == 0
        return p.min_score, p.top_k
    assert params() == (MS, TOP)
    assert e.L.niqki_dereplicate_from(e.h, FIRST, THR, None, None, None, 0) == E_INVALID      # a failing call
    assert params() == (MS, TOP)
    after = e.query(q)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    e.close()
