"""GPU: the kernels against what the REAL reference produced -- the recorded sweep of oracle/make_goldens_sweep.py
(tests/golden/reference_sweep.*: designed rows at the edges of K, S, W, H, J and -G, then seeded random cases), not
against the oracle -- and, where the reference's value is undefined (get_fingerprint(0) at H >= 7: bsr on 0), against
the oracle, by decision: both count 64 leading zeros there."""
import hashlib

import numpy as np
import pytest

import reference_sweep_worker as rsw

pytestmark = pytest.mark.gpu

GROUP = 10
_vec, _meta = rsw.load_sweep()
N_CASES = len(_meta["cases"])


def length_class(n):
    """Batches of one class take one shape of the sketch launch rule (nq_sketch_plan.h): the one-wavefront kernel with its 192- or 384-entry list,
    the 256-thread workgroup kernel, 1024 threads with 128 or 512 k-mers per lane."""
    return 0 if n <= 200 else 1 if n <= 415 else 2 if n < 16384 else 3 if n < (1 << 18) else 4


@pytest.mark.parametrize("first", range(0, N_CASES, GROUP))
def test_kernels_reproduce_the_recorded_sweep(native, po, first):
    vec, meta = _vec, _meta
    for i in range(first, min(first + GROUP, N_CASES)):
        m = meta["cases"][i]
        tag = rsw.case_tag(i, m)
        recs = rsw.sweep_records(native, po, vec, m)
        e = native.Engine(K=m["K"], S=m["S"], W=m["W"], H=m["H"], J=m["J"])
        try:
            assert e.min_score == m["min_score"], tag
            if m["G"]:
                assert e.select_best_H(m["G"]) == m["H_final"], tag
            sk = np.empty((len(recs), 1 << m["S"]), np.int32)
            for cls in sorted({length_class(s.size) for s in recs}):
                idx = [j for j, s in enumerate(recs) if length_class(s.size) == cls]
                sk[idx] = e.sketch([recs[j] for j in idx])
            rsw.check_sketches(po, vec, i, m, sk, tag)
            e.insert(sk)
            off, hc, hg = e.query(sk)
            for q in range(len(recs)):
                ec, eg = rsw.recorded_hits(vec, m, q)
                lo, hi = int(off[q]), int(off[q + 1])
                assert np.array_equal(hc[lo:hi], ec) and np.array_equal(hg[lo:hi], eg), (tag, "query", q)
            raw = bytes(e.export_dump()) + rsw.dump_names(len(recs))
            assert len(raw) == m["dump_len"] and hashlib.md5(raw).hexdigest() == m["dump_md5"], tag
        finally:
            e.close()


def zero_hash_records(rng, K, L):
    """Records of L bases that DO hold k-mers whose canonical word is 0 (their hash is 0: get_fingerprint(0)), plus a
    relative of the first one so that queries have hits to order."""
    a = rsw.clean(rng, L)
    n = min(L, K + 3)
    at = int(rng.integers(0, L - n + 1))
    a[at:at + n] = ord("A")                                   # A x (K + 3): four k-mers of A x K
    b = rsw.clean(rng, L)
    b[int(rng.integers(0, K - 1))] = ord("N")                 # a foreign byte inside the first K-1 bases: prefix zeroed
    if L > 3 * K:
        b[L // 2:L // 2 + K + 2] = ord("n")                   # ... and a run of >= K foreign bytes
    c = rsw.clean(rng, L)
    c[L - n:] = ord("T")                                      # T x K: the reverse complement is A x K
    if L > 3 * K:
        c[K + 5:2 * K + 7] |= 0x20                            # lower case past the prefix
    d = rsw.mutate(rng, a, 0.02)
    recs = [a, b, c, d]
    if L <= 64:
        recs.append(np.full(L, ord("A"), np.uint8))           # nothing but the zero word: no pass fills the other cells
    return recs


@pytest.mark.parametrize("K", [15, 31])
@pytest.mark.parametrize("S", [4, 10])
@pytest.mark.parametrize("W,H", [(7, 7), (12, 9), (15, 15), (14, 7)])
def test_zero_hash_kmers_at_h7_and_above_vs_oracle(native, po, W, H, S, K):
    """2^H - 1 > 64: the fingerprint of hash 0 is no longer 0 but (2^H - 1 - 64) << M -- 64 leading zeros, one more than
    any other hash has, so still the smallest value of its cell (what the long-record path's candidate filter, which
    orders by leading zeros, relies on at max_rem > 64).  Sketches (cells the passes cannot fill stay -1, as in the
    oracle), counters, hits, dump."""
    rng = np.random.default_rng(1000 * W + 100 * H + 10 * S + K)
    p = po.make_params(K, S, W, H, 0.05)
    e = native.Engine(K=K, S=S, W=W, H=H, J=0.05)
    try:
        recs, sks = [], []
        for L in (40, 150, 1000, 20000):
            batch = zero_hash_records(rng, K, L)
            assert all(rsw.depends_on_bsr0(K, s) for s in batch[:3])
            got = e.sketch(batch)                                 # one launch form per length
            for s, g in zip(batch, got):
                exp = po.densify(p, po.sketch_accumulate(p, s))[0]
                assert np.array_equal(g, exp), (K, S, W, H, L, len(recs))
                recs.append(s)
                sks.append(exp)
        sk = np.stack(sks)
        zero_fp = po.fingerprint(0, W, H)
        assert zero_fp == ((1 << H) - 1 - 64) << (W - H) and (sk == zero_fp).any()
        e.insert(sk)
        ix = po.Index(p, sk)
        cnt = e.query_counts(sk)
        off, hc, hg = e.query(sk)
        for q in range(len(recs)):
            assert np.array_equal(cnt[q].astype(np.uint32), ix.counts(sk[q])), (K, S, W, H, q)
            ec, eg = ix.query(sk[q])
            lo, hi = int(off[q]), int(off[q + 1])
            assert np.array_equal(hc[lo:hi], ec) and np.array_equal(hg[lo:hi], eg), (K, S, W, H, q)
        assert bytes(e.export_dump()) == ix.dump_bytes()
    finally:
        e.close()
