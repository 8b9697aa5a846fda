"""CPU: the oracle (oracle/niqki_oracle.c) against the REAL reference across the parameter space -- K 1..31, S, W up to
15, H up to W, J, -G -- where tests/test_oracle_golden.py pins it at a handful of points: a recorded sweep
(oracle/make_goldens_sweep.py -> tests/golden/reference_sweep.*) and, where oracle/_ref has been built, a live
campaign against the reference in a child process (tests/reference_sweep_worker.py).

Two corners are the reference's own and stay out of both: records on which it never returns (the oracle predicts
them: at most 15 % of the generated records, asserted; the prediction's other direction has a test below), and
get_fingerprint(0) where the constructor's H is >= 7 -- bsr on 0, undefined; those cases hold records without a
canonical word of 0 only, and the oracle's own value there (lz = 64) is pinned by a test of its own."""
import hashlib
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

import reference_sweep_worker as rsw

@pytest.fixture(scope="module")
def sweep():
    return rsw.load_sweep()


def test_sweep_fixture_shape(sweep):
    """What the issue sets for the recorded sweep: 120..200 cases, the designed rows, at most 15 % of the generated
    records left out, nothing at H >= 7 that could reach get_fingerprint(0)."""
    vec, meta = sweep
    cases = meta["cases"]
    assert 120 <= len(cases) <= 200
    assert meta["records_left_out"] <= rsw.MAX_LEFT_OUT * meta["records_generated"]
    # (the records of a random case that lost all of them count as generated and left out; the case itself is not recorded)
    assert meta["records_generated"] - meta["records_left_out"] == sum(len(m["records"]) for m in cases)
    assert {1, 2, 3, 15, 16, 17, 30, 31} <= {m["K"] for m in cases}
    assert {1, 2, 13, 14, 15} <= {m["W"] for m in cases} and {1, 2, 3, 10} <= {m["S"] for m in cases}
    for W in (1, 2, 13, 14, 15):
        assert {0, 1, W - 1, W} <= {m["H"] for m in cases if m["W"] == W}, W
    assert {7, 8, 11, 15} <= {m["H"] for m in cases}
    assert {0.0, 0.1, 0.33, 0.9} <= {m["J"] for m in cases} and {0.0, 3.0, 150.0, 1e4, 5e6} <= {m["G"] for m in cases}
    assert sorted(m["K"] for m in cases if any(r["len"] == 300_000 for r in m["records"])) == [9, 17, 21, 31]
    for m in cases:
        assert m["S"] + m["W"] <= 20 and m["H"] <= m["W"]
        if m["H"] >= 7:
            assert m["K"] >= 8
            for r in m["records"]:
                if "verbatim" in r:
                    s = vec["seqs"][int(vec["seq_off"][r["verbatim"]]):int(vec["seq_off"][r["verbatim"] + 1])]
                    assert not rsw.depends_on_bsr0(m["K"], s), m["seed"]


def test_oracle_reproduces_the_recorded_sweep(po, native, sweep):
    """min_score, H after -G, every sketch, every hit list and the dump of every recorded case."""
    vec, meta = sweep
    n_rec = 0
    for i, m in enumerate(meta["cases"]):
        tag = rsw.case_tag(i, m)
        p = po.make_params(m["K"], m["S"], m["W"], m["H"], m["J"], genome_size=m["G"])
        assert p.min_score == m["min_score"], tag
        assert p.H == m["H_final"], tag
        recs = rsw.sweep_records(native, po, vec, m)
        if m["H"] >= 7:
            assert not any(rsw.depends_on_bsr0(m["K"], s) for s in recs), tag
        sk = np.stack([po.compute_sketch(p, s) for s in recs])
        rsw.check_sketches(po, vec, i, m, sk, tag)
        ix = po.Index(p, sk)
        for q in range(len(recs)):
            hc, hg = ix.query(sk[q])
            ec, eg = rsw.recorded_hits(vec, m, q)
            assert np.array_equal(hc, ec) and np.array_equal(hg, eg), (tag, "query", q)
        raw = ix.dump_bytes() + rsw.dump_names(len(recs))
        assert len(raw) == m["dump_len"] and hashlib.md5(raw).hexdigest() == m["dump_md5"], tag
        n_rec += len(recs)
    assert n_rec == meta["records_recorded"]


def test_fingerprint_of_zero_takes_64_leading_zeros(po):
    """get_fingerprint(0): the oracle (and the kernels' clz64) count 64 leading zeros -- 0 up to H = 6, the
    saturating part 2^H - 1 - 64 above.  The reference runs bsr on 0 there; the live reference is not asserted."""
    for W in range(1, 16):
        for H in range(0, W + 1):
            assert po.fingerprint(0, W, H) == max(0, (1 << H) - 1 - 64) << (W - H), (W, H)
            assert po.fingerprint_stale(0, W, H, H) == po.fingerprint(0, W, H)
            assert po.fingerprint(1, W, H) == (1 if H < W else 0) + (max(0, (1 << H) - 1 - 63) << (W - H))


def test_live_reference_campaign(po, native):
    """>= 2000 sketches, and every one of them queried against its case's index, over seeded random parameters (H up
    to W): oracle == reference."""
    if not po.have_ref():
        pytest.skip("oracle/_ref/libniqki_ref.so not built (no reference sources here)")
    rng = np.random.default_rng(20261019)
    cases, generated, left_out = [], 0, 0
    for i in range(280):
        c = rsw.random_case(rng, max_S=10)
        kept, n, out = rsw.case_records(native, po, c, 500_000 + i, long_len=5000 if i % 8 == 0 else 0)
        generated += n
        left_out += out
        if kept:
            cases.append(dict(c, records=[s for s, _ in kept]))
    assert left_out <= rsw.MAX_LEFT_OUT * generated, (left_out, generated)
    t0 = time.time()
    results = rsw.run_reference(cases, timeout=300)
    t_ref = time.time() - t0
    n_sk = n_hits = 0
    for c, r in zip(cases, results):
        tag = "K=%(K)d S=%(S)d W=%(W)d H=%(H)d J=%(J)g G=%(G)g" % c
        p = po.make_params(c["K"], c["S"], c["W"], c["H"], c["J"], genome_size=c["G"])
        assert p.min_score == r["min_score"] and p.H == r["H_final"], tag
        sk = np.stack([po.compute_sketch(p, s) for s in c["records"]])
        bad = [j for j in range(len(sk)) if not np.array_equal(sk[j], r["sketches"][j])]
        assert not bad, (tag, "records", bad, [len(c["records"][j]) for j in bad])
        ix = po.Index(p, sk)
        off = np.concatenate([[0], np.cumsum(r["hit_n"], dtype=np.int64)])
        for q in range(len(sk)):
            hc, hg = ix.query(sk[q])
            assert np.array_equal(hc, r["hit_counts"][off[q]:off[q + 1]]), (tag, "query", q)
            assert np.array_equal(hg, r["hit_gids"][off[q]:off[q + 1]]), (tag, "query", q)
        raw = ix.dump_bytes() + rsw.dump_names(len(sk))
        assert len(raw) == r["dump_len"] and hashlib.md5(raw).hexdigest() == r["dump_md5"], tag
        n_sk += len(sk)
        n_hits += int(off[-1])
    print("live campaign: %d cases, %d sketches and queries compared (%d hits), %d of %d generated records left out "
          "(%.1f %%), reference child %.1f s" % (len(cases), n_sk, n_hits, left_out, generated,
                                                 100.0 * left_out / generated, t_ref))
    assert n_sk >= 2000


def test_reference_does_not_return_where_the_oracle_says_so(po, tmp_path):
    """The hang predictor's other direction: on records whose densification the oracle reports as never ending, the
    reference's compute_sketch is still running 2 s after it began (children of their own, all at once)."""
    if not po.have_ref():
        pytest.skip("oracle/_ref/libniqki_ref.so not built (no reference sources here)")
    rng = np.random.default_rng(5)
    jobs = [dict(K=31, S=12, W=10, H=4, records=[np.frombuffer(b"A" * 100, np.uint8)]),          # one value, even step
            dict(K=31, S=12, W=10, H=4, records=[np.frombuffer(b"N" * 60, np.uint8)]),
            dict(K=21, S=10, W=1, H=0, records=[rsw.clean(rng, 400)])]                           # two values: 0 stays put, 1 steps evenly
    p = po.make_params(31, 10, 12, 4, 0.0)
    one = next(s for s in (rsw.clean(rng, 32) for _ in range(200)) if not rsw.will_return(po, p, s))
    jobs.append(dict(K=31, S=10, W=12, H=4, records=[one]))                                      # a 1-k-mer read
    for j in jobs:
        assert not rsw.will_return(po, po.make_params(j["K"], j["S"], j["W"], j["H"], 0.0), j["records"][0])
    procs = []
    try:
        for n, j in enumerate(jobs):
            path = tmp_path / ("job%d.pkl" % n)
            path.write_bytes(pickle.dumps(j))
            procs.append(subprocess.Popen([sys.executable, rsw.__file__, "--one", str(path)], stdout=subprocess.PIPE,
                                          env=dict(os.environ, OMP_NUM_THREADS="1")))
        for pr in procs:
            assert pr.stdout.readline().strip() == b"ready"
        deadline = time.time() + 2.0
        for pr in procs:
            with pytest.raises(subprocess.TimeoutExpired):
                pr.wait(timeout=max(0.0, deadline - time.time()))
    finally:
        for pr in procs:
            pr.kill()
            pr.wait()
            pr.stdout.close()
