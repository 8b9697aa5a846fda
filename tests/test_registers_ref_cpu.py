"""CPU: the reference of the register histograms (tests/registers_ref.py) against a plain loop on designed cells; the
size estimator against exact distinct-k-mer counts on the oracle's sketches of random sequences and of two of the
example genomes; its range (below, above); the containment of a sequence in a longer one; and
niqki_amd/host/size_estimate.h, compiled into a stand-alone program, against the same histograms text for text (so is
niqki_amd/size_estimate.py).

Bounds.  A HyperLogLog estimate of F registers has standard error 1.04 / sqrt(F); every size is held to four of them.
A containment is I / q with I = J (q + g) / (1 + J): J = c / F is a binomial share with relative standard error
sqrt((1 - J) / (J F)), the sizes add theirs, and the margin is four times the sum."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import registers_ref as rr
from conftest import ROOT

EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
K, W = 31, 12


def se4(S):
    return 4 * 1.04 / math.sqrt(1 << S)


def random_seq(seed, n_kmers):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n_kmers + K - 1)]


def hist_loop(cells, W_, H):
    out = [[0] * rr.bins(H) for _ in cells]
    for row, h in zip(cells, out):
        for c in row:
            c = int(c)
            h[c >> (W_ - H) if 0 <= c < (1 << W_) else 1 << H] += 1
    return out


@pytest.mark.parametrize("H", range(7))
def test_reference_against_a_plain_loop(H):
    W_, F = 10, 64
    rng = np.random.default_rng(H)
    cells = rng.integers(0, 1 << W_, (6, F)).astype(np.int32)
    cells[0, ::3] = -1
    cells[1, ::5] = -7
    cells[1, 1] = np.iinfo(np.int32).min
    cells[2, :4] = [(1 << W_) - 1, 1 << W_, (1 << W_) + 1, np.iinfo(np.int32).max]
    cells[3, :] = (1 << W_) - 1                   # all cells in the last register's bin
    cells[4, :] = 0                               # ... in the first
    cells[5, :] = -1                              # all empty
    got = rr.hist_ref(cells, W_, H)
    assert got.dtype == np.uint32 and got.shape == (6, rr.bins(H))
    assert got.tolist() == hist_loop(cells, W_, H)
    assert (got.sum(axis=1) == F).all()
    assert got[3, (1 << H) - 1] == F and got[4, 0] == F and got[5, 1 << H] == F


@pytest.fixture(scope="module")
def random_cases(po):
    """(S, H, n, histogram row, exact count) of random sequences, fixed seeds"""
    out = []
    for S in (10, 12):
        p = po.make_params(K, S, W, 4, 0.0)
        for i, mult in enumerate((10, 16, 64, 500)):
            seq = random_seq(1000 * S + i, mult << S)
            out.append((S, 4, mult, rr.hist_ref(po.compute_sketch(p, seq), W, 4)[0], rr.distinct_kmers([seq], K).size))
    return out


def test_estimator_against_exact_counts(random_cases):
    worst = 0.0
    for S, H, mult, hist, exact in random_cases:
        E, status = rr.estimate(hist, S, H)
        print("S=%d n=%dF exact=%d estimate=%.0f ratio=%.4f (%.2f standard errors) %s"
              % (S, mult, exact, E, E / exact, abs(E / exact - 1) / (se4(S) / 4), status))
        worst = max(worst, abs(E / exact - 1) / (se4(S) / 4))
    print("worst: %.2f standard errors" % worst)
    for S, H, mult, hist, exact in random_cases:
        E, status = rr.estimate(hist, S, H)
        assert status == rr.OK, (S, mult)
        assert abs(E / exact - 1) <= se4(S), (S, mult, E, exact)


def test_sum_is_exact_in_a_double(random_cases):
    from fractions import Fraction
    for S, H, _, hist, _ in random_cases:
        Z = Fraction(int(hist[1 << H])) + sum(Fraction(int(hist[r]), 1 << ((1 << H) - r)) for r in range(1 << H))
        alpha = 0.7213 / (1.0 + 1.079 / (1 << S))
        assert float(Z) == Z and rr.estimate(hist, S, H)[0] == alpha * (1 << S) * (1 << S) / float(Z)


@pytest.mark.parametrize("S", (10, 12))
def test_short_sequences_are_below(po, S):
    p = po.make_params(K, S, W, 4, 0.0)
    F = 1 << S
    for i, n in enumerate((120, F // 4, F, 4 * F)):
        hist = rr.hist_ref(po.compute_sketch(p, random_seq(77 * S + i, n)), W, 4)[0]
        assert rr.estimate(hist, S, 4)[1] == rr.BELOW, (S, n)


def test_small_parameters_are_always_below(po):
    seq = random_seq(5, 64 << 10)
    for S, H in ((10, 1), (10, 0), (3, 2)):
        p = po.make_params(K, S, W, H, 0.0)
        assert rr.estimate(rr.hist_ref(po.compute_sketch(p, seq), W, H)[0], S, H)[1] == rr.BELOW


def test_saturated_registers_are_above(po):
    S, H = 10, 3
    p = po.make_params(K, S, W, H, 0.0)
    hist = rr.hist_ref(po.compute_sketch(p, random_seq(9, 64 << S)), W, H)[0]
    assert 8 * int(hist[0]) > (1 << S)
    assert rr.estimate(hist, S, H)[1] == rr.ABOVE


@pytest.mark.parametrize("S", (10, 12))
def test_containment_of_a_part_in_the_whole(po, S):
    p = po.make_params(K, S, W, 4, 0.0)
    F = 1 << S
    whole = random_seq(31 * S, 256 * F)
    part = whole[: 64 * F + K - 1]
    sa, sb = po.compute_sketch(p, part), po.compute_sketch(p, whole)
    count = int(((sa == sb) & (sa >= 0)).sum())
    q, g = rr.estimate(rr.hist_ref(sa, W, 4)[0], S, 4), rr.estimate(rr.hist_ref(sb, W, 4)[0], S, 4)
    J, cq, cg = rr.containment(count, S, q, g)
    margin = 4 * (math.sqrt((1 - J) / (J * F)) + 1.04 / math.sqrt(F))
    print("S=%d J=%.4f cq=%.4f cg=%.4f margin=%.4f" % (S, J, cq, cg, margin))
    assert q[1] == g[1] == rr.OK
    assert abs(cq - 1.0) <= margin and abs(cg - 0.25) <= margin


def test_containment_is_undefined_outside_the_range():
    F = 1 << 10
    ok = np.zeros(17, dtype=np.uint32)
    ok[8] = F
    empty = np.zeros(17, dtype=np.uint32)
    empty[16] = F
    q, g = rr.estimate(ok, 10, 4), rr.estimate(empty, 10, 4)
    assert q[1] == rr.OK and g[1] == rr.BELOW
    assert rr.containment(100, 10, q, g)[1:] == (None, None) and rr.containment(100, 10, g, q)[1:] == (None, None)
    assert rr.containment_entry("x", 512, 10, q, q) == "x:0.5:0.666667:0.666667"
    assert rr.containment_entry("x", 512, 10, q, g) == "x:0.5:-:-"
    assert rr.containment(F, 10, q, q)[1:] == (1.0, 1.0)


@pytest.fixture(scope="module")
def ecoli(po):
    """ecoli01p and ecoli09p at the defaults: the oracle's sketches and the exact distinct canonical 31-mers"""
    p = po.make_params(K, 15, W, 4, 0.0)
    out = []
    for name in ("ecoli01p.fa.gz", "ecoli09p.fa.gz"):
        records = [seq for _, _, seq in po.frame_records(gzip.open(os.path.join(EDIR, name), "rb").read(), "A", K)]
        acc = np.full(1 << 15, -1, dtype=np.int32)
        for seq in records:                       # a file is one entry: its records share a sketch
            po.sketch_accumulate(p, seq, acc)
        out.append((po.densify(p, acc)[0], rr.distinct_kmers(records, K)))
    return out


def test_example_genomes_against_their_exact_counts(ecoli):
    S, H = 15, 4
    (s1, k1), (s9, k9) = ecoli
    q, g = rr.estimate(rr.hist_ref(s1, W, H)[0], S, H), rr.estimate(rr.hist_ref(s9, W, H)[0], S, H)
    for (E, status), kmers in ((q, k1), (g, k9)):
        print("exact=%d estimate=%.0f error=%+.2f%%" % (kmers.size, E, 100 * (E / kmers.size - 1)))
        assert status == rr.OK and abs(E / kmers.size - 1) <= se4(S)
    count = int(((s1 == s9) & (s1 >= 0)).sum())
    common = np.intersect1d(k1, k9, assume_unique=True).size
    J, cq, cg = rr.containment(count, S, q, g)
    margin = 4 * (math.sqrt((1 - J) / (J * (1 << S))) + 1.04 / math.sqrt(1 << S))
    print("count=%d J=%.4f cq=%.4f (exact %.4f) cg=%.4f (exact %.4f) margin=%.4f"
          % (count, J, cq, common / k1.size, cg, common / k9.size, margin))
    assert abs(cq - common / k1.size) <= margin and abs(cg - common / k9.size) <= margin


# ---- size_estimate.h and size_estimate.py print what the reference prints ----

@pytest.fixture(scope="module")
def estimate_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("size_estimate") / "size_estimate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", out,
                           os.path.join(ROOT, "tests", "host_san", "size_estimate_main.cpp")])
    return out


def designed_histograms():
    """(S, H, row): every status, both ends of the range, every H the engine takes, the F below 128"""
    rng = np.random.default_rng(3)
    out = []
    for S in (3, 4, 5, 6, 7, 10, 15, 16):
        F = 1 << S
        for H in range(7):
            B = rr.bins(H)
            rows = [rng.multinomial(F, rng.dirichlet(np.ones(B))) for _ in range(3)]
            for one in (0, B // 2, B - 2, B - 1):          # all cells in one bin
                r = np.zeros(B, dtype=np.int64)
                r[one] = F
                rows.append(r)
            r = np.zeros(B, dtype=np.int64)                 # exactly at and just over the saturation threshold
            r[0], r[B - 2] = F // 8, F - F // 8
            rows.append(r.copy())
            if F >= 8 and B > 2:
                r[0] += 1
                r[B - 2] -= 1
                rows.append(r)
            out += [(S, H, np.asarray(x, dtype=np.uint32)) for x in rows]
    return out


def test_header_prints_the_reference_text(estimate_program, random_cases, ecoli):
    cases = designed_histograms() + [(S, H, h) for S, H, _, h, _ in random_cases]
    cases += [(15, 4, rr.hist_ref(s, W, 4)[0]) for s, _ in ecoli]
    lines, want = [], []
    for S, H, h in cases:
        lines.append("E %d %d %s" % (S, H, " ".join(map(str, h.tolist()))))
        want.append("%.0f\t%s" % rr.estimate(h, S, H))
    for (S, H, a), (S2, H2, b), count_of in zip(cases, cases[1:], range(len(cases))):
        if (S, H) == (S2, H2):
            count = (count_of * 2654435761) % ((1 << S) + 1)
            lines.append("C %d %d %d %s %s" % (S, H, count, " ".join(map(str, a.tolist())), " ".join(map(str, b.tolist()))))
            want.append(rr.containment_entry("", count, S, rr.estimate(a, S, H), rr.estimate(b, S, H))[1:])
    r = subprocess.run([estimate_program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    assert got == want
    assert {w.split("\t")[1] for w in want if "\t" in w} == {"ok", "below", "above"}
    assert any(w.endswith(":-:-") for w in want) and any(":" in w and not w.endswith("-") for w in want)


def test_python_mirror_equals_the_reference(random_cases):
    from niqki_amd import size_estimate as se
    for S, H, h in designed_histograms() + [(S, H, h) for S, H, _, h, _ in random_cases]:
        E, st = se.estimate(h, S, H)
        assert (E, se.STATUS_TEXT[st]) == rr.estimate(h, S, H)
    assert se.sizes_lines(["a"], [random_cases[0][3]], 10, 4) == rr.sizes_text(["a"], [random_cases[0][3]], 10, 4).splitlines()
