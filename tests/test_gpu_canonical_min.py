"""The canonical choice of the sketch kernels is one v_min_f64 on the two k-mer words (nq_sketch_ops.h min62()).
That is exact as long as the instruction keeps subnormal bit patterns: a k-mer word below 2^52 is one, and a
kernel that flushed them to zero would sketch a k-mer of all A instead.  These inputs are rich in such words
(A and T at 0.4 each, poly-A and poly-T runs longer than K; for K <= 26 EVERY word is below 2^52), and every
sketch is held to the oracle: the filtered long path and the unfiltered one, K = 17 / 21 / 31, the one-wavefront
kernel of short reads and a record cut over several workgroups."""
import numpy as np
import pytest

BASES = np.frombuffer(b"ACGT", np.uint8)


def skewed_record(seed, n, runs=12):
    """n bases, A and T at 0.4 each, C and G at 0.1 each, with `runs` poly-A / poly-T runs of 40..200 bases."""
    rng = np.random.default_rng(seed)
    g = BASES[rng.choice(4, size=n, p=[0.4, 0.1, 0.1, 0.4])].copy()
    for r in range(runs):
        ln = int(rng.integers(40, 201))
        if ln + 1 >= n:
            continue
        at = int(rng.integers(0, n - ln))
        g[at:at + ln] = ord("A") if r % 2 == 0 else ord("T")
    return g


def subnormal_fraction_k31(g):
    """Share of the 31-mers of g whose canonical word is below 2^52: the forward word's top ten bits are zero
    when the k-mer starts with AAAAA (A = 0), the reverse-complement word's when it ends with TTTTT."""
    a = (g == ord("A")).astype(np.int32)
    t = (g == ord("T")).astype(np.int32)
    n = g.size - 31
    ca = np.concatenate(([0], np.cumsum(a)))
    ct = np.concatenate(([0], np.cumsum(t)))
    lead = (ca[5:5 + n] - ca[0:n]) == 5
    tail = (ct[31:31 + n] - ct[26:26 + n]) == 5
    return float(np.mean(lead | tail))


def test_inputs_are_rich_in_subnormal_words():
    """The premise of the tests below (no GPU work): about 2 % of the 31-mers of such a record, ten times a
    uniform record's share."""
    f = subnormal_fraction_k31(skewed_record(7, 400_000))
    print("share of 31-mers with a canonical word below 2^52: %.4f" % f)
    assert f > 0.015


@pytest.mark.gpu
@pytest.mark.parametrize("K", [17, 21, 31])
@pytest.mark.parametrize("S", [10, 15])
@pytest.mark.parametrize("mode", ["1", "0", "3"])
def test_long_record(native, po, K, S, mode, monkeypatch):
    """A 400 kbp record: NIQKI_SKETCH_FILTER 1 (automatic: the filtered fast loop at S = 10, too few k-mers per
    slot for it at S = 15), 0 (the unfiltered loop) and 3 (the fast loop forced at both sizes, then the exact
    re-run where it left slots open)."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    p = po.make_params(K, S, 12, 4, 0.0)
    e = native.Engine(K=K, S=S, W=12, H=4)
    g = [skewed_record(100 + K, 400_000), skewed_record(200 + K, 70_001)]
    g[1][5000:5100] = ord("N")
    sk = e.sketch(g)
    for i in range(2):
        exp = po.compute_sketch(p, g[i])
        diff = int(np.count_nonzero(sk[i] != exp))
        print("K=%d S=%d filter=%s record %d: %d of %d cells differ" % (K, S, mode, i, diff, exp.size))
        assert diff == 0, (K, S, mode, i)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [17, 21, 31])
def test_short_reads(native, po, K):
    """200 reads of 150 bases at S = 12: the one-wavefront kernel has its own copy of the canonical choice."""
    p = po.make_params(K, 12, 12, 4, 0.0)
    e = native.Engine(K=K, S=12, W=12, H=4)
    src = skewed_record(300 + K, 200 * 150, runs=40)
    reads = [src[i * 150:(i + 1) * 150].copy() for i in range(200)]
    sk = e.sketch(reads)
    exp = np.stack([po.compute_sketch(p, r) for r in reads])
    diff = int(np.count_nonzero(sk != exp))
    print("K=%d: %d of %d cells differ over 200 reads" % (K, diff, exp.size))
    assert diff == 0, K
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [17, 21, 31])
@pytest.mark.parametrize("mode", ["1", "0"])
def test_record_split_over_workgroups(native, po, K, mode, monkeypatch):
    """One 2.5 Mbp record on its own is cut over several workgroups, each exact on its own share."""
    monkeypatch.setenv("NIQKI_SKETCH_FILTER", mode)
    p = po.make_params(K, 10, 12, 4, 0.0)
    e = native.Engine(K=K, S=10, W=12, H=4)
    big = skewed_record(400 + K, 2_500_000, runs=60)
    sk = e.sketch([big])[0]
    exp = po.compute_sketch(p, big)
    diff = int(np.count_nonzero(sk != exp))
    print("K=%d filter=%s: %d of %d cells differ" % (K, mode, diff, exp.size))
    assert diff == 0, (K, mode)
    e.close()
