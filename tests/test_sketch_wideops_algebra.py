"""The arithmetic identities behind the 64-bit-wide forms of the sketch kernel's hot step (nq_sketch_ops.h: min62(),
shl2_add64(), mix_round_hi()), restated with exact integers on the host.  No GPU: the kernels themselves are held to
the oracle by the GPU suite (tests/test_gpu_canonical_min.py for the subnormal words)."""
import numpy as np
import pytest

M64 = (1 << 64) - 1


@pytest.mark.parametrize("K", list(range(17, 32)))
def test_roll_with_the_entry_as_addend(K):
    """fw = ((fw << 2) + entry) & mask and rc = (rc | entry_hi:0) >> 2 with the rc code at bit 2K - 32 of the entry's
    high word give what the separate updates give; the warm-up from zero needs no mask before the first hash step.
    Entries include those of dirty bytes, whose rc code is not 3 - forward code."""
    rng = np.random.default_rng(K)
    mask = (1 << (2 * K)) - 1
    fw = rc = 0          # reference: separate updates, masked every step
    nfw = nrc = 0        # the kernel's: unmasked during the K - 1 warm-up steps
    for i in range(3000):
        f = int(rng.choice(4, p=[0.55, 0.1, 0.1, 0.25]))
        r = 3 - f if rng.random() < 0.9 else int(rng.integers(0, 4))
        entry = (r << (2 * K - 32 + 32)) | f
        fw = ((fw << 2) | f) & mask
        rc = (rc >> 2) | (r << (2 * K - 2))
        nfw = ((nfw << 2) + entry) & M64
        if i >= K - 1:
            nfw &= (mask & 0xFFFFFFFF00000000) | 0xFFFFFFFF    # the `and` of the high word
        nrc = (nrc | (entry & 0xFFFFFFFF00000000)) >> 2
        assert nrc == rc
        if i >= K - 1:
            assert nfw == fw
        else:
            assert nfw & mask == fw


def test_double_minimum_is_the_integer_minimum_below_2_62():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1 << 62, size=200_000, dtype=np.uint64)
    b = rng.integers(0, 1 << 62, size=200_000, dtype=np.uint64)
    # words of every size: subnormal patterns (< 2^52), zero, equal words
    a >>= rng.integers(0, 62, size=a.size).astype(np.uint64)
    b >>= rng.integers(0, 62, size=b.size).astype(np.uint64)
    a[:100] = 0
    b[50:150] = a[50:150]
    m = np.minimum(a.view(np.float64), b.view(np.float64)).view(np.uint64)
    assert np.array_equal(m, np.minimum(a, b))
    assert int(np.count_nonzero((np.minimum(a, b) < (1 << 52)) & (np.minimum(a, b) > 0))) > 10_000


def test_second_hash_round_in_four_instructions():
    """High word of ((x >> 32) ^ x) * c: the v_mul_hi rides in the low word of the first mad's addend, whose high
    word holds anything."""
    rng = np.random.default_rng(2)
    for c in (0xD6E8FEB86659FD93, 0xCFEE444D8B59A89B, int(rng.integers(1, 1 << 63)) | 1):
        clo, chi = c & 0xFFFFFFFF, c >> 32
        for _ in range(20_000):
            x = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            lo, hi = x & 0xFFFFFFFF, x >> 32
            y = lo ^ hi
            junk = int(rng.integers(0, 1 << 32))
            a = (junk << 32) | ((y * clo) >> 32)
            t = (hi * clo + a) & M64
            p = (y * chi + t) & M64
            assert p & 0xFFFFFFFF == ((((x >> 32) ^ x) * c) & M64) >> 32
