"""The algebra the candidate drain rests on (nq_sketch.hip candidate_update), in exact Python integers.

The filtered fast loops push x1 = fold(canon) * C mod 2^64, the word after the first round of revhash64, with
fold(x) = x ^ (x >> 32), C = kRevMul, U = kUnrevMul.  Because C * U = 1 mod 2^64 and fold is an involution,

    rev(canon)   = fold(fold(x1) * C)                    one round instead of two
    unrev(canon) = fold(fold(x1 * U2) * U),  U2 = U * U  a plain product, then the usual second round

where rev / unrev are the two-round definitions (src/niqki_index.cpp:291-305; nq_common.h mix64)."""
import random

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
C = 0xD6E8FEB86659FD93
U = 0xCFEE444D8B59A89B
U2 = 0xEB9041BCFCD1CDD9


def fold(x):
    return x ^ (x >> 32)


def mix64(x, c):
    x = (fold(x) * c) & M64
    x = (fold(x) * c) & M64
    return fold(x)


def x1_of(canon):
    return (fold(canon) * C) & M64


def rev_from_x1(x1):
    return fold((fold(x1) * C) & M64)


def unrev_from_x1(x1):
    return fold((fold((x1 * U2) & M64) * U) & M64)


def mul_round_limbs(lo, hi, clo, chi):
    """nq_sketch.hip mul_round: three 32 x 32 -> 64 multiply-adds and one 32-bit add.  Of t and p only the low word
    is used, the carry of the last add is dropped."""
    t = (hi * clo) & M64                       # v_mad_u64_u32, addend 0
    p = (lo * chi + t) & M64                   # v_mad_u64_u32
    q = (lo * clo) & M64                       # v_mad_u64_u32, addend 0
    return q & M32, ((p & M32) + (q >> 32)) & M32


def _check(canon):
    x1 = x1_of(canon)
    assert fold(fold(canon)) == canon
    assert (x1 * U) & M64 == fold(canon)
    assert rev_from_x1(x1) == mix64(canon, C), hex(canon)
    assert unrev_from_x1(x1) == mix64(canon, U), hex(canon)
    lo, hi = mul_round_limbs(x1 & M32, x1 >> 32, U2 & M32, U2 >> 32)
    assert (hi << 32) | lo == (x1 * U2) & M64, hex(canon)


def test_multipliers_are_inverses():
    assert (C * U) & M64 == 1
    assert (U * U) & M64 == U2
    assert (C * C * U2) & M64 == 1


def test_identities_on_random_62_bit_words():
    rng = random.Random(20261018)
    for _ in range(20000):
        canon = rng.getrandbits(62)
        _check(canon)
        assert mix64(mix64(canon, C), U) == canon


def test_identities_on_the_edges():
    # poly-A: everything is 0
    assert x1_of(0) == 0 and rev_from_x1(0) == 0 and unrev_from_x1(0) == 0
    edges = [0, 1, (1 << 62) - 1, 1 << 61, M32, M32 - 1, 1 << 31, 1 << 32, (1 << 32) + 1, 0x3FFFFFFF00000000, 12345]
    rng = random.Random(7)
    edges += [rng.getrandbits(32) for _ in range(200)]             # words below 2^32
    edges += [rng.getrandbits(30) << 32 for _ in range(50)]        # a zero low word
    for canon in edges:
        _check(canon)
    # words whose x1 has a zero high or a zero low word: canon = fold(x1 * U), any 64-bit word (the identities hold
    # for all of them; those below 2^62 are k-mers)
    n62 = 0
    for _ in range(2000):
        w = rng.getrandbits(32)
        for x1 in (w, w << 32, 1, 1 << 32, M32, M32 << 32):
            canon = fold((x1 * U) & M64)
            assert x1_of(canon) == x1
            n62 += canon < (1 << 62)
            _check(canon)
    assert n62 > 1000   # about a quarter of them


def test_mul_round_limbs_on_random_words():
    rng = random.Random(99)
    cases = [(0, 0), (M64, M64), (M64, U2), (M32, U2), (M32 << 32, U2), (1, M64)]
    cases += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(20000)]
    for x, c in cases:
        lo, hi = mul_round_limbs(x & M32, x >> 32, c & M32, c >> 32)
        assert (hi << 32) | lo == (x * c) & M64, (hex(x), hex(c))
