"""CPU: the reference of the contained lists (tests/contain_ref.py) against fractions.Fraction on designed and random
values; niqki_amd/csrc/nq_contain_share.h -- the code the kernels run -- compiled by g++ into a stand-alone program (plain,
and under the undefined-behaviour and address sanitizers) against the reference over a designed table; the list builder
on a hand-made list; and the share of a part in its whole on the oracle's sketches.

Bounds of the part and the whole: those of tests/test_registers_ref_cpu.py (four standard errors of the Jaccard share
and of the size estimate).  The integer share and registers_ref's double cq differ by the rounding of the two sizes to
integers and by the 2^-32 of the floor; the two are held to 1e-6 of each other and the figures are printed."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import contain_ref as cr
import registers_ref as rr
from conftest import ROOT

K, W = 31, 12
TOP = (1 << 40) - 1

SRC = r"""
#include <cstdio>
#include <cstdint>
#include "nq_contain_share.h"

// stdin: lines "s c F q g mode" -> the share; "k share pos" -> "key share pos" (the two decoded from the key);
// "f size" -> "0" or "1"
int main() {
  char what;
  unsigned long long a, b, c, d, e;
  while (scanf(" %c", &what) == 1) {
    if (what == 's') {
      if (scanf("%llu %llu %llu %llu %llu", &a, &b, &c, &d, &e) != 5) return 2;
      printf("%u\n", nq::contain_share((uint32_t)a, (uint32_t)b, c, d, (uint32_t)e));
    } else if (what == 'k') {
      if (scanf("%llu %llu", &a, &b) != 2) return 2;
      const uint64_t key = nq::contain_key((uint32_t)a, (uint32_t)b);
      printf("%llu %u %u\n", (unsigned long long)key, nq::contain_key_share(key), nq::contain_key_pos(key));
    } else if (what == 'f') {
      if (scanf("%llu", &a) != 1) return 2;
      printf("%d\n", nq::contain_size_fits(a) ? 1 : 0);
    } else {
      return 2;
    }
  }
  printf("ONE %u\n", nq::kContainOne);
  return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("contain_share_" + request.param)
    (d / "main.cpp").write_text(SRC)
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "niqki_amd", "csrc"),
                           "-o", str(d / "share"), str(d / "main.cpp")])
    return str(d / "share")


def ask(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == "ONE %d" % cr.ONE
    return out[:-1]


def designed_table():
    """(c, F, q, g, mode): c in {0, 1, F - 1, F}; S in {4, 10, 15, 16}; sizes 1, 2, 2^40 - 1, equal, 1000 : 1; every
    mode; the two example genomes at the defaults"""
    sizes = [(1, 1), (1, 2), (2, 1), (2, 2), (1, TOP), (TOP, 1), (2, TOP), (TOP, 2), (TOP, TOP), (TOP - 1, TOP),
             (5_000_000, 5_000_000), (5_000_000_000, 5_000_000), (5_000_000, 5_000_000_000), (4_568_563, 4_604_317)]
    out = []
    for S in (4, 10, 15, 16):
        F = 1 << S
        for c in (0, 1, F - 1, F):
            for q, g in sizes:
                for mode in (cr.QUERY, cr.GENOME, cr.MAX):
                    out.append((c, F, q, g, mode))
    out += [(25930, 1 << 15, 4_568_563, 4_604_317, mode) for mode in (cr.QUERY, cr.GENOME, cr.MAX)]
    return out


def by_fraction(c, F, q, g, mode):
    d = q if mode == cr.QUERY else g if mode == cr.GENOME else min(q, g)
    J = Fraction(c, F)
    x = J * (q + g) / (1 + J) / d                       # |A n B| / d
    return cr.ONE if x >= 1 else math.floor(x * (1 << 32))


def test_reference_against_fractions():
    rng = np.random.default_rng(4)
    cases = designed_table()
    for _ in range(20000):
        S = int(rng.integers(1, 17))
        F = 1 << S
        c = int(rng.integers(0, F + 1))
        q, g = (int(rng.integers(1, 1 << int(rng.integers(1, 41)))) for _ in range(2))
        cases.append((c, F, q, g, int(rng.integers(0, 3))))
    for case in cases:
        assert cr.share(*case) == by_fraction(*case), case
    # the example genomes: the shares the README's cq and cg round from
    assert cr.share(25930, 1 << 15, 4_568_563, 4_604_317, cr.QUERY) == 3_809_475_352
    assert cr.share(25930, 1 << 15, 4_568_563, 4_604_317, cr.GENOME) == 3_779_893_553
    assert "%.6f" % (3_809_475_352 / 2 ** 32) == "0.886963" and "%.6f" % (3_779_893_553 / 2 ** 32) == "0.880075"
    # what the definition implies
    assert cr.share(0, 1024, 5, 7, cr.QUERY) == 0 and cr.share(1024, 1024, 9, 9, cr.MAX) == cr.ONE
    assert cr.share(512, 1024, 100, 100, cr.QUERY) == (2 << 32) // 3
    for case in cases[:2000]:
        c, F, q, g, _ = case
        assert cr.share(c, F, q, g, cr.MAX) == max(cr.share(c, F, q, g, cr.QUERY), cr.share(c, F, q, g, cr.GENOME))


def test_threshold_of_a_containment():
    assert cr.min_share_of(1) == cr.ONE and cr.min_share_of(1.0) == cr.ONE
    assert cr.min_share_of(0.5) == 1 << 31 and cr.min_share_of(0.25) == 1 << 30
    assert cr.min_share_of(0.8) == math.ceil(Fraction(0.8) * (1 << 32)) == 3435973837
    assert cr.min_share_of(2.0 ** -40) == 1 and cr.min_share_of(1 - 2.0 ** -40) == cr.ONE


def test_header_prints_the_reference_shares(program):
    rng = np.random.default_rng(5)
    cases = designed_table()
    for _ in range(3000):
        S = int(rng.integers(1, 17))
        F = 1 << S
        cases.append((int(rng.integers(0, F + 1)), F, int(rng.integers(1, 1 << int(rng.integers(1, 41)))),
                      int(rng.integers(1, 1 << int(rng.integers(1, 41)))), int(rng.integers(0, 3))))
    out = ask(program, ["s %d %d %d %d %d" % x for x in cases])
    assert len(out) == len(cases)
    for case, line in zip(cases, out):
        assert int(line) == cr.share(*case), case
    assert {int(x) for x in out} >= {0, cr.ONE}


def test_key_order_is_share_then_list_order(program):
    rng = np.random.default_rng(6)
    n = 3000
    shares = rng.choice(np.array([0, 1, 1 << 31, cr.ONE - 1, cr.ONE], np.int64), n)
    pos = rng.permutation(n).astype(np.int64)
    pos[:3] = [0, (1 << 32) - 2, 1 << 31]
    shares[:3] = [0, 0, cr.ONE]
    out = ask(program, ["k %d %d" % x for x in zip(shares, pos)])
    keys = []
    for s, p, line in zip(shares, pos, out):
        key, ds, dp = (int(x) for x in line.split())
        assert (ds, dp) == (s, p) and key == (int(s) << 32 | (0xFFFFFFFF - int(p))) and key != 0
        keys.append(key)
    assert len(set(keys[3:])) == n - 3
    by_key = sorted(range(3, n), key=lambda i: -keys[i])
    by_order = sorted(range(3, n), key=lambda i: (-int(shares[i]), int(pos[i])))
    assert by_key == by_order
    assert ask(program, ["f %d" % x for x in (0, 1, TOP, TOP + 1, 1 << 41, (1 << 64) - 1)]) == ["1", "1", "1", "0", "0", "0"]


def test_lists_on_a_hand_made_list():
    F = 16
    # two queries; genome sizes: 3 has none
    full = (np.array([0, 5, 7]), np.array([16, 8, 8, 4, 2, 8, 8]), np.array([4, 2, 1, 3, 0, 1, 0]))
    sizes = [100, 100, 50, 0, 400]
    qs = [100, 0]
    off, s, c, g, nu = cr.contain_lists(full, sizes, qs, cr.QUERY, 0, F=F)
    assert off.tolist() == [0, 4, 4] and nu.tolist() == [1, 2] and off.dtype == np.uint64 and nu.dtype == np.uint32
    sh = [cr.share(16, F, 100, 400, 0), cr.share(8, F, 100, 50, 0), cr.share(8, F, 100, 100, 0), cr.share(2, F, 100, 100, 0)]
    assert sh[0] == cr.ONE and sh[2] > sh[1] > sh[3]
    assert s.tolist() == [sh[0], sh[2], sh[1], sh[3]] and g.tolist() == [4, 1, 2, 0] and c.tolist() == [16, 8, 8, 2]
    cut = cr.contain_lists(full, sizes, qs, cr.QUERY, sh[1], 2, F=F)
    assert cut[0].tolist() == [0, 2, 2] and cut[3].tolist() == [4, 1] and cut[4].tolist() == [1, 2]
    edge = cr.contain_lists(full, sizes, qs, cr.QUERY, sh[1], F=F)
    assert edge[3].tolist() == [4, 1, 2]                     # share == min_share stays
    # equal sizes: a sub-list of H in H's order (here all of it), ties included
    same = cr.contain_lists(full, [7] * 5, [7, 7], cr.MAX, 0, F=F)
    assert same[0].tolist() == [0, 5, 7] and same[2].tolist() == full[1].tolist() and same[3].tolist() == full[2].tolist()


def test_share_of_a_part_in_the_whole(po):
    """the oracle's sketches of a 64 F part and its 256 F whole, S = 10, the seeds of test_registers_ref_cpu.py"""
    S = 10
    F = 1 << S
    p = po.make_params(K, S, W, 4, 0.0)
    whole = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(31 * S).integers(0, 4, 256 * F + K - 1)]
    part = whole[: 64 * F + K - 1]
    sa, sb = po.compute_sketch(p, part), po.compute_sketch(p, whole)
    count = int(((sa == sb) & (sa >= 0)).sum())
    q, g = rr.estimate(rr.hist_ref(sa, W, 4)[0], S, 4), rr.estimate(rr.hist_ref(sb, W, 4)[0], S, 4)
    assert q[1] == g[1] == rr.OK
    J, cq, cg = rr.containment(count, S, q, g)
    qi, gi = math.floor(q[0] + 0.5), math.floor(g[0] + 0.5)
    s_q, s_g = cr.share(count, F, qi, gi, cr.QUERY), cr.share(count, F, qi, gi, cr.GENOME)
    margin = 4 * (math.sqrt((1 - J) / (J * F)) + 1.04 / math.sqrt(F))
    print("count=%d q=%d g=%d share_q=%d (%.7f, cq %.7f) share_g=%d (%.7f, cg %.7f) margin=%.4f"
          % (count, qi, gi, s_q, s_q / 2 ** 32, cq, s_g, s_g / 2 ** 32, cg, margin))
    assert abs(s_q / 2 ** 32 - 1.0) <= margin and abs(s_g / 2 ** 32 - 0.25) <= margin
    assert abs(s_q / 2 ** 32 - cq) <= 1e-6
    assert cr.share(count, F, qi, gi, cr.MAX) == s_q
    assert J < 0.5 and s_q >= cr.min_share_of(0.8) > s_g     # what the host program's example shows
