"""The edge key of niqki_linkage (niqki_amd/csrc/nq_linkage_key.h), on the CPU: the header is the code the forest
kernels run.  It is compiled here with g++ into a stand-alone program that packs and unpacks the edges it is given.
The key must decode back to its edge at the corners of the three fields, a LARGER key must be EARLIER in the edge order
(larger count, then smaller lo, then smaller hi), and the id limit must be 2^23 genomes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 23) - 1

SRC = r"""
#include <cstdio>
#include <cstdint>
#include "nq_linkage_key.h"

// stdin: lines "e count lo hi" -> "key count lo hi" (the three decoded from the key); "n genomes" -> "0" or "1"
int main() {
  char what;
  unsigned long long a, b, c;
  while (scanf(" %c", &what) == 1) {
    if (what == 'e') {
      if (scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
      const uint64_t key = nq::linkage_pack((uint32_t)a, (uint32_t)b, (uint32_t)c);
      printf("%llu %u %u %u\n", (unsigned long long)key, nq::linkage_count(key), nq::linkage_lo(key), nq::linkage_hi(key));
    } else if (what == 'n') {
      if (scanf("%llu", &a) != 1) return 2;
      printf("%d\n", nq::linkage_fits(a) ? 1 : 0);
    } else {
      return 2;
    }
  }
  printf("M %u\n", nq::kLinkageIdMax);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("linkage_key")
    (d / "main.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "csrc"),
                           "-o", str(d / "key"), str(d / "main.cpp")])
    return str(d / "key")


def ask(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == "M %d" % M
    return out[:-1]


def test_the_key_decodes_back_to_its_edge_at_the_corners(program):
    edges = [(c, lo, hi) for c in (0, 1, 65535, 65536, (1 << 17) - 1) for lo in (0, 1, M - 1) for hi in (lo + 1, M) if lo < hi]
    edges.append((65536, 0, M))
    out = ask(program, ["e %d %d %d" % e for e in edges])
    for e, line in zip(edges, out):
        key, c, lo, hi = (int(x) for x in line.split())
        assert (c, lo, hi) == e
        assert key == (e[0] << 46) | ((M - e[1]) << 23) | (M - e[2]) and key < 1 << 63
        assert key != 0                                      # (only count 0 with lo = hi = M would be, and that is no edge)


def test_key_order_is_the_edge_order(program):
    rng = np.random.default_rng(1)
    n = 4000
    # few distinct values per field, so that every tie rule decides many pairs
    c = rng.choice([1, 2, 700, 65535, 65536], n)
    lo = rng.choice([0, 1, 5, 4000, M - 2], n)
    hi = lo + rng.choice([1, 2, 1 << 20], n)
    hi = np.minimum(hi, M)
    keep = lo < hi
    c, lo, hi = c[keep], lo[keep], hi[keep]
    out = ask(program, ["e %d %d %d" % e for e in zip(c, lo, hi)])
    keys = np.array([int(line.split()[0]) for line in out], dtype=np.uint64)
    by_key = np.argsort(keys, kind="stable")[::-1]                       # descending key
    by_order = np.lexsort((hi, lo, -c))                                  # the edge order
    edge = np.stack([c, lo, hi], 1)
    assert np.array_equal(edge[by_key], edge[by_order])
    a, b = rng.integers(0, c.size, 20000), rng.integers(0, c.size, 20000)
    first = [(-int(c[i]), int(lo[i]), int(hi[i])) < (-int(c[j]), int(lo[j]), int(hi[j])) for i, j in zip(a, b)]
    assert np.array_equal(keys[a] > keys[b], np.array(first))
    assert np.array_equal(keys[a] == keys[b], np.all(edge[a] == edge[b], axis=1))


def test_the_id_limit_is_2_to_the_23_genomes(program):
    ns = [0, 1, M, M + 1, M + 2, 1 << 24, (1 << 32) - 1, 1 << 32]
    out = ask(program, ["n %d" % n for n in ns])
    assert [int(x) for x in out] == [1 if n <= 1 << 23 else 0 for n in ns]
