"""The three texts of the linkage phase (niqki_amd/host/linkage_text.h: --mst, --linkage, --tree), on the CPU.  A
stand-alone main over the header reads the arrays and the names and prints one of the texts; the texts are compared
with a restatement in Python that is built the other way round (every genome's own Newick pattern first, children
before parents, then one flattening pass; the header walks down from the roots with a stack) on random hierarchies:
deep chains of 200 000, wide ties, singletons, names with quotes, parentheses, colons, commas and blanks.  The same
program is built once more with AddressSanitizer + UBSan and run on the same inputs (a stand-alone program: no
preloaded runtime)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "linkage_text.h"

// argv: mst | linkage | tree, input file.  Input: "N E F", N lines "merge_into merge_count", E lines "lo hi count",
// N names (one per line).  The text goes to stdout, through a sink that also checks the chunks stay bounded.
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const std::string what = argv[1];
  std::ifstream in(argv[2]);
  uint32_t N = 0, E = 0, F = 0;
  if (!(in >> N >> E >> F)) return 2;
  std::vector<uint32_t> into(N), cnt(N), lo(E), hi(E), ec(E);
  for (uint32_t g = 0; g < N; ++g) if (!(in >> into[g] >> cnt[g])) return 2;
  for (uint32_t e = 0; e < E; ++e) if (!(in >> lo[e] >> hi[e] >> ec[e])) return 2;
  std::vector<std::string> names(N);
  std::string line;
  std::getline(in, line);
  for (uint32_t g = 0; g < N; ++g) if (!std::getline(in, names[g])) return 2;
  size_t longest = 0;
  const auto sink = [&](const std::string &text) {
    if (text.size() > longest) longest = text.size();
    fwrite(text.data(), 1, text.size(), stdout);
  };
  if (what == "mst") nqhost::write_mst(lo, hi, ec, names, F, sink);
  else if (what == "linkage") nqhost::write_linkage(into, cnt, names, F, sink);
  else if (what == "tree") nqhost::write_tree(into, cnt, names, F, sink);
  else return 2;
  if (what != "tree" && longest > nqhost::kLinkageTextChunk + (1u << 16)) return 3;   // (a deep tree is one long line)
  return 0;
}
"""


# ---- the restatement ---------------------------------------------------------------------------------------------

def fmt(x):
    return "%g" % x


def mst_text(lo, hi, count, names, F):
    return "".join("%s\t%s\t%s\n" % (names[a], names[b], fmt(int(c) / F)) for a, b, c in zip(lo, hi, count))


def linkage_text(into, count, names, F):
    return "".join("%s\t%s\t%s\n" % (names[g], names[int(into[g])], fmt(int(count[g]) / F)) for g in range(len(names)))


def tree_text(into, count, names, F):
    """one Newick line per root, in index order.  Every genome's pattern: '(' per group, its quoted name, then per group
    of equal counts (descending) the children's subtrees (ascending id) as references, each with its branch."""
    n = len(names)
    kids = [[] for _ in range(n)]
    for g in range(n):
        if into[g] != g:
            kids[int(into[g])].append(g)

    def height(c):
        return 1.0 - int(c) / F

    top = [0.0] * n
    pattern = [None] * n
    for p in range(n):
        ks = sorted(kids[p], key=lambda g: (-int(count[g]), g))
        levels = sorted({int(count[g]) for g in ks}, reverse=True)
        if levels:
            top[p] = height(levels[-1])
    for p in range(n):
        ks = sorted(kids[p], key=lambda g: (-int(count[g]), g))
        levels = sorted({int(count[g]) for g in ks}, reverse=True)
        items = ["(" * len(levels) + "'" + names[p].replace("'", "''") + "'"]
        below = 0.0
        for c in levels:
            items.append(":" + fmt(height(c) - below))
            for g in ks:
                if int(count[g]) == c:
                    items += [",", g, ":" + fmt(height(c) - top[g])]
            items.append(")")
            below = height(c)
        pattern[p] = items
    out = []
    for r in range(n):
        if into[r] != r:
            continue
        stack = [iter(pattern[r])]
        while stack:
            for item in stack[-1]:
                if isinstance(item, str):
                    out.append(item)
                else:
                    stack.append(iter(pattern[item]))
                    break
            else:
                stack.pop()
        out.append(";\n")
    return "".join(out)


# ---- hierarchies -------------------------------------------------------------------------------------------------

NASTY = ["it's", "''", "a(b)c", "x:0.5", "two words", "comma,semi;", "[bracket]", "'", "tab's neighbour\x0b", "(:;,)"]


def random_hierarchy(rng, n, p_root, window, steps):
    """merge_into[g] < g, a child's count strictly above its parent's, a root's 0; small steps make ties among siblings"""
    into, cnt = np.arange(n), np.zeros(n, np.int64)
    for g in range(1, n):
        if rng.random() < p_root:
            continue
        p = int(rng.integers(max(0, g - window), g))
        into[g] = p
        cnt[g] = cnt[p] + int(rng.integers(1, steps + 1))
    return into, cnt


def cases():
    rng = np.random.default_rng(9)
    out = {}
    out["random"] = random_hierarchy(rng, 3000, 0.05, 40, 3) + (1 << 15,)
    out["wide_ties"] = random_hierarchy(rng, 2000, 0.01, 2000, 1) + (1 << 10,)
    out["singletons"] = (np.arange(50), np.zeros(50, np.int64), 1 << 15)
    n = 200000                                                            # one chain: depth n - 1
    out["chain"] = (np.maximum(np.arange(n) - 1, 0), np.arange(n), 1 << 18)
    into, cnt = np.maximum(np.arange(n) - 1, 0), np.arange(n)             # two chains and a star on the second one's end
    into[n // 2] = n // 2
    cnt[n // 2:] -= n // 2
    into[n - 500:] = n - 501
    cnt[n - 500:] = cnt[n - 501] + 1 + (np.arange(500) % 3)
    out["chains_star"] = (into, cnt, 1 << 18)
    out["floor0"] = (np.array([0, 0, 1, 0, 3, 0]), np.array([0, 0, 9, 0, 9, 0]), 16)      # count-0 merges: height 1
    return out


def names_of(n, rng):
    names = ["genome%d.fa.gz" % g for g in range(n)]
    for i, g in enumerate(rng.choice(n, min(n, 3 * len(NASTY)), replace=False)):
        names[g] = NASTY[i % len(NASTY)] + ("" if i < len(NASTY) else str(i))
    return names


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("linkage_text")
    (d / "main.cpp").write_text(SRC)
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "host")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "text"), str(d / "main.cpp")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                  "-o", str(d / "text_san"), str(d / "main.cpp")])
    return str(d / "text"), str(d / "text_san")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("linkage_text_in")
    rng = np.random.default_rng(4)
    out = {}
    for name, (into, cnt, F) in cases().items():
        n = into.size
        ids = np.arange(n)
        child = into != ids
        assert np.all(into[child] < ids[child]) and np.all(cnt[~child] == 0)
        assert np.all((cnt[child] > cnt[into[child]]) | ((cnt[child] == 0) & (into[child] == 0)))    # (floor 0: roots join 0 at 0)
        names = names_of(n, rng)
        e = min(n - 1, 5000)
        lo = rng.integers(0, n - 1, e)
        hi = lo + 1 + rng.integers(0, n - 1 - lo)
        ec = np.sort(rng.integers(0, F + 1, e))[::-1]
        with open(d / (name + ".txt"), "w") as f:
            f.write("%d %d %d\n" % (n, e, F))
            f.write("".join("%d %d\n" % (a, b) for a, b in zip(into, cnt)))
            f.write("".join("%d %d %d\n" % (a, b, c) for a, b, c in zip(lo, hi, ec)))
            f.write("".join(nm + "\n" for nm in names))
        out[name] = (str(d / (name + ".txt")), into, cnt, F, names, lo, hi, ec)
    return out


_memo = {}


def expected(what, inp):
    """(computed once per input: the plain and the sanitizer run share it)"""
    if (what, inp[0]) not in _memo:
        _memo[what, inp[0]] = restated(what, inp)
    return _memo[what, inp[0]]


def restated(what, inp):
    _, into, cnt, F, names, lo, hi, ec = inp
    if what == "mst":
        return mst_text(lo, hi, ec, names, F)
    if what == "linkage":
        return linkage_text(into, cnt, names, F)
    return tree_text(into, cnt, names, F)


CASES = ["random", "wide_ties", "singletons", "chain", "chains_star", "floor0"]


@pytest.mark.parametrize("san", [0, 1], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("case", CASES)
def test_the_texts_equal_the_restatement(programs, inputs, case, san):
    for what in ("mst", "linkage", "tree"):
        r = subprocess.run([programs[san], what, inputs[case][0]], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stderr == b""                                           # (the sanitizers report there)
        assert r.stdout.decode() == expected(what, inputs[case]), (case, what)


def test_small_trees_by_hand():
    names = ["a", "b'c", "d", "e", "f"]
    # b'c and d join a at 12 (one node of three), e joins a at 8; f is a singleton.  F = 16.
    into, cnt = [0, 0, 0, 0, 4], [0, 12, 12, 8, 0]
    assert tree_text(into, cnt, names, 16) == "(('a':0.25,'b''c':0.25,'d':0.25):0.25,'e':0.5);\n'f';\n"
    # d joins b'c at 14 first; then b'c (with d) and e join a at 12
    into, cnt = [0, 0, 1, 0, 4], [0, 12, 14, 12, 0]
    assert tree_text(into, cnt, names, 16) == "('a':0.25,('b''c':0.125,'d':0.125):0.125,'e':0.25);\n'f';\n"
    assert linkage_text(into, cnt, names, 16) == "a\ta\t0\nb'c\ta\t0.75\nd\tb'c\t0.875\ne\ta\t0.75\nf\tf\t0\n"
    assert mst_text([1, 0, 0], [2, 1, 3], [14, 12, 12], names, 16) == "b'c\td\t0.875\na\tb'c\t0.75\na\te\t0.75\n"
