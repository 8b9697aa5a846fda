"""CPU: the text of `niqki --report` (niqki_amd/host/report_file.h).  A stand-alone main over the header reads the
taxon texts, the parents, the four arrays of a tally, the totals and F from a file and prints the report; the bytes must
equal tests/tally_ref.report_text.  The same program is built once more with AddressSanitizer + UBSan and run on the
same inputs (a stand-alone program: no preloaded runtime)."""
import os
import subprocess

import numpy as np
import pytest

from tally_ref import NONE, report_text, tally

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>
#include "report_file.h"

// argv: one input file.  Line 1: "<n_taxa> <F> <queries> <classified> <no_hit> <no_common>"; then per taxon a line
// "<parent> <direct> <clade> <direct_best> <clade_best>\t<text>" (the text is the rest of the line, TABs included).
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::string line;
  if (!std::getline(in, line)) return 2;
  unsigned long long n = 0, F = 0, q = 0, c = 0, nh = 0, nc = 0;
  if (sscanf(line.c_str(), "%llu %llu %llu %llu %llu %llu", &n, &F, &q, &c, &nh, &nc) != 6) return 2;
  std::vector<std::string> texts;
  std::vector<uint32_t> parent;
  std::vector<uint64_t> direct, clade, direct_best, clade_best;
  for (unsigned long long t = 0; t < n; ++t) {
    if (!std::getline(in, line)) return 2;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos) return 2;
    unsigned long long p = 0, d = 0, cl = 0, db = 0, cb = 0;
    if (sscanf(line.substr(0, tab).c_str(), "%llu %llu %llu %llu %llu", &p, &d, &cl, &db, &cb) != 5) return 2;
    parent.push_back((uint32_t)p);
    direct.push_back(d);
    clade.push_back(cl);
    direct_best.push_back(db);
    clade_best.push_back(cb);
    texts.push_back(line.substr(tab + 1));
  }
  nqhost::ReportTotals totals;
  totals.queries = q;
  totals.classified = c;
  totals.no_hit = nh;
  totals.no_common = nc;
  const std::string out = nqhost::report_text(texts, parent, direct, clade, direct_best, clade_best, totals, (uint32_t)F);
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("report_file")
    (d / "main.cpp").write_text(SRC)
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "host")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "plain"), str(d / "main.cpp")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                  "-o", str(d / "san"), str(d / "main.cpp")])
    return [str(d / "plain"), str(d / "san")]


def report(programs, tmp_path, texts, parent, rows, F):
    """the program's bytes for the tally of `rows`; both builds agree"""
    direct, clade, direct_best, clade_best, totals = tally(rows, parent)
    head = "%d %d %d %d %d %d\n" % (len(texts), F, totals["queries"], totals["classified"], totals["no_hit"], totals["no_common"])
    body = "".join("%d %d %d %d %d\t%s\n" % (parent[t], direct[t], clade[t], direct_best[t], clade_best[t], texts[t]) for t in range(len(texts)))
    (tmp_path / "in.txt").write_bytes((head + body).encode())
    outs = []
    for prog in programs:
        r = subprocess.run([prog, "in.txt"], cwd=tmp_path, capture_output=True, timeout=60)
        assert r.returncode == 0, (prog, r.returncode, r.stderr.decode())
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    exp = report_text(texts, parent, direct, clade, direct_best, clade_best, totals, F)
    assert outs[0] == exp.encode()
    return exp


def rows_of(taxa, best=None, considered=None):
    t = np.array(taxa, np.uint32)
    return t, None if best is None else np.array(best, np.uint32), None if considered is None else np.array(considered, np.uint32)


F = 1 << 15


def test_two_roots(programs, tmp_path):
    texts = ["a.fa", "b.fa", "c.fa", "genus", "other tree"]
    parent = [3, 3, 4, 3, 4]
    text = report(programs, tmp_path, texts, parent,
                  rows_of([0, 0, 1, 2, 2, 2, 2, 3, NONE, NONE, NONE], [F, F // 2, F // 4, 100, 200, 300, 400, 5, 0, 7, 0], [1, 1, 2, 1, 1, 1, 1, 9, 0, 2, 0]), F)
    assert text == ("18.18\t2\t2\t-\t-\tunclassified\n"
                    "9.09\t1\t1\t-\t-\tno_common_taxon\n"
                    "36.36\t4\t1\t0\t0.437538\tgenus\n"                    # the two roots tie at 4: taxon 3 before taxon 4
                    "18.18\t2\t2\t1\t0.75\t  a.fa\n"
                    "9.09\t1\t1\t1\t0.25\t  b.fa\n"
                    "36.36\t4\t0\t0\t0.00762939\tother tree\n"
                    "36.36\t4\t4\t1\t0.00762939\t  c.fa\n")


def test_a_tie_between_siblings_comes_out_in_id_order(programs, tmp_path):
    texts = ["z", "y", "x", "root"]                                             # texts do not order anything
    parent = [3, 3, 3, 3]
    text = report(programs, tmp_path, texts, parent, rows_of([2, 0, 1, 2, 0, 1, 1], [10] * 7, [1] * 7), F)
    assert [ln.split("\t")[5] for ln in text.split("\n")[2:-1]] == ["root", "  y", "  z", "  x"]      # y: 3; z and x: 2 each, id 0 before id 2


def test_an_ancestor_without_rows_of_its_own(programs, tmp_path):
    texts = ["leaf", "mid", "top", "unused"]
    parent = [1, 2, 2, 2]
    text = report(programs, tmp_path, texts, parent, rows_of([0, 0, 0], [F, F, F], [1, 1, 1]), F)
    assert text.split("\n")[2:-1] == ["100.00\t3\t0\t0\t1\ttop", "100.00\t3\t0\t1\t1\t  mid", "100.00\t3\t3\t2\t1\t    leaf"]
    assert "unused" not in text


def test_no_queries(programs, tmp_path):
    text = report(programs, tmp_path, ["a", "b"], [1, 1], rows_of([]), F)
    assert text == "0.00\t0\t0\t-\t-\tunclassified\n0.00\t0\t0\t-\t-\tno_common_taxon\n"
    # only queries without a taxon: the two lines carry everything
    text = report(programs, tmp_path, ["a", "b"], [1, 1], rows_of([NONE, NONE, NONE], None, [0, 3, 0]), F)
    assert text == "66.67\t2\t2\t-\t-\tunclassified\n33.33\t1\t1\t-\t-\tno_common_taxon\n"


def test_a_text_with_a_tab_and_a_deep_path(programs, tmp_path):
    texts = ["tabs\tin a\tname", "Escherichia coli\tK-12"]
    text = report(programs, tmp_path, texts, [1, 1], rows_of([0, 1], [3, F], [1, 1]), 1 << 12)
    assert text.split("\n")[3] == "50.00\t1\t1\t1\t0.000732422\t  tabs\tin a\tname"
    n = 3000                                                                    # a path of 3000 levels: no recursion
    texts = ["t%d" % i for i in range(n)]
    parent = [0] + list(range(n - 1))
    text = report(programs, tmp_path, texts, parent, rows_of([n - 1, 5], [1, 2], [1, 1]), F)
    lines = text.split("\n")[2:-1]
    assert len(lines) == n and lines[0].startswith("100.00\t2\t0\t0\t") and lines[6].startswith("50.00\t1\t0\t6\t")
    assert lines[-1].endswith("\t" + "  " * (n - 1) + "t%d" % (n - 1))
