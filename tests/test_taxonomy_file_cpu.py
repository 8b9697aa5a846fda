"""CPU: the taxonomy file of `niqki --lca` (niqki_amd/host/taxonomy_file.h).  A stand-alone main over the header reads
the run's label texts and the file's bytes and prints what the parser made of them; the same program is built once more
with AddressSanitizer + UBSan and run on the same inputs (a stand-alone program: no preloaded runtime)."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "label_file.h"
#include "taxonomy_file.h"

// argv: labels file (one label text per line, '\n' only), taxonomy file (its bytes as the parser gets them).
// ok: "OK <taxa>", then per taxon "<parent id>\t<text>"; else "ERR <line>\t<message>".
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<std::string> labels;
  {
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) labels.push_back(line);
  }
  std::ifstream in(argv[2], std::ios::binary);
  const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const nqhost::TaxonomyFile tf = nqhost::parse_taxonomy_file(bytes.data(), bytes.size(), labels);
  if (!tf.error.empty()) {
    printf("ERR %zu\t%s\n", tf.error_line, tf.error.c_str());
    return tf.parent.empty() && tf.texts.empty() ? 0 : 3;
  }
  if (tf.parent.size() != tf.texts.size() || tf.texts.size() < labels.size()) return 3;
  printf("OK %zu\n", tf.texts.size());
  for (size_t t = 0; t < tf.texts.size(); ++t) {
    if (tf.parent[t] >= tf.texts.size()) return 3;
    printf("%u\t%s\n", tf.parent[t], tf.texts[t].c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxonomy_file")
    (d / "main.cpp").write_text(SRC)
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "host")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "plain"), str(d / "main.cpp")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                  "-o", str(d / "san"), str(d / "main.cpp")])
    return [str(d / "plain"), str(d / "san")]


def parse(programs, tmp_path, labels, data):
    (tmp_path / "labels.txt").write_bytes(b"".join(n.encode() + b"\n" for n in labels))
    (tmp_path / "taxonomy.txt").write_bytes(data)
    outs = []
    for prog in programs:
        r = subprocess.run([prog, "labels.txt", "taxonomy.txt"], cwd=tmp_path, capture_output=True, timeout=60)
        assert r.returncode == 0, (prog, r.returncode, r.stderr.decode())
        outs.append(r.stdout.decode())
    assert outs[0] == outs[1]
    lines = outs[0].split("\n")[:-1]
    if lines[0].startswith("ERR "):
        n, msg = lines[0][4:].split("\t", 1)
        return ("ERR", int(n), msg)
    rows = [ln.split("\t", 1) for ln in lines[1:]]
    return ("OK", int(lines[0][3:]), [int(a) for a, _ in rows], [b for _, b in rows])


LABELS = ["g01.fa", "g02.fa", "g03.fa", "g04.fa"]


def test_two_levels_over_the_labels(programs, tmp_path):
    data = b"genus A\tsp1\nsp1\tg01.fa\nsp1\tg02.fa\nsp2\tg03.fa\ngenus A\tsp2\n"
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, data)
    # the label texts keep their ids; new texts follow in order of first appearance, a line's parent before its child
    assert (ok, n) == ("OK", 7) and texts == LABELS + ["genus A", "sp1", "sp2"]
    assert parent == [5, 5, 6, 3, 4, 4, 4]                   # g04.fa, which no line names as a child, is a root; so is genus A
    # ... the same bytes once they were gzip'd and inflated again, without the last newline, with empty lines
    for other in (gzip.decompress(gzip.compress(data)), data[:-1], b"\n\n" + data.replace(b"\n", b"\n\n")):
        assert parse(programs, tmp_path, LABELS, other) == (ok, n, parent, texts)
    # the same line twice is one line
    assert parse(programs, tmp_path, LABELS, data + b"sp1\tg02.fa\ngenus A\tsp1\n") == (ok, n, parent, texts)


def test_no_file_no_labels_and_a_taxon_with_no_genome(programs, tmp_path):
    assert parse(programs, tmp_path, LABELS, b"") == ("OK", 4, [0, 1, 2, 3], LABELS)
    assert parse(programs, tmp_path, [], b"") == ("OK", 0, [], [])
    # a whole branch that carries no genome is fine, also without any label
    assert parse(programs, tmp_path, [], b"a\tb\nb\tc\n") == ("OK", 3, [0, 0, 1], ["a", "b", "c"])
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, b"fam\tgen\ngen\tg02.fa\nfam\tempty genus\nempty genus\tempty species\n")
    assert (ok, n) == ("OK", 8) and texts[4:] == ["fam", "gen", "empty genus", "empty species"]
    assert parent == [0, 5, 2, 3, 4, 4, 4, 6]
    # a label may be an interior taxon: g01.fa is the parent of g02.fa
    assert parse(programs, tmp_path, LABELS, b"g01.fa\tg02.fa\n") == ("OK", 4, [0, 0, 2, 3], LABELS)


def test_a_root_line(programs, tmp_path):
    """a line whose two texts are equal declares a root and is otherwise ignored: it names the taxon, and a later line
    may still put it under a parent"""
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, b"life\tlife\nlife\tg01.fa\ng03.fa\tg03.fa\n")
    assert (ok, n) == ("OK", 5) and texts == LABELS + ["life"] and parent == [4, 1, 2, 3, 4]
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, b"x\tx\ny\tx\nx\tx\nx\tg01.fa\n")
    assert (ok, n) == ("OK", 6) and texts == LABELS + ["x", "y"] and parent == [4, 1, 2, 3, 5, 5]


def test_the_child_is_the_rest_behind_the_first_tab(programs, tmp_path):
    labels = ["tabs\tin a name", "plain"]
    ok, n, parent, texts = parse(programs, tmp_path, labels, b"Escherichia coli K-12\ttabs\tin a name\n\tplain\n")
    assert (ok, n) == ("OK", 4) and texts == labels + ["Escherichia coli K-12", ""] and parent == [2, 3, 2, 3]   # (an empty text is a text)


def test_each_error_names_its_line(programs, tmp_path):
    ok, line, msg = parse(programs, tmp_path, LABELS, b"x\tg01.fa\n\nno tab here\nx\tg02.fa\n")
    assert (ok, line) == ("ERR", 3) and msg.startswith("line 3: ") and "TAB" in msg
    ok, line, msg = parse(programs, tmp_path, LABELS, b"x\tg01.fa\ny\tg02.fa\nx\tg03.fa\ny\tg01.fa")
    assert (ok, line) == ("ERR", 4) and "line 4: " in msg and "'g01.fa'" in msg and "'x'" in msg and "'y'" in msg
    # a two-cycle, a long cycle, a cycle closed through a label; the line that closes it is named
    ok, line, msg = parse(programs, tmp_path, LABELS, b"a\tb\nb\ta\n")
    assert (ok, line) == ("ERR", 2) and "line 2: " in msg and "cycle" in msg and "'a'" in msg
    ok, line, msg = parse(programs, tmp_path, LABELS, b"a\tb\nb\tc\nc\td\n\nd\te\nz\ta\ne\ta\n")
    assert (ok, line) == ("ERR", 7) and "two parents" in msg and "'z'" in msg and "'e'" in msg   # (z is a's parent already)
    ok, line, msg = parse(programs, tmp_path, LABELS, b"a\tb\nb\tc\nc\td\n\nd\te\ne\ta\n")
    assert (ok, line) == ("ERR", 6) and "line 6: " in msg and "cycle" in msg
    ok, line, msg = parse(programs, tmp_path, LABELS, b"g01.fa\tq\nq\tg02.fa\ng02.fa\tg01.fa\n")
    assert (ok, line) == ("ERR", 3) and "cycle" in msg
    # a chain of many levels is no cycle
    deep = b"".join(b"t%d\tt%d\n" % (i, i + 1) for i in range(3000)) + b"t3000\tg01.fa\n"
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, deep)
    assert (ok, n) == ("OK", 4 + 3001) and parent[0] == 4 + 3000 and parent[4] == 4 and parent[5] == 4


def test_crlf_is_not_trimmed(programs, tmp_path):
    """the carriage return belongs to the child's text, as in the label file: such a file names other taxa than the
    labels unless they end in it too"""
    ok, n, parent, texts = parse(programs, tmp_path, LABELS, b"x\tg01.fa\r\nx\tg02.fa\r\n")
    assert (ok, n) == ("OK", 7) and texts == LABELS + ["x", "g01.fa\r", "g02.fa\r"] and parent[:4] == [0, 1, 2, 3]
    ok, n, parent, texts = parse(programs, tmp_path, ["g01.fa\r", "g02.fa"], b"x\tg01.fa\r\nx\tg02.fa")
    assert (ok, n) == ("OK", 3) and parent == [2, 2, 2]
    ok, line, msg = parse(programs, tmp_path, LABELS, b"x\tg01.fa\n\r\n")                # "\r" is a line without a TAB
    assert (ok, line) == ("ERR", 2)
