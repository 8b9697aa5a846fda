"""CPU: the label file of `niqki --collapse` (niqki_amd/host/label_file.h).  A stand-alone main over the header reads
the index's names and the file's bytes and prints what the parser made of them; the same program is built once more
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

// argv: names file (one name per line, '\n' only), label file (its bytes as the parser gets them).
// ok: "OK <labels>", then per genome "<label id>\t<label text>"; else "ERR <line>\t<message>".
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<std::string> names;
  {
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) names.push_back(line);
  }
  std::ifstream in(argv[2], std::ios::binary);
  const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const nqhost::LabelFile lf = nqhost::parse_label_file(bytes.data(), bytes.size(), names);
  if (!lf.error.empty()) {
    printf("ERR %zu\t%s\n", lf.error_line, lf.error.c_str());
    return lf.label_of.empty() && lf.texts.empty() ? 0 : 3;
  }
  if (lf.label_of.size() != names.size()) return 3;
  printf("OK %zu\n", lf.texts.size());
  for (uint32_t id : lf.label_of) {
    if (id >= lf.texts.size()) return 3;
    printf("%u\t%s\n", id, lf.texts[id].c_str());
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("label_file")
    (d / "main.cpp").write_text(SRC)
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "niqki_amd", "host")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "plain"), str(d / "main.cpp")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                  "-o", str(d / "san"), str(d / "main.cpp")])
    return [str(d / "plain"), str(d / "san")]


def parse(programs, tmp_path, names, data):
    (tmp_path / "names.txt").write_bytes(b"".join(n.encode() + b"\n" for n in names))
    (tmp_path / "labels.txt").write_bytes(data)
    outs = []
    for prog in programs:
        r = subprocess.run([prog, "names.txt", "labels.txt"], cwd=tmp_path, capture_output=True, timeout=60)
        assert r.returncode == 0, (prog, r.returncode, r.stderr.decode())
        outs.append(r.stdout.decode())
    assert outs[0] == outs[1]
    lines = outs[0].split("\n")[:-1]
    if lines[0].startswith("ERR "):
        n, msg = lines[0][4:].split("\t", 1)
        return ("ERR", int(n), msg)
    rows = [ln.split("\t", 1) for ln in lines[1:]]
    return ("OK", int(lines[0][3:]), [int(a) for a, _ in rows], [b for _, b in rows])


NAMES = ["g01.fa", "g02.fa", "g03.fa", "g04.fa", "g05.fa", "g06.fa"]


def test_a_derep_shaped_file(programs, tmp_path):
    data = b"g01.fa\tg01.fa\ng01.fa\tg02.fa\ng01.fa\tg03.fa\ng04.fa\tg04.fa\ng04.fa\tg06.fa\ng05.fa\tg05.fa\n"
    ok, n, ids, texts = parse(programs, tmp_path, NAMES, data)
    assert (ok, n) == ("OK", 3)
    assert texts == ["g01.fa", "g01.fa", "g01.fa", "g04.fa", "g05.fa", "g04.fa"]
    assert ids[0] == ids[1] == ids[2] and ids[3] == ids[5] and len({ids[0], ids[3], ids[4]}) == 3
    # ... the same bytes once they were gzip'd and inflated again, without the last newline, with empty lines
    for other in (gzip.decompress(gzip.compress(data)), data[:-1], b"\n\n" + data.replace(b"\n", b"\n\n")):
        assert parse(programs, tmp_path, NAMES, other) == (ok, n, ids, texts)


def test_free_text_labels_and_unnamed_genomes(programs, tmp_path):
    data = "Escherichia coli K-12\tg02.fa\nEscherichia coli K-12\tg05.fa\nno\ttabs\tin members? yes\tg03.fa\n".encode()
    names = NAMES[:5] + ["tabs\tin members? yes\tg03.fa"]
    ok, n, ids, texts = parse(programs, tmp_path, names, data)
    assert ok == "OK"
    # a genome that no line names is a label of its own, named by its own name; the member is the rest behind the FIRST tab
    assert texts == ["g01.fa", "Escherichia coli K-12", "g03.fa", "g04.fa", "Escherichia coli K-12", "no"]
    assert n == 5 and ids[1] == ids[4] and len(set(ids)) == 5
    assert parse(programs, tmp_path, NAMES, b"") == ("OK", 6, list(range(6)), NAMES)
    assert parse(programs, tmp_path, [], b"") == ("OK", 0, [], [])


def test_a_name_that_several_genomes_carry(programs, tmp_path):
    names = ["a", "b", "a", "c", "a"]
    ok, n, ids, texts = parse(programs, tmp_path, names, b"x\ta\ny\tc\nx\ta\n")       # (the same line twice is one statement)
    assert (ok, n) == ("OK", 3) and texts == ["x", "b", "x", "y", "x"] and ids[0] == ids[2] == ids[4]
    # unnamed, they share their name's label; and an unnamed genome whose name is a label's text joins that label
    ok, n, ids, texts = parse(programs, tmp_path, names, b"a\tc\n")
    assert (ok, n) == ("OK", 2) and texts == ["a", "b", "a", "a", "a"] and ids[0] == ids[3]


def test_each_error_names_its_line(programs, tmp_path):
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\tg01.fa\n\nno tab here\nx\tg02.fa\n")
    assert (ok, line) == ("ERR", 3) and msg.startswith("line 3: ") and "TAB" in msg
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\tg01.fa\nx\tg99.fa\n")
    assert (ok, line) == ("ERR", 2) and "line 2: " in msg and "'g99.fa'" in msg
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\tg01.fa\ny\tg02.fa\nx\tg03.fa\ny\tg01.fa")
    assert (ok, line) == ("ERR", 4) and "line 4: " in msg and "'g01.fa'" in msg and "'x'" in msg and "'y'" in msg
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\t\n")                         # an empty member names no genome
    assert (ok, line) == ("ERR", 1)


def test_crlf_is_not_trimmed(programs, tmp_path):
    """the carriage return belongs to the member's name, as in the program's other inputs: such a file names genomes
    only if they were indexed under names that end in it"""
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\tg01.fa\r\nx\tg02.fa\r\n")
    assert (ok, line) == ("ERR", 1) and "g01.fa\r" in msg
    ok, n, ids, texts = parse(programs, tmp_path, ["g01.fa\r", "g02.fa"], b"x\tg01.fa\r\nx\tg02.fa")
    assert (ok, n) == ("OK", 1) and texts == ["x", "x"]
    ok, line, msg = parse(programs, tmp_path, NAMES, b"x\tg01.fa\n\r\n")                # "\r" is a line without a TAB
    assert (ok, line) == ("ERR", 2)
