"""GPU: `niqki --merge <dump>` and `niqki --novel <file>` on the nine E. coli genomes.  A merged index must be the one
a run over all the genomes builds: the dump bytes and the query output are compared with such runs.  The novelty
filter is held to rules 0-2 of niqki_dereplicate_from restated here over the REFERENCE's golden matrix
(test_cli_selfjoin_cpu.golden_counts), and its dump to a run that indexes the kept genomes alone."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_selfjoin_cpu import golden_counts

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
FIRST = 5


def run(work, args, code=0):
    assert os.path.exists(BIN), "%s missing: run __graft_entry__.build()" % BIN
    r = subprocess.run([BIN] + args, cwd=work, capture_output=True, text=True, timeout=600)
    assert r.returncode == code, r.stdout + r.stderr
    return r


def gunzip(p):
    return gzip.open(str(p), "rb").read()


def indexed_genomes(stdout):
    return int(re.search(r"\| Number of indexed genomes\s+\|\s+(\d+) \|", stdout).group(1))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the nine genomes under their own names (links), the lists, and the dumps of 01-05, 06-09 and all nine"""
    d = tmp_path_factory.mktemp("merge_cli")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "nine.txt").write_text("".join(n + "\n" for n in NAMES))
    (d / "a.txt").write_text("".join(n + "\n" for n in NAMES[:FIRST]))
    (d / "b.txt").write_text("".join(n + "\n" for n in NAMES[FIRST:]))
    for part in ("a", "b", "nine"):
        run(d, ["-I", part + ".txt", "-J", "0.9", "-D", part + ".dump", "-O", "o_" + part + ".gz"])
    return d


def test_a_merged_index_is_the_index_of_all_nine(work):
    r = run(work, ["-L", "a.dump", "--merge", "b.dump", "-D", "ab.dump", "-Q", "nine.txt", "-O", "q_ab.gz"])
    assert indexed_genomes(r.stdout) == 9
    run(work, ["-L", "nine.dump", "-Q", "nine.txt", "-O", "q_nine.gz"])
    got = gunzip(work / "ab.dump")
    assert got == gunzip(work / "nine.dump")                                 # header, inflated payload and names
    assert got.endswith("".join(n + "\n" for n in NAMES).encode())
    text = gunzip(work / "q_ab.gz")
    assert text == gunzip(work / "q_nine.gz") and len(text.splitlines()) == 9


def test_two_merges_are_taken_in_command_line_order(work):
    r = run(work, ["--merge", "b.dump", "--merge", "a.dump", "-J", "0.9", "-D", "ba.dump", "-O", "o_ba.gz"])
    assert indexed_genomes(r.stdout) == 9
    order = NAMES[FIRST:] + NAMES[:FIRST]
    (work / "ba.txt").write_text("".join(n + "\n" for n in order))
    run(work, ["-I", "ba.txt", "-J", "0.9", "-D", "ba_ref.dump", "-O", "o_ba_ref.gz"])
    got = gunzip(work / "ba.dump")
    assert got.endswith("".join(n + "\n" for n in order).encode()) and got == gunzip(work / "ba_ref.dump")


def novel(counts, first, thr):
    """rules 0-2 of niqki_dereplicate_from over a matrix of counts: labels"""
    n = len(counts)
    rep = [g < first for g in range(n)]
    for t in range(first, n):
        rep[t] = not any(rep[g] and counts[t][g] >= thr for g in range(t))
    labels = list(range(n))
    for t in range(first, n):
        if not rep[t]:
            labels[t] = max((r for r in range(n) if rep[r] and r != t and counts[t][r] >= thr), key=lambda r: (counts[t][r], -r))
    return labels


def novel_lines(names, labels, first):
    """the --derep format and order, for the genomes from `first` on only"""
    out = []
    for r in sorted(set(labels[first:])):
        out += ["%s\t%s\n" % (names[r], names[g]) for g in [r] + [g for g in range(first, len(names)) if labels[g] == r and g != r]
                if g >= first]
    return "".join(out)


def test_the_novelty_filter_keeps_the_given_genomes_and_the_new_representatives(work):
    names, counts = golden_counts()
    assert names == NAMES
    thr = int(np.uint32(0.9 * 32768))
    labels = novel(counts, FIRST, thr)
    kept = [g for g in range(9) if labels[g] == g]
    assert kept[:FIRST] == list(range(FIRST)) and FIRST < len(kept) < 9      # 01-05 survive; the filter drops and keeps
    assert any(labels[g] < FIRST for g in range(FIRST, 9))                   # ... a new genome that a given one covers
    r = run(work, ["-L", "a.dump", "--merge", "b.dump", "--novel", "added.txt", "-J", "0.9", "-D", "db2.dump", "-O", "o_db2.gz"])
    assert gunzip(work / "added.txt").decode() == novel_lines(NAMES, labels, FIRST)
    assert r.stdout.count("| Novelty filter lasted (s)         |") == 1
    assert indexed_genomes(r.stdout) == len(kept)
    (work / "kept.txt").write_text("".join(NAMES[g] + "\n" for g in kept))
    run(work, ["-I", "kept.txt", "-J", "0.9", "-D", "kept.dump", "-O", "o_kept.gz"])
    got = gunzip(work / "db2.dump")
    assert got == gunzip(work / "kept.dump") and got.endswith("".join(NAMES[g] + "\n" for g in kept).encode())


def test_the_novelty_filter_after_an_index_input(work):
    """-L db.dump -I new.list --novel: the genomes of -L are given, whatever brings the others"""
    names, counts = golden_counts()
    labels = novel(counts, FIRST, int(np.uint32(0.9 * 32768)))
    kept = [g for g in range(9) if labels[g] == g]
    r = run(work, ["-L", "a.dump", "-I", "b.txt", "--novel", "added2.txt", "-J", "0.9", "-D", "db3.dump", "-O", "o_db3.gz"])
    assert gunzip(work / "added2.txt").decode() == novel_lines(NAMES, labels, FIRST) and indexed_genomes(r.stdout) == len(kept)
    assert gunzip(work / "db3.dump").endswith("".join(NAMES[g] + "\n" for g in kept).encode())
    # without -L nothing is given: --novel is --derep-dump's selection
    r = run(work, ["-I", "nine.txt", "--novel", "added3.txt", "-J", "0.9", "-O", "o_db4.gz"])
    plain = novel(counts, 0, int(np.uint32(0.9 * 32768)))
    assert gunzip(work / "added3.txt").decode() == novel_lines(NAMES, plain, 0)
    assert indexed_genomes(r.stdout) == sum(plain[g] == g for g in range(9))


def test_a_dump_with_other_parameters_is_refused_and_nothing_is_written(work):
    run(work, ["-I", "b.txt", "-S", "12", "-J", "0.9", "-D", "b12.dump", "-O", "o_b12.gz"])
    r = run(work, ["-L", "a.dump", "--merge", "b12.dump", "-D", "x.dump", "-Q", "nine.txt", "-O", "x.gz"], code=1)
    assert "--merge 'b12.dump'" in r.stderr and "lF" in r.stderr
    assert not (work / "x.dump").exists() and not (work / "x.gz").exists()
