"""GPU: the `niqki` program's --report <file> beside --lca: after the last query the taxon tally of all -Q / -l queries
of the run, one line per taxon (niqki_tally_begin + niqki_tally_read, niqki_amd/host/report_file.h).  The expected
bytes are tests/tally_ref.report_text over the tally that tests/tally_ref.tally derives from the -O lines of the same
run, with the taxonomy of the file read here -- never the engine's own tally -- and the values README.md states for
the nine example E. coli genomes are spelled out."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tally_ref import NONE, report_text, tally

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
F = 1 << 15                                                   # the program's default sketch: -S 15
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
GROUP = {1: "group01", 2: "group01", 3: "group05", 4: "group05", 5: "group05", 6: "group05", 7: "group09", 8: "group09", 9: "group09"}
TABLE = "".join("%s\t%s\n" % (GROUP[i], NAMES[i - 1]) for i in range(1, 10)) + "".join("E.coli\t%s\n" % g for g in ("group01", "group05", "group09"))
TEXTS = NAMES + ["group01", "group05", "group09", "E.coli"]    # taxonomy_file.h: the label texts, then first appearance
PARENT = [9, 9, 10, 10, 10, 10, 11, 11, 11, 12, 12, 12, 12]
BASE = ["-I", "file_of_file.txt", "-P", "-J", "0.1"]


def run(args, code=0):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=EDIR, capture_output=True, text=True, timeout=600)
    assert r.returncode == code, r.stdout + r.stderr
    return r


def text_of(path):
    return gzip.open(str(path), "rt").read()


def rows_of(out_text):
    """the LCA rows behind the -O lines of an --lca run: (taxon, best_count, considered), one per line; an entry's count
    is jaccard x F, which %g's six digits give back exactly"""
    taxon, best, considered = [], [], []
    for line in out_text.split("\n"):
        if not line:
            continue
        toks = line.rstrip(" ").split(" ")
        assert len(toks) <= 2
        if len(toks) == 1:                                     # no hit: no entry
            taxon.append(NONE), best.append(0), considered.append(0)
            continue
        text, jac = toks[1].rsplit(":", 1)
        c = float(jac) * F
        assert abs(c - round(c)) < 0.05
        best.append(int(round(c)))
        taxon.append(NONE if text == "no_common_taxon" else TEXTS.index(text))
        considered.append(2 if text == "no_common_taxon" else 1)
    return np.array(taxon, np.uint32), np.array(best, np.uint32), np.array(considered, np.uint32)


def table_of(report):
    """{taxon text: (clade, direct)} of a report's lines"""
    out = {}
    for line in report.split("\n")[:-1]:
        pct, clade, direct, depth, mean, text = line.split("\t", 5)
        out[text.lstrip(" ")] = (int(clade), int(direct))
    return out


@pytest.fixture(scope="module")
def td(tmp_path_factory):
    d = tmp_path_factory.mktemp("report")
    (d / "tax.tsv").write_text(TABLE)
    return d


def lca_run(td, tag, more):
    out, rep = td / (tag + ".gz"), td / (tag + ".report.gz")
    run(BASE + ["-O", str(out), "--lca", str(td / "tax.tsv"), "--report", str(rep)] + more)
    rows = rows_of(text_of(out))
    got = text_of(rep)
    assert got == report_text(TEXTS, PARENT, *tally(rows, PARENT), F)
    return rows, got, table_of(got)


def test_lca_top_35(td):
    rows, text, t = lca_run(td, "a35", ["-Q", "file_of_file.txt", "--lca-top", "35"])
    assert rows[0].size == 9
    assert t["unclassified"] == (0, 0) and t["no_common_taxon"] == (0, 0)
    assert t["E.coli"] == (9, 4) and t["group01"][1] == 1 and t["group05"][1] == 2 and t["group09"][1] == 2
    assert text.split("\n")[2].startswith("100.00\t9\t4\t0\t1\tE.coli")
    assert not any(n in t for n in NAMES)                      # no query stays on a genome: none has clade > 0


def test_lca_top_0(td):
    _, text, t = lca_run(td, "a0", ["-Q", "file_of_file.txt", "--lca-top=0"])
    assert t["unclassified"] == (0, 0) and t["no_common_taxon"] == (0, 0)
    assert all(t[n] == (1, 1) for n in NAMES)
    assert t["group01"] == (2, 0) and t["group05"] == (4, 0) and t["group09"] == (3, 0) and t["E.coli"] == (9, 0)
    lines = text.split("\n")
    assert [ln.split("\t")[5] for ln in lines[2:5]] == ["E.coli", "  group05", "    ecoli03p.fa.gz"]      # by clade, then by id
    assert lines[3].split("\t")[:5] == ["44.44", "4", "0", "1", "1"]


def test_the_default_lca_top(td):
    _, text, t = lca_run(td, "a100", ["-Q", "file_of_file.txt"])
    assert t == {"unclassified": (0, 0), "no_common_taxon": (0, 0), "E.coli": (9, 9)}
    assert text.count("\n") == 3


def test_lines_mode_feeds_the_same_tally(td):
    """-Q and -l in one run: whole files, then every line of a file of reads -- long pieces of three of the genomes and
    one of random bases, which hits nothing"""
    rng = np.random.default_rng(2)
    with open(td / "reads.fa", "wb") as f:
        for i, name in enumerate((NAMES[0], NAMES[4], NAMES[8])):
            seq = gzip.open(os.path.join(EDIR, name), "rb").read().split(b"\n")[1]
            for k in range(2):
                f.write(b">r%d_%d\n" % (i, k) + seq[k * 1500000:k * 1500000 + 1400000] + b"\n")
        f.write(b">random\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 200000)) + b"\n")
    rows, text, t = lca_run(td, "lines", ["-Q", "file_of_file.txt", "-l", str(td / "reads.fa"), "--lca-top", "35"])
    assert rows[0].size == 9 + 7
    assert t["unclassified"] == (1, 1)                         # the random read
    assert t["E.coli"][0] == 15 and t["E.coli"][1] >= 4
    assert text.split("\n")[0] == "6.25\t1\t1\t-\t-\tunclassified"


def test_refusals_write_nothing(td):
    out, rep = td / "no.gz", td / "no.report.gz"
    r = run(BASE + ["-Q", "file_of_file.txt", "-O", str(out), "--report", str(rep)], code=1)
    assert "niqki: --report needs --lca" in r.stderr and not out.exists() and not rep.exists()
    r = run(BASE + ["-Q", "file_of_file.txt", "-O", str(out), "--gpus", "2", "--lca", str(td / "tax.tsv"), "--report", str(rep)], code=1)
    assert "--lca needs a single-GPU index" in r.stderr and not out.exists() and not rep.exists()
