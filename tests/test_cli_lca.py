"""GPU: the `niqki` program's --lca <file> / --lca-top <permille>: the list written for every -Q query holds at most one
entry, the text of the lowest taxon that contains all its near-best hits with the jaccard of its best hit, in the
unchanged -O format (niqki_set_taxonomy + niqki_staged_query_lca).  The expected text is tests/lca_ref.py over the lines
a plain run of the same index and queries writes, with the taxonomy of the file read here -- never the LCA run's own."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lca_ref import NONE, lca_lists

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
F = 1 << 15                                                   # the program's default sketch: -S 15
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
REPS = ["ecoli01p.fa.gz", "ecoli05p.fa.gz", "ecoli09p.fa.gz"]


def run(td, args, code=0):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=str(td), capture_output=True, text=True, timeout=600)
    assert r.returncode == code, r.stdout + r.stderr
    return r


def text_of(path):
    return gzip.open(str(path), "rt").read()


def parse(text):
    """[(query name, [(name, jaccard text), ...])] of -P lines whose names hold no blank"""
    out = []
    for line in text.split("\n"):
        if line:
            toks = line.rstrip(" ").split(" ")
            out.append((toks[0], [tuple(t.rsplit(":", 1)) for t in toks[1:]]))
    return out


def lca_text(plain, label_of, table, permille):
    """the text an --lca run must write, from the lists of the plain run (count = jaccard x F, which %g's six digits
    give back exactly), the label text of every genome name and the lines of the taxonomy file"""
    texts = list(dict.fromkeys(label_of[n] for n in NAMES))    # the labels first ...
    ids = {t: i for i, t in enumerate(texts)}
    parent = list(range(len(texts)))
    for line in table.split("\n"):
        if line:
            par, child = line.split("\t", 1)
            for t in (par, child):                             # ... then every new text
                if t not in ids:
                    ids[t] = len(texts)
                    texts.append(t)
                    parent.append(ids[t])
            if par != child:
                parent[ids[child]] = ids[par]
    genome_taxon = [ids[label_of[n]] for n in NAMES]
    off, counts, gids = [0], [], []
    for _, hits in plain:
        for gname, jac in hits:
            c = float(jac) * F
            assert abs(c - round(c)) < 0.05
            counts.append(int(round(c)))
            gids.append(NAMES.index(gname))
        off.append(len(counts))
    taxon, best, _, considered = lca_lists((off, counts, gids), genome_taxon, parent, permille)
    lines = []
    for (qname, hits), t, b, m in zip(plain, taxon, best, considered):
        entry = ""
        if hits:
            assert int(b) == int(round(float(hits[0][1]) * F)) and m >= 1
            entry = ("no_common_taxon" if t == NONE else texts[t]) + ":" + hits[0][1] + " "
        lines.append(qname + " " + entry + "\n")
    return "".join(lines)


@pytest.fixture(scope="module")
def ecoli(tmp_path_factory):
    """the --derep -J 0.9 groups of the nine genomes (representatives 01, 05, 09) and the plain -Q lists at -J 0.1"""
    td = tmp_path_factory.mktemp("lca")
    d = str(td / "derep.tsv")
    run(EDIR, ["-I", "file_of_file.txt", "-J", "0.9", "--derep", d, "-O", str(td / "unused.gz")])
    pairs = [ln.split("\t") for ln in text_of(d).split("\n") if ln]
    rep_of = {member: rep for rep, member in pairs}
    assert sorted(rep_of) == NAMES and sorted(set(rep_of.values())) == REPS
    run(EDIR, ["-I", "file_of_file.txt", "-Q", "file_of_file.txt", "-P", "-J", "0.1", "-O", str(td / "plain.gz")])
    plain = parse(text_of(td / "plain.gz"))
    assert [q for q, _ in plain] == NAMES and all(len(h) == 9 for _, h in plain)
    return td, d, rep_of, plain


BASE = ["-I", "file_of_file.txt", "-Q", "file_of_file.txt", "-P", "-J", "0.1"]


def test_genome_names_as_leaves(ecoli):
    """a two-level taxonomy over the genome names: the derep groups under one species; plain and gzip'd"""
    td, _, rep_of, plain = ecoli
    table = "".join("group_%s\t%s\n" % (rep_of[n][5:7], n) for n in NAMES) + "".join("E.coli\tgroup_%s\n" % r[5:7] for r in REPS)
    (td / "tax.tsv").write_text("\n" + table)
    (td / "tax.tsv.gz").write_bytes(gzip.compress(table.encode()))
    own = {n: n for n in NAMES}
    exp = {p: lca_text(plain, own, table, p) for p in (0, 100, 1000)}
    assert all(len(h) == 1 for _, h in parse(exp[0]))
    assert exp[1000] == "".join("%s E.coli:%s \n" % (q, h[0][1]) for q, h in plain)       # every hit considered: the species
    seen0 = {h[0][0] for _, h in parse(exp[0])}
    assert seen0 <= set(NAMES) | {"group_01", "group_05", "group_09", "E.coli"} and seen0 & set(NAMES)   # a query is its own best hit
    run(EDIR, BASE + ["-O", str(td / "a0.gz"), "--lca", str(td / "tax.tsv"), "--lca-top", "0"])
    run(EDIR, BASE + ["-O", str(td / "a100.gz"), "--lca=" + str(td / "tax.tsv.gz"), "--top", "1"])     # the default, gzip'd; --top is ignored
    run(EDIR, BASE + ["-O", str(td / "a1000.gz"), "--lca", str(td / "nowhere.tsv"), "--lca", str(td / "tax.tsv"), "--lca-top=1000"])
    assert text_of(td / "a0.gz") == exp[0]
    assert text_of(td / "a100.gz") == exp[100]
    assert text_of(td / "a1000.gz") == exp[1000]


def test_labels_of_collapse_as_leaves_and_two_roots(ecoli):
    """--collapse supplies the labels (the three representatives' names) and no collapsed list is written; groups 01 and
    05 under one species, group 09 a tree of its own: no_common_taxon where hits of both trees are considered"""
    td, derep, rep_of, plain = ecoli
    table = "species_A\t%s\nspecies_A\t%s\nspecies_B\tspecies_B\n" % (REPS[0], REPS[1])
    (td / "two.tsv").write_text(table)
    exp = {p: lca_text(plain, rep_of, table, p) for p in (0, 100, 1000)}
    assert exp[1000] == "".join("%s no_common_taxon:%s \n" % (q, h[0][1]) for q, h in plain)
    assert {h[0][0] for _, h in parse(exp[0])} <= set(REPS) | {"species_A", "no_common_taxon"}
    for p in (0, 100, 1000):
        out = td / ("b%d.gz" % p)
        run(EDIR, BASE + ["-O", str(out), "--collapse", derep, "--lca", str(td / "two.tsv"), "--lca-top", str(p)])
        assert text_of(out) == exp[p], p
    # --neighbors is not affected: its lines name genomes, and here they are the plain run's
    run(EDIR, BASE + ["-O", str(td / "both.gz"), "--collapse", derep, "--lca", str(td / "two.tsv"), "--neighbors"])
    both = parse(text_of(td / "both.gz"))
    assert both[:9] == plain and both[9:] == parse(exp[100])


def test_a_cyclic_file_ends_the_run_without_an_output_file(ecoli):
    td, derep, _, _ = ecoli
    (td / "cycle.tsv").write_text("a\t%s\nb\ta\n\nc\tb\na\tc\n" % NAMES[0])
    out = td / "cycle.gz"
    r = run(EDIR, BASE + ["-O", str(out), "--lca", str(td / "cycle.tsv")], code=1)
    assert "niqki: --lca" in r.stderr and "line 5: " in r.stderr and "cycle" in r.stderr
    assert not out.exists()
    r = run(EDIR, BASE + ["-O", str(out), "--lca", str(td / "missing.tsv")], code=1)
    assert "niqki: --lca" in r.stderr and not out.exists()
    (td / "bad_labels.tsv").write_text("x\tno_such_genome\n")
    r = run(EDIR, BASE + ["-O", str(out), "--collapse", str(td / "bad_labels.tsv"), "--lca", str(td / "two_unused.tsv")], code=1)
    assert "niqki: --collapse" in r.stderr and "line 1: " in r.stderr and not out.exists()
