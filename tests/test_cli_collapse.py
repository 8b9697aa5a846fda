"""GPU: the `niqki` program's --collapse <file>: the list written for every -Q / -l query holds one entry per label, the
label's text with the jaccard of its best member, in the unchanged -O format (niqki_set_labels +
niqki_staged_query_collapsed).  The expected text is the collapse, computed here, of the lines a plain run of the same
index and queries writes: per line the first entry of every label, in the line's order."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT, make_cli_workdir

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")


def run(td, args, code=0):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=str(td), capture_output=True, text=True, timeout=600)
    assert r.returncode == code, r.stdout + r.stderr
    return r


def text_of(path):
    return gzip.open(str(path), "rt").read()


def parse(text, name_tokens=1):
    """[(query name, [(genome name, jaccard text), ...])] of -P lines whose names are name_tokens blank-separated tokens"""
    out = []
    for line in text.split("\n"):
        if line:
            toks = line.rstrip(" ").split(" ")
            assert len(toks) % name_tokens == 0
            groups = [" ".join(toks[i:i + name_tokens]) for i in range(0, len(toks), name_tokens)]
            out.append((groups[0], [tuple(g.rsplit(":", 1)) for g in groups[1:]]))
    return out


def collapsed_text(plain, label_of, top=0):
    """the text a --collapse run must write, from the lists of the plain run: a genome without a label is its own"""
    lines = []
    for qname, hits in plain:
        seen, kept = set(), []
        for gname, jac in hits:
            lab = label_of.get(gname, gname)
            if lab not in seen:
                seen.add(lab)
                kept.append(lab + ":" + jac + " ")
        lines.append(qname + " " + "".join(kept[:top] if top else kept) + "\n")
    return "".join(lines)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, native, gold):
    _, meta = gold
    td = make_cli_workdir(tmp_path_factory.mktemp("collapse"), native, meta)
    (td / "reads2.fa").write_bytes((td / "reads.fa").read_bytes() * 2)
    return td


def test_e_coli_derep_file_fed_back(tmp_path):
    d = str(tmp_path / "derep.tsv")
    base = ["-I", "file_of_file.txt", "-Q", "file_of_file.txt", "-P"]
    run(EDIR, ["-I", "file_of_file.txt", "-J", "0.9", "--derep", d, "-O", str(tmp_path / "unused.gz")])
    pairs = [ln.split("\t") for ln in text_of(d).split("\n") if ln]
    label_of = {member: rep for rep, member in pairs}
    assert len(label_of) == 9 and sorted(set(label_of.values())) == ["ecoli01p.fa.gz", "ecoli05p.fa.gz", "ecoli09p.fa.gz"]
    run(EDIR, base + ["-J", "0.1", "-O", str(tmp_path / "plain.gz")])
    run(EDIR, base + ["-J", "0.1", "-O", str(tmp_path / "col.gz"), "--collapse", d])
    run(EDIR, base + ["-J", "0.1", "-O", str(tmp_path / "col2.gz"), "--collapse", "nowhere.txt", "--top", "2", "--collapse", d])
    plain = parse(text_of(tmp_path / "plain.gz"))
    assert len(plain) == 9 and all(len(h) == 9 for _, h in plain)       # nine genomes under -J 0.1: nine entries a line ...
    got = text_of(tmp_path / "col.gz")
    assert got == collapsed_text(plain, label_of)
    assert all(len(h) == 3 for _, h in parse(got))                      # ... three with the labels
    assert [h[0][0] for _, h in parse(got)] == [label_of[q] for q, _ in plain]
    assert text_of(tmp_path / "col2.gz") == collapsed_text(plain, label_of, top=2)
    # --neighbors is not affected: its lines name genomes, and here they are the plain run's
    run(EDIR, base + ["-J", "0.1", "-O", str(tmp_path / "both.gz"), "--collapse", d, "--neighbors"])
    both = parse(text_of(tmp_path / "both.gz"))
    assert both[:9] == plain and both[9:] == parse(got)


def test_a_taxonomy_style_file_plain_and_gzip(workdir):
    table = "".join("s__Synthetic:fam%d|strain (x)\tsyn%02d.fa\n" % (i // 4, i) for i in range(12) if i not in (3, 7))
    table = table.replace(" ", "_")                                      # (parse() splits lines at blanks)
    (workdir / "tax.tsv").write_text("\n" + table)
    (workdir / "tax.tsv.gz").write_bytes(gzip.compress(table.encode()))
    label_of = dict(reversed(ln.split("\t")) for ln in table.split("\n") if ln)
    assert len(label_of) == 10 and len(set(label_of.values())) == 3
    base = ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-J", "0.05", "-P"]
    run(workdir, base + ["-O", "plain.gz"])
    run(workdir, base + ["-O", "tax.gz", "--collapse", "tax.tsv"])
    run(workdir, base + ["-O", "taxz.gz", "--collapse=tax.tsv.gz"])
    plain = parse(text_of(workdir / "plain.gz"))
    exp = collapsed_text(plain, label_of)
    assert max(len(h) for _, h in plain) > 3 and "syn03.fa:" in exp and "s__Synthetic:fam0|strain_(x):" in exp
    assert text_of(workdir / "tax.gz") == exp and text_of(workdir / "taxz.gz") == exp


@pytest.mark.parametrize("name,table,line,word", [
    ("no_tab", "a\tsyn00.fa\nb syn01.fa\n", 2, "TAB"),
    ("unknown", "a\tsyn00.fa\n\na\tsyn99.fa\n", 3, "syn99.fa"),
    ("two_labels", "a\tsyn00.fa\nb\tsyn01.fa\nb\tsyn00.fa\n", 3, "two labels"),
])
def test_file_errors_end_the_run_without_an_output_file(workdir, name, table, line, word):
    (workdir / (name + ".tsv")).write_text(table)
    out = name + ".gz"
    r = run(workdir, ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-J", "0.05", "-P", "-O", out, "--collapse", name + ".tsv"], code=1)
    assert "niqki: --collapse" in r.stderr and "line %d: " % line in r.stderr and word in r.stderr
    assert not (workdir / out).exists()
    r = run(workdir, ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-P", "-O", out, "--collapse", "missing_" + name], code=1)
    assert "niqki: --collapse" in r.stderr and not (workdir / out).exists()


def test_lines_mode(workdir):
    # every read indexed twice under the same name (its header line): a line of the file applies to both copies
    table = "".join("R%d\t>read%d some text\n" % (i % 5, i) for i in range(30) if i % 7)
    (workdir / "reads.tsv").write_text(table)
    label_of = dict(reversed(ln.split("\t")) for ln in table.split("\n") if ln)
    base = ["-i", "reads2.fa", "-l", "reads.fa", "-S", "10", "-W", "10", "-J", "0.2", "-P"]
    run(workdir, base + ["-O", "lplain.gz"])
    run(workdir, base + ["-O", "lcol.gz", "--collapse", "reads.tsv"])
    plain = parse(text_of(workdir / "lplain.gz"), name_tokens=3)
    assert len(plain) == 30 and all(len(h) > 1 for _, h in plain)
    got = text_of(workdir / "lcol.gz")
    assert got == collapsed_text(plain, label_of)
    assert got.count("R3:") >= 4 and ">read7 some text:" in got      # labelled reads, and one that is its own label
