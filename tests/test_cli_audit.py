"""GPU: `niqki --audit <file>` on the nine E. coli genomes with the three groups --derep -J 0.9 makes of them: a line per
indexed genome with its nearest neighbour under its own label and under another one (niqki_set_labels + niqki_audit).
The expected lines are built from the oracle's count matrix of its own sketches of the nine files through
audit_ref.audit_matrix; genome 02 is the one the groups misplace."""
import gzip
import os

import numpy as np
import pytest

from audit_ref import NAMES as VERDICTS, NONE, audit_matrix
from conftest import ROOT
from test_cli_cover import file_sketch
from test_cli_pan import EDIR, F, GROUP_OF, NAMES
from test_cli_retain import gunzip, indexed_genomes, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("audit_cli")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "file_of_file.txt").write_text("".join(n + "\n" for n in NAMES))
    (d / "groups.tsv").write_text("".join("%s\t%s\n" % (GROUP_OF[n], n) for n in reversed(NAMES)))
    return d


def expected_lines(po, k):
    p = po.make_params(31, 15, 12, 4, 0.9)
    sk = np.stack([file_sketch(po, p, gzip.open(os.path.join(EDIR, n), "rb").read()) for n in NAMES])
    M = po.Index(p, sk).matrix_range(0, len(NAMES)).astype(np.uint32)
    texts = sorted(set(GROUP_OF.values()))
    labels = np.array([texts.index(GROUP_OF[n]) for n in NAMES], np.uint32)
    rows = audit_matrix(M, labels, p.min_score, k)
    near = lambda g, c: "-" if g == NONE else "%s:%g" % (NAMES[g], c / F)
    lines = []
    for i, (v, oc, og, fc, fg, vg, vn) in enumerate(zip(*[a.tolist() for a in rows])):
        lines.append("\t".join([NAMES[i], GROUP_OF[NAMES[i]], VERDICTS[v], near(og, oc), near(fg, fc),
                                "-" if fg == NONE else GROUP_OF[NAMES[fg]], "-" if vg == NONE else "%s:%d" % (GROUP_OF[NAMES[vg]], vn)]))
    return lines


@pytest.fixture(scope="module")
def expected(po):
    lines = expected_lines(po, 1)
    two = lines[1].split("\t")
    assert two[:3] == ["ecoli02p.fa.gz", "group01", "misplaced"]
    assert two[3].startswith("ecoli01p.fa.gz:") and two[4].startswith("ecoli03p.fa.gz:") and two[5] == "group05"
    assert two[3] == "ecoli01p.fa.gz:0.967773" and two[4] == "ecoli03p.fa.gz:0.968567" and two[6] == "group05:1"
    return lines


def test_audit_beside_collapse(work, expected):
    r = run(work, ["-I", "file_of_file.txt", "--collapse", "groups.tsv", "--audit", "a.gz", "-J", "0.9", "-O", "o.gz"])
    assert gunzip(work / "a.gz").decode().splitlines() == expected
    assert r.stdout.count("| Audit lasted (s)                  |") == 1 and indexed_genomes(r.stdout) == 9
    totals = [ln for ln in r.stdout.splitlines() if ln.startswith("Audit: ")]
    want = ", ".join("%d %s" % (sum(ln.split("\t")[2] == v for ln in expected), v) for v in VERDICTS)
    assert totals == ["Audit: " + want]


def test_audit_before_pan(work, expected):
    r = run(work, ["-I", "file_of_file.txt", "--pan", "groups.tsv", "--audit", "b.gz", "-J", "0.9", "-O", "p.gz"])
    assert gunzip(work / "b.gz").decode().splitlines() == expected       # the genomes were audited, not the unions
    assert indexed_genomes(r.stdout) == 3
    assert r.stdout.count("| Audit lasted (s)                  |") == 1 and r.stdout.count("| Pan sketches lasted (s)           |") == 1


def test_audit_k_votes(work, po):
    run(work, ["-I", "file_of_file.txt", "--collapse", "groups.tsv", "--audit", "k3.gz", "--audit-k", "3", "-J", "0.9", "-O", "k.gz"])
    assert gunzip(work / "k3.gz").decode().splitlines() == expected_lines(po, 3)


def test_a_bad_label_file_ends_the_run(work):
    (work / "bad.tsv").write_text("group01\tnobody.fa\n")
    r = run(work, ["-I", "file_of_file.txt", "--pan", "bad.tsv", "--audit", "c.gz", "-J", "0.9", "-O", "c_out.gz"], code=1)
    assert "niqki: --pan 'bad.tsv': line 1: " in r.stderr
    assert not (work / "c.gz").exists() and not (work / "c_out.gz").exists()
