"""CPU: the `niqki` option parser knows --derep (long only), and a host program built on an engine without
niqki_dereplicate says so before any work: the program is built on the fake engine of tests/host_san (the C ABI
answered on the CPU, niqki_dereplicate not among its symbols), as test_cli_selfjoin_cpu.py does, into its own path.
Also here, because it needs no device: the definition of the dereplication in plain Python (expected_derep) and what
it gives on the reference's golden matrix of the nine E. coli genomes -- what tests/test_cli_derep.py holds the
program to."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_selfjoin_cpu import expected_clusters, golden_counts

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_derep")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_derep_option(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    assert "--derep <filename>" in r.stderr + r.stdout


def test_derep_needs_a_file_name(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--derep"], tmp_path)
    assert r.returncode == 1 and "Option 'derep' requires a non-empty argument" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--derep="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--derep", "out.tsv"], tmp_path)
    assert r.returncode == 1 and "niqki: this engine has no dereplication" in r.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "o.gz").exists()      # before any work


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "--derep", "out.tsv"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "no dereplication" not in r.stderr
    assert not (tmp_path / "out.tsv").exists()


# ---- the definition, and the expectation of the E. coli dereplication tests -------------------------------------

def derep_labels(counts, thr):
    """The definition.  counts: a symmetric matrix (anything indexable as counts[a][b] or counts[a, b]).  Genomes in
    index order: t is a representative iff no representative g < t has count(t, g) >= thr; any other genome gets the
    linked representative (of any index position) with the largest count, among equal counts the smallest."""
    n = len(counts)
    reps = []
    for t in range(n):
        if not any(counts[t][g] >= thr for g in reps):
            reps.append(t)
    is_rep = set(reps)
    labels = []
    for t in range(n):
        if t in is_rep:
            labels.append(t)
        else:
            labels.append(max((r for r in reps if counts[t][r] >= thr), key=lambda r: (counts[t][r], -r)))
    return labels, reps


def expected_derep(names, counts, min_score):
    """lines of `niqki --derep`: groups in the index order of their representative, its own line first, then its
    members in index order"""
    labels, reps = derep_labels(counts, min_score)
    out = []
    for r in reps:
        out.append("%s\t%s\n" % (names[r], names[r]))
        out += ["%s\t%s\n" % (names[r], names[g]) for g in range(len(names)) if labels[g] == r and g != r]
    return "".join(out)


TABLE = [  # -J, min_score, representatives, labels of 01..09
    (0.97, 31784, "01 02 03 05 07 09", "01 02 03 03 05 05 07 07 09"),
    (0.9, 29491, "01 05 09", "01 01 05 05 05 05 09 09 09"),
    (0.8, 26214, "01 09", "01 01 01 01 09 09 09 09 09"),
    (0.1, 3276, "01", "01 01 01 01 01 01 01 01 01"),
]


@pytest.mark.parametrize("j,ms,reps,labels", TABLE)
def test_what_the_golden_matrix_says_about_the_e_coli_representatives(j, ms, reps, labels):
    names, c = golden_counts()
    assert int(np.uint32(j * 32768)) == ms
    lines = expected_derep(names, c, ms).splitlines()
    assert len(lines) == 9
    pairs = [tuple(x[5:7] for x in ln.split("\t")) for ln in lines]
    assert [r for r, m in pairs if r == m] == reps.split()
    assert [dict((m, r) for r, m in pairs)["%02d" % i] for i in range(1, 10)] == labels.split()
    # groups in the order of their representative, whose own line leads; members in index order
    order = [r for r, _ in pairs]
    assert order == sorted(order)
    for rep in reps.split():
        members = [m for r, m in pairs if r == rep]
        assert members[0] == rep and members[1:] == sorted(members[1:])
    # no oracle needed: independent, dominating
    lab, rp = derep_labels(c, ms)
    assert all(c[a, b] < ms for a in rp for b in rp if a != b)
    assert all(lab[g] in rp and (lab[g] == g or c[g, lab[g]] >= ms) for g in range(9))


def test_genome_03_goes_to_a_representative_that_comes_after_it():
    names, c = golden_counts()
    assert c[2, 0] == 30737 and c[2, 4] == 30858 and min(c[2, 0], c[2, 4]) >= 29491
    lab, _ = derep_labels(c, 29491)
    assert lab[2] == 4


@pytest.mark.parametrize("j", [0.9, 0.8])
def test_dereplication_is_not_single_linkage(j):
    names, c = golden_counts()
    ms = int(np.uint32(j * 32768))
    assert expected_derep(names, c, ms) != expected_clusters(names, c, ms)
    assert len(derep_labels(c, ms)[1]) > 1                 # ... which gives ONE cluster there
