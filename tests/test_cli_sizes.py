"""GPU: `niqki --sizes <file>` and `niqki --containment` on the nine E. coli genomes.  The expected text is the
reference's: the oracle's sketches of the nine files, tests/registers_ref.py's histograms, estimator and containment over
them, and an oracle Index for the counts -- never the register calls themselves."""
import gzip
import os

import numpy as np
import pytest

import registers_ref as rr
from conftest import ROOT
from test_cli_cover import file_sketch
from test_cli_retain import gunzip, indexed_genomes, run

pytestmark = pytest.mark.gpu
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
GROUP_OF = dict(zip(NAMES, ["group01"] * 2 + ["group05"] * 4 + ["group09"] * 3))
GROUPS = ["group01", "group05", "group09"]
S, W, H = 15, 12, 4


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("sizes_cli")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "file_of_file.txt").write_text("".join(n + "\n" for n in NAMES))
    (d / "groups.tsv").write_text("".join("%s\t%s\n" % (GROUP_OF[n], n) for n in NAMES))
    return d


@pytest.fixture(scope="module")
def oracle(po):
    """the nine sketches, their sizes, and the text of the --sizes file"""
    p = po.make_params(31, S, W, H, 0.1)
    sk = np.stack([file_sketch(po, p, gzip.open(os.path.join(EDIR, n), "rb").read()) for n in NAMES])
    hist = rr.hist_ref(sk, W, H)
    return p, sk, [rr.estimate(h, S, H) for h in hist], rr.sizes_text(NAMES, hist, S, H)


def expected_lines(po, oracle, top=0):
    p, sk, sizes, _ = oracle
    ix = po.Index(p, sk)
    out = []
    for n, q, qs in zip(NAMES, sk, sizes):
        hc, hg = ix.query(q, min_score=p.min_score)
        hits = list(zip(hc, hg))[: top or None]
        out.append(n + " " + "".join(rr.containment_entry(NAMES[int(g)], int(c), S, qs, sizes[int(g)]) + " " for c, g in hits))
    return out


def lines(path):
    return gunzip(path).decode().split("\n")[:-1]


@pytest.fixture(scope="module")
def plain_run(work):
    return run(work, ["-I", "file_of_file.txt", "--sizes", "sizes.gz", "-D", "nine.dump", "-Q", "file_of_file.txt", "-J", "0.1",
                      "-O", "plain.gz"])


def test_sizes_file_is_the_reference_text(work, plain_run, oracle):
    assert gunzip(work / "sizes.gz").decode() == oracle[3]
    assert all(s == rr.OK for _, s in oracle[2])
    assert plain_run.stdout.count("| Sizes lasted (s)                  |") == 1
    assert indexed_genomes(plain_run.stdout) == 9


def test_containment_extends_the_plain_list(work, plain_run, po, oracle):
    run(work, ["-I", "file_of_file.txt", "--containment", "-Q", "file_of_file.txt", "-J", "0.1", "-O", "cont.gz"])
    got, plain, want = lines(work / "cont.gz"), lines(work / "plain.gz"), expected_lines(po, oracle)
    assert got == want
    assert len(plain) == 9
    for g, pl in zip(got, plain):                  # the plain list with two more fields
        gt, pt = g.split(" "), pl.split(" ")
        assert len(gt) == len(pt) and gt[0] == pt[0]
        assert all(a.rsplit(":", 2)[0] == b and a.count(":") == 3 for a, b in zip(gt[1:-1], pt[1:-1]))
    # ecoli01p in ecoli09p: 0.887 of the first's k-mers against 0.884 exact (test_registers_ref_cpu.py)
    entry = [t for t in got[0].split(" ") if t.startswith(NAMES[8] + ":")][0].split(":")
    assert entry[1] == "0.791321" and abs(float(entry[2]) - 0.887) < 5e-4


def test_top_keeps_the_first_three(work, po, oracle):
    run(work, ["-I", "file_of_file.txt", "--containment", "--top", "3", "-Q", "file_of_file.txt", "-J", "0.1", "-O", "top.gz"])
    got = lines(work / "top.gz")
    assert got == expected_lines(po, oracle, top=3)
    assert all(len(g.split(" ")) == 5 for g in got)


def test_a_paged_index_answers_the_same(work, po, oracle):
    run(work, ["-I", "file_of_file.txt", "--resident-mib", "1", "--containment", "--sizes", "paged_sizes.gz", "-Q", "file_of_file.txt",
               "-J", "0.1", "-O", "paged.gz"])
    assert lines(work / "paged.gz") == expected_lines(po, oracle)
    assert gunzip(work / "paged_sizes.gz").decode() == oracle[3]


def test_a_loaded_dump_gives_the_same_sizes(work, plain_run, oracle):
    r = run(work, ["-L", "nine.dump", "--sizes", "loaded_sizes.gz", "-O", "loaded.gz"])
    assert indexed_genomes(r.stdout) == 9
    assert gunzip(work / "loaded_sizes.gz").decode() == oracle[3]


def test_pan_sizes_list_the_labels(work, oracle):
    r = run(work, ["-I", "file_of_file.txt", "--pan", "groups.tsv", "--sizes", "pan_sizes.gz", "-O", "pan.gz"])
    assert indexed_genomes(r.stdout) == 3
    rows = [ln.split("\t") for ln in lines(work / "pan_sizes.gz")]
    assert [r_[0] for r_ in rows] == GROUPS and all(r_[2] == "ok" for r_ in rows)
    # a union is at least as large as its largest member, up to the estimator's error on both
    _, _, sizes, _ = oracle
    for (name, kmers, _), members in zip(rows, ([0, 1], [2, 3, 4, 5], [6, 7, 8])):
        assert float(kmers) >= max(sizes[m][0] for m in members) * (1 - 2 * 4 * 1.04 / (1 << S) ** 0.5), name


def test_refused_with_what_replaces_the_list(work):
    r = run(work, ["-I", "file_of_file.txt", "--containment", "--cover", "-Q", "file_of_file.txt", "-O", "no.gz"], code=1)
    assert "--containment" in r.stderr and not (work / "no.gz").exists()
