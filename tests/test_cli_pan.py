"""GPU: `niqki --pan <file>` on the nine E. coli genomes: the index holds one entry per label of the file, named by the
label, whose sketch is the union of the members' sketches (niqki_unite).  The expected lines are the oracle's: its
sketches of the nine files, tests/unite_ref.py's minimum over each group, an oracle Index of the three results and its
answers to the nine queries."""
import gzip
import os

import numpy as np
import pytest

from conftest import ROOT
from test_cli_cover import file_sketch, lists, same_lists
from test_cli_retain import REF, gunzip, indexed_genomes, run
from unite_ref import unite_ref

pytestmark = pytest.mark.gpu
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
GROUP_OF = dict(zip(NAMES, ["group01"] * 2 + ["group05"] * 4 + ["group09"] * 3))
GROUPS = ["group01", "group05", "group09"]
F = 1 << 15


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("pan_cli")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "file_of_file.txt").write_text("".join(n + "\n" for n in NAMES))
    # (the lines in another order than the genomes: the entries follow the genomes, not the file)
    (d / "groups.tsv").write_text("".join("%s\t%s\n" % (GROUP_OF[n], n) for n in reversed(NAMES)))
    (d / "twice.tsv").write_text("group01\t%s\ngroup05\t%s\n\ngroup05\t%s\n" % (NAMES[0], NAMES[2], NAMES[0]))
    (d / "tax.tsv").write_text("E.coli\tgroup01\nE.coli\tgroup05\n")
    return d


@pytest.fixture(scope="module")
def expected(po):
    """the lists of the nine queries against the three unions, by the oracle: [(query name, [(group, jaccard)])]"""
    p = po.make_params(31, 15, 12, 4, 0.1)
    sk = np.stack([file_sketch(po, p, gzip.open(os.path.join(EDIR, n), "rb").read()) for n in NAMES])
    u, ids = unite_ref(sk, [GROUPS.index(GROUP_OF[n]) for n in NAMES])
    assert u.shape == (3, F) and list(ids) == [0, 0, 1, 1, 1, 1, 2, 2, 2]
    ix = po.Index(p, u)
    out = []
    for n, q in zip(NAMES, sk):
        hc, hg = ix.query(q, min_score=p.min_score)
        out.append((n, [(GROUPS[int(g)], float("%g" % (int(c) / F))) for c, g in zip(hc, hg)]))
    return out


@pytest.fixture(scope="module")
def pan_run(work):
    return run(work, ["-I", "file_of_file.txt", "--pan", "groups.tsv", "-D", "pan.dump", "-Q", "file_of_file.txt", "-J", "0.1",
                      "-O", "out.gz"])


def test_the_index_is_the_pan_index(work, pan_run, expected):
    assert indexed_genomes(pan_run.stdout) == 3
    assert pan_run.stdout.count("| Pan sketches lasted (s)           |") == 1
    got = lists(work / "out.gz")
    assert len(got) == 9 and all(name in GROUPS for _, hits in got for name, _ in hits)
    same_lists(got, expected)
    assert gunzip(work / "pan.dump").endswith("".join(g + "\n" for g in GROUPS).encode())


def test_the_dump_loads_as_the_pan_index(work, pan_run, expected):
    r = run(work, ["-L", "pan.dump", "-Q", "file_of_file.txt", "-J", "0.1", "-O", "loaded.gz"])
    assert indexed_genomes(r.stdout) == 3
    assert gunzip(work / "loaded.gz") == gunzip(work / "out.gz")
    # -L db.dump --pan species.tsv -D species.dump rewrites a dump without reading a genome
    run(work, ["-I", "file_of_file.txt", "-J", "0.1", "-D", "nine.dump", "-O", "nine.gz"])
    r = run(work, ["-L", "nine.dump", "--pan", "groups.tsv", "-D", "pan2.dump", "-O", "pan2.gz"])
    assert indexed_genomes(r.stdout) == 3 and gunzip(work / "pan2.dump") == gunzip(work / "pan.dump")


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/niqki_ref is built where the reference's sources exist (oracle/Makefile)")
def test_the_reference_program_answers_the_same_from_the_dump(work, pan_run):
    run(work, ["-L", "pan.dump", "-Q", "file_of_file.txt", "-J", "0.1", "-O", "ref.gz"], binary=REF, env={"OMP_NUM_THREADS": "1"})
    same_lists(lists(work / "ref.gz"), lists(work / "out.gz"))


def test_the_groups_are_the_leaves_of_lca(work, pan_run):
    plain = lists(work / "out.gz")
    for permille in (0, 1000):
        out = "lca%d.gz" % permille
        run(work, ["-I", "file_of_file.txt", "--pan", "groups.tsv", "--lca", "tax.tsv", "--lca-top", str(permille), "-Q",
                   "file_of_file.txt", "-J", "0.1", "-O", out])
        got = lists(work / out)
        assert [q for q, _ in got] == NAMES
        for (q, hits), (_, entry) in zip(plain, got):
            best = hits[0][1]
            taken = {g for g, j in hits if permille == 1000 or j == best}
            want = taken.pop() if len(taken) == 1 else "E.coli" if taken <= {"group01", "group05"} else "no_common_taxon"
            assert len(entry) == 1 and entry[0] == (want, best), (q, permille)
    assert {e[0][0] for _, e in lists(work / "lca0.gz")} & set(GROUPS)         # the group texts resolve as leaves


def test_a_member_under_two_labels_ends_the_run(work):
    r = run(work, ["-I", "file_of_file.txt", "--pan", "twice.tsv", "-D", "t.dump", "-Q", "file_of_file.txt", "-O", "t.gz"], code=1)
    assert "niqki: --pan 'twice.tsv': line 4: " in r.stderr and "two labels" in r.stderr
    assert not (work / "t.gz").exists() and not (work / "t.dump").exists()
    r = run(work, ["-I", "file_of_file.txt", "--pan", "nowhere.tsv", "-O", "t.gz"], code=1)
    assert "niqki: --pan" in r.stderr and not (work / "t.gz").exists()


def test_pan_needs_one_gpu(work):
    r = run(work, ["-I", "file_of_file.txt", "--gpus", "2", "--pan", "groups.tsv", "-D", "g.dump", "-O", "g.gz"], code=1,
            env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr
    assert not (work / "g.dump").exists() and not (work / "g.gz").exists()


def test_a_paged_index_unites_too(work, pan_run):
    r = run(work, ["-I", "file_of_file.txt", "--resident-mib", "1", "--pan", "groups.tsv", "-D", "paged.dump", "-Q", "file_of_file.txt",
                   "-J", "0.1", "-O", "paged.gz"])
    assert indexed_genomes(r.stdout) == 3
    assert gunzip(work / "paged.dump") == gunzip(work / "pan.dump") and gunzip(work / "paged.gz") == gunzip(work / "out.gz")
