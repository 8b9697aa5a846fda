"""GPU: `niqki --remove <file>` and `niqki --derep-dump <file>` on the nine E. coli genomes.  Dropping genomes must leave
the index a run that never saw them would have built: the dump bytes and the query output are compared with runs that
index the shorter list, the dereplication list with the definition on the REFERENCE's golden matrix
(test_cli_derep_cpu.py), and the dereplicated dump, where oracle/_ref holds the reference's own program, with the dump
the reference writes for the three representatives."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_derep_cpu import expected_derep
from test_cli_selfjoin_cpu import golden_counts

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
REF = os.path.join(ROOT, "oracle", "_ref", "niqki_ref")
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
REPS = [NAMES[0], NAMES[4], NAMES[8]]                     # -J 0.9: test_cli_derep_cpu.py TABLE
TWO = [NAMES[2], NAMES[6]]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the nine genomes under their own names (links), and the lists of the tests"""
    d = tmp_path_factory.mktemp("retain_cli")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "file_of_file.txt").write_text("".join(n + "\n" for n in NAMES))
    (d / "three.txt").write_text("".join(n + "\n" for n in REPS))
    (d / "seven.txt").write_text("".join(n + "\n" for n in NAMES if n not in TWO))
    (d / "two.txt").write_text("".join(n + "\n" for n in TWO))
    (d / "empty.txt").write_text("")
    (d / "unknown.txt").write_text(TWO[0] + "\necoli10p.fa.gz\n")
    return d


def run(work, args, code=0, env=None, binary=BIN):
    assert os.path.exists(binary), "%s missing: run __graft_entry__.build()" % binary
    r = subprocess.run([binary] + args, cwd=work, capture_output=True, text=True, timeout=600,
                       env=None if env is None else dict(os.environ, **env))
    assert r.returncode == code, r.stdout + r.stderr
    return r


def gunzip(p):
    return gzip.open(str(p), "rb").read()


def indexed_genomes(stdout):
    return int(re.search(r"\| Number of indexed genomes\s+\|\s+(\d+) \|", stdout).group(1))


@pytest.fixture(scope="module")
def derep_run(work):
    r = run(work, ["-I", "file_of_file.txt", "-J", "0.9", "--derep", "d.tsv", "--derep-dump", "r.dump", "-O", "o_derep.gz"])
    return r


def test_derep_dump_holds_the_representatives_only(work, derep_run):
    names, counts = golden_counts()
    assert gunzip(work / "d.tsv").decode() == expected_derep(names, counts, int(np.uint32(0.9 * 32768)))   # of the FULL index
    assert derep_run.stdout.count("| Dereplication lasted (s)          |") == 1
    assert indexed_genomes(derep_run.stdout) == 3
    run(work, ["-I", "three.txt", "-J", "0.9", "-D", "three.dump", "-O", "o_three.gz"])
    got = gunzip(work / "r.dump")
    assert got == gunzip(work / "three.dump")
    assert got.endswith("".join(n + "\n" for n in REPS).encode())


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/niqki_ref is built where the reference's sources exist (oracle/Makefile)")
def test_derep_dump_equals_the_reference_programs_dump_of_the_representatives(work, derep_run):
    run(work, ["-I", "three.txt", "-J", "0.9", "-D", "ref_three.dump", "-O", "o_ref.gz"], binary=REF,
        env={"OMP_NUM_THREADS": "1"})
    assert gunzip(work / "r.dump") == gunzip(work / "ref_three.dump")


def test_the_rest_of_a_derep_dump_run_is_answered_by_the_dereplicated_index(work):
    a = run(work, ["-I", "file_of_file.txt", "-J", "0.9", "--derep-dump", "r2.dump", "-Q", "file_of_file.txt", "-O", "q_derep.gz"])
    b = run(work, ["-L", "r2.dump", "-Q", "file_of_file.txt", "-O", "q_loaded.gz"])
    text = gunzip(work / "q_derep.gz").decode()
    assert text == gunzip(work / "q_loaded.gz").decode() and len(text.splitlines()) == 9
    assert indexed_genomes(a.stdout) == indexed_genomes(b.stdout) == 3
    for n in NAMES:                                        # only representatives are ever a hit
        assert (n + ":" in text) == (n in REPS), n


def test_remove_equals_a_run_that_never_indexed_them(work):
    r = run(work, ["-I", "file_of_file.txt", "-J", "0.8", "--remove", "two.txt", "-D", "x.dump", "-Q", "file_of_file.txt", "-O", "o_removed.gz"])
    run(work, ["-I", "seven.txt", "-J", "0.8", "-D", "seven.dump", "-Q", "file_of_file.txt", "-O", "o_seven.gz"])
    assert r.stdout.count("| Remove lasted (s)                 |") == 1 and indexed_genomes(r.stdout) == 7
    assert gunzip(work / "x.dump") == gunzip(work / "seven.dump")
    text = gunzip(work / "o_removed.gz").decode()
    assert text == gunzip(work / "o_seven.gz").decode() and len(text.splitlines()) == 9
    assert not any(n + ":" in text for n in TWO)
    # -L old --remove names -D new
    run(work, ["-I", "file_of_file.txt", "-J", "0.8", "-D", "nine.dump", "-O", "o_nine.gz"])
    run(work, ["-L", "nine.dump", "--remove", "two.txt", "-D", "x2.dump", "-O", "o_x2.gz"])
    assert gunzip(work / "x2.dump") == gunzip(work / "seven.dump")


def test_remove_of_an_unknown_name_writes_nothing(work):
    r = run(work, ["-I", "file_of_file.txt", "--remove", "unknown.txt", "-D", "u.dump", "-Q", "file_of_file.txt", "-O", "u.gz"], code=1)
    assert "niqki: --remove: no indexed genome is named 'ecoli10p.fa.gz'" in r.stderr
    assert not (work / "u.dump").exists() and not (work / "u.gz").exists()


def test_an_empty_remove_file_drops_nothing(work):
    a = run(work, ["-I", "file_of_file.txt", "-J", "0.8", "--remove", "empty.txt", "-D", "e1.dump", "-Q", "file_of_file.txt", "-O", "e1.gz"])
    b = run(work, ["-I", "file_of_file.txt", "-J", "0.8", "-D", "e2.dump", "-Q", "file_of_file.txt", "-O", "e2.gz"])
    assert indexed_genomes(a.stdout) == indexed_genomes(b.stdout) == 9
    assert gunzip(work / "e1.dump") == gunzip(work / "e2.dump") and gunzip(work / "e1.gz") == gunzip(work / "e2.gz")


@pytest.mark.parametrize("option,arg", [("--remove", "two.txt"), ("--derep-dump", "g.dump")])
def test_dropping_genomes_needs_one_gpu(work, option, arg):
    r = run(work, ["-I", "file_of_file.txt", "--gpus", "2", option, arg, "-D", "g2.dump", "-O", "g.gz"], code=1,
            env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr
    assert not any((work / f).exists() for f in ("g.dump", "g2.dump", "g.gz"))
