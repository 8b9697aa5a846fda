"""GPU: `niqki --derep <file>` writes the greedy representatives at the -J threshold as representative<TAB>member
lines, held here to what the definition (test_cli_derep_cpu.py's expected_derep, plain Python) gives on the
REFERENCE's golden matrix of the nine E. coli genomes: integer counts, not floats."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_derep_cpu import expected_derep
from test_cli_selfjoin_cpu import expected_clusters, golden_counts

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")


def run(args, code=0, env=None):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=EDIR, capture_output=True, text=True, timeout=600,
                       env=None if env is None else dict(os.environ, **env))
    assert r.returncode == code, r.stdout + r.stderr
    return r


def gunzip(p):
    return gzip.open(str(p), "rb").read()


@pytest.mark.parametrize("j,n_rep", [("0.97", 6), ("0.9", 3), ("0.8", 2), ("0.1", 1)])
def test_derep_file_equals_the_definition_on_the_reference_matrix(tmp_path, j, n_rep):
    names, counts = golden_counts()
    r = run(["-I", "file_of_file.txt", "-J", j, "--derep", str(tmp_path / "d.tsv"), "-O", str(tmp_path / "o.gz")])
    assert r.stdout.count("| Dereplication lasted (s)          |") == 1 and "Cluster lasted" not in r.stdout
    got = gunzip(tmp_path / "d.tsv").decode()              # a gzip file whatever its name, like -O
    assert got == expected_derep(names, counts, int(np.uint32(float(j) * 32768)))
    assert sum(1 for a, b in (ln.split("\t") for ln in got.splitlines()) if a == b) == n_rep


def test_derep_after_dump_and_load(tmp_path):
    names, counts = golden_counts()
    exp = expected_derep(names, counts, int(np.uint32(0.9 * 32768)))
    run(["-I", "file_of_file.txt", "-J", "0.9", "-D", str(tmp_path / "d.dump"), "--derep", str(tmp_path / "i.tsv"),
         "-O", str(tmp_path / "o1.gz")])
    run(["-L", str(tmp_path / "d.dump"), "--derep", str(tmp_path / "l.tsv"), "-O", str(tmp_path / "o2.gz")])
    assert gunzip(tmp_path / "i.tsv").decode() == exp and gunzip(tmp_path / "l.tsv").decode() == exp


def test_derep_and_cluster_in_one_run(tmp_path):
    names, counts = golden_counts()
    ms = int(np.uint32(0.9 * 32768))
    r = run(["-I", "file_of_file.txt", "-J", "0.9", "--derep", str(tmp_path / "d.tsv"), "--cluster", str(tmp_path / "c.tsv"),
             "-O", str(tmp_path / "o.gz")])
    assert r.stdout.index("| Cluster lasted (s)") < r.stdout.index("| Dereplication lasted (s)")   # cluster first
    assert gunzip(tmp_path / "d.tsv").decode() == expected_derep(names, counts, ms)
    assert gunzip(tmp_path / "c.tsv").decode() == expected_clusters(names, counts, ms)


def test_derep_needs_one_gpu(tmp_path):
    r = run(["-I", "file_of_file.txt", "--gpus", "2", "--derep", str(tmp_path / "x.tsv"), "-O", str(tmp_path / "o.gz")],
            code=1, env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr
    assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "o.gz").exists()
