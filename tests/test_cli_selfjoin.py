"""GPU: the `niqki` program's self-join options.  --neighbors writes what a second run with -Q <the same list> writes;
--cluster <file> writes the single-linkage clusters at the -J threshold as representative<TAB>member lines, held here
to the clusters that the REFERENCE's golden matrix of the nine E. coli genomes gives (thresholded and united by
test_cli_selfjoin_cpu.py's helpers: integer counts, not floats)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
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


@pytest.mark.parametrize("j", ["0.97", "0.9", "0.8"])
def test_cluster_file_equals_the_clusters_of_the_reference_matrix(tmp_path, j):
    names, counts = golden_counts()
    r = run(["-I", "file_of_file.txt", "-J", j, "--cluster", str(tmp_path / "c.tsv"), "-O", str(tmp_path / "o.gz")])
    assert r.stdout.count("| Cluster lasted (s)") == 1
    got = gunzip(tmp_path / "c.tsv").decode()              # a gzip file whatever its name, like -O
    exp = expected_clusters(names, counts, int(np.uint32(float(j) * 32768)))
    assert got == exp
    assert len(set(line.split("\t")[0] for line in got.splitlines())) == (4 if j == "0.97" else 1)


@pytest.mark.parametrize("extra", [["-P"], [], ["-P", "--top", "2"]])
def test_neighbors_equal_a_query_with_the_same_list(tmp_path, extra):
    base = ["-I", "file_of_file.txt", "-S", "12", "-J", "0.5"] + extra
    run(base + ["--neighbors", "-O", str(tmp_path / "a.gz")])
    run(base + ["-Q", "file_of_file.txt", "-O", str(tmp_path / "b.gz")])
    a, b = gunzip(tmp_path / "a.gz"), gunzip(tmp_path / "b.gz")
    assert a == b and a.count(b"\n") == 9
    if "--top" in extra:
        assert all(line.count(b":") == 2 for line in a.splitlines())


def test_cluster_after_load_and_lines_mode(tmp_path):
    small = ["-S", "10", "-W", "8", "-J", "0.9"]
    run(["-I", "file_of_file.txt"] + small + ["-D", str(tmp_path / "d.dump"), "--cluster", str(tmp_path / "i.tsv"),
                                              "-O", str(tmp_path / "o1.gz")])
    run(["-L", str(tmp_path / "d.dump"), "--cluster", str(tmp_path / "l.tsv"), "-O", str(tmp_path / "o2.gz")])
    a, b = gunzip(tmp_path / "i.tsv"), gunzip(tmp_path / "l.tsv")
    assert a == b and a.count(b"\n") == 9
    # -i: every record of the file is a genome, named by its header line
    with open(tmp_path / "recs.fa", "wb") as f:
        for name in ("ecoli01p.fa.gz", "ecoli02p.fa.gz"):
            f.write(gunzip(os.path.join(EDIR, name)))
    run(["-i", str(tmp_path / "recs.fa")] + small + ["--cluster", str(tmp_path / "r.tsv"), "-O", str(tmp_path / "o3.gz")])
    lines = gunzip(tmp_path / "r.tsv").decode().splitlines()
    assert len(lines) >= 2 and all(len(ln.split("\t")) == 2 for ln in lines)
    assert lines[0].split("\t")[0] == lines[0].split("\t")[1]                 # the first genome represents its cluster


def test_self_join_needs_one_gpu(tmp_path):
    r = run(["-I", "file_of_file.txt", "--gpus", "2", "--cluster", str(tmp_path / "x.tsv"), "-O", str(tmp_path / "o.gz")],
            code=1, env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr
    assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "o.gz").exists()
    r = run(["-I", "file_of_file.txt", "--gpus", "2", "--neighbors", "-O", str(tmp_path / "o.gz")], code=1,
            env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr and not (tmp_path / "o.gz").exists()
