"""GPU: the `niqki` program's linkage phase on the nine E. coli genomes.  --mst / --linkage / --tree write, from ONE
engine call at the -J threshold, the maximum spanning forest, the merge table and the Newick dendrograms; they are
held here to the texts that the REFERENCE's golden matrix gives through the definition restated in
test_cli_linkage_cpu.py (integer counts, a plain Kruskal, labels at every level) and test_linkage_text_cpu.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_derep_cpu import derep_labels
from test_cli_linkage_cpu import expected_texts, groups_of_linkage_text
from test_cli_selfjoin_cpu import golden_counts

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
    return gzip.open(str(p), "rb").read().decode()


def three(tmp_path, tag):
    return [x for o in ("mst", "linkage", "tree") for x in ("--" + o, str(tmp_path / ("%s.%s" % (tag, o))))]


def texts(tmp_path, tag):
    return tuple(gunzip(tmp_path / ("%s.%s" % (tag, o))) for o in ("mst", "linkage", "tree"))   # gzip files, like -O


@pytest.mark.parametrize("j,trees", [("0.9", 1), ("0.97", 4)])
def test_the_three_files_equal_the_texts_of_the_reference_matrix(tmp_path, j, trees):
    names, counts = golden_counts()
    ms = int(np.uint32(float(j) * 32768))
    r = run(["-I", "file_of_file.txt", "-J", j, "-O", str(tmp_path / "o.gz"), "--cluster", str(tmp_path / "c.tsv")] + three(tmp_path, "a"))
    assert r.stdout.count("| Linkage lasted (s)") == 1 and r.stdout.count("| Cluster lasted (s)") == 1
    assert r.stdout.index("| Cluster lasted (s)") < r.stdout.index("| Linkage lasted (s)") < r.stdout.index("| Query lasted (s)")
    got = texts(tmp_path, "a")
    assert got == expected_texts(names, counts, ms)
    assert got[2].count(";\n") == trees == len(got[2].splitlines())
    # cutting --linkage's lines at the -J of the --cluster run reproduces that file's groups
    assert groups_of_linkage_text(got[1], ms) == gunzip(tmp_path / "c.tsv")


def test_one_option_alone_and_a_cut_above_the_floor(tmp_path):
    names, counts = golden_counts()
    run(["-I", "file_of_file.txt", "-J", "0.9", "-O", str(tmp_path / "o.gz"), "--linkage", str(tmp_path / "only.tsv")])
    link = gunzip(tmp_path / "only.tsv")
    assert link == expected_texts(names, counts, int(np.uint32(0.9 * 32768)))[1]
    run(["-I", "file_of_file.txt", "-J", "0.97", "-O", str(tmp_path / "o2.gz"), "--cluster", str(tmp_path / "c97.tsv")])
    assert groups_of_linkage_text(link, int(np.uint32(0.97 * 32768))) == gunzip(tmp_path / "c97.tsv")


def test_after_derep_dump_the_files_describe_the_dereplicated_index(tmp_path):
    names, counts = golden_counts()
    ms = int(np.uint32(0.9 * 32768))
    _, reps = derep_labels(counts, ms)
    assert 1 < len(reps) < 9
    r = run(["-I", "file_of_file.txt", "-J", "0.9", "-O", str(tmp_path / "o.gz"), "--derep-dump", str(tmp_path / "r.dump")]
            + three(tmp_path, "d"))
    assert r.stdout.index("| Dereplication lasted (s)") < r.stdout.index("| Linkage lasted (s)")
    sub = counts[np.ix_(reps, reps)]
    assert texts(tmp_path, "d") == expected_texts([names[g] for g in reps], sub, ms)


def test_the_linkage_phase_needs_one_gpu(tmp_path):
    r = run(["-I", "file_of_file.txt", "--gpus", "2", "-O", str(tmp_path / "o.gz")] + three(tmp_path, "x"), code=1,
            env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert "single-GPU index" in r.stderr
    assert not any((tmp_path / ("x." + o)).exists() for o in ("mst", "linkage", "tree")) and not (tmp_path / "o.gz").exists()
