"""CPU: the `niqki` option parser knows --neighbors and --cluster (long only), and a host program built on an engine
without the two self-join calls says so instead of failing to link: the program is built on the fake engine of
tests/host_san (the C ABI answered on the CPU, niqki_neighbors_range / niqki_cluster not among its symbols), as
test_cli_topk_cpu.py does, into its own path.  Also here, because it needs no device: the clusters the E. coli
goldens must give, derived from the reference's matrix text (what tests/test_cli_selfjoin.py holds the program to)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_selfjoin")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_self_join_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    text = r.stderr + r.stdout
    assert "--neighbors  " in text and "--cluster <filename>" in text


def test_cluster_needs_a_file_name(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--cluster"], tmp_path)
    assert r.returncode == 1 and "Option 'cluster' requires a non-empty argument" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--cluster="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


@pytest.mark.parametrize("args", [["--cluster", "out.tsv"], ["--neighbors"], ["--neighbors", "--cluster", "out.tsv"]])
def test_an_engine_without_the_calls_says_so(niqki_fake, tmp_path, args):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz"] + args, tmp_path)
    assert r.returncode == 1 and "niqki: this engine has no self-join" in r.stderr
    assert not (tmp_path / "out.tsv").exists() and not (tmp_path / "o.gz").exists()      # before any work


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "--cluster", "out.tsv"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and not (tmp_path / "out.tsv").exists()


# ---- the expectation of the E. coli cluster tests, from the reference's golden matrix ---------------------------

def golden_counts():
    """(names, integer co-occurrence counts) of the reference's matrix of the nine E. coli genomes (default S = 15).
    The text has six significant digits: a cell is count / 32768, recovered as round(cell * 32768)."""
    text = json.load(open(os.path.join(GOLD, "reference_meta.json")))["ecoli_cli"]["matrix"]
    lines = [ln for ln in text.split("\n") if ln]
    assert lines[0].startswith("##Names")
    names = [t for t in lines[0].split("\t")[1:] if t]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r[0] for r in rows] == names
    cells = np.array([[float(x) for x in r[1:1 + len(names)]] for r in rows])
    counts = np.rint(cells * 32768).astype(np.int64)
    assert np.all(np.abs(counts / 32768 - cells) < 1e-5) and np.array_equal(counts, counts.T)
    return names, counts


def expected_clusters(names, counts, min_score):
    """lines of `niqki --cluster`: single linkage at count >= min_score, representative = first member in index order"""
    n = len(names)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a in range(n):
        for b in range(a):
            if counts[a, b] >= min_score:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    roots = [find(g) for g in range(n)]
    return "".join("%s\t%s\n" % (names[r], names[g]) for r in sorted(set(roots)) for g in range(n) if roots[g] == r)


def test_what_the_golden_matrix_says_about_the_e_coli_clusters():
    names, c = golden_counts()
    assert names == ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
    assert [int(c[i, i + 1]) for i in range(8)] == [31712, 31738, 31797, 31788, 31823, 31755, 31804, 31785]
    ms = int(np.uint32(0.97 * 32768))
    assert ms == 31784                                      # 08-09 links by one count, 06-07 misses by 29
    groups = {}
    for line in expected_clusters(names, c, ms).splitlines():
        rep, member = line.split("\t")
        groups.setdefault(rep[5:7], []).append(member[5:7])
    assert groups == {"01": ["01"], "02": ["02"], "03": ["03", "04", "05", "06"], "07": ["07", "08", "09"]}
    # chaining: at 0.9 and 0.8 the nine are ONE cluster although the first and the last share 0.79
    assert c[0, 8] < int(0.8 * 32768)
    for j in (0.9, 0.8):
        lines = expected_clusters(names, c, int(np.uint32(j * 32768))).splitlines()
        assert lines == ["%s\t%s" % (names[0], m) for m in names]
