"""CPU: the `niqki` option parser knows --mst, --linkage and --tree (long only), and a host program built on an engine
without niqki_linkage says so before any work: the program is built on the fake engine of tests/host_san (the C ABI
answered on the CPU, niqki_linkage not among its symbols), as test_cli_selfjoin_cpu.py does, into its own path.
Also here, because it needs no device: cut_linkage against the definition walked genome by genome, the hierarchy and
the forest of a matrix of counts in plain Python (what tests/test_cli_linkage.py holds the program to), and what they
give on the reference's golden matrix of the nine E. coli genomes."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cli_selfjoin_cpu import expected_clusters, golden_counts
from test_linkage_text_cpu import linkage_text, mst_text, tree_text

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_linkage")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"
OPTIONS = ["mst", "linkage", "tree"]


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_three_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    text = r.stderr + r.stdout
    assert all("--%s <filename>" % o in text for o in OPTIONS)


@pytest.mark.parametrize("option", OPTIONS)
def test_each_needs_a_file_name(niqki_fake, tmp_path, option):
    r = run(niqki_fake, ["-I", "fof.txt", "--" + option], tmp_path)
    assert r.returncode == 1 and "Option '%s' requires a non-empty argument" % option in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--%s=" % option], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


@pytest.mark.parametrize("options", [["mst"], ["linkage"], ["tree"], OPTIONS])
def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path, options):
    (tmp_path / "fof.txt").write_text("")
    args = [x for o in options for x in ("--" + o, o + ".out")]
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz"] + args, tmp_path)
    assert r.returncode == 1 and "niqki: this engine has no linkage" in r.stderr
    assert not any((tmp_path / (o + ".out")).exists() for o in options) and not (tmp_path / "o.gz").exists()     # before any work


@pytest.mark.parametrize("option", OPTIONS)
def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path, option):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "--" + option, "out.txt"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "no linkage" not in r.stderr
    assert not (tmp_path / "out.txt").exists()


# ---- cut_linkage ---------------------------------------------------------------------------------------------------

def test_cut_linkage_equals_the_walk_of_the_definition():
    from niqki_amd.capi import cut_linkage          # (pure numpy: no library is loaded)
    rng = np.random.default_rng(2)
    for n, p_root, window in ((1, 1.0, 1), (400, 0.1, 30), (400, 0.0, 1), (2000, 0.02, 2000)):
        into, cnt = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)
        for g in range(1, n):
            if rng.random() >= p_root:
                into[g] = rng.integers(max(0, g - window), g)
                cnt[g] = cnt[into[g]] + rng.integers(1, 4)
        for t in sorted({1, 2, 5, int(cnt.max()), int(cnt.max()) + 1, int(np.median(cnt))}):
            exp = np.empty(n, np.uint32)
            for g in range(n):
                x = g
                while into[x] != x and cnt[x] >= t:               # follow merge_into while merge_count >= t
                    x = into[x]
                exp[g] = x
            got = cut_linkage(into, cnt, t)
            assert got.dtype == np.uint32 and np.array_equal(got, exp), (n, t)
    assert cut_linkage(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3).size == 0
    # floor 0: the roots joined genome 0 at count 0
    into, cnt = np.array([0, 0, 1, 0, 3], np.uint32), np.array([0, 0, 7, 0, 7], np.uint32)
    assert cut_linkage(into, cnt, 0).tolist() == [0, 0, 0, 0, 0] and cut_linkage(into, cnt, 1).tolist() == [0, 1, 1, 3, 3]


# ---- the definition over a matrix of counts, and the expectation of the E. coli tests -------------------------------

def labels_at(counts, t):
    """single linkage at count >= t: the smallest id of every genome's component"""
    n = len(counts)
    lab = list(range(n))
    changed = True
    while changed:                                   # (nine genomes: plain relaxation)
        changed = False
        for a in range(n):
            for b in range(n):
                if a != b and counts[a][b] >= t and lab[b] < lab[a]:
                    lab[a] = lab[b]
                    changed = True
    return lab


def hierarchy_of(counts, floor):
    """(merge_into, merge_count) from the definition: labels_t at every distinct count >= max(floor, 1), descending"""
    n = len(counts)
    into, cnt = list(range(n)), [0] * n
    levels = sorted({int(counts[a][b]) for a in range(n) for b in range(a)} - set(range(max(floor, 1))), reverse=True)
    for t in levels:
        lab = labels_at(counts, t)
        for g in range(n):
            if lab[g] != g and into[g] == g:
                into[g], cnt[g] = lab[g], t
    if floor == 0:
        into = [0 if into[g] == g else into[g] for g in range(n)]
    return into, cnt


def forest_of(counts, floor):
    """Kruskal in the edge order over the pairs with count >= max(floor, 1); floor 0: then (0, r, 0) for the roots left"""
    n = len(counts)
    pairs = sorted((-int(counts[a][b]), a, b) for b in range(n) for a in range(b) if counts[a][b] >= max(floor, 1))
    lab = list(range(n))
    out = []
    for c, a, b in pairs:
        if lab[a] != lab[b]:
            out.append((a, b, -c))
            lo, hi = min(lab[a], lab[b]), max(lab[a], lab[b])
            lab = [lo if x == hi else x for x in lab]
    if floor == 0:
        out += [(0, r, 0) for r in range(1, n) if lab[r] == r]
    return [e[0] for e in out], [e[1] for e in out], [e[2] for e in out]


def expected_texts(names, counts, min_score, F=32768):
    """what `niqki --mst a --linkage b --tree c` writes at that min_score: (mst, linkage, tree)"""
    into, cnt = hierarchy_of(counts, min_score)
    lo, hi, ec = forest_of(counts, min_score)
    return mst_text(lo, hi, ec, names, F), linkage_text(into, cnt, names, F), tree_text(into, cnt, names, F)


def groups_of_linkage_text(text, threshold_jaccard_count, F=32768):
    """the --cluster lines that cutting a --linkage file at a count gives (the file has %g jaccards: six digits, enough
    to tell counts of a 2^15 sketch apart)"""
    rows = [ln.split("\t") for ln in text.splitlines()]
    names = [r[0] for r in rows]
    at = {nm: i for i, nm in enumerate(names)}
    into = [at[r[1]] for r in rows]
    cnt = [int(round(float(r[2]) * F)) for r in rows]
    lab = []
    for g in range(len(names)):
        x = g
        while into[x] != x and cnt[x] >= threshold_jaccard_count:
            x = into[x]
        lab.append(x)
    return "".join("%s\t%s\n" % (names[r], names[g]) for r in sorted(set(lab)) for g in range(len(names)) if lab[g] == r)


def test_what_the_golden_matrix_says_about_the_e_coli_hierarchy():
    names, c = golden_counts()
    short = [nm[5:7] for nm in names]
    ms97, ms90 = int(np.uint32(0.97 * 32768)), int(np.uint32(0.9 * 32768))
    # at 0.97 four trees: {01}, {02}, {03-06}, {07-09}
    mst, link, tree = expected_texts(short, c, ms97)
    trees = tree.splitlines()
    assert len(trees) == 4 and all(t.endswith(";") for t in trees)
    leaves = [sorted(x for x in t.replace("(", ",").replace(")", ",").replace(":", ",").replace(";", ",").split(",") if x.startswith("'"))
              for t in trees]
    assert leaves == [["'01'"], ["'02'"], ["'03'", "'04'", "'05'", "'06'"], ["'07'", "'08'", "'09'"]]
    assert trees[0] == "'01';" and trees[1] == "'02';"
    assert len(mst.splitlines()) == 9 - 4 and len(link.splitlines()) == 9
    roots = [ln.split("\t")[0] for ln in link.splitlines() if ln.split("\t")[0] == ln.split("\t")[1]]
    assert roots == ["01", "02", "03", "07"] and all(ln.endswith("\t0") for ln in link.splitlines() if ln[:2] in roots)
    # at 0.9 one tree of all nine, eight edges, each at or above 0.9, best first
    mst, link, tree = expected_texts(short, c, ms90)
    assert len(tree.splitlines()) == 1 and tree.count("'") == 18 and len(mst.splitlines()) == 8
    j = [float(ln.split("\t")[2]) for ln in mst.splitlines()]
    assert j == sorted(j, reverse=True) and j[-1] >= ms90 / 32768 - 1e-6
    # the 08-09 link (31785, one count above 0.97's min_score) is a forest edge
    assert "08\t09\t%g\n" % (31785 / 32768) in mst
    # one hierarchy answers every threshold: its cuts are --cluster's groups
    for t in (ms97, ms90, int(np.uint32(0.8 * 32768)), 31785, 31786):
        if t >= ms90:
            assert groups_of_linkage_text(link, t) == expected_clusters(short, c, t), t
    assert groups_of_linkage_text(expected_texts(short, c, 1)[1], int(np.uint32(0.8 * 32768))) == expected_clusters(short, c, int(np.uint32(0.8 * 32768)))
