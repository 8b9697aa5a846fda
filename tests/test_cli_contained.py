"""GPU: `niqki --min-containment <x> [--containment-of query|genome|either]` on a part and its whole, and on the nine
E. coli genomes.  The expected text is the reference's: the oracle's sketches of the files, an oracle Index for the full
ordered lists, tests/registers_ref.py for the sizes and the two printed shares, tests/contain_ref.py for which entries
stay and in which order -- never the calls under test, and no number is typed in here."""
import gzip
import math
import os

import numpy as np
import pytest

import contain_ref as cr
import registers_ref as rr
from conftest import ROOT
from test_cli_cover import file_sketch
from test_cli_retain import gunzip, run

pytestmark = pytest.mark.gpu
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")
NAMES = ["ecoli%02dp.fa.gz" % i for i in range(1, 10)]
W, H = 12, 4


def bases(seed, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def part_and_whole():
    """[(file name, FASTA bytes)]: genome A of 262 144 random bases, an unrelated B of the same length, a genome of 1000
    bases (below the estimator's range: no size); the queries: A's first 65 536 bases, and the short genome again"""
    a, b = bases(101, 262144), bases(202, 262144)
    short = bases(303, 1000)
    fasta = lambda name, seq: b">" + name.encode() + b"\n" + seq + b"\n"
    index = [("A.fa", fasta("A", a)), ("B.fa", fasta("B", b)), ("below.fa", fasta("below", short))]
    queries = [("part.fa", fasta("part", a[:65536])), ("below_again.fa", fasta("below", short))]
    return index, queries


def int_size(e):
    return math.floor(e[0] + 0.5) if e[1] == rr.OK else 0


def expected(po, S, J, index, queries, x, mode=cr.QUERY, top=0):
    """(the -O lines, the hits without a size estimate) of a run with --min-containment x at -J J"""
    p = po.make_params(31, S, W, H, J)
    names = [n for n, _ in index]
    sk = np.stack([file_sketch(po, p, d) for _, d in index])
    gsize = [rr.estimate(h, S, H) for h in rr.hist_ref(sk, W, H)]
    ix = po.Index(p, sk)
    lines, unsized = [], 0
    for qn, d in queries:
        q = file_sketch(po, p, d)
        qsize = rr.estimate(rr.hist_ref(q[None, :], W, H)[0], S, H)
        hc, hg = ix.query(q, min_score=p.min_score)
        full = (np.array([0, len(hc)]), hc, hg)
        _, _, kc, kg, nu = cr.contain_lists(full, [int_size(e) for e in gsize], [int_size(qsize)], mode, cr.min_share_of(x), top, F=1 << S)
        unsized += int(nu[0])
        lines.append(qn + " " + "".join(rr.containment_entry(names[int(g)], int(c), S, qsize, gsize[int(g)]) + " " for c, g in zip(kc, kg)))
    return lines, unsized


def claims(po):
    """what the example must show, from the reference alone"""
    index, queries = part_and_whole()
    plain = expected(po, 10, 0.5, index, queries[:1], 2.0 ** -32)[0]
    by_query = expected(po, 10, 0.1, index, queries, 0.8)
    by_genome = expected(po, 10, 0.1, index, queries, 0.8, cr.GENOME)
    either = expected(po, 10, 0.1, index, queries, 0.8, cr.MAX)
    assert plain == ["part.fa "]                                          # J near 0.25: nothing at -J 0.5, whatever the share
    name, jac, cq, cg = by_query[0][0].split(" ")[1].split(":")
    assert by_query[0][0].split(" ")[2:] == [""] and name == "A.fa"       # A, and not B
    assert float(jac) < 0.5 and abs(float(cq) - 1.0) < 0.05 and abs(float(cg) - 0.25) < 0.05
    assert by_genome[0][0] == "part.fa " and either[0][0] == by_query[0][0]
    assert by_query[1] > 0 and by_query[0][1] == "below_again.fa "        # the short genome hits itself: no size, not listed
    return by_query, by_genome, either


def lines(path):
    return gunzip(path).decode().split("\n")[:-1]


def unsized_line(stdout):
    return [ln for ln in stdout.split("\n") if ln.startswith("Hits without a size estimate: ")]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("contained_cli")
    index, queries = part_and_whole()
    for n, data in index + queries:
        (d / n).write_bytes(data)
    (d / "index.txt").write_text("".join(n + "\n" for n, _ in index))
    (d / "queries.txt").write_text("".join(n + "\n" for n, _ in queries))
    (d / "part_only.txt").write_text("part.fa\n")
    for n in NAMES:
        os.symlink(os.path.join(EDIR, n), d / n)
    (d / "file_of_file.txt").write_text("".join(n + "\n" for n in NAMES))
    return d


def test_a_part_finds_its_whole(work, po):
    by_query, by_genome, either = claims(po)
    r = run(work, ["-S", "10", "-I", "index.txt", "-Q", "part_only.txt", "-J", "0.5", "-O", "plain.gz"])
    assert lines(work / "plain.gz") == ["part.fa "] and not unsized_line(r.stdout)
    base = ["-S", "10", "-I", "index.txt", "-Q", "queries.txt", "-J", "0.1", "--min-containment", "0.8"]
    for of, want, out in (([], by_query, "q.gz"), (["--containment-of", "query"], by_query, "q2.gz"),
                          (["--containment-of", "genome"], by_genome, "g.gz"), (["--containment-of", "either"], either, "e.gz")):
        r = run(work, base + of + ["-O", out])
        assert lines(work / out) == want[0], of
        assert unsized_line(r.stdout) == ["Hits without a size estimate: %d" % want[1]], of


def test_ecoli_top_three_by_containment(work, po):
    index = [(n, gzip.open(os.path.join(EDIR, n), "rb").read()) for n in NAMES]
    want, unsized = expected(po, 15, 0.1, index, index, 0.88, top=3)
    assert unsized == 0 and all(len(w.split(" ")) == 5 for w in want)
    r = run(work, ["-I", "file_of_file.txt", "-Q", "file_of_file.txt", "-J", "0.1", "--min-containment", "0.88", "--top", "3", "-O", "ecoli.gz"])
    assert lines(work / "ecoli.gz") == want
    assert unsized_line(r.stdout) == ["Hits without a size estimate: 0"]
    # a paged index answers the same
    run(work, ["-I", "file_of_file.txt", "--resident-mib", "1", "-Q", "file_of_file.txt", "-J", "0.1", "--min-containment", "0.88", "--top", "3",
               "-O", "paged.gz"])
    assert lines(work / "paged.gz") == want


def test_refused_with_what_replaces_the_list(work):
    r = run(work, ["-I", "file_of_file.txt", "--min-containment", "0.5", "--cover", "-Q", "file_of_file.txt", "-O", "no.gz"], code=1)
    assert "--min-containment" in r.stderr and not (work / "no.gz").exists()
