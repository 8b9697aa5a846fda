"""GPU: the `niqki` program's --cover: the list written for every -Q / -l query is its greedy cover (niqki_staged_cover)
in the unchanged -O format.  Expected lists come from the oracle: pyoracle sketches of the very files (frame_records +
sketch_accumulate + densify) and tests/cover_ref.cover_by_oracle, the oracle's query on the masked sketch round by
round."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_cli_workdir
from cover_ref import cover_by_oracle

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")
EDIR = os.path.join(ROOT, "tests", "golden", "ecoli")


def run(td, args, code=0):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=str(td), capture_output=True, text=True, timeout=600)
    assert r.returncode == code, r.stdout + r.stderr
    return r


def lists(path):
    """[(query name, [(genome name, jaccard), ...])] of a -O file whose names hold no blank"""
    out = []
    for line in gzip.open(str(path), "rt").read().split("\n"):
        if line:
            toks = line.rstrip(" ").split(" ")
            out.append((toks[0], [(t.rsplit(":", 1)[0], float(t.rsplit(":", 1)[1])) for t in toks[1:]]))
    return out


def file_sketch(po, p, data):
    acc = np.full(1 << p.S, -1, dtype=np.int32)
    for _, _, seq in po.frame_records(data, "A", p.K):
        po.sketch_accumulate(p, seq, acc)
    return po.densify(p, acc)[0]


def expected(po, p, index_files, query_files, max_picks=0, cover=True):
    """the lists the program must write: (query name, [(genome name, count / F)])"""
    names = [n for n, _ in index_files]
    sk = np.stack([file_sketch(po, p, d) for _, d in index_files])
    ix = po.Index(p, sk)
    out = []
    for qn, d in query_files:
        q = file_sketch(po, p, d)
        if cover:
            picks = [(c, g) for c, g, _ in cover_by_oracle(ix, sk, q, p.min_score, max_picks)]
        else:
            picks = list(zip(*ix.query(q)))
        out.append((qn, [(names[int(g)], float("%g" % (int(c) / (1 << p.S)))) for c, g in picks]))
    return out


def same_lists(got, exp):
    assert [n for n, _ in got] == [n for n, _ in exp]
    for (qn, a), (_, b) in zip(got, exp):
        assert [x[0] for x in a] == [x[0] for x in b], qn
        assert all(abs(x[1] - y[1]) <= 1e-6 for x, y in zip(a, b)), qn


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, native, gold):
    _, meta = gold
    td = make_cli_workdir(tmp_path_factory.mktemp("cover"), native, meta)
    (td / "mix.fa").write_bytes((td / "syn00.fa").read_bytes() + (td / "syn05.fa").read_bytes())
    (td / "one.fa").write_bytes((td / "syn03.fa").read_bytes())
    (td / "qlist.txt").write_text("mix.fa\none.fa\n")
    (td / "reads2.fa").write_bytes((td / "reads.fa").read_bytes() * 2)
    return td


def test_whole_files_cover_top_and_the_format_without_p(workdir, po):
    p = po.make_params(31, 10, 12, 4, 0.1)
    index_files = [(n, (workdir / n).read_bytes()) for n in (workdir / "fof.txt").read_text().split()]
    query_files = [(n, (workdir / n).read_bytes()) for n in ("mix.fa", "one.fa")]
    base = ["-I", "fof.txt", "-Q", "qlist.txt", "-S", "10", "-J", "0.1"]
    run(workdir, base + ["-P", "-O", "plain.gz"])
    run(workdir, base + ["-P", "-O", "cover.gz", "--cover"])
    run(workdir, base + ["-P", "-O", "cover1.gz", "--cover", "--top", "1"])
    run(workdir, base + ["-O", "cover.bin.gz", "--cover"])
    exp = expected(po, p, index_files, query_files)
    same_lists(lists(workdir / "cover.gz"), exp)
    same_lists(lists(workdir / "cover1.gz"), expected(po, p, index_files, query_files, max_picks=1))
    same_lists(lists(workdir / "plain.gz"), expected(po, p, index_files, query_files, cover=False))
    assert gzip.open(str(workdir / "cover.bin.gz")).read() == gzip.open(str(workdir / "cover.gz")).read()
    # the mixed file: both of its genomes, first; the plain run lists strictly more genomes for it
    mix = dict(lists(workdir / "cover.gz"))["mix.fa"]
    assert sorted(n for n, _ in mix[:2]) == ["syn00.fa", "syn05.fa"]
    assert len(dict(lists(workdir / "plain.gz"))["mix.fa"]) > len(mix)
    assert [n for n, _ in dict(lists(workdir / "cover.gz"))["one.fa"]][:1] == ["syn03.fa"]


def test_lines_mode(workdir):
    # every read indexed twice: a read's plain list holds both copies (the later one first) and its chance neighbours
    base = ["-i", "reads2.fa", "-l", "reads.fa", "-S", "10", "-W", "10", "-J", "0.2", "-P"]
    run(workdir, base + ["-O", "lplain.gz"])
    run(workdir, base + ["-O", "lcover.gz", "--cover"])

    def by_read(path):       # a lines-mode name, of a query or a genome, is its whole header line: ">readN some text"
        out = []
        for line in gzip.open(str(path), "rt").read().split("\n"):
            if line:
                toks = line.rstrip(" ").split(" ")
                assert len(toks) % 3 == 0
                out.append((" ".join(toks[:3]), [" ".join(toks[i:i + 3]) for i in range(3, len(toks), 3)]))
        return out

    plain, cover = by_read(workdir / "lplain.gz"), by_read(workdir / "lcover.gz")
    assert len(plain) == 30 and [n for n, _ in plain] == [n for n, _ in cover]
    assert all(len(h) > 1 for _, h in plain)
    for (name, a), (_, b) in zip(plain, cover):
        assert b == a[:1], name


def test_e_coli_01_and_09_in_one_file(tmp_path, po):
    p = po.make_params(31, 15, 12, 4, 0.1)
    assert p.min_score == 3276
    names = open(os.path.join(EDIR, "file_of_file.txt")).read().split()
    index_files = [(n, gzip.open(os.path.join(EDIR, n), "rb").read()) for n in names]
    by_name = dict(index_files)
    mix = tmp_path / "mix0109.fa"
    mix.write_bytes(by_name["ecoli01p.fa.gz"] + by_name["ecoli09p.fa.gz"])
    (tmp_path / "q.txt").write_text(str(mix) + "\n")
    query_files = [(str(mix), mix.read_bytes())]
    base = ["-I", "file_of_file.txt", "-Q", str(tmp_path / "q.txt"), "-J", "0.1", "-P"]
    run(EDIR, base + ["-O", str(tmp_path / "plain.gz")])
    run(EDIR, base + ["-O", str(tmp_path / "cover.gz"), "--cover"])
    exp = expected(po, p, index_files, query_files)
    F = 1 << 15
    # what the oracle says of this file: 09 explains 29 435 slots, 01 then 3 333 more, nobody a further one
    assert exp[0][1] == [("ecoli09p.fa.gz", float("%g" % (29435 / F))), ("ecoli01p.fa.gz", float("%g" % (3333 / F)))]
    same_lists(lists(tmp_path / "cover.gz"), exp)
    plain = expected(po, p, index_files, query_files, cover=False)
    assert len(plain[0][1]) == 9
    same_lists(lists(tmp_path / "plain.gz"), plain)
