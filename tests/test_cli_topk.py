"""GPU: the `niqki` program's --top <k> (niqki_params.top_k): per query the first k entries of the list the same run
without --top writes, with and without -P, on the whole-file, lines, load and --gpus paths."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT, make_cli_workdir

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "niqki_amd", "bin", "niqki")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, native, gold):
    _, meta = gold
    return make_cli_workdir(tmp_path_factory.mktemp("cli_topk"), native, meta)


def run(td, args, code=0, env=None):
    assert os.path.exists(BIN), "niqki_amd/bin/niqki missing: run __graft_entry__.build()"
    r = subprocess.run([BIN] + args, cwd=td, capture_output=True, text=True, timeout=600,
                       env=None if env is None else dict(os.environ, **env))
    assert r.returncode == code, r.stdout + r.stderr
    return r


def pretty(td, out):
    """(query name, its 'file:jaccard' tokens) per line, in file order (a lines-mode name is its whole header line)"""
    res = []
    for line in gzip.open(os.path.join(str(td), out), "rt").read().split("\n"):
        if line:
            toks = line.rstrip(" ").split(" ")
            hits = [t for t in toks if t.startswith("syn") and ".fa:" in t]
            res.append((" ".join(t for t in toks if t not in hits), hits))
    return res


def assert_cut(got, full, k):
    assert [n for n, _ in got] == [n for n, _ in full]
    for (_, a), (_, b) in zip(got, full):
        assert a == b[:k]
    assert any(len(b) > k for _, b in full)


def test_top_on_whole_files_pretty_and_binary(workdir):
    base = ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-J", "0"]
    run(workdir, base + ["-P", "-O", "all.gz"])
    run(workdir, base + ["-P", "-O", "top3.gz", "--top", "3"])
    assert_cut(pretty(workdir, "top3.gz"), pretty(workdir, "all.gz"), 3)
    run(workdir, base + ["-P", "-O", "top0.gz", "--top", "0"])
    assert gzip.open(str(workdir / "top0.gz")).read() == gzip.open(str(workdir / "all.gz")).read()
    # without -P: the program writes the query lines of src/niqki_index.cpp:546-553 all the same (the binary records of
    # output_query, :555-564, are unreachable from the command line); --top cuts them alike
    run(workdir, base + ["-O", "all.bin.gz"])
    run(workdir, base + ["-O", "top3.bin.gz", "--top", "3"])
    assert_cut(pretty(workdir, "top3.bin.gz"), pretty(workdir, "all.bin.gz"), 3)


def test_top_lines_and_load(workdir):
    run(workdir, ["-I", "fof.txt", "-l", "reads.fa", "-S", "10", "-J", "0", "-P", "-O", "lall.gz", "-D", "topk.dump"])
    run(workdir, ["-I", "fof.txt", "-l", "reads.fa", "-S", "10", "-J", "0", "-P", "-O", "ltop.gz", "--top", "2"])
    assert_cut(pretty(workdir, "ltop.gz"), pretty(workdir, "lall.gz"), 2)
    run(workdir, ["-L", "topk.dump", "-Q", "fof.txt", "-P", "-O", "dall.gz"])
    run(workdir, ["-L", "topk.dump", "-Q", "fof.txt", "-P", "-O", "dtop.gz", "--top", "2"])
    assert_cut(pretty(workdir, "dtop.gz"), pretty(workdir, "dall.gz"), 2)


def test_top_sharded_equals_one_gpu(workdir):
    base = ["-I", "fof.txt", "-Q", "fof.txt", "-S", "10", "-J", "0", "-P", "--top", "3"]
    run(workdir, base + ["-O", "g1.gz", "--gpus", "1"])
    run(workdir, base + ["-O", "g2.gz", "--gpus", "2"], env={"NIQKI_SHARDS_ON_ONE_DEVICE": "1"})
    assert gzip.open(str(workdir / "g2.gz")).read() == gzip.open(str(workdir / "g1.gz")).read()


def test_top_bad_arguments(workdir):
    r = run(workdir, ["-I", "fof.txt", "--top", "x"], code=1)
    assert "requires a numeric argument" in r.stderr
    r = run(workdir, ["-I", "fof.txt", "--top", "-1"], code=1)
    assert "top" in r.stderr
