"""CPU: the `niqki` option parser knows --lca and --lca-top (long only, with an argument), and the runs the program
refuses are refused before any work and before any file exists: a bad --lca-top, an index over several GPUs, together
with --cover, an engine without niqki_staged_query_lca (the program is built on the fake engine of tests/host_san, which
answers the C ABI on the CPU without it, as test_cli_collapse_cpu.py does, into a path of its own).  Also here, because
it needs no device: the product library exports the three calls, capi.ABI names them and Engine has their methods."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_lca")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_both_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    text = (r.stderr + r.stdout).splitlines()
    lines = [ln for ln in text if ln.startswith("  --lca ")]
    assert len(lines) == 1 and "<filename>" in lines[0] and "parent<TAB>child" in lines[0] and "no_common_taxon" in lines[0]
    lines = [ln for ln in text if ln.startswith("  --lca-top ")]
    assert len(lines) == 1 and "<permille>" in lines[0] and "0..1000" in lines[0] and "(100)" in lines[0]


def test_they_need_their_arguments(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for args in (["--lca"], ["--lca="], ["--lca", "t.txt", "--lca-top"], ["--lca", "t.txt", "--lca-top="]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz"] + args, tmp_path)
        assert r.returncode == 1 and "lca" in r.stderr + r.stdout and not (tmp_path / "o.gz").exists(), args


@pytest.mark.parametrize("value", ["1001", "-1", "ten", "10x", "1e2", "0.5", " 5", "+5", "99999999999999999999"])
def test_a_bad_lca_top_ends_the_run_before_any_work(niqki_fake, tmp_path, value):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--lca", "t.txt", "--lca-top=" + value], tmp_path)
    assert r.returncode == 1 and "lca-top" in r.stderr and "0..1000" in r.stderr
    assert "no LCA query" not in r.stderr and not (tmp_path / "o.gz").exists()


def test_a_good_lca_top_is_taken(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for value in ("0", "100", "1000", "007"):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--lca", "t.txt", "--lca-top", value], tmp_path)
        assert r.returncode == 1 and "lca-top" not in r.stderr and "no LCA query" in r.stderr   # (the next refusal in line)


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    for more in ([], ["--cover"], ["--collapse", "l.txt"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--lca", "t.txt"] + more, tmp_path)
        assert r.returncode == 1 and "single-GPU index" in r.stderr
        assert "no LCA query" not in r.stderr and "choose one" not in r.stderr
        assert not (tmp_path / "o.gz").exists()


def test_with_cover_choose_one(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--cover", "--lca", "t.txt"], tmp_path)
    assert r.returncode == 1 and "choose one" in r.stderr and "--lca" in r.stderr and "no LCA query" not in r.stderr
    assert not (tmp_path / "o.gz").exists()
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--lca", "t.txt", "--lca", "u.txt", "--top", "2", "--lca=v.txt"], tmp_path)
    assert r.returncode == 1 and "choose one" not in r.stderr                      # (several occurrences are no conflict)


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "q.txt").write_text("")
    (tmp_path / "t.txt").write_text("")
    (tmp_path / "l.txt").write_text("")
    for more in ([], ["--collapse", "l.txt"], ["--top", "3"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--lca", "t.txt"] + more, tmp_path)
        assert r.returncode == 1 and "niqki: this engine has no LCA query" in r.stderr
        assert "no collapsed query" not in r.stderr              # beside --lca the --collapse file supplies labels only
        assert not (tmp_path / "o.gz").exists()                  # before any work
    # ... and the same run without the option is none of its business, nor is --lca-top alone
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--lca-top", "50"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "o.gz").exists()


def test_the_library_and_the_engine_class_have_the_calls(native):
    L = native.lib()
    calls = ("niqki_set_taxonomy", "niqki_query_lca", "niqki_staged_query_lca")
    assert all(getattr(L, c) is not None for c in calls)
    names = [a[0] for a in native.capi.ABI]
    assert all(c in names for c in calls)
    assert all(callable(getattr(native.Engine, m, None))
               for m in ("set_taxonomy", "query_lca", "staged_query_lca", "query_lca_dev"))
    assert native.capi.TAXON_NONE == 0xFFFFFFFF
