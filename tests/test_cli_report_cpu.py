"""CPU: the `niqki` option parser knows --report (long only, with an argument), and the runs the program refuses are
refused before any work and before any file exists: --report without --lca, an index over several GPUs (--lca's own
refusal), an engine without the calls (the program is built on the fake engine of tests/host_san, which answers the C
ABI on the CPU without the LCA query and without the tally, as test_cli_lca_cpu.py does, into a path of its own).  Also
here, because it needs no device: the product library exports the four calls, capi.ABI names them and Engine has
their methods."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_report")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def nothing_written(tmp_path):
    return not (tmp_path / "o.gz").exists() and not (tmp_path / "r.gz").exists()


def test_help_lists_the_option_once(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    lines = [ln for ln in (r.stderr + r.stdout).splitlines() if ln.startswith("  --report ")]
    assert len(lines) == 1 and lines[0].startswith("  --report <filename> ") and "--lca" in lines[0]
    assert "unclassified" in lines[0] and "no_common_taxon" in lines[0]


def test_it_needs_its_argument(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for args in (["--report"], ["--report="], ["--lca", "t.txt", "--report"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz"] + args, tmp_path)
        assert r.returncode == 1 and "Option 'report' requires a non-empty argument" in r.stderr, args
        assert "Unknown option" not in r.stderr and nothing_written(tmp_path), args
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-r", "r.gz"], tmp_path)         # a long option only
    assert r.returncode == 1 and "Unknown option" in r.stderr


def test_without_lca_it_is_refused(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "q.txt").write_text("")
    for more in ([], ["--lca-top", "50"], ["--collapse", "l.txt"], ["--gpus", "2"]):
        r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--report", "r.gz"] + more, tmp_path)
        assert r.returncode == 1 and "niqki: --report needs --lca" in r.stderr
        assert "no taxon tally" not in r.stderr and nothing_written(tmp_path)


def test_more_than_one_gpu_is_lcas_own_refusal(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--lca", "t.txt", "--report", "r.gz"], tmp_path)
    assert r.returncode == 1 and "--lca needs a single-GPU index" in r.stderr
    assert "no taxon tally" not in r.stderr and "no LCA query" not in r.stderr and nothing_written(tmp_path)


def test_an_engine_without_the_calls_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "q.txt").write_text("")
    (tmp_path / "t.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--lca", "t.txt", "--report", "r.gz"], tmp_path)
    # (this engine lacks the LCA query too, and that refusal is first in line)
    assert r.returncode == 1 and ("niqki: this engine has no taxon tally" in r.stderr or "niqki: this engine has no LCA query" in r.stderr)
    assert nothing_written(tmp_path)
    # ... and the same run without the two options is none of its business
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "o.gz").exists() and not (tmp_path / "r.gz").exists()


def test_the_tally_has_a_row_of_its_own_in_the_feature_table():
    """the text of an engine with the LCA query and without the tally: the fake engine cannot show it, the table can"""
    text = open(os.path.join(HOST, "index_host.cpp")).read()
    assert '{{"niqki_tally_begin", "niqki_tally_read"}, "this engine has no taxon tally"}' in text
    header = open(os.path.join(HOST, "index_host.h")).read()
    assert "COLLAPSE, TALLY }" in header


def test_the_library_and_the_engine_class_have_the_calls(native):
    L = native.lib()
    calls = ("niqki_tally_begin", "niqki_tally_add", "niqki_tally_read", "niqki_tally_end")
    assert all(getattr(L, c) is not None for c in calls)
    names = [a[0] for a in native.capi.ABI]
    assert all(names.count(c) == 1 for c in calls)
    assert all(callable(getattr(native.Engine, m, None))
               for m in ("tally_begin", "tally_add", "tally_read", "tally_end", "tally_add_dev", "tally_read_dev"))
    assert L.niqki_abi_version() == 2
