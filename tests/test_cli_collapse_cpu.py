"""CPU: the `niqki` option parser knows --collapse (long only, with an argument), and the runs the program refuses are
refused before any work and before any file exists: together with --cover, an index over several GPUs, an engine
without niqki_staged_query_collapsed (the program is built on the fake engine of tests/host_san, which answers the C ABI
on the CPU without it, as test_cli_cover_cpu.py does, into a path of its own).  Also here, because it needs no device:
the product library exports the three calls, capi.ABI names them and Engine has their methods."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_collapse")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_option(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    lines = [ln for ln in (r.stderr + r.stdout).splitlines() if ln.startswith("  --collapse ")]
    assert len(lines) == 1 and "<filename>" in lines[0] and "label<TAB>member" in lines[0] and "--top" in lines[0]


def test_it_needs_its_argument(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    for args in (["--collapse"], ["--collapse="]):
        r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz"] + args, tmp_path)
        assert r.returncode == 1 and "collapse" in r.stderr + r.stdout and not (tmp_path / "o.gz").exists()


def test_with_cover_choose_one(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--cover", "--collapse", "l.txt"], tmp_path)
    assert r.returncode == 1 and "choose one" in r.stderr and not (tmp_path / "o.gz").exists()
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--collapse", "l.txt", "--collapse", "m.txt", "--top", "2", "--collapse=n.txt"], tmp_path)
    assert r.returncode == 1 and "choose one" not in r.stderr                      # (several occurrences are no conflict)


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--collapse", "l.txt"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "no collapsed query" not in r.stderr
    assert not (tmp_path / "o.gz").exists()


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "q.txt").write_text("")
    (tmp_path / "l.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--collapse", "l.txt"], tmp_path)
    assert r.returncode == 1 and "niqki: this engine has no collapsed query" in r.stderr
    assert not (tmp_path / "o.gz").exists()                                        # before any work
    # ... and the same run without the option is none of its business
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "o.gz").exists()


def test_the_library_and_the_engine_class_have_the_calls(native):
    L = native.lib()
    calls = ("niqki_set_labels", "niqki_query_collapsed", "niqki_staged_query_collapsed")
    assert all(getattr(L, c) is not None for c in calls)
    names = [a[0] for a in native.capi.ABI]
    assert all(c in names for c in calls)
    assert all(callable(getattr(native.Engine, m, None))
               for m in ("set_labels", "query_collapsed", "staged_query_collapsed", "query_collapsed_dev"))
