"""CPU: the `niqki` option parser knows --cover (long only, no argument), and the runs the program refuses are refused
before any work and before any file exists: an engine without niqki_staged_cover (the program is built on the fake
engine of tests/host_san, which answers the C ABI on the CPU without it, as test_cli_linkage_cpu.py does, into a path of
its own), an index over several GPUs, a paged index.  Also here, because it needs no device: the product library
exports the two calls and Engine has their methods."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_cover")
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
    lines = [ln for ln in (r.stderr + r.stdout).splitlines() if ln.startswith("  --cover ")]
    assert len(lines) == 1 and "--top" in lines[0]


def test_it_takes_no_argument(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--cover=x"], tmp_path)
    assert r.returncode == 1 and "cover" in r.stderr + r.stdout and not (tmp_path / "o.gz").exists()


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "q.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz", "--cover"], tmp_path)
    assert r.returncode == 1 and "niqki: this engine has no cover" in r.stderr
    assert not (tmp_path / "o.gz").exists()                                        # before any work
    # ... and the same run without the option is none of its business
    r = run(niqki_fake, ["-I", "fof.txt", "-Q", "q.txt", "-O", "o.gz"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "o.gz").exists()


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--resident-mib", "4", "--cover"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "no cover" not in r.stderr
    assert not (tmp_path / "o.gz").exists()


def test_a_paged_index_is_refused(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--resident-mib", "4", "--cover"], tmp_path)
    assert r.returncode == 1 and "resident index" in r.stderr and "no cover" not in r.stderr
    assert not (tmp_path / "o.gz").exists()


def test_the_library_and_the_engine_class_have_the_calls(native):
    L = native.lib()
    assert L.niqki_cover is not None and L.niqki_staged_cover is not None
    names = [a[0] for a in native.capi.ABI]
    assert "niqki_cover" in names and "niqki_staged_cover" in names
    assert all(callable(getattr(native.Engine, m, None)) for m in ("cover", "staged_cover", "cover_dev"))
