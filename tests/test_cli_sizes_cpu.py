"""CPU: the `niqki` option parser knows --sizes and --containment (long only), and a host program built on an engine
without niqki_registers / niqki_staged_registers says so before any work: the program is built on the fake engine of
tests/host_san (the C ABI answered on the CPU, the register calls not among its symbols), as test_cli_pan_cpu.py does,
into its own path.  The combinations the program refuses on its own are refused first."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_sizes")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"
LACKS = "niqki: this engine cannot read sketch registers"


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_both_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0 and "--sizes <filename>" in r.stderr + r.stdout and "--containment  " in r.stderr + r.stdout


def test_sizes_needs_a_file_name(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--sizes"], tmp_path)
    assert r.returncode == 1 and "Option 'sizes' requires a non-empty argument" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--sizes="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


def test_the_options_are_long_only(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--containment=x"], tmp_path)       # (a flag: an attached value is not an argument)
    assert "Unknown option" not in r.stderr
    r = run(niqki_fake, ["--size", "s.gz"], tmp_path)
    assert r.returncode == 1 and "Unknown option 'size'" in r.stderr


@pytest.mark.parametrize("args", (["--sizes", "s.gz"], ["--containment", "-Q", "fof.txt"], ["--sizes", "s.gz", "--containment"]))
def test_an_engine_without_the_calls_says_so(niqki_fake, tmp_path, args):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump"] + args, tmp_path)
    assert r.returncode == 1 and LACKS in r.stderr
    assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump", "s.gz"))      # before any work


@pytest.mark.parametrize("other, text", ((["--cover"], "--cover"), (["--collapse", "g.tsv"], "--collapse"), (["--lca", "t.tsv"], "--lca"),
                                         (["--gpus", "2"], "single-GPU index")))
def test_the_refused_combinations_are_refused_first(niqki_fake, tmp_path, other, text):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--containment", "-Q", "fof.txt"] + other, tmp_path)
    assert r.returncode == 1 and text in r.stderr and "--containment" in r.stderr and "sketch registers" not in r.stderr
    assert not (tmp_path / "o.gz").exists()


def test_sizes_on_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "--gpus", "2", "--sizes", "s.gz"], tmp_path)
    assert r.returncode == 1 and "--sizes needs a single-GPU index" in r.stderr and "sketch registers" not in r.stderr
    assert not (tmp_path / "o.gz").exists() and not (tmp_path / "s.gz").exists()
