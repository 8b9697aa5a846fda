"""CPU: the `niqki` option parser knows --remove and --derep-dump (long only), and a host program built on an engine
without niqki_retain says so before any work: the program is built on the fake engine of tests/host_san (the C ABI
answered on the CPU, niqki_retain not among its symbols), as test_cli_derep_cpu.py does, into its own path."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_retain")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"
OPTIONS = [("--remove", "names.txt"), ("--derep-dump", "r.dump")]


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_two_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    assert r.returncode == 0
    assert "--remove <filename>" in r.stderr + r.stdout and "--derep-dump <filename>" in r.stderr + r.stdout


@pytest.mark.parametrize("option,arg", OPTIONS)
def test_the_options_need_a_file_name(niqki_fake, tmp_path, option, arg):
    r = run(niqki_fake, ["-I", "fof.txt", option], tmp_path)
    assert r.returncode == 1 and "Option '%s' requires a non-empty argument" % option[2:] in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", option + "="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


@pytest.mark.parametrize("option,arg", OPTIONS)
def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path, option, arg):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "names.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump", option, arg], tmp_path)
    assert r.returncode == 1 and "niqki: this engine cannot drop genomes" in r.stderr
    assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump", "r.dump"))      # before any work


@pytest.mark.parametrize("option,arg", OPTIONS)
def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path, option, arg):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "-O", "o.gz", option, arg], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "cannot drop genomes" not in r.stderr
    assert not (tmp_path / "o.gz").exists() and not (tmp_path / "r.dump").exists()
