"""CPU: the `niqki` option parser knows --pan (long only), and a host program built on an engine without niqki_unite
says so before any work: the program is built on the fake engine of tests/host_san (the C ABI answered on the CPU,
niqki_unite not among its symbols), as test_cli_retain_cpu.py does, into its own path."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_pan")
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
    assert r.returncode == 0 and "--pan <filename>" in r.stderr + r.stdout


def test_the_option_needs_a_file_name(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--pan"], tmp_path)
    assert r.returncode == 1 and "Option 'pan' requires a non-empty argument" in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", "--pan="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


def test_an_engine_without_the_call_says_so(niqki_fake, tmp_path):
    (tmp_path / "fof.txt").write_text("")
    (tmp_path / "groups.tsv").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump", "--pan", "groups.tsv"], tmp_path)
    assert r.returncode == 1 and "niqki: this engine cannot unite genomes" in r.stderr
    assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump"))      # before any work


def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "-O", "o.gz", "--pan", "groups.tsv"], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and "cannot unite genomes" not in r.stderr
    assert not (tmp_path / "o.gz").exists()
