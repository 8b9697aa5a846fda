"""CPU: the `niqki` option parser knows --merge and --novel (long only), and a host program built on an engine without
niqki_append_* / niqki_dereplicate_from says so before any work: the program is built on the fake engine of
tests/host_san (the C ABI answered on the CPU, those calls not among its symbols), as test_cli_retain_cpu.py does, into
its own path."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "niqki_amd", "host")
OUT = os.path.join(ROOT, "tests", "host_san", "bin", "niqki_fake_merge")
ENGINE = "../../tests/host_san/fake_engine.cpp ../../oracle/niqki_oracle.c"
OPTIONS = [("--merge", "b.dump", "niqki: this engine cannot merge dumps"), ("--novel", "added.txt", "niqki: this engine has no dereplication")]


@pytest.fixture(scope="module")
def niqki_fake():
    subprocess.check_call(["make", "-C", HOST, "-B", "ENGINE=" + ENGINE, "SAN=none", "OUT=" + os.path.relpath(OUT, HOST)],
                          stdout=subprocess.DEVNULL)
    return OUT


def run(binary, args, tmp_path):
    return subprocess.run([binary] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_help_lists_the_two_options(niqki_fake, tmp_path):
    r = run(niqki_fake, ["--help"], tmp_path)
    text = r.stderr + r.stdout
    assert r.returncode == 0
    assert "--merge <filename>" in text and "--novel <filename>" in text
    merge = next(ln for ln in text.splitlines() if "--merge <filename>" in ln)
    assert "may be repeated" in merge and "every occurrence" in merge       # the one option where not only the last counts


@pytest.mark.parametrize("option,arg,message", OPTIONS)
def test_the_options_need_a_file_name(niqki_fake, tmp_path, option, arg, message):
    r = run(niqki_fake, ["-I", "fof.txt", option], tmp_path)
    assert r.returncode == 1 and "Option '%s' requires a non-empty argument" % option[2:] in r.stderr
    r = run(niqki_fake, ["-I", "fof.txt", option + "="], tmp_path)
    assert r.returncode == 1 and "requires a non-empty argument" in r.stderr


@pytest.mark.parametrize("option,arg,message", OPTIONS)
def test_an_engine_without_the_calls_says_so(niqki_fake, tmp_path, option, arg, message):
    (tmp_path / "fof.txt").write_text("")
    r = run(niqki_fake, ["-I", "fof.txt", "-O", "o.gz", "-D", "d.dump", option, arg], tmp_path)
    assert r.returncode == 1 and message in r.stderr
    assert not any((tmp_path / f).exists() for f in ("o.gz", "d.dump", "added.txt"))   # before any work


@pytest.mark.parametrize("option,arg,message", OPTIONS)
def test_more_than_one_gpu_is_refused_first(niqki_fake, tmp_path, option, arg, message):
    r = run(niqki_fake, ["-I", "fof.txt", "--gpus", "2", "-O", "o.gz", option, arg], tmp_path)
    assert r.returncode == 1 and "single-GPU index" in r.stderr and message not in r.stderr
    assert "--merge" in r.stderr and "--novel" in r.stderr                  # the message names them
    assert not (tmp_path / "o.gz").exists() and not (tmp_path / "added.txt").exists()
